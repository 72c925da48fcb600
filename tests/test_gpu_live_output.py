"""Audio out at any rate, on the GPU (mbexwn_vocoder_amd/live.py, csrc/resample_stream.hip through
include/mbexwn_live_out.h): the streaming output resampler against the offline device resampler bit for bit, the memory
contract of the entry point between guard bands and its refusals, the output stage with several streams and rates, the live
pipeline with ``output_rate``, the offline ``out_rate`` and the two tools.  Every comparison is on the int32 view."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

from guarded import FILLS, GuardSet, fill_word

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM_TOOL = os.path.join(ROOT, "mbexwn_vocoder_amd", "bin", "stream_transpose.py")
RESYNTH_TOOL = os.path.join(ROOT, "mbexwn_vocoder_amd", "bin", "resynth_mel.py")
SMALL = {"mbexwn_config:pp_mod_subnet:n_channels": 32, "mbexwn_config:pp_mod_subnet:n_layers": 5}
MODEL_RATE = 24000
TILE = 256                                    # outputs per block of the stream kernels


def bits(arr):
    return np.ascontiguousarray(arr, dtype=np.float32).view(np.int32)


def sound(seed, n, rate=MODEL_RATE):
    rng = np.random.default_rng(seed)
    tt = np.arange(n) / float(rate)
    return (0.3 * np.sin(2 * np.pi * 170.0 * tt) + 0.05 * rng.normal(size=n)).astype(np.float32)


def geometry(rate):
    """(up, down, half, n_taps) of the output filter for 24 kHz -> rate."""
    from mbexwn_vocoder_amd.resample import reference_filter
    taps, up, down = reference_filter(MODEL_RATE, rate)
    return up, down, (taps.size - 1) // 2, int(taps.size)


def random_cuts(rng, n, big, forced=()):
    """Push sizes that sum to n: the forced ones first, then pushes of 1 sample, of a few and of up to `big`, at random."""
    cuts, left = [], n
    for cc in forced:
        cc = min(cc, left)
        if cc:
            cuts.append(cc)
            left -= cc
    while left:
        kind = int(rng.integers(0, 3))
        cc = min(left, 1 if kind == 0 else int(rng.integers(2, 6)) if kind == 1 else int(rng.integers(6, big + 1)))
        cuts.append(cc)
        left -= cc
    return cuts


def offline_at(snd, rate):
    """resample_device of a whole model-rate sound to `rate`."""
    import torch
    from mbexwn_vocoder_amd.resample import resample_device
    out, n_out = resample_device(torch.as_tensor(np.ascontiguousarray(snd, dtype=np.float32)[None]).cuda(), None, MODEL_RATE, rate)
    assert int(n_out[0]) == out.shape[1]
    return out[0].cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernel alone
# ---------------------------------------------------------------------------------------------------------------------
def emit_through_ring(snd, rate, cuts, ring):
    """Append every cut to a one-slot model-rate ring (mbxl_ring_append) and produce every output that became final
    (mbxo_resample_emit) into a packed buffer of exactly that many floats behind 3 floats that belong to nobody; the last
    cut closes the stream."""
    import torch
    from mbexwn_vocoder_amd import live
    from mbexwn_vocoder_amd.engine import load_library
    from mbexwn_vocoder_amd.resample import device_taps
    lib = load_library()
    dev = torch.device("cuda", torch.cuda.current_device())
    taps, up, down = device_taps(MODEL_RATE, rate, dev)
    n_taps = int(taps.numel())
    half = (n_taps - 1) // 2
    rings = torch.full((1, ring), float("nan"), dtype=torch.float32, device=dev)
    whole = torch.as_tensor(snd).to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    have = produced = 0
    got, ready_before_close = [], []
    assert sum(cuts) == snd.size
    for ii, cc in enumerate(cuts):
        closed = ii == len(cuts) - 1
        # the ring holds every sample a pending output reads: never overwrite one
        assert have + cc - live.input_keep_from(produced, up, down, half, n_taps) <= ring
        desc = torch.as_tensor(np.asarray([[0, have, cc, have]], dtype=np.int64)).to(dev)
        assert lib.mbxl_ring_append(whole.data_ptr(), snd.size, desc.data_ptr(), 1, cc, rings.data_ptr(), 1, ring, stream) == 0
        have += cc
        ready = live.outputs_ready(have, up, down, half, closed)
        if not closed:
            ready_before_close.append(ready)
        new = ready - produced
        if new:
            out = torch.full((new + 3,), float("nan"), dtype=torch.float32, device=dev)
            row = torch.as_tensor(np.asarray([[0, produced, new, have if closed else -1, 3, 0]], dtype=np.int64)).to(dev)
            status = lib.mbxo_resample_emit(rings.data_ptr(), 1, ring, row.data_ptr(), 1, new, up, down, taps.data_ptr(), n_taps,
                                            out.data_ptr(), new + 3, stream)
            assert status == 0, lib.mbx_last_error()
            out = out.cpu().numpy()
            assert np.all(np.isnan(out[:3]))
            got.append(out[3:])
            produced += new
    return np.concatenate(got) if got else np.zeros(0, dtype=np.float32), ready_before_close


@pytest.mark.parametrize("rate", [48000, 44100, 16000, 12345])
def test_output_resampler_equals_the_offline_resampler(rate):
    """Model-rate sounds of 1 sample, of half // up samples (nothing is final before the close) and of three tiles of
    outputs plus one, appended in seeded random cuts with 1-sample cuts among them into a ring only just larger than the
    filter span plus the largest cut (indices wrap many times): the packed outputs of all calls, concatenated, are those of
    resample_device on the whole sound, the last ones with the trailing clip included.  12345 Hz has 69 955 taps: the tap
    table is read from global memory, the other rates stage it in LDS."""
    from mbexwn_vocoder_amd.live import _pow2_at_least
    up, down, half, n_taps = geometry(rate)
    assert (n_taps * 4 > 65536) == (rate == 12345)
    big = 24
    span = (n_taps - 1) // up + 1
    ring = _pow2_at_least(span + big + down // up + 2)
    assert ring < 2 * (span + big + down // up + 2)
    rng = np.random.default_rng(rate)
    long_n = (3 * TILE * down) // up + 1                                  # the shortest sound with 3 * TILE + 1 outputs or more
    assert 3 * TILE + 1 <= -(-long_n * up // down) <= 3 * TILE + 1 + up // down
    for n in (1, half // up, long_n):
        snd = sound(rate + n, n)
        cuts = random_cuts(rng, n, big, forced=(1, 1))
        assert n < 100 or (1 in cuts[2:] and max(cuts) > 6)
        got, early = emit_through_ring(snd, rate, cuts, ring)
        want = offline_at(snd, rate)
        assert got.shape == want.shape == (-(-n * up // down),)
        assert np.array_equal(bits(got), bits(want)), f"{rate} Hz, {n} samples"
        if n <= half // up:
            assert not any(early)                                           # nothing before the close
        else:
            assert n >= 3 * ring                                            # the long sound wraps the ring
            assert early[-1] < want.size                                    # the trailing outputs came with the close


# ---------------------------------------------------------------------------------------------------------------------
# 2. the entry point between guard bands
# ---------------------------------------------------------------------------------------------------------------------
RATE = 44100                                   # up 147, down 80, 6615 taps, half 3307
OUT_FLOATS = 500


def emit_buffers(fill):
    """Two model-rate slots of 256 samples and 500 floats of output.  Slot 0: samples [100, 330) of a running stream (the
    append wraps the ring), of which outputs 300 .. 339 go to out[5:45] (they read samples 141 .. 206).  Slot 1: a closed
    stream of 200 samples, whose 368 outputs (more than one tile) go to out[60:428].  A third row produces nothing."""
    from mbexwn_vocoder_amd.resample import reference_filter, scaled_taps
    taps, up, down = reference_filter(MODEL_RATE, RATE)
    assert (up, down, taps.size) == (147, 80, 6615)
    running, closed = sound(7, 400), sound(8, 200)
    gs = GuardSet(fill, device="cuda")
    return dict(
        gs=gs, running=running, closed=closed,
        rings=gs.new("rings", 2 * 256 * 4),
        packed=gs.put("packed", np.concatenate((closed, running[100:330]))),
        append=gs.put("append desc", np.asarray([[0, 100, 230, 200], [1, 0, 200, 0]], dtype=np.int64)),
        desc=gs.put("emit desc", np.asarray([[0, 300, 40, -1, 5, 0], [0, 0, 0, -1, 50, 0], [1, 0, 368, 200, 60, 0]], dtype=np.int64)),
        taps=gs.put("taps", scaled_taps(taps, up)),
        out=gs.new("out", OUT_FLOATS * 4))


def call_emit(lib, buf, **change):
    import torch
    args = dict(in_rings=buf["rings"].ptr, n_in_slots=2, in_ring_samples=256, desc=buf["desc"].ptr, n_rows=3, max_new_out=368,
                up=147, down=80, taps=buf["taps"].ptr, n_taps=6615, out=buf["out"].ptr, out_floats=OUT_FLOATS)
    args.update(change)
    return lib.mbxo_resample_emit(args["in_rings"], args["n_in_slots"], args["in_ring_samples"], args["desc"], args["n_rows"],
                                  args["max_new_out"], args["up"], args["down"], args["taps"], args["n_taps"], args["out"],
                                  args["out_floats"], torch.cuda.current_stream().cuda_stream)


def append_inputs(lib, buf):
    import torch
    status = lib.mbxl_ring_append(buf["packed"].ptr, 430, buf["append"].ptr, 2, 230, buf["rings"].ptr, 2, 256,
                                  torch.cuda.current_stream().cuda_stream)
    assert status == 0, lib.mbx_last_error()


@pytest.fixture(scope="module")
def offline_pair():
    """resample_device of the two sounds of emit_buffers (computed once)."""
    return offline_at(sound(7, 400), RATE), offline_at(sound(8, 200), RATE)


def expected_out(word, offline_pair):
    want = np.empty(OUT_FLOATS, dtype=np.float32)
    want.view(np.int32)[:] = word
    want[5:45] = offline_pair[0][300:340]
    want[60:428] = offline_pair[1]
    return want


@pytest.mark.parametrize("fill", FILLS)
def test_memory_contract_between_guard_bands(fill, offline_pair):
    """The rings, the descriptors, the taps and `out` between guard bands, every payload of exactly the size the header
    states; two live rows and one with n_out_new = 0.  No guard changes; every word of `out` outside the two named ranges
    keeps its fill; what is written is the offline resampler's output; the ring is not written.  The ring words that were
    never appended hold the fill (NaN, 1e30): no output that is asked for reads them."""
    import torch
    from mbexwn_vocoder_amd.engine import load_library
    lib = load_library()
    buf = emit_buffers(fill)
    assert offline_pair[1].size == 368 > TILE
    append_inputs(lib, buf)
    before = buf["rings"].view(torch.float32, 2, 256).cpu().numpy().copy()
    assert call_emit(lib, buf) == 0, lib.mbx_last_error()
    torch.cuda.synchronize()
    buf["gs"].check()
    out = buf["out"].view(torch.float32).cpu().numpy()
    assert np.array_equal(bits(out), bits(expected_out(fill_word(fill), offline_pair)))
    assert np.array_equal(bits(buf["rings"].view(torch.float32, 2, 256).cpu().numpy()), bits(before))


def test_wrong_descriptors_are_skipped_and_refusals_launch_nothing(offline_pair):
    import torch
    from mbexwn_vocoder_amd.engine import load_library
    lib = load_library()
    buf = emit_buffers("nan")
    append_inputs(lib, buf)
    # every refusal of the header: status 1 and a message, nothing written
    for change in (dict(in_rings=None), dict(desc=None), dict(taps=None), dict(out=None), dict(n_rows=-1), dict(n_rows=65536),
                   dict(max_new_out=-1), dict(up=0), dict(down=0), dict(n_taps=0), dict(n_in_slots=0), dict(in_ring_samples=200),
                   dict(in_ring_samples=0), dict(out_floats=-1)):
        status = call_emit(lib, buf, **change)
        message = lib.mbx_last_error().decode()
        assert status == 1 and message.startswith("resample emit:") and len(message) > 16, (change, status, message)
    torch.cuda.synchronize()
    assert buf["out"].payload_untouched()
    buf["gs"].check()
    # rows that point outside the caller's buffers are skipped, not followed: a bad in_slot, a negative and a huge first_out
    buf["desc"].put(np.asarray([[2, 300, 40, -1, 5, 0], [-1, 300, 40, -1, 5, 0], [0, -5, 40, -1, 5, 0]], dtype=np.int64))
    assert call_emit(lib, buf) == 0
    buf["desc"].put(np.asarray([[0, 2 ** 62, 40, -1, 5, 0], [0, 2 ** 62 // 80, 40, -1, 5, 0], [0, 2 ** 63 - 41, 40, -1, 5, 0]],
                               dtype=np.int64))
    assert call_emit(lib, buf) == 0
    # ... a negative out_offset, and rows that end behind out_floats or start there
    buf["desc"].put(np.asarray([[0, 300, 40, -1, -1, 0], [0, 300, 40, -1, OUT_FLOATS - 39, 0], [0, 300, 40, -1, OUT_FLOATS + 1, 0]],
                               dtype=np.int64))
    assert call_emit(lib, buf) == 0
    buf["desc"].put(np.asarray([[0, 300, 2 ** 62, -1, 5, 0], [0, 300, 40, -1, 2 ** 62, 0], [0, 300, 40, -1, -2 ** 63, 0]],
                               dtype=np.int64))
    assert call_emit(lib, buf) == 0
    # the same rows against an `out` that is said to be shorter than it is: nothing behind what the call was told
    buf["desc"].put(np.asarray([[0, 300, 40, -1, 5, 0], [0, 0, 0, -1, 50, 0], [1, 0, 368, 200, 60, 0]], dtype=np.int64))
    assert call_emit(lib, buf, out_floats=44) == 0 and call_emit(lib, buf, out_floats=0) == 0
    torch.cuda.synchronize()
    assert buf["out"].payload_untouched()
    buf["gs"].check()
    # max_new_out sizes the launch only: with 1, one block per row strides over the 368 outputs of the closed stream
    assert call_emit(lib, buf, max_new_out=1) == 0
    torch.cuda.synchronize()
    buf["gs"].check()
    out = buf["out"].view(torch.float32).cpu().numpy()
    assert np.array_equal(bits(out), bits(expected_out(fill_word("nan"), offline_pair)))
    # a row that ends exactly at out_floats is produced
    buf["out"].refill()
    buf["desc"].put(np.asarray([[0, 300, 40, -1, OUT_FLOATS - 40, 0], [0, 0, -3, -1, 50, 0], [1, 0, 0, 200, 60, 0]], dtype=np.int64))
    assert call_emit(lib, buf) == 0
    torch.cuda.synchronize()
    buf["gs"].check()
    out = buf["out"].view(torch.float32).cpu().numpy()
    assert np.array_equal(bits(out[-40:]), bits(offline_pair[0][300:340])) and np.all(bits(out[:-40]) == fill_word("nan"))


# ---------------------------------------------------------------------------------------------------------------------
# 3. the stage
# ---------------------------------------------------------------------------------------------------------------------
def serve_stage(stage, source, starts, lengths, rates, cuts, join_late, close_when_done):
    """Push every stream's cuts, one push of every stream between two ticks, from the one device tensor `source` (stream
    sid's sound starts at starts[sid]).  Streams in `close_when_done` leave as soon as they are finished (their slots are
    free for a late joiner)."""
    n_streams = len(rates)
    got = {sid: [] for sid in range(n_streams)}
    pos, step = [0] * n_streams, [0] * n_streams
    opened, closed, rounds = set(), set(), 0
    while not (len(opened) == n_streams and all(sid in closed or stage.finished(sid) for sid in got)):
        for sid in range(n_streams):
            if sid in closed or rounds < join_late.get(sid, 0):
                continue
            if sid not in opened:
                stage.open(sid, rates[sid])
                opened.add(sid)
            if step[sid] < len(cuts[sid]):
                cc = cuts[sid][step[sid]]
                stage.push(sid, source, starts[sid] + pos[sid], cc, last=pos[sid] + cc == lengths[sid])
                pos[sid], step[sid] = pos[sid] + cc, step[sid] + 1
        for sid, audio in stage.tick().items():
            assert audio.ndim == 1 and audio.size > 0 and audio.dtype == np.float32
            got[sid].append(audio)
        for sid in close_when_done:
            if sid in opened and sid not in closed and stage.finished(sid):
                stage.close(sid)
                closed.add(sid)
        rounds += 1
        assert rounds < 100000
    return {sid: np.concatenate(vv) for sid, vv in got.items()}


def test_stage_equals_the_offline_resampler():
    """Four streams in one StreamingOutputResampler -- 48 kHz, 44.1 kHz (with a cut longer than the ring the store starts
    with: it grows), 16 kHz, and a second 44.1 kHz stream that joins late into the slot the 16 kHz stream has left -- fed
    from one device tensor in random cuts: every stream is resample_device of its whole sound.  The same pushes again into
    the grown store allocate nothing and give the same bits."""
    import torch
    from mbexwn_vocoder_amd.live import StreamingOutputResampler
    rates = [48000, 44100, 16000, 44100]
    lengths = [1500, 1300, 150, 333]
    starts = [7, 1600, 3000, 3200]
    sounds = [sound(900 + ii, nn) for ii, nn in enumerate(lengths)]
    host = np.full(3600, np.nan, dtype=np.float32)
    for ss, at in zip(sounds, starts):
        host[at:at + ss.size] = ss
    source = torch.as_tensor(host).cuda()
    want = [offline_at(ss, rr) for ss, rr in zip(sounds, rates)]
    stage = StreamingOutputResampler(MODEL_RATE, ring_samples=256, slots=4)
    assert stage.rings is None and stage.ring_samples == 256
    rng = np.random.default_rng(77)
    cuts = [random_cuts(rng, nn, 120, forced=(1, 1)) for nn in lengths]
    cuts[1] = random_cuts(rng, lengths[1], 120, forced=(1, 7, 256 + 200))
    cuts[2] = random_cuts(rng, lengths[2], 120, forced=(1, 1, 100))           # done, and its slot free, before round 60

    def run():
        return serve_stage(stage, source, starts, lengths, rates, cuts, join_late={3: 60}, close_when_done=(2,))

    got = run()
    assert stage.ring_samples > 256 and tuple(stage.rings.shape) == (4, stage.ring_samples)
    for sid in range(4):
        up, down, _, _ = geometry(rates[sid])
        assert got[sid].shape == want[sid].shape == (-(-lengths[sid] * up // down),), sid
        assert np.array_equal(bits(got[sid]), bits(want[sid])), f"stream {sid} at {rates[sid]} Hz"
    assert stage.streams[3].slot == 2 and 2 not in stage.streams          # the late stream sits where the 16 kHz one sat
    before = stage.device_allocations
    assert before > 0
    for sid in (0, 1, 3):
        stage.close(sid)
    again = run()
    assert stage.device_allocations == before
    for sid in range(4):
        assert np.array_equal(bits(again[sid]), bits(want[sid])), f"grown store, stream {sid} at {rates[sid]} Hz"


def test_late_stream_takes_the_released_slot():
    """Host bookkeeping behind the test above: the stream that joins late takes the slot the closed one had, and the samples
    that slot still holds do not reach its output."""
    import torch
    from mbexwn_vocoder_amd.live import StreamingOutputResampler
    stage = StreamingOutputResampler(MODEL_RATE, slots=4)
    first, second = sound(31, 150), sound(32, 333)
    source = torch.as_tensor(np.concatenate((first, second))).cuda()
    stage.open("a", 48000)
    stage.open("b", 16000)
    slot = stage.streams["b"].slot
    stage.push("b", source, 0, 150, last=True)
    got = stage.tick()["b"]
    assert stage.finished("b") and np.array_equal(bits(got), bits(offline_at(first, 16000)))
    stage.close("b")
    stage.open("c", 44100)
    assert stage.streams["c"].slot == slot
    stage.push("c", source, 150, 100)
    stage.push("c", source, 250, 233, last=True)                  # two pushes of one stream between two ticks
    got = stage.tick()["c"]
    assert stage.finished("c") and stage.tick() == {}
    assert np.array_equal(bits(got), bits(offline_at(second, 44100)))


# ---------------------------------------------------------------------------------------------------------------------
# 4. the live pipeline
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    from mbexwn_vocoder_amd.mel_inverter import create_synthetic_model_dir
    return create_synthetic_model_dir(str(tmp_path_factory.mktemp("model") / "speech_small"), "SPEECH", **SMALL)


def test_live_pipeline_gives_its_audio_back_at_the_input_rate(model_dir):
    """0.6 s at 44.1 kHz through a LiveResynthesizer in 80 ms pushes whose transposition changes between pushes, opened with
    output_rate="input": the audio is resample_device(want, None, 24000, 44100), ceil(frames * 300 * 147 / 80) samples, with
    `want` the offline synthesis of test_live_pipeline_at_44k1_equals_the_offline_synthesis (test_gpu_live_resample.py).  A
    second stream of the same resynthesizer with the same input, opened without output_rate, gets `want` itself.  A
    resynthesizer that never sees an output rate leaves the stage's store unallocated."""
    from mbexwn_vocoder_amd.analysis import generate_mels
    from mbexwn_vocoder_amd.live import LiveResynthesizer, frame_factors, output_lookahead_ms
    from mbexwn_vocoder_amd.mel_inverter import MELInverter
    from mbexwn_vocoder_amd.resample import reference_filter
    inv = MELInverter(model_dir, conv_form="f23")
    cfg = inv.preprocess_config
    hop, spf = inv.hop_size, inv.model.dims.steps_per_frame
    rate = 44100
    _, up, down = reference_filter(rate, MODEL_RATE)
    assert (up, down, hop) == (80, 147, 300)
    snd = sound(44, 26460 + 123, rate)
    tick = 3528                                                          # 80 ms at 44.1 kHz
    pushes = [(min(tick, snd.size - start), (1.0, 1.3, 0.8, None)[ii % 4]) for ii, start in enumerate(range(0, snd.size, tick))]
    n_out = -(-snd.size * up // down)
    frames = n_out // hop + 1
    noise = np.random.default_rng(5).normal(size=frames * spf).astype(np.float32)
    live = LiveResynthesizer(inv, chunk_frames=(6, 6, 7, 6, 7))
    assert live.output.rings is None
    assert live.lookahead_ms_for(rate, "input") == live.lookahead_ms_for(rate) + output_lookahead_ms(MODEL_RATE, rate)
    assert 0.93 < live.lookahead_ms_for(None, rate) - live.lookahead_ms < 0.94
    assert live.lookahead_ms_for(None, "input") == live.lookahead_ms_for(None, MODEL_RATE) == live.lookahead_ms
    for sid, rates in ((0, dict(output_rate="input")), (1, dict())):
        live.open(sid, noise_fn=lambda ss, a, b: noise[a * spf:b * spf], sample_rate=rate, **rates)
    got, pos, rounds = {0: [], 1: []}, 0, 0

    def tick_once():
        for sid, audio in live.tick().items():
            got[sid].append(np.array(audio))

    for count, factor in pushes:
        for sid in (0, 1):
            live.push_audio(sid, snd[pos:pos + count], last=pos + count == snd.size, transposition=factor, sample_rate=rate)
        pos += count
        tick_once()
    while not (live.finished(0) and live.finished(1)):
        tick_once()
        rounds += 1
        assert rounds < 1000
    assert live.output.rings is not None and sorted(live.output.streams) == [0]
    per_frame = frame_factors(pushes, hop, up, down)
    mell = generate_mels([snd], [rate], cfg, on_device=True)[0]
    assert mell["mell"].shape[1] == frames
    want = inv.synth_from_mel(inv.scale_mel(mell), noise=noise[None], transposition=per_frame)
    assert want.shape == (frames * hop,)
    plain = np.concatenate(got[1])
    assert plain.shape == want.shape and np.array_equal(bits(plain), bits(want))          # without output_rate: as before
    want_out = offline_at(want, rate)
    audio = np.concatenate(got[0])
    assert audio.shape == want_out.shape == (-(-frames * 300 * 147 // 80),)
    assert np.array_equal(bits(audio), bits(want_out))
    live.close(0)
    live.close(1)
    assert not live.output.streams
    # a resynthesizer that never sees an output rate: "input" on a stream at the model rate is none
    never = LiveResynthesizer(inv, chunk_frames=(6, 6, 7, 6, 7))
    never.open("m", seed=1, output_rate="input")
    never.open("r", seed=2, sample_rate=rate, output_rate=MODEL_RATE)
    never.push_audio("m", sound(3, 2400), last=True)
    never.push_audio("r", snd[:4410], last=True)
    rounds, total = 0, {"m": 0, "r": 0}
    while not (never.finished("m") and never.finished("r")):
        for sid, chunk in never.tick().items():
            total[sid] += chunk.size
        rounds += 1
        assert rounds < 1000
    assert total == {"m": (2400 // hop + 1) * hop, "r": (2400 // hop + 1) * hop}
    assert never.output.rings is None and never.output.device_allocations == 0 and not never.output.streams


def test_replayed_ticks_feed_the_output_stage(model_dir):
    """Two streams at the model rate and 8-frame ticks, which the synthesizer replays as captured graphs once they are
    steady: the chunks the output stage takes from the replayed graph's buffer (48 kHz, 16 kHz) give resample_device of the
    offline synthesis, as the ones of the launch-by-launch ticks do."""
    from mbexwn_vocoder_amd.analysis import generate_mels
    from mbexwn_vocoder_amd.live import LiveResynthesizer
    from mbexwn_vocoder_amd.mel_inverter import MELInverter
    inv = MELInverter(model_dir, conv_form="f23")
    hop, spf = inv.hop_size, inv.model.dims.steps_per_frame
    n = 20 * 8 * hop + 77
    frames = n // hop + 1
    rates = {0: 48000, 1: 16000}
    sounds = {sid: sound(600 + sid, n) for sid in rates}
    noises = {sid: np.random.default_rng(60 + sid).normal(size=frames * spf).astype(np.float32) for sid in rates}
    live = LiveResynthesizer(inv, chunk_frames=8)
    for sid, rate in rates.items():
        live.open(sid, noise_fn=lambda ss, a, b: noises[ss][a * spf:b * spf], output_rate=rate)
    got, replayed, rounds = {0: [], 1: []}, 0, 0
    for start in range(0, n, 8 * hop):
        for sid in rates:
            live.push_audio(sid, sounds[sid][start:start + 8 * hop], last=start + 8 * hop >= n)
        for sid, audio in live.tick().items():
            got[sid].append(np.array(audio))
        replayed += bool(live.synthesizer.last_tick_replayed)
    while not (live.finished(0) and live.finished(1)):
        for sid, audio in live.tick().items():
            got[sid].append(np.array(audio))
        rounds += 1
        assert rounds < 1000
    assert replayed >= 3 and live.synthesizer.graph_ticks >= replayed
    for sid, rate in rates.items():
        mell = generate_mels([sounds[sid]], [MODEL_RATE], inv.preprocess_config, on_device=True)[0]
        want = offline_at(inv.synth_from_mel(inv.scale_mel(mell), noise=noises[sid][None]), rate)
        up, down, _, _ = geometry(rate)
        audio = np.concatenate(got[sid])
        assert audio.shape == want.shape == (-(-frames * hop * up // down),)
        assert np.array_equal(bits(audio), bits(want)), f"stream {sid} at {rate} Hz"


# ---------------------------------------------------------------------------------------------------------------------
# 5. offline: out_rate
# ---------------------------------------------------------------------------------------------------------------------
def test_synth_from_mels_at_an_output_rate(model_dir):
    """synth_from_mels of three ragged items with out_rate=48000 under batch_invariant: each equals resample_device of its
    own synth_from_mel audio; with flac=True, flac_compression="fixed" the bytes are flac.encode(that audio, 48000, "fixed")
    and decode at 48000; out_rate=24000 is no out_rate; synth_from_mel takes the argument too."""
    import torch
    from mbexwn_vocoder_amd import flac
    from mbexwn_vocoder_amd.mel_inverter import MELInverter
    inv = MELInverter(model_dir, batch_invariant=True)
    rng = np.random.default_rng(12)
    mels = [rng.normal(-5, 2, size=(1, int(tt), 80)).astype(np.float32) for tt in (17, 33, 5)]
    torch.manual_seed(5)
    singles = [inv.synth_from_mel(mm) for mm in mels]
    want = [offline_at(aa, 48000) for aa in singles]
    torch.manual_seed(5)
    got = inv.synth_from_mels(mels, max_batch=3, out_rate=48000)
    for gg, ww, mm in zip(got, want, mels):
        assert gg.dtype == np.float32 and gg.shape == ww.shape == (2 * 300 * mm.shape[1],)
        assert np.array_equal(bits(gg), bits(ww))
    torch.manual_seed(5)
    files = inv.synth_from_mels(mels, max_batch=3, flac=True, flac_compression="fixed", out_rate=48000)
    for ff, ww in zip(files, want):
        assert ff == flac.encode(ww, 48000, "fixed")
        pcm, rate = flac.decode(ff)
        assert rate == 48000 and np.array_equal(pcm, flac.to_pcm16(ww))
    torch.manual_seed(5)
    same = inv.synth_from_mels(mels, max_batch=3, out_rate=24000)
    assert all(np.array_equal(bits(ss), bits(aa)) for ss, aa in zip(same, singles))
    torch.manual_seed(5)
    one = inv.synth_from_mel(mels[0], out_rate=48000)
    assert np.array_equal(bits(one), bits(want[0]))
    torch.manual_seed(5)
    assert np.array_equal(bits(inv.synth_from_mel(mels[0], out_rate=24000.0)), bits(singles[0]))
    for bad in (0, -16000, float("nan"), "input"):
        with pytest.raises(ValueError, match="out_rate"):
            inv.synth_from_mel(mels[0], out_rate=bad)


# ---------------------------------------------------------------------------------------------------------------------
# 6. the tools
# ---------------------------------------------------------------------------------------------------------------------
def test_resynth_mel_tool_writes_at_the_output_rate(model_dir, tmp_path):
    """resynth_mel.py --out-rate 16000 --batch 2 --format flac on two small .mell files: each file decodes to rate 16000
    and to the 16-bit samples of resample_device of the file's own model-rate synthesis."""
    import torch
    from mbexwn_vocoder_amd import flac
    from mbexwn_vocoder_amd.audioio import read_audio
    from mbexwn_vocoder_amd.batched import have_soundfile
    from mbexwn_vocoder_amd.fileio import load_var, save_var
    from mbexwn_vocoder_amd.mel_inverter import MELInverter
    files = []
    for ii, frames in enumerate((23, 7)):
        rng = np.random.default_rng(40 + ii)
        files.append(str(tmp_path / f"utt{ii}.mell"))
        save_var(files[-1], {"nfft": 2048, "hoplen": 300, "winlen": 1200, "nmels": 80, "sr": 24000, "fmin": 0.0, "fmax": 12000.0,
                             "lin_spec_offset": 1e-5, "lin_spec_scale": 1, "log_spec_offset": 0.0, "log_spec_scale": 1,
                             "time_axis": 1, "mell": rng.normal(-5, 2, size=(80, frames)).astype(np.float32)})
    out = str(tmp_path / "out")
    res = subprocess.run([sys.executable, RESYNTH_TOOL, model_dir, "-i", *files, "-o", out, "--batch", "2", "--batch-invariant",
                          "--format", "flac", "--out-rate", "16000"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    assert sorted(os.listdir(out)) == ["syn_utt0.flac", "syn_utt1.flac"]
    torch.manual_seed(42)                                          # the tool's default seed, set as the tool sets it
    inv = MELInverter(model_dir, batch_invariant=True)
    for ii, (path, frames) in enumerate(zip(files, (23, 7))):
        want = offline_at(inv.synth_from_mel(inv.scale_mel(load_var(path))), 16000)
        assert want.shape == (frames * 300 * 2 // 3,)
        written = os.path.join(out, f"syn_utt{ii}.flac")
        audio, rate = read_audio(written)
        assert rate == 16000 and audio.shape == want.shape
        if not have_soundfile():                                   # the built-in writer: the device encoder's bytes
            data = open(written, "rb").read()
            pcm, rate = flac.decode(data)
            assert rate == 16000 and np.array_equal(pcm, flac.to_pcm16(want)) and data == flac.encode(want, 16000)


def test_resynth_mel_tool_one_file_at_a_time_at_the_output_rate(model_dir, tmp_path):
    """Without --batch the host writer gets the rate: --out-rate 48000 --format wav writes a 48 kHz file with the float32
    samples of resample_device of the file's model-rate synthesis."""
    import torch
    from scipy.io import wavfile
    from mbexwn_vocoder_amd.batched import have_soundfile
    from mbexwn_vocoder_amd.fileio import load_var, save_var
    from mbexwn_vocoder_amd.mel_inverter import MELInverter
    path = str(tmp_path / "utt.mell")
    save_var(path, {"nfft": 2048, "hoplen": 300, "winlen": 1200, "nmels": 80, "sr": 24000, "fmin": 0.0, "fmax": 12000.0,
                    "lin_spec_offset": 1e-5, "lin_spec_scale": 1, "log_spec_offset": 0.0, "log_spec_scale": 1,
                    "time_axis": 1, "mell": np.random.default_rng(44).normal(-5, 2, size=(80, 9)).astype(np.float32)})
    out = str(tmp_path / "out")
    res = subprocess.run([sys.executable, RESYNTH_TOOL, model_dir, "-i", path, "-o", out, "--format", "wav", "--out-rate", "48000"],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    rate, audio = wavfile.read(os.path.join(out, "syn_utt.wav"))
    torch.manual_seed(42)
    inv = MELInverter(model_dir)
    want = offline_at(inv.synth_from_mel(inv.scale_mel(load_var(path))), 48000)
    assert rate == 48000 and audio.shape == want.shape == (9 * 300 * 2,)
    if not have_soundfile():                                       # scipy's writer keeps the float32 samples as they are
        assert audio.dtype == np.float32 and np.array_equal(bits(audio), bits(want))


def test_stream_transpose_tool_writes_at_the_input_rate(model_dir, tmp_path):
    """stream_transpose.py --resample --output-rate input on a 44.1 kHz wav writes, at 44.1 kHz, the samples its own
    stream_file gives for the same pushes with output_rate="input"."""
    from scipy.io import wavfile
    from mbexwn_vocoder_amd.audioio import read_audio
    from mbexwn_vocoder_amd.live import LiveResynthesizer
    from mbexwn_vocoder_amd.mel_inverter import MELInverter
    snd = sound(901, 4 * 3528 + 333, 44100)
    src, dst = str(tmp_path / "in44.wav"), str(tmp_path / "out" / "out.wav")
    wavfile.write(src, 44100, snd)
    res = subprocess.run([sys.executable, STREAM_TOOL, src, "-o", dst, "--model_id", model_dir, "--transposition", "1.25",
                          "--seed", "3", "--resample", "--output-rate", "input"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    assert "44100 Hz" in res.stderr
    audio, rate = read_audio(dst)
    assert rate == 44100 and wavfile.read(dst)[0] == 44100
    spec = importlib.util.spec_from_file_location("stream_transpose", STREAM_TOOL)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    want = tool.stream_file(LiveResynthesizer(MELInverter(model_dir)), snd, 3528, 1.25, seed=3, sample_rate=44100,
                            output_rate="input")
    n_model = (-(-snd.size * 80 // 147) // 300 + 1) * 300
    assert audio.dtype == np.float32 and audio.shape == want.shape == (-(-n_model * 147 // 80),)
    assert np.array_equal(bits(audio), bits(want))
