"""Live streams at any input rate, on the GPU (mbexwn_vocoder_amd/live.py, csrc/resample_stream.hip through
include/mbexwn_live_resample.h): the streaming resampler against the offline device resampler bit for bit, the analyzer with
resampled streams against the offline tool path (generate_mels) bit for bit, the memory contract of the entry point between
guard bands and its refusals, and the live pipeline and the tool at 44.1 kHz.  Every comparison is on the int32 view."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

from guarded import FILLS, GuardSet, fill_word

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "mbexwn_vocoder_amd", "bin", "stream_transpose.py")
SMALL = {"mbexwn_config:pp_mod_subnet:n_channels": 32, "mbexwn_config:pp_mod_subnet:n_layers": 5}
TINY = {"sample_rate": 24000, "hop_size": 12, "win_size": 48, "fft_size": 64, "mel_channels": 8, "fmin": 0.0, "fmax": None,
        "lin_amp_off": 1e-5, "lin_amp_scale": 1, "mel_amp_scale": 1}
MODEL_RATE = 24000
TILE = 256                                    # outputs per block of resample_stream_kernel


def bits(arr):
    return np.ascontiguousarray(arr, dtype=np.float32).view(np.int32)


def sound(seed, n, rate=MODEL_RATE):
    rng = np.random.default_rng(seed)
    tt = np.arange(n) / float(rate)
    return (0.3 * np.sin(2 * np.pi * 170.0 * tt) + 0.05 * rng.normal(size=n)).astype(np.float32)


def geometry(rate):
    """(up, down, half, n_taps) of the stream filter for rate -> 24 kHz."""
    from mbexwn_vocoder_amd.resample import reference_filter
    taps, up, down = reference_filter(rate, MODEL_RATE)
    return up, down, (taps.size - 1) // 2, int(taps.size)


def input_length(n_out, up, down, exact=True):
    """The shortest input whose resampled length ceil(n * up / down) is n_out (not `exact`: at least n_out; going up in
    rate, not every length occurs)."""
    n = ((n_out - 1) * down) // up + 1
    assert -(-n * up // down) == n_out or (not exact and n_out < -(-n * up // down) <= n_out + up // down)
    return n


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


def offline_resampled(snd, rate):
    import torch
    from mbexwn_vocoder_amd.resample import resample_device
    out, n_out = resample_device(torch.as_tensor(snd[None]).cuda(), None, rate, MODEL_RATE)
    assert int(n_out[0]) == out.shape[1]
    return out[0].cpu().numpy()


def offline_rows(snd, rate, cfg=TINY):
    """The rows of the offline tool path: generate_mels on the whole sound at its own rate."""
    from mbexwn_vocoder_amd.analysis import generate_mels
    return np.ascontiguousarray(generate_mels([snd], [rate], cfg, on_device=True)[0]["mell"].T)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the resampler alone
# ---------------------------------------------------------------------------------------------------------------------
def stream_through_rings(snd, rate, cuts, in_ring, out_ring):
    """Append every cut to a one-slot input ring (mbxl_ring_append), produce every output that became final
    (mbxr_resample_rings) into a one-slot model-rate ring and gather it; the last cut closes the stream."""
    import torch
    from mbexwn_vocoder_amd import live
    from mbexwn_vocoder_amd.engine import load_library
    from mbexwn_vocoder_amd.resample import device_taps
    lib = load_library()
    dev = torch.device("cuda", torch.cuda.current_device())
    taps, up, down = device_taps(rate, MODEL_RATE, dev)
    n_taps = int(taps.numel())
    half = (n_taps - 1) // 2
    in_rings = torch.full((1, in_ring), float("nan"), dtype=torch.float32, device=dev)
    out_rings = torch.full((1, out_ring), float("nan"), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    have = produced = 0
    got, ready_before_close = [], []
    assert sum(cuts) == snd.size
    for ii, cc in enumerate(cuts):
        closed = ii == len(cuts) - 1
        # the ring holds every sample a pending output reads: never overwrite one
        assert have + cc - live.input_keep_from(produced, up, down, half, n_taps) <= in_ring
        packed = torch.as_tensor(snd[have:have + cc]).to(dev)
        desc = torch.as_tensor(np.asarray([[0, have, cc, 0]], dtype=np.int64)).to(dev)
        assert lib.mbxl_ring_append(packed.data_ptr(), cc, desc.data_ptr(), 1, cc, in_rings.data_ptr(), 1, in_ring, stream) == 0
        have += cc
        ready = live.outputs_ready(have, up, down, half, closed)
        if not closed:
            ready_before_close.append(ready)
        while produced < ready:                                 # no more than the out ring holds per call
            new = min(ready - produced, out_ring)
            row = torch.as_tensor(np.asarray([[0, 0, produced, new, have if closed else -1, 0]], dtype=np.int64)).to(dev)
            status = lib.mbxr_resample_rings(in_rings.data_ptr(), 1, in_ring, row.data_ptr(), 1, new, up, down, taps.data_ptr(),
                                             n_taps, out_rings.data_ptr(), 1, out_ring, stream)
            assert status == 0, lib.mbx_last_error()
            idx = (torch.arange(produced, produced + new, device=dev) & (out_ring - 1))
            got.append(out_rings[0, idx].cpu().numpy())
            produced += new
    return np.concatenate(got) if got else np.zeros(0, dtype=np.float32), ready_before_close


@pytest.mark.parametrize("rate", [44100, 48000, 16000, 12345])
def test_streaming_resampler_equals_the_offline_resampler(rate):
    """Sounds of 1 sample, of half // up samples (nothing is final before the close) and of three tiles of outputs plus
    one, pushed in seeded random cuts with 1-sample pushes among them into an input ring only just larger than the filter
    span (indices wrap many times), out of a model-rate ring of one tile (wraps too): the gathered outputs are those of
    resample_device on the whole sound, the last ones with the trailing clip included.  12345 Hz has 72 000 taps: the tap
    table is read from global memory, the other rates stage it in LDS."""
    from mbexwn_vocoder_amd.live import _pow2_at_least
    up, down, half, n_taps = geometry(rate)
    assert (n_taps * 4 > 64 * 1024) == (rate == 12345)
    big = 24
    span = (n_taps - 1) // up + 1
    in_ring = _pow2_at_least(span + big + down // up + 2)
    assert in_ring < 2 * (span + big + down // up + 2)
    rng = np.random.default_rng(rate)
    for n in (1, half // up, input_length(3 * TILE + 1, up, down, exact=False)):
        snd = sound(rate + n, n, rate)
        cuts = random_cuts(rng, n, big, forced=(1, 1))
        assert n < 100 or (1 in cuts[2:] and max(cuts) > 6)
        got, early = stream_through_rings(snd, rate, cuts, in_ring, TILE)
        want = offline_resampled(snd, rate)
        assert got.shape == want.shape == (-(-n * up // down),)
        assert np.array_equal(bits(got), bits(want)), f"{rate} Hz, {n} samples"
        if n <= half // up:
            assert not any(early)                               # nothing before the close
        else:
            assert n >= 3 * in_ring                             # the long sound wraps the input ring (11 times at 44.1 kHz)
            assert early[-1] < want.size                        # the trailing outputs came with the close


# ---------------------------------------------------------------------------------------------------------------------
# 2. and 3. the analyzer with resampled streams
# ---------------------------------------------------------------------------------------------------------------------
def serve(an, sounds, rates, cuts, join_late=None, close_when_done=()):
    """Push every sound in its cuts, one push of every stream between two ticks; a stream with a rate is opened at it.
    Streams in `close_when_done` leave as soon as they are finished (their slots are free for a late joiner)."""
    got = {sid: [] for sid in range(len(sounds))}
    pos = {sid: 0 for sid in got}
    step = {sid: 0 for sid in got}
    opened, closed, rounds = set(), set(), 0
    while not (len(opened) == len(sounds) and all(sid in closed or an.finished(sid) for sid in got)):
        for sid, ss in enumerate(sounds):
            if sid in closed or (join_late and rounds < join_late.get(sid, 0)):
                continue
            if sid not in opened:
                if rates[sid] is None:
                    an.open(sid)
                else:
                    an.open(sid, sample_rate=rates[sid])
                opened.add(sid)
            if step[sid] < len(cuts[sid]):
                end = pos[sid] + cuts[sid][step[sid]]
                an.push(sid, ss[pos[sid]:end], last=end == ss.size, sample_rate=rates[sid])
                pos[sid], step[sid] = end, step[sid] + 1
        for sid, rows in an.tick().items():
            assert rows.ndim == 2 and rows.shape[0] > 0 and rows.dtype == np.float32
            got[sid].append(rows)
        for sid in close_when_done:
            if sid in opened and sid not in closed and an.finished(sid):
                an.close(sid)
                closed.add(sid)
        rounds += 1
        assert rounds < 100000
    return {sid: np.concatenate(vv) for sid, vv in got.items()}


def test_push_cuts_do_not_change_a_bit():
    """A 44.1 kHz sound as one push, as pushes of one sample and in random cuts: the same rows, those of generate_mels."""
    from mbexwn_vocoder_amd.live import StreamingAnalyzer
    rate = 44100
    snd = sound(21, 700, rate)
    want = offline_rows(snd, rate)
    rng = np.random.default_rng(3)
    for cuts in ([snd.size], [1] * snd.size, random_cuts(rng, snd.size, 60)):
        got = serve(StreamingAnalyzer(TINY), [snd], [rate], [cuts])[0]
        assert got.shape == want.shape == (-(-snd.size * 80 // 147) // 12 + 1, 8)
        assert np.array_equal(bits(got), bits(want)), f"{len(cuts)} pushes"


def test_analyzer_equals_the_offline_tool_path():
    """Five streams in one analyzer -- 44.1 kHz (487 = 40 hops + 7 resampled samples, with a push longer than the input ring
    and the model-rate ring it starts with: both stores grow), 48 kHz (25 = win / 2 + 1), 16 kHz (23 = win / 2 - 1), one at
    the model rate opened without a sample_rate (36 = 3 hops), and a second 44.1 kHz stream of one resampled sample that
    joins late into the slots the 48 kHz stream has left: every stream's rows are those of generate_mels on its whole sound
    at its own rate.  The same pushes again into the grown stores allocate nothing and give the same bits, and the
    model-rate stream's rows are those of an analyzer that has no resampled stream at all."""
    from mbexwn_vocoder_amd.live import StreamingAnalyzer
    win, hop = 48, 12
    rates = [44100, 48000, 16000, None, 44100]
    targets = [40 * hop + 7, win // 2 + 1, win // 2 - 1, 3 * hop, 1]
    lengths = [nn if rr is None else input_length(nn, *geometry(rr)[:2]) for nn, rr in zip(targets, rates)]
    sounds = [sound(500 + ii, nn, rr or MODEL_RATE) for ii, (nn, rr) in enumerate(zip(lengths, rates))]
    want = [offline_rows(ss, rr or MODEL_RATE) for ss, rr in zip(sounds, rates)]
    for ww, nn in zip(want, targets):
        assert ww.shape == (nn // hop + 1, 8)
    an = StreamingAnalyzer(TINY, ring_samples=win, slots=4, input_ring_samples=128)
    ring0, in_ring0 = an.ring_samples, an.input_ring_samples
    rng = np.random.default_rng(2025)
    cuts = [random_cuts(rng, nn, 30) for nn in lengths]
    cuts[0] = random_cuts(rng, lengths[0], 30, forced=(1, 1, 7, in_ring0 + 200))
    assert (in_ring0 + 200) * 80 // 147 > ring0

    def run():
        return serve(an, sounds, rates, cuts, join_late={4: 60}, close_when_done=(1,))

    got = run()
    assert an.ring_samples > ring0 and an.input_ring_samples > in_ring0
    assert an.streams[4].slot is not None and an.streams[4].rate == 44100 and an.streams[3].rate is None
    for sid in range(5):
        assert got[sid].shape == want[sid].shape, sid
        assert np.array_equal(bits(got[sid]), bits(want[sid])), f"stream {sid} at {rates[sid]} Hz"
    before = an.device_allocations
    for sid in (0, 2, 3, 4):
        an.close(sid)
    again = run()
    assert an.device_allocations == before
    for sid in range(5):
        assert np.array_equal(bits(again[sid]), bits(want[sid])), f"grown stores, stream {sid} at {rates[sid]} Hz"
    plain = StreamingAnalyzer(TINY, ring_samples=win, slots=4)
    alone = serve(plain, [sounds[3]], [None], [cuts[3]])[0]
    assert plain.input_rings is None and np.array_equal(bits(alone), bits(got[3]))


def test_late_stream_reuses_both_slots():
    """Host bookkeeping behind the test above: the late 44.1 kHz stream takes the slots the closed 48 kHz stream had."""
    from mbexwn_vocoder_amd.live import StreamingAnalyzer
    an = StreamingAnalyzer(TINY, slots=4)
    an.open("a", sample_rate=44100)
    an.open("b", sample_rate=48000)
    slots = (an.streams["b"].slot, an.streams["b"].in_slot)
    an.push("b", sound(1, 49, 48000), last=True)
    while not an.finished("b"):
        an.tick()
    an.close("b")
    an.open("c", sample_rate=44100)
    assert (an.streams["c"].slot, an.streams["c"].in_slot) == slots
    snd = sound(2, 300, 44100)
    an.push("c", snd, last=True)
    rows = []
    while not an.finished("c"):
        rows.append(an.tick()["c"])
    assert np.array_equal(bits(np.concatenate(rows)), bits(offline_rows(snd, 44100)))


# ---------------------------------------------------------------------------------------------------------------------
# 4. the entry point between guard bands
# ---------------------------------------------------------------------------------------------------------------------
RATE = 44100                                   # up 80, down 147, 6480 taps, half 3239


def resample_buffers(fill):
    """Two input slots of 256 samples, three model-rate slots of 64.  Input slot 0: samples [100, 330) of a running stream
    (the append wraps the ring), of which outputs 100 .. 139 are produced into model-rate slot 0 (they wrap its ring).
    Input slot 1: a closed stream of 60 samples, whose 33 outputs go to model-rate slot 2.  A third row produces nothing;
    model-rate slot 1 belongs to nobody."""
    from mbexwn_vocoder_amd.resample import reference_filter, scaled_taps
    taps, up, down = reference_filter(RATE, MODEL_RATE)
    assert (up, down, taps.size) == (80, 147, 6480)
    running, closed = sound(7, 400, RATE), sound(8, 60, RATE)
    gs = GuardSet(fill, device="cuda")
    return dict(
        gs=gs, running=running, closed=closed,
        in_rings=gs.new("in rings", 2 * 256 * 4),
        packed=gs.put("packed", np.concatenate((closed, running[100:330]))),
        append=gs.put("append desc", np.asarray([[0, 100, 230, 60], [1, 0, 60, 0]], dtype=np.int64)),
        desc=gs.put("resample desc", np.asarray([[0, 0, 100, 40, -1, 0], [0, 1, 0, 0, -1, 0], [1, 2, 0, 33, 60, 0]], dtype=np.int64)),
        taps=gs.put("taps", scaled_taps(taps, up)),
        out_rings=gs.new("out rings", 3 * 64 * 4))


def call_resample(lib, buf, **change):
    import torch
    args = dict(in_rings=buf["in_rings"].ptr, n_in_slots=2, in_ring_samples=256, desc=buf["desc"].ptr, n_rows=3, max_new_out=40,
                up=80, down=147, taps=buf["taps"].ptr, n_taps=6480, out_rings=buf["out_rings"].ptr, n_out_slots=3,
                out_ring_samples=64)
    args.update(change)
    return lib.mbxr_resample_rings(args["in_rings"], args["n_in_slots"], args["in_ring_samples"], args["desc"], args["n_rows"],
                                   args["max_new_out"], args["up"], args["down"], args["taps"], args["n_taps"],
                                   args["out_rings"], args["n_out_slots"], args["out_ring_samples"],
                                   torch.cuda.current_stream().cuda_stream)


def append_inputs(lib, buf):
    import torch
    status = lib.mbxl_ring_append(buf["packed"].ptr, 290, buf["append"].ptr, 2, 230, buf["in_rings"].ptr, 2, 256,
                                  torch.cuda.current_stream().cuda_stream)
    assert status == 0, lib.mbx_last_error()


@pytest.fixture(scope="module")
def offline_pair():
    """resample_device of the two sounds of resample_buffers (computed once)."""
    return offline_resampled(sound(7, 400, RATE), RATE), offline_resampled(sound(8, 60, RATE), RATE)


@pytest.mark.parametrize("fill", FILLS)
def test_memory_contract_between_guard_bands(fill, offline_pair):
    """Both ring stores, the descriptors, the taps and the packed samples between guard bands, every payload of exactly the
    size the header states.  No guard changes; every word of the model-rate rings other than the named outputs keeps its
    fill; what is written is the offline resampler's output.  The input ring words that were never appended hold the fill
    (NaN, 1e30): no output that is asked for reads them."""
    import torch
    from mbexwn_vocoder_amd.engine import load_library
    lib = load_library()
    buf = resample_buffers(fill)
    word = fill_word(fill)
    want_running, want_closed = offline_pair
    assert want_closed.size == 33
    append_inputs(lib, buf)
    before = buf["in_rings"].view(torch.float32, 2, 256).cpu().numpy().copy()
    assert call_resample(lib, buf) == 0, lib.mbx_last_error()
    torch.cuda.synchronize()
    buf["gs"].check()
    out = buf["out_rings"].view(torch.float32, 3, 64).cpu().numpy()
    want0 = np.empty(64, dtype=np.float32)
    want0.view(np.int32)[:] = word
    ks = np.arange(100, 140)
    want0[ks & 63] = want_running[ks]
    assert np.array_equal(bits(out[0]), bits(want0))                    # wrapped; the other 24 words keep the fill
    assert np.all(bits(out[1]) == word)
    assert np.array_equal(bits(out[2, :33]), bits(want_closed)) and np.all(bits(out[2, 33:]) == word)
    # the inputs are inputs
    assert np.array_equal(bits(buf["in_rings"].view(torch.float32, 2, 256).cpu().numpy()), bits(before))


def test_wrong_descriptors_are_skipped_and_refusals_launch_nothing(offline_pair):
    import torch
    from mbexwn_vocoder_amd.engine import load_library
    lib = load_library()
    buf = resample_buffers("nan")
    append_inputs(lib, buf)
    # every refusal of the header: status 1 and a message, nothing written
    for change in (dict(in_rings=None), dict(desc=None), dict(taps=None), dict(out_rings=None), dict(n_rows=-1),
                   dict(n_rows=65536), dict(max_new_out=-1), dict(up=0), dict(down=0), dict(n_taps=0), dict(n_in_slots=0),
                   dict(n_out_slots=0), dict(in_ring_samples=200), dict(in_ring_samples=0), dict(out_ring_samples=48),
                   dict(out_ring_samples=0)):
        status = call_resample(lib, buf, **change)
        message = lib.mbx_last_error().decode()
        assert status == 1 and message.startswith("resample rings:") and len(message) > 17, (change, status, message)
    torch.cuda.synchronize()
    assert buf["out_rings"].payload_untouched()
    buf["gs"].check()
    # rows that point outside the caller's buffers are skipped, not followed
    buf["desc"].put(np.asarray([[2, 0, 100, 40, -1, 0], [0, 3, 100, 40, -1, 0], [-1, 0, 100, 40, -1, 0]], dtype=np.int64))
    assert call_resample(lib, buf) == 0
    buf["desc"].put(np.asarray([[0, -1, 100, 40, -1, 0], [0, 0, -5, 40, -1, 0], [0, 0, 2 ** 62, 40, -1, 0]], dtype=np.int64))
    assert call_resample(lib, buf) == 0
    torch.cuda.synchronize()
    assert buf["out_rings"].payload_untouched()
    buf["gs"].check()
    # n_out_new beyond the ring is clipped to the ring: outputs 90 .. 153 of the running stream (all final with 330 samples,
    # none reads in front of sample 100), each written once, nothing else; max_new_out sizes the launch only
    buf["desc"].put(np.asarray([[0, 0, 90, 1000, -1, 0], [0, 1, 0, -3, -1, 0], [1, 2, 0, 0, 60, 0]], dtype=np.int64))
    assert call_resample(lib, buf, max_new_out=1) == 0
    torch.cuda.synchronize()
    buf["gs"].check()
    out = buf["out_rings"].view(torch.float32, 3, 64).cpu().numpy()
    ks = np.arange(90, 154)
    want0 = np.empty(64, dtype=np.float32)
    want0[ks & 63] = offline_pair[0][ks]
    assert np.array_equal(bits(out[0]), bits(want0))
    assert np.all(bits(out[1:]) == fill_word("nan"))


# ---------------------------------------------------------------------------------------------------------------------
# 5. audio in at 44.1 kHz, audio out
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    from mbexwn_vocoder_amd.mel_inverter import create_synthetic_model_dir
    return create_synthetic_model_dir(str(tmp_path_factory.mktemp("model") / "speech_small"), "SPEECH", **SMALL)


def test_live_pipeline_at_44k1_equals_the_offline_synthesis(model_dir):
    """0.6 s at 44.1 kHz through a LiveResynthesizer in 80 ms pushes whose transposition changes between pushes: the audio is
    synth_from_mel of the scale_mel-scaled generate_mels of the whole sound, with the same noise and the per-frame factors
    of frame_factors(pushes, hop, up, down), on an engine pinned to f23."""
    from mbexwn_vocoder_amd.analysis import generate_mels
    from mbexwn_vocoder_amd.live import LiveResynthesizer, frame_factors
    from mbexwn_vocoder_amd.mel_inverter import MELInverter
    inv = MELInverter(model_dir, conv_form="f23")
    cfg = inv.preprocess_config
    hop, spf = inv.hop_size, inv.model.dims.steps_per_frame
    rate, (up, down, half, _) = 44100, geometry(44100)
    snd = sound(44, 26460 + 123, rate)
    tick = 3528                                                          # 80 ms at 44.1 kHz
    pushes = [(min(tick, snd.size - start), (1.0, 1.3, 0.8, None)[ii % 4]) for ii, start in enumerate(range(0, snd.size, tick))]
    n_out = -(-snd.size * up // down)
    frames = n_out // hop + 1
    noise = np.random.default_rng(5).normal(size=frames * spf).astype(np.float32)
    live = LiveResynthesizer(inv, chunk_frames=(6, 6, 7, 6, 7))
    assert abs(live.lookahead_ms_for(rate) - (live.lookahead_ms + 1000.0 * half / up / rate)) < 1e-9
    assert 0.9 < live.lookahead_ms_for(rate) - live.lookahead_ms < 0.95
    assert live.lookahead_ms_for(None) == live.lookahead_ms_for(24000) == live.lookahead_ms
    live.open(0, noise_fn=lambda ss, a, b: noise[a * spf:b * spf], sample_rate=rate)
    got, pos, rounds = [], 0, 0
    for count, factor in pushes:
        live.push_audio(0, snd[pos:pos + count], last=pos + count == snd.size, transposition=factor, sample_rate=rate)
        pos += count
        got += [np.array(aa) for aa in [live.tick().get(0)] if aa is not None]
    while not live.finished(0):
        got += [np.array(aa) for aa in [live.tick().get(0)] if aa is not None]
        rounds += 1
        assert rounds < 1000
    per_frame = frame_factors(pushes, hop, up, down)
    assert per_frame.shape == (frames,) and len(set(per_frame.tolist())) == 3
    mell = generate_mels([snd], [rate], cfg, on_device=True)[0]
    assert mell["mell"].shape[1] == frames
    want = inv.synth_from_mel(inv.scale_mel(mell), noise=noise[None], transposition=per_frame)
    audio = np.concatenate(got)
    assert audio.shape == want.shape == (frames * hop,)
    assert np.array_equal(bits(audio), bits(want))


def test_stream_transpose_tool_resamples(model_dir, tmp_path):
    """stream_transpose.py --resample on a 44.1 kHz wav writes, at 24 kHz, the samples its own stream_file gives for the same
    pushes at the file's rate."""
    from scipy.io import wavfile
    from mbexwn_vocoder_amd.audioio import read_audio
    from mbexwn_vocoder_amd.live import LiveResynthesizer
    from mbexwn_vocoder_amd.mel_inverter import MELInverter
    snd = sound(901, 4 * 3528 + 333, 44100)
    src, dst = str(tmp_path / "in44.wav"), str(tmp_path / "out" / "out.wav")
    wavfile.write(src, 44100, snd)
    res = subprocess.run([sys.executable, TOOL, src, "-o", dst, "--model_id", model_dir, "--transposition", "1.25", "--seed", "3",
                          "--resample"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    audio, rate = read_audio(dst)
    assert rate == 24000 and wavfile.read(dst)[0] == 24000
    spec = importlib.util.spec_from_file_location("stream_transpose", TOOL)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    want = tool.stream_file(LiveResynthesizer(MELInverter(model_dir)), snd, 3528, 1.25, seed=3, sample_rate=44100)
    n_out = -(-snd.size * 80 // 147)
    assert audio.dtype == np.float32 and audio.shape == want.shape == ((n_out // 300 + 1) * 300,)
    assert np.array_equal(bits(audio), bits(want))
