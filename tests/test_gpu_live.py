"""Live streams on the GPU (mbexwn_vocoder_amd/live.py, csrc/mel_stream.hip through include/mbexwn_live.h): the streaming
analysis against the offline device analysis bit for bit, its memory contract between guard bands and its refusals; the
live pipeline (analysis -> scale_mel -> streaming synthesis) against the offline synthesis bit for bit; the tool."""
import ctypes
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

from guarded import FILLS, GuardSet, fill_word
from helpers import build_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "mbexwn_vocoder_amd", "bin", "stream_transpose.py")
SMALL = {"mbexwn_config:pp_mod_subnet:n_channels": 32, "mbexwn_config:pp_mod_subnet:n_layers": 5}
TINY = {"sample_rate": 24000, "hop_size": 12, "win_size": 48, "fft_size": 64, "mel_channels": 8, "fmin": 0.0, "fmax": None,
        "lin_amp_off": 1e-5, "lin_amp_scale": 1, "mel_amp_scale": 1}
EPS = ctypes.c_float(float(np.finfo(np.float32).eps))


def preprocess(name):
    return TINY if name == "tiny" else build_case("SPEECH", {})[0]["preprocess_config"]


def geometry(cfg):
    return int(cfg.get("win_size", cfg["fft_size"])), int(cfg["hop_size"])


def sound(seed, n):
    rng = np.random.default_rng(seed)
    tt = np.arange(n) / 24000.0
    return (0.3 * np.sin(2 * np.pi * 170.0 * tt) + 0.05 * rng.normal(size=n)).astype(np.float32)


def offline_rows(cfg, sounds):
    """compute_log_mel_device of every sound (one ragged launch), trimmed to its n // hop + 1 rows."""
    import torch
    from mbexwn_vocoder_amd.analysis import compute_log_mel_device
    win, hop = geometry(cfg)
    lengths = [ss.size for ss in sounds]
    host = np.zeros((len(sounds), max(max(lengths), win // 2 + 1)), dtype=np.float32)
    for bb, ss in enumerate(sounds):
        host[bb, :ss.size] = ss
    mel, _ = compute_log_mel_device(torch.as_tensor(host).cuda(), cfg, n_samples=torch.as_tensor(lengths, dtype=torch.int32).cuda())
    mel = mel.cpu().numpy()
    return [mel[bb, :nn // hop + 1].copy() for bb, nn in enumerate(lengths)]


def serve(an, sounds, cuts, join_late=None, pushes_per_tick=1):
    """Push every sound in its cuts (a list of push sizes that sums to its length), `pushes_per_tick` pushes of every stream
    between two ticks; returns the concatenated rows per stream."""
    got = {sid: [] for sid in range(len(sounds))}
    pos = {sid: 0 for sid in got}
    step = {sid: 0 for sid in got}
    opened = set()
    rounds = 0
    while not (len(opened) == len(sounds) and all(an.finished(sid) for sid in got)):
        for sid, ss in enumerate(sounds):
            if join_late and rounds < join_late.get(sid, 0):
                continue
            if sid not in opened:
                an.open(sid)
                opened.add(sid)
            for _ in range(pushes_per_tick):
                if step[sid] < len(cuts[sid]):
                    end = pos[sid] + cuts[sid][step[sid]]
                    an.push(sid, ss[pos[sid]:end], last=end == ss.size)
                    pos[sid], step[sid] = end, step[sid] + 1
        for sid, rows in an.tick().items():
            assert rows.ndim == 2 and rows.shape[0] > 0 and rows.dtype == np.float32
            got[sid].append(rows)
        rounds += 1
        assert rounds < 100000
    return {sid: np.concatenate(vv) for sid, vv in got.items()}


def random_cuts(rng, n, hop, forced=()):
    """Push sizes that sum to n: the forced ones first (as far as they fit), then pushes of 1 sample, of less than a hop and
    of up to three hops, drawn at random."""
    cuts, left = [], n
    for cc in forced:
        cc = min(cc, left)
        if cc:
            cuts.append(cc)
            left -= cc
    while left:
        kind = int(rng.integers(0, 3))
        cc = 1 if kind == 0 else int(rng.integers(2, hop + 1)) if kind == 1 else int(rng.integers(hop, 3 * hop + 1))
        cc = min(cc, left)
        cuts.append(cc)
        left -= cc
    return cuts


def five_lengths(cfg):
    win, hop = geometry(cfg)
    return [1, win // 2 - 1, win // 2 + 1, 3 * hop, 40 * hop + 7]


@pytest.fixture(scope="module", params=["speech", "tiny"])
def case(request):
    """The five sounds of a configuration and their offline rows (computed once)."""
    from mbexwn_vocoder_amd.analysis import compute_log_mel
    cfg = preprocess(request.param)
    win, hop = geometry(cfg)
    sounds = [sound(100 + ii, nn) for ii, nn in enumerate(five_lengths(cfg))]
    for ss in sounds:                                   # the host analysis agrees on the row count of every length used
        assert compute_log_mel(ss[None], cfg)[0].shape == (1, ss.size // hop + 1, cfg["mel_channels"])
    return cfg, sounds, offline_rows(cfg, sounds)


def test_analyzer_equals_the_offline_analysis(case):
    """Five streams (1 sample; win / 2 - 1: folded more than once at the end; win / 2 + 1; exactly 3 hops; 40 hops + 7) in
    pushes cut at random from a fixed seed -- among them pushes of 1 sample and one longer than the ring the analyzer starts
    with (the rings grow) -- with the fifth stream opened after the others have started, into a store of 4 slots (the slots
    grow): every stream's rows are the offline rows, bit for bit.  Then both kinds of growth in one tick: a fifth stream's
    first push and six windows for a stream that has samples on the device."""
    from mbexwn_vocoder_amd.live import StreamingAnalyzer
    cfg, sounds, want = case
    win, hop = geometry(cfg)
    an = StreamingAnalyzer(cfg, ring_samples=win, slots=4)
    ring0 = an.ring_samples
    assert ring0 < sounds[4].size - 2
    rng = np.random.default_rng(2024)
    cuts = [random_cuts(rng, ss.size, hop) for ss in sounds]
    cuts[4] = random_cuts(rng, sounds[4].size, hop, forced=(1, 1, hop, ring0 + 5))
    cuts[3] = random_cuts(rng, sounds[3].size, hop, forced=(1, hop - 1))
    # the long stream first, the 3-hop stream last and late: it takes the fifth slot while the long one is in flight
    order = [4, 0, 1, 2, 3]
    got = serve(an, [sounds[ii] for ii in order], [cuts[ii] for ii in order], join_late={4: 6})
    assert an.ring_samples > ring0 and an.rings.shape[0] == 8
    for pos, ii in enumerate(order):
        assert got[pos].shape == want[ii].shape == (sounds[ii].size // hop + 1, cfg["mel_channels"])
        assert np.array_equal(got[pos].view(np.int32), want[ii].view(np.int32)), f"stream of {sounds[ii].size} samples"
    # a steady tick allocates nothing: the same pushes again into the grown stores
    before = an.device_allocations
    for sid in range(5):
        an.close(sid)
    again = serve(an, [sounds[ii] for ii in order], [cuts[ii] for ii in order], join_late={4: 6})
    assert an.device_allocations == before
    for pos, ii in enumerate(order):
        assert np.array_equal(again[pos].view(np.int32), want[ii].view(np.int32)), f"reused slot, {sounds[ii].size} samples"
    # one tick in which the store both gains slots and lengthens its rings: four streams have samples on the device (the
    # long one a hop of them, which has to move), then a fifth opens and the long one gets six windows at once
    an = StreamingAnalyzer(cfg, ring_samples=win, slots=4)
    got = {sid: [] for sid in range(5)}

    def tick():
        for sid, rows in an.tick().items():
            got[sid].append(rows)

    long_one = sounds[4]
    assert long_one.size > hop + 6 * win > ring0
    for sid, ii in enumerate(order[:4]):
        an.open(sid)
        an.push(sid, sounds[ii][:hop] if ii == 4 else sounds[ii], last=ii != 4)
    tick()
    assert tuple(an.rings.shape) == (4, ring0) and an.streams[0].on_device == hop
    an.open(4)
    an.push(4, sounds[order[4]], last=True)
    an.push(0, long_one[hop:hop + 6 * win])
    tick()
    assert an.rings.shape[0] == 8 and an.ring_samples > ring0 and an.rings.shape[1] == an.ring_samples
    an.push(0, long_one[hop + 6 * win:], last=True)
    tick()
    assert all(an.finished(sid) for sid in range(5))
    for sid, ii in enumerate(order):
        rows = np.concatenate(got[sid])
        assert np.array_equal(rows.view(np.int32), want[ii].view(np.int32)), f"slots and rings grow at once, {sounds[ii].size} samples"


def test_push_cuts_do_not_change_a_bit(case):
    """Each sound as one push and as pushes of one sample give the same bits (and the offline rows)."""
    from mbexwn_vocoder_amd.live import StreamingAnalyzer
    cfg, sounds, want = case
    per_tick = 1 if cfg is TINY else 211
    whole = serve(StreamingAnalyzer(cfg), sounds, [[ss.size] for ss in sounds])
    single = serve(StreamingAnalyzer(cfg), sounds, [[1] * ss.size for ss in sounds], pushes_per_tick=per_tick)
    for sid in range(len(sounds)):
        assert np.array_equal(whole[sid].view(np.int32), single[sid].view(np.int32))
        assert np.array_equal(whole[sid].view(np.int32), want[sid].view(np.int32))


# ---------------------------------------------------------------------------------------------------------------------
# the two entry points between guard bands
# ---------------------------------------------------------------------------------------------------------------------
def live_buffers(fill):
    """Three slots of 64 samples at the tiny configuration.  Slot 0: samples [40, 100) of a running stream (the append wraps
    the ring; ring words 36 .. 39 are not written), frame 6 of it (samples [48, 96)).  Slot 2: a stream with nothing to
    append and no frame.  Slot 1: a closed stream of 60 samples, frames 0 .. 5.  max_new_frames = 7."""
    from mbexwn_vocoder_amd.analysis import mel_analysis_tables
    running, closed = sound(7, 200), sound(8, 60)
    gs = GuardSet(fill, device="cuda")
    packed = np.concatenate((closed, running[40:100]))
    buf = dict(
        gs=gs, running=running, closed=closed,
        rings=gs.new("rings", 3 * 64 * 4),
        packed=gs.put("packed", packed),
        append=gs.put("append desc", np.asarray([[0, 40, 60, 60], [2, 0, 0, 0], [1, 0, 60, 0]], dtype=np.int64)),
        frames=gs.put("frame desc", np.asarray([[0, 6, 1, -1], [2, 0, 0, -1], [1, 0, 6, 60]], dtype=np.int64)),
        tables=[gs.put(f"table {ii}", tt) for ii, tt in enumerate(mel_analysis_tables(TINY))],
        out=gs.new("out", 3 * 7 * 8 * 4))
    return buf


def call_append(lib, buf, **change):
    import torch
    args = dict(packed=buf["packed"].ptr, packed_samples=120, desc=buf["append"].ptr, n_streams=3, max_count=60,
                rings=buf["rings"].ptr, n_slots=3, ring_samples=64)
    args.update(change)
    return lib.mbxl_ring_append(args["packed"], args["packed_samples"], args["desc"], args["n_streams"], args["max_count"],
                                args["rings"], args["n_slots"], args["ring_samples"], torch.cuda.current_stream().cuda_stream)


def call_frames(lib, buf, **change):
    import torch
    tabs = buf["tables"]
    args = dict(rings=buf["rings"].ptr, n_slots=3, ring_samples=64, desc=buf["frames"].ptr, n_streams=3, max_new_frames=7,
                win=48, hop=12, fft_size=64, n_mels=8, window=tabs[0].ptr, twiddle=tabs[1].ptr, basis=tabs[2].ptr,
                bin_lo=tabs[3].ptr, bin_hi=tabs[4].ptr, out=buf["out"].ptr)
    args.update(change)
    return lib.mbxl_mel_frames(args["rings"], args["n_slots"], args["ring_samples"], args["desc"], args["n_streams"],
                               args["max_new_frames"], args["win"], args["hop"], args["fft_size"], args["n_mels"],
                               args["window"], args["twiddle"], args["basis"], args["bin_lo"], args["bin_hi"], EPS, args["out"],
                               torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("fill", FILLS)
def test_memory_contract_between_guard_bands(fill):
    """Rings, packed samples, both descriptor tables, the analysis tables and the output between guard bands, one call of
    each entry point.  No guard changes; ring words outside the appended ranges and output rows beyond a stream's n_frames
    keep the fill; what is written is the offline analysis."""
    import torch
    from mbexwn_vocoder_amd.engine import load_library
    lib = load_library()
    buf = live_buffers(fill)
    word = fill_word(fill)
    assert call_append(lib, buf) == 0, lib.mbx_last_error()
    torch.cuda.synchronize()
    buf["gs"].check()
    rings = buf["rings"].view(torch.float32, 3, 64).cpu().numpy()
    want0 = np.empty(64, dtype=np.float32)
    want0.view(np.int32)[:] = word
    idx = np.arange(40, 100)
    want0[idx & 63] = buf["running"][idx]
    assert np.array_equal(rings[0].view(np.int32), want0.view(np.int32))             # wrapped; words 36 .. 39 keep the fill
    assert np.all(rings[0, 36:40].view(np.int32) == word)
    assert np.array_equal(rings[1, :60], buf["closed"]) and np.all(rings[1, 60:].view(np.int32) == word)
    assert np.all(rings[2].view(np.int32) == word)                                    # count = 0 writes nothing
    assert call_frames(lib, buf) == 0, lib.mbx_last_error()
    torch.cuda.synchronize()
    buf["gs"].check()
    out = buf["out"].view(torch.float32, 3, 7, 8).cpu().numpy()
    want_running, want_closed = offline_rows(TINY, [buf["running"], buf["closed"]])
    assert want_closed.shape[0] == 6
    assert np.array_equal(out[0, 0].view(np.int32), want_running[6].view(np.int32))
    assert np.array_equal(out[2, :6].view(np.int32), want_closed.view(np.int32))
    assert np.all(out[0, 1:].view(np.int32) == word) and np.all(out[1].view(np.int32) == word)
    assert np.all(out[2, 6:].view(np.int32) == word)
    # the inputs are inputs
    assert np.array_equal(buf["rings"].view(torch.float32, 3, 64).cpu().numpy().view(np.int32), rings.view(np.int32))


def test_refusals_launch_nothing():
    """Every refusal of the header: status 1 and a message, rings and output still hold their fill."""
    import torch
    from mbexwn_vocoder_amd.engine import load_library
    lib = load_library()
    buf = live_buffers("nan")
    for change in (dict(packed=None), dict(desc=None), dict(rings=None), dict(ring_samples=48), dict(ring_samples=0),
                   dict(n_streams=-1), dict(n_streams=65536), dict(n_slots=0), dict(packed_samples=-1), dict(max_count=-1)):
        status = call_append(lib, buf, **change)
        message = lib.mbx_last_error().decode()
        assert status == 1 and message.startswith("ring append:") and len(message) > 14, (change, status, message)
    torch.cuda.synchronize()
    assert buf["rings"].payload_untouched()
    for change in (dict(rings=None), dict(desc=None), dict(window=None), dict(twiddle=None), dict(basis=None),
                   dict(bin_lo=None), dict(bin_hi=None), dict(out=None), dict(ring_samples=96), dict(ring_samples=32),
                   dict(fft_size=48), dict(fft_size=4), dict(fft_size=4096), dict(win=65), dict(win=1), dict(hop=0),
                   dict(n_mels=0), dict(n_streams=-1), dict(max_new_frames=-1), dict(n_slots=0)):
        status = call_frames(lib, buf, **change)
        message = lib.mbx_last_error().decode()
        assert status == 1 and message.startswith("mel frames:") and len(message) > 13, (change, status, message)
    torch.cuda.synchronize()
    assert buf["out"].payload_untouched()
    buf["gs"].check()
    # descriptors that point outside the caller's buffers are skipped, not followed
    bad = np.asarray([[3, 0, 60, 0], [-1, 0, 60, 0], [1, 0, 60, 61]], dtype=np.int64)
    buf["append"].put(bad)
    assert call_append(lib, buf) == 0
    buf["frames"].put(np.asarray([[3, 0, 1, 60], [-1, 0, 1, 60], [1, -1, 1, 60]], dtype=np.int64))
    assert call_frames(lib, buf) == 0
    torch.cuda.synchronize()
    assert buf["rings"].payload_untouched() and buf["out"].payload_untouched()
    buf["gs"].check()


# ---------------------------------------------------------------------------------------------------------------------
# audio in, audio out
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    from mbexwn_vocoder_amd.mel_inverter import create_synthetic_model_dir
    return create_synthetic_model_dir(str(tmp_path_factory.mktemp("model") / "speech_small"), "SPEECH", **SMALL)


def test_live_pipeline_equals_the_offline_synthesis(model_dir):
    """Three streams through a LiveResynthesizer at the 80 ms schedule: one whose pushes carry transposition factors that
    change mid-stream, one without control, one opened after the others have started.  Each equals synth_from_mel of its
    device-analysed, scale_mel-scaled mel with the same noise and the per-frame factors, on an engine pinned to f23."""
    from mbexwn_vocoder_amd.analysis import mell_header
    from mbexwn_vocoder_amd.live import LiveResynthesizer, frame_factors
    from mbexwn_vocoder_amd.mel_inverter import MELInverter
    inv = MELInverter(model_dir, conv_form="f23")
    cfg = inv.preprocess_config
    hop, spf = inv.hop_size, inv.model.dims.steps_per_frame
    lengths = [52 * hop + 77, 30 * hop, 41 * hop + 151]               # the second ends on a frame boundary
    sounds = [sound(300 + ii, nn) for ii, nn in enumerate(lengths)]
    rng = np.random.default_rng(5)
    noises = [rng.normal(size=(nn // hop + 1) * spf).astype(np.float32) for nn in lengths]
    factors = {0: lambda start: 1.0 if start < 15 * hop else 1.3 if start < 33 * hop else 0.8, 2: lambda start: 1.1}
    cuts = [random_cuts(rng, nn, hop, forced=(1920,) * 3) for nn in lengths]
    pushes = [[(cc, factors[sid](sum(cuts[sid][:ii])) if sid in factors else None) for ii, cc in enumerate(cuts[sid])]
              for sid in range(3)]
    live = LiveResynthesizer(inv, chunk_frames=(6, 6, 7, 6, 7))
    assert abs(live.lookahead_ms - (25.0 + live.synthesizer.lookahead_ms)) < 1e-9      # win / 2 = 600 samples = 2 frames
    got = {sid: [] for sid in range(3)}
    step = {sid: 0 for sid in range(3)}
    pos = {sid: 0 for sid in range(3)}
    opened, rounds = set(), 0
    while not (len(opened) == 3 and all(live.finished(sid) for sid in range(3))):
        for sid in range(3):
            if sid == 2 and rounds < 4:
                continue
            if sid not in opened:
                live.open(sid, noise_fn=lambda ss, a, b: noises[ss][a * spf:b * spf])
                opened.add(sid)
            if step[sid] < len(pushes[sid]):
                count, factor = pushes[sid][step[sid]]
                end = pos[sid] + count
                live.push_audio(sid, sounds[sid][pos[sid]:end], last=end == lengths[sid], transposition=factor)
                pos[sid], step[sid] = end, step[sid] + 1
        for sid, audio in live.tick().items():
            got[sid].append(np.array(audio))
        rounds += 1
        assert rounds < 5000
    mels = offline_rows(cfg, sounds)
    for sid in range(3):
        scaled = inv.scale_mel(dict(mell_header(cfg), mell=mels[sid].T))
        per_frame = frame_factors(pushes[sid], hop) if sid in factors else None
        want = inv.synth_from_mel(scaled, noise=noises[sid][None], transposition=per_frame)
        audio = np.concatenate(got[sid])
        assert audio.shape == want.shape == ((lengths[sid] // hop + 1) * hop,)
        assert np.array_equal(audio.view(np.int32), want.view(np.int32)), f"stream {sid} differs from the offline synthesis"
    plain = inv.synth_from_mel(inv.scale_mel(dict(mell_header(cfg), mell=mels[0].T)), noise=noises[0][None])
    assert not np.array_equal(plain, np.concatenate(got[0]))                            # the control does something


def test_stream_transpose_tool(model_dir, tmp_path):
    """stream_transpose.py on a wav file writes the samples a LiveResynthesizer gives for the same pushes; a file at another
    rate is refused by name, pointing at the resamplers."""
    from scipy.io import wavfile
    from mbexwn_vocoder_amd.audioio import read_audio
    from mbexwn_vocoder_amd.live import LiveResynthesizer
    from mbexwn_vocoder_amd.mel_inverter import MELInverter
    snd = sound(900, 11 * 1920 + 333)
    src, dst = str(tmp_path / "in.wav"), str(tmp_path / "out" / "out.wav")
    wavfile.write(src, 24000, snd)
    res = subprocess.run([sys.executable, TOOL, src, "-o", dst, "--model_id", model_dir, "--transposition", "1.25", "--seed", "3"],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    audio, rate = read_audio(dst)
    spec = importlib.util.spec_from_file_location("stream_transpose", TOOL)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    want = tool.stream_file(LiveResynthesizer(MELInverter(model_dir)), snd, 1920, 1.25, seed=3)
    assert rate == 24000 and audio.dtype == np.float32 and audio.shape == want.shape == ((snd.size // 300 + 1) * 300,)
    assert np.array_equal(audio.view(np.int32), want.view(np.int32))
    other = str(tmp_path / "in44.wav")
    wavfile.write(other, 44100, snd)
    res = subprocess.run([sys.executable, TOOL, other, "-o", dst, "--model_id", model_dir], capture_output=True, text=True,
                         timeout=600)
    assert res.returncode == 1 and "generate_mel.py" in res.stderr and "resample.resample_host" in res.stderr
