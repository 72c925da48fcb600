"""The streaming F0 tracker on the GPU (csrc/f0_stream.hip through include/mbexwn_live_pitch.h, live.py; DESIGN.md section
6j): a tracking StreamingAnalyzer against the definition f0track.track_f0_host and the offline mel analysis, however the
sound is cut into pushes; a resampled stream against generate_mels; the entry point's memory contract between guard bands and
its refusals; the live pipeline with f0_source="audio" against transform_audio(f0_fill="hold"); the tool.  Every comparison
is on bits: both sides make the same separately rounded float32 operations."""
import ctypes
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

from guarded import FILLS, GuardSet, fill_word
from mbexwn_vocoder_amd import f0track

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "mbexwn_vocoder_amd", "bin", "stream_transpose.py")
SMALL = {"mbexwn_config:pp_mod_subnet:n_channels": 32, "mbexwn_config:pp_mod_subnet:n_layers": 5}
SR, SEED = 24000, 7
# (window, tau_min, tau_max, hop): the smallest frame with an odd L = 69; the defaults at 24 kHz, L = 1461
SETS = {"small": (64, 2, 5, 16), "default": (1024, 24, 437, 300)}
TINY16 = {"sample_rate": SR, "hop_size": 16, "win_size": 48, "fft_size": 64, "mel_channels": 8, "fmin": 0.0, "fmax": None,
          "lin_amp_off": 1e-5, "lin_amp_scale": 1, "mel_amp_scale": 1}


def bits(arr):
    return np.ascontiguousarray(arr, dtype=np.float32).view(np.uint32)


def harmonic(n, f0, rng, noise=1e-3, amp=0.5):
    tt = np.arange(n) / SR
    x = sum((amp / h) * np.sin(2 * np.pi * f0 * h * tt + h) for h in range(1, 9))
    return (x + noise * rng.standard_normal(n)).astype(np.float32)


def make_sounds():
    """The kinds of test_gpu_f0track.py at 6000 samples (the high tone has a period of 4 samples: what the small parameter set
    can call voiced), and the lengths 700 (shorter than the default L), 37 and 1."""
    rng = np.random.default_rng(20)
    n = 6000
    broken = harmonic(n, 180.0, rng)
    broken[[900, 2400, 4000]] = [np.nan, np.inf, 1e20]
    return {"tone+noise": harmonic(n, 220.0, rng), "noise": (0.1 * rng.standard_normal(n)).astype(np.float32),
            "silence": np.zeros(n, np.float32), "not finite": broken, "high tone": harmonic(n, 6000.0, rng),
            "n=700": harmonic(700, 440.0, rng), "n=37": (0.1 * rng.standard_normal(37)).astype(np.float32), "n=1": np.ones(1, np.float32)}


def config_of(name):
    from mbexwn_vocoder_amd.config import canonical_config
    return TINY16 if name == "small" else canonical_config("SPEECH")["preprocess_config"]


def params_of(name):
    window, tau_min, tau_max, _ = SETS[name]
    return {"sample_rate": SR, "window": window, "tau_min": tau_min, "tau_max": tau_max, "threshold": float(np.float32(0.15)),
            "e_min": float(f0track.params(SR, window=window)["e_min"])}


def offline_rows(cfg, sounds):
    """compute_log_mel_device of every sound (one ragged launch), trimmed to its n // hop + 1 rows."""
    import torch
    from mbexwn_vocoder_amd.analysis import compute_log_mel_device
    win, hop = int(cfg.get("win_size", cfg["fft_size"])), int(cfg["hop_size"])
    lengths = [ss.size for ss in sounds]
    host = np.zeros((len(sounds), max(max(lengths), win // 2 + 1)), dtype=np.float32)
    for bb, ss in enumerate(sounds):
        host[bb, :ss.size] = ss
    mel, _ = compute_log_mel_device(torch.as_tensor(host).cuda(), cfg, n_samples=torch.as_tensor(lengths, dtype=torch.int32).cuda())
    mel = mel.cpu().numpy()
    return [mel[bb, :nn // hop + 1].copy() for bb, nn in enumerate(lengths)]


@pytest.fixture(scope="module", params=list(SETS))
def case(request):
    """A parameter set: its analysis configuration, the sounds, and per sound the host definition's (f0, periodicity) and the
    offline mel rows -- the references of the tests below, computed once."""
    name = request.param
    cfg, prm, hop = config_of(name), params_of(name), SETS[name][3]
    assert int(cfg["hop_size"]) == hop and int(round(cfg["sample_rate"])) == SR
    sounds = make_sounds()
    tracks = {kk: f0track.track_f0_host(x, np.arange(0, x.size + 1, hop), prm) for kk, x in sounds.items()}
    assert np.count_nonzero(tracks["high tone" if name == "small" else "tone+noise"][0]) > 3      # the comparisons see picks
    assert not np.count_nonzero(tracks["silence"][0]) and not np.count_nonzero(tracks["noise"][0])
    broken = tracks["not finite"]
    assert np.any((broken[0] == 0) & (broken[1] == 1)) and np.any(broken[1] != 1)          # the unvoiced-with-periodicity-1 rule
    mels = dict(zip(sounds, offline_rows(cfg, list(sounds.values()))))
    return name, cfg, prm, hop, sounds, tracks, mels


def random_cuts(rng, n, hop, forced=()):
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


def serve(an, prm, sounds, cuts, pushes_per_tick=1, stream_ids=None):
    """Push every sound (a dict) in its cuts, `pushes_per_tick` pushes of every stream between two ticks; returns per stream
    the concatenated (mel rows, f0, periodicity).  Every tick's last_f0 has one value per mel row handed out."""
    ids = stream_ids or {kk: kk for kk in sounds}
    got = {kk: ([], [], []) for kk in sounds}
    pos, step = dict.fromkeys(sounds, 0), dict.fromkeys(sounds, 0)
    for kk in sounds:
        an.open(ids[kk], f0_params=prm)
    back = {vv: kk for kk, vv in ids.items()}
    rounds = 0
    while not all(an.finished(ids[kk]) for kk in sounds):
        for kk, ss in sounds.items():
            for _ in range(pushes_per_tick):
                if step[kk] < len(cuts[kk]):
                    end = pos[kk] + cuts[kk][step[kk]]
                    an.push(ids[kk], ss[pos[kk]:end], last=end == ss.size)
                    pos[kk], step[kk] = end, step[kk] + 1
        rows = an.tick()
        assert sorted(map(str, an.last_f0)) == sorted(map(str, rows))
        for sid, mel in rows.items():
            f0, per = an.last_f0[sid]
            assert f0.dtype == per.dtype == np.float32 and f0.shape == per.shape == (mel.shape[0],) and mel.shape[0] > 0
            for part, value in zip(got[back[sid]], (mel, f0, per)):
                part.append(value)
        rounds += 1
        assert rounds < 100000
    return {kk: tuple(np.concatenate(part) for part in parts) for kk, parts in got.items()}


def assert_streams_equal(got, case, what=""):
    _, _, _, hop, sounds, tracks, mels = case
    for kk, (mel, f0, per) in got.items():
        n = sounds[kk].size
        assert f0.shape == per.shape == (n // hop + 1,) and mel.shape == mels[kk].shape, (kk, what)
        assert np.array_equal(bits(f0), bits(tracks[kk][0])), (kk, what, f0, tracks[kk][0])
        assert np.array_equal(bits(per), bits(tracks[kk][1])), (kk, what, per, tracks[kk][1])
        # the mel promise is untouched (a NaN is a NaN: which payload a sum of two keeps is not part of it)
        nan = np.isnan(mels[kk])
        assert np.array_equal(np.isnan(mel), nan) and np.array_equal(bits(mel)[~nan], bits(mels[kk])[~nan]), (kk, what)
        assert kk == "not finite" or not nan.any()


def test_kernel_equals_the_definition(case):
    """All eight sounds as concurrent tracking streams, cut at random from a fixed seed, a tick after every push: the
    concatenated last_f0 of a stream is track_f0_host on the whole sound, and the mel rows are still the offline rows."""
    from mbexwn_vocoder_amd.live import StreamingAnalyzer
    name, cfg, prm, hop, sounds, _, _ = case
    rng = np.random.default_rng(2025)
    cuts = {kk: random_cuts(rng, ss.size, hop if name == "default" else 8 * hop) for kk, ss in sounds.items()}
    an = StreamingAnalyzer(cfg, slots=4)
    assert_streams_equal(serve(an, prm, sounds, cuts), case, "random cuts")
    assert an.ring_samples >= prm["window"] + prm["tau_max"]


def test_cuts_do_not_change_a_bit(case):
    from mbexwn_vocoder_amd.live import StreamingAnalyzer
    name, cfg, prm, hop, sounds, tracks, _ = case
    L = prm["window"] + prm["tau_max"]
    # one push each
    assert_streams_equal(serve(StreamingAnalyzer(cfg), prm, sounds, {kk: [ss.size] for kk, ss in sounds.items()}), case, "one push")
    # single samples on n = 700 (and the two shorter ones): a tick after every push, and one every 7 pushes
    short = {kk: sounds[kk] for kk in ("n=700", "n=37", "n=1")}
    ones = {kk: [1] * ss.size for kk, ss in short.items()}
    assert_streams_equal(serve(StreamingAnalyzer(cfg), prm, short, ones), case, "single samples")
    assert_streams_equal(serve(StreamingAnalyzer(cfg), prm, short, ones, pushes_per_tick=7), case, "single samples, 7 a tick")
    # a start ring of 2048 that 6000 samples wrap (with the default set a pending frame reaches back 730 samples and waits
    # for 731 more, so pushes of up to 3 hops double the ring once: 6000 samples wrap that too)
    long_ones = {kk: ss for kk, ss in sounds.items() if ss.size == 6000}
    rng = np.random.default_rng(77)
    an = StreamingAnalyzer(cfg, ring_samples=2048)
    step = hop if name == "default" else 8 * hop
    assert_streams_equal(serve(an, prm, long_ones, {kk: random_cuts(rng, 6000, step) for kk in long_ones}), case, "wrapped ring")
    assert L <= an.ring_samples == (2048 if name == "small" else 4096)
    # one 5000-sample push into that ring, behind 600 samples that are on the device already: the ring grows mid-stream
    an = StreamingAnalyzer(cfg, ring_samples=2048)
    assert_streams_equal(serve(an, prm, long_ones, {kk: [600, 5000, 400] for kk in long_ones}), case, "grown ring")
    assert an.ring_samples > 2048
    # a released slot whose ring holds NaN: the next stream in it starts from nothing of that
    an = StreamingAnalyzer(cfg, ring_samples=2048, slots=1)
    poison = {"poison": np.full(2500, np.nan, dtype=np.float32)}
    first = serve(an, prm, poison, {"poison": [1000, 1500]})["poison"]
    assert np.all(first[1] == 0) and np.all(first[2] == 1)               # every frame touches a NaN: unvoiced, periodicity 1
    slot = an.streams["poison"].slot
    an.close("poison")
    two = {kk: sounds[kk] for kk in ("n=700", "tone+noise")}
    got = serve(an, prm, two, {"n=700": [700], "tone+noise": [700] * 8 + [400]})
    assert an.streams["n=700"].slot == slot
    assert_streams_equal(got, case, "reused slot")


def test_resampled_stream_equals_generate_mels(case):
    """3000 samples at 44 100 Hz through a stream opened at that rate: last_f0 is the f0_out of generate_mels on the whole
    sound (device resampler, then the offline tracker), the rows are its mel."""
    from mbexwn_vocoder_amd.analysis import generate_mels
    from mbexwn_vocoder_amd.live import StreamingAnalyzer
    name, cfg, prm, hop, _, _, _ = case
    rng = np.random.default_rng(44)
    tt, tone = np.arange(3000) / 44100.0, 6000.0 if name == "small" else 196.0       # a pitch the parameter set can find
    x = (0.4 * np.sin(2 * np.pi * tone * tt) + 1e-3 * rng.standard_normal(3000)).astype(np.float32)
    tracked = []
    dicts = generate_mels([x], [44100], cfg, on_device=True, f0_out=tracked, f0_params=prm)
    an = StreamingAnalyzer(cfg)
    an.open("r", sample_rate=44100, f0_params=prm)
    parts, pos = ([], [], []), 0
    for count in random_cuts(rng, 3000, 441):
        an.push("r", x[pos:pos + count], last=pos + count == 3000)
        pos += count
        rows = an.tick()
        if "r" in rows:
            for part, value in zip(parts, (rows["r"], *an.last_f0["r"])):
                part.append(value)
    assert an.finished("r")
    mel, f0, per = (np.concatenate(part) for part in parts)
    assert f0.shape == tracked[0][0].shape and np.count_nonzero(tracked[0][0]) > 0
    assert np.array_equal(bits(f0), bits(tracked[0][0])) and np.array_equal(bits(per), bits(tracked[0][1]))
    assert np.array_equal(bits(mel), bits(np.asarray(dicts[0]["mell"]).T))


# ---------------------------------------------------------------------------------------------------------------------
# the entry point between guard bands
# ---------------------------------------------------------------------------------------------------------------------
RING, HOP = 128, 16
DESC = [[0, 7, 4, -1], [1, 0, 4, 60], [2, 0, 0, -1], [3, 0, 1, 60], [-1, 0, 1, 60], [1, -1, 1, 60]]


def raw_buffers(fill):
    """Three rings of 128 samples, the small parameter set (L = 69, hop 16).  Slot 0: a running stream that holds its samples
    [72, 200): frames 7 .. 10 read [78, 195).  Slot 1: a closed stream of 60 samples, frames 0 .. 3 -- they read in front of
    sample 0 and behind sample 59, where the ring holds the fill.  Slot 2: nothing to do.  Then three rows to skip: a slot
    outside the store, a negative slot, a negative first frame.  max_new_frames = 5."""
    import torch
    rng = np.random.default_rng(9)
    running, closed = harmonic(200, 6000.0, rng, amp=0.3), harmonic(60, 8000.0, rng, amp=0.3)
    gs = GuardSet(fill, device="cuda")
    rings = gs.new("rings", 3 * RING * 4)
    view = rings.view(torch.float32, 3, RING)
    idx = np.arange(72, 200)
    view[0, torch.as_tensor(idx & (RING - 1)).cuda()] = torch.as_tensor(running[idx]).cuda()
    view[1, :60] = torch.as_tensor(closed).cuda()
    return dict(gs=gs, running=running, closed=closed, rings=rings, desc=gs.put("desc", np.asarray(DESC, dtype=np.int64)),
                f0=gs.new("f0", len(DESC) * 5 * 4), per=gs.new("periodicity", len(DESC) * 5 * 4))


def call_raw(lib, buf, **change):
    import torch
    args = dict(rings=buf["rings"].ptr, n_slots=3, ring_samples=RING, desc=buf["desc"].ptr, n_streams=len(DESC),
                max_new_frames=5, hop=HOP, sample_rate=SR, window=64, tau_min=2, tau_max=5, threshold=0.15, e_min=0.0,
                f0=buf["f0"].ptr, periodicity=buf["per"].ptr)
    args.update(change)
    return lib.mbxt_f0_frames(args["rings"], args["n_slots"], args["ring_samples"], args["desc"], args["n_streams"],
                              args["max_new_frames"], args["hop"], args["sample_rate"], args["window"], args["tau_min"],
                              args["tau_max"], ctypes.c_float(args["threshold"]), ctypes.c_float(args["e_min"]), args["f0"],
                              args["periodicity"], torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("fill", FILLS)
def test_memory_contract_between_guard_bands(fill):
    import torch
    from mbexwn_vocoder_amd.engine import load_library
    lib = load_library()
    buf = raw_buffers(fill)
    word = fill_word(fill)
    before = buf["rings"].view(torch.int32).clone()
    assert call_raw(lib, buf) == 0, lib.mbx_last_error()
    torch.cuda.synchronize()
    buf["gs"].check()
    prm = {"sample_rate": SR, "window": 64, "tau_min": 2, "tau_max": 5, "threshold": float(np.float32(0.15)), "e_min": 0.0}
    # the running stream is open: frames 7 .. 10 of any sound that continues its 200 samples
    want_running = f0track.track_f0_host(np.concatenate((buf["running"], np.zeros(100, np.float32))), HOP * np.arange(7, 11), prm)
    want_closed = f0track.track_f0_host(buf["closed"], HOP * np.arange(4), prm)
    for got, want_r, want_c in zip((buf["f0"], buf["per"]), want_running, want_closed):
        out = got.view(torch.float32, len(DESC), 5).cpu().numpy()
        assert np.array_equal(bits(out[0, :4]), bits(want_r)) and np.array_equal(bits(out[1, :4]), bits(want_c)), got.name
        raw = out.view(np.int32)
        assert np.all(raw[0, 4:] == word) and np.all(raw[1, 4:] == word)             # rows behind n_frames keep the fill
        assert np.all(raw[2:] == word)                                               # no frames; the three skipped rows
    assert np.count_nonzero(want_running[0]) and np.all(np.isfinite(want_closed[1]))
    assert torch.equal(buf["rings"].view(torch.int32), before)                       # the input is an input


def test_refusals_leave_the_outputs_untouched():
    import torch
    from mbexwn_vocoder_amd.engine import load_library
    lib = load_library()
    buf = raw_buffers("huge")
    cases = [dict(rings=None), dict(desc=None), dict(f0=None), dict(periodicity=None), dict(n_streams=-1), dict(n_streams=65536),
             dict(max_new_frames=-1), dict(n_slots=0), dict(hop=0), dict(hop=-3),
             # the bounds of check_track_f0
             dict(sample_rate=0), dict(window=0), dict(window=32), dict(window=96), dict(window=2112), dict(tau_max=1),
             dict(tau_min=-1), dict(tau_min=5), dict(tau_min=2, tau_max=2), dict(window=2048, tau_max=2049, ring_samples=8192),
             dict(threshold=float("nan")), dict(e_min=float("nan")),
             # the ring: a power of two, at least window + tau_max = 69
             dict(ring_samples=0), dict(ring_samples=-128), dict(ring_samples=96), dict(ring_samples=64),
             dict(ring_samples=1024, window=1024, tau_max=437)]
    for change in cases:
        status = call_raw(lib, buf, **change)
        message = lib.mbx_last_error().decode()
        assert status == 1 and message.startswith("f0 frames:") and len(message) > 12, (change, status, message)
    torch.cuda.synchronize()
    assert buf["f0"].payload_untouched() and buf["per"].payload_untouched()
    buf["gs"].check()
    assert call_raw(lib, buf, n_streams=0) == 0 and call_raw(lib, buf, max_new_frames=0) == 0        # nothing to do
    torch.cuda.synchronize()
    assert buf["f0"].payload_untouched() and buf["per"].payload_untouched()
    assert call_raw(lib, buf) == 0                                                    # and the same buffers do run
    torch.cuda.synchronize()
    assert not buf["f0"].payload_untouched() and not buf["per"].payload_untouched()
    buf["gs"].check()


# ---------------------------------------------------------------------------------------------------------------------
# audio in, audio out, with the pitch of the audio
# ---------------------------------------------------------------------------------------------------------------------
NAME = "pitch.wav"


def pipeline_sound():
    """0.15 s of silence, 0.3 s of a 200 Hz harmonic tone, 0.15 s of noise at 0.05, 0.3 s of a 260 Hz tone."""
    rng = np.random.default_rng(31)
    return np.concatenate((np.zeros(3600, np.float32), harmonic(7200, 200.0, rng),
                           (0.05 * rng.standard_normal(3600)).astype(np.float32), harmonic(7200, 260.0, rng)))


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    from mbexwn_vocoder_amd.mel_inverter import create_synthetic_model_dir
    return create_synthetic_model_dir(str(tmp_path_factory.mktemp("model") / "speech_small"), "SPEECH", **SMALL)


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("stream_transpose", TOOL)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


@pytest.fixture(scope="module")
def pipeline(model_dir, tool):
    """The sound streamed with f0_source="audio" in 80 ms pieces at a transposition of 1.5 under keyed noise, with what the
    stream tracked: the reference of the two tests below, computed once."""
    from mbexwn_vocoder_amd.live import LiveResynthesizer, keyed_noise_fn
    from mbexwn_vocoder_amd.mel_inverter import MELInverter
    inv = MELInverter(model_dir, conv_form="f23")
    snd = pipeline_sound()
    live = LiveResynthesizer(inv)
    tracked = []
    audio = tool.stream_file(live, snd, 1920, 1.5, stream_id=NAME, noise_fn=keyed_noise_fn(inv.model, SEED), f0_source="audio",
                             f0_out=tracked)
    return inv, live, snd, audio, tracked


def test_live_pipeline_equals_transform_audio_with_the_hold_fill(pipeline, tool):
    from mbexwn_vocoder_amd.live import keyed_noise_fn
    inv, live, snd, audio, tracked = pipeline
    hop = inv.hop_size
    want_f0, want_per = f0track.track_f0_host(snd, np.arange(0, snd.size + 1, hop), f0track.params(SR))
    # the fixture has what the causal rule is about: unvoiced frames in front, and a gap between voiced frames
    voiced = np.flatnonzero(want_f0 > 0)
    assert voiced.size and voiced[0] >= 1
    assert np.max(np.diff(voiced)) >= 3                                  # voiced frames on both sides of an unvoiced run of >= 2
    f0 = np.concatenate([pair[0] for pair in tracked])
    per = np.concatenate([pair[1] for pair in tracked])
    assert np.array_equal(bits(f0), bits(want_f0)) and np.array_equal(bits(per), bits(want_per))
    want = inv.transform_audio([snd], [SR], [NAME], transposition=1.5, noise_seed=SEED, f0_source="audio", f0_fill="hold")[0]
    assert audio.shape == want.shape == ((snd.size // hop + 1) * hop,)
    assert np.array_equal(bits(audio), bits(want))                       # sample for sample
    # the source and the fill do something
    net = tool.stream_file(live, snd, 1920, 1.5, stream_id=NAME, noise_fn=keyed_noise_fn(inv.model, SEED))
    assert net.shape == audio.shape and not np.array_equal(net, audio)
    other = inv.transform_audio([snd], [SR], [NAME], transposition=1.5, noise_seed=SEED, f0_source="audio")[0]
    assert not np.array_equal(other, want)
    with pytest.raises(ValueError, match="hold"):
        inv.transform_audio([snd], [SR], [NAME], f0_fill="hold")
    assert live.lookahead_ms_for(f0_source="audio") == live.lookahead_ms + 12.5      # 3 frames of analysis instead of 2


@pytest.mark.timeout(600)
def test_stream_transpose_tool_tracks_and_writes_the_contour(pipeline, model_dir, tmp_path):
    from scipy.io import wavfile
    from mbexwn_vocoder_amd.audioio import read_audio
    inv, _, snd, audio, _ = pipeline
    src, dst = str(tmp_path / NAME), str(tmp_path / "out" / "out.wav")
    wavfile.write(src, SR, snd)
    res = subprocess.run([sys.executable, TOOL, src, "-o", dst, "--model_id", model_dir, "--transposition", "1.5", "--noise-seed",
                          str(SEED), "--f0-source", "audio", "--write-f0"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    got, rate = read_audio(dst)
    assert rate == SR and got.shape == audio.shape and np.array_equal(bits(got), bits(audio))
    assert "look-ahead" in res.stderr
    want_f0, want_per = f0track.track_f0_host(snd, np.arange(0, snd.size + 1, inv.hop_size), f0track.params(SR))
    times, f0, per = f0track.read_f0(str(tmp_path / "out" / "out.f0"), n_frames=want_f0.size)
    assert np.array_equal(bits(f0), bits(want_f0)) and np.array_equal(bits(per), bits(want_per))
    assert np.allclose(times, np.arange(want_f0.size) * inv.hop_size / SR)
    res = subprocess.run([sys.executable, TOOL, src, "-o", dst, "--model_id", model_dir, "--write-f0"], capture_output=True,
                         text=True, timeout=600)
    assert res.returncode == 1 and "--f0-source audio" in res.stderr
