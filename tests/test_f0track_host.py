"""The F0 tracker's host side (no GPU needed): the accuracy of its definition f0track.track_f0_host on tones, a vibrato glide,
noise and silence; fill_unvoiced; the .f0 file; params(); the header and export of mbxp_track_f0; the new flags of the three
tools; and the refusals of the ``f0s`` argument.

The accuracy bounds are those of the float32 prototype this definition was fixed with (24 kHz, hop 300, the defaults, eight
harmonics at 0.5 / h, noise of 1e-3), with about twice its error: 2.3 cents worst on the ten tones, 5.2 cents on the glide."""
import importlib.util
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

from mbexwn_vocoder_amd import engine, f0track

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mbexwn_vocoder_amd", "bin")
SR, HOP = 24000, 300
TONES = [60, 82.4, 110, 146.8, 220, 330, 440, 523.25, 700, 880]


def load_script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(BIN, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_script(name, args):
    return subprocess.run([sys.executable, os.path.join(BIN, name + ".py"), *args], capture_output=True, text=True, timeout=600)


def inside(centres, n, prm):
    """Frames whose L samples lie inside the sound."""
    L = prm["window"] + prm["tau_max"]
    first = centres - (L >> 1)
    return (first >= 0) & (first + L <= n)


def cents(f0, true):
    return 1200.0 * np.log2(np.asarray(f0, np.float64) / true)


# ------------------------------------------------------------------------------------------------------------------------
# the definition on signals with a known pitch
# ------------------------------------------------------------------------------------------------------------------------
def test_steady_tones_within_five_cents():
    prm = f0track.params(SR)
    rng = np.random.default_rng(0)
    n = 12000
    tt = np.arange(n) / SR
    centres = np.arange(n // HOP + 1) * HOP
    keep = inside(centres, n, prm)
    assert keep.sum() >= 30
    worst = 0.0
    for f in TONES:
        x = sum((0.5 / h) * np.sin(2 * np.pi * f * h * tt + h) for h in range(1, 9) if f * h < 11000)
        x = (x + 1e-3 * rng.standard_normal(n)).astype(np.float32)
        f0, per = f0track.track_f0_host(x, centres, prm)
        assert f0.dtype == np.float32 and per.dtype == np.float32 and f0.shape == per.shape == centres.shape
        assert np.all(f0[keep] > 0), f                                   # every frame inside the sound is voiced
        err = float(np.abs(cents(f0[keep], f)).max())
        print(f"{f} Hz: worst {err:.2f} cents, periodicity <= {per[keep].max():.4f}")
        worst = max(worst, err)
        assert err <= 5.0, (f, err)
    print(f"worst of the ten tones: {worst:.2f} cents")


def test_vibrato_glide_within_ten_cents():
    prm = f0track.params(SR)
    n = 24000
    tt = np.arange(n) / SR
    fi = 200 * 2 ** (0.5 * np.sin(2 * np.pi * 5.5 * tt) / 12) * (1 + 0.2 * tt)       # 200 -> 240 Hz, +- half a semitone
    ph = 2 * np.pi * np.cumsum(fi) / SR
    x = sum((0.5 / h) * np.sin(h * ph) for h in range(1, 9)).astype(np.float32)
    centres = np.arange(n // HOP + 1) * HOP
    keep = inside(centres, n, prm)
    f0, _ = f0track.track_f0_host(x, centres, prm)
    assert np.all(f0[keep] > 0)
    err = cents(f0[keep], fi[centres[keep]])                            # against the instantaneous frequency at the centre
    print(f"glide: worst {np.abs(err).max():.2f} cents, rms {np.sqrt(np.mean(err ** 2)):.2f} cents")
    assert np.abs(err).max() <= 10.0


def test_noise_and_silence_are_unvoiced():
    prm = f0track.params(SR)
    centres = np.arange(41) * HOP
    noise = (0.1 * np.random.default_rng(1).standard_normal(12000)).astype(np.float32)
    f0, per = f0track.track_f0_host(noise, centres, prm)
    print(f"noise: least periodicity {per.min():.3f}")
    assert np.all(f0 == 0) and per.min() > 0.5
    f0, per = f0track.track_f0_host(np.zeros(12000, np.float32), centres, prm)
    assert np.all(f0 == 0) and np.all(per == 1)
    # a tone below the energy floor is unvoiced too, and voiced without the floor; so is a frame over a sample that is not finite
    quiet = (1e-6 * np.sin(2 * np.pi * 200 * np.arange(12000) / SR)).astype(np.float32)
    assert np.all(f0track.track_f0_host(quiet, centres, prm)[0] == 0)
    assert np.all(f0track.track_f0_host(quiet, centres[5:35], dict(prm, e_min=0.0))[0] > 0)
    loud = (0.5 * np.sin(2 * np.pi * 200 * np.arange(12000) / SR)).astype(np.float32)
    loud[6000] = np.nan
    f0, per = f0track.track_f0_host(loud, centres, prm)
    touched = np.abs(centres - 6000) < 700
    assert np.all(f0[touched] == 0) and np.all(per[touched] == 1) and np.all(f0[~touched][3:-3] > 0)
    # empty sounds and empty tables
    f0, per = f0track.track_f0_host(np.zeros(0, np.float32), np.arange(3), prm)
    assert np.all(f0 == 0) and np.all(per == 1)
    assert f0track.track_f0_host(noise, np.zeros(0, np.int64), prm)[0].shape == (0,)


def test_lane_sum_order():
    rng = np.random.default_rng(2)
    p = rng.standard_normal(192).astype(np.float32) ** 2
    acc = [np.float32(p[ll]) for ll in range(64)]
    for kk in (1, 2):
        acc = [np.float32(acc[ll] + p[ll + 64 * kk]) for ll in range(64)]
    m = 32
    while m:
        acc = [np.float32(acc[ll] + acc[ll + m]) for ll in range(m)]
        m >>= 1
    assert f0track.lane_sum(p).view(np.uint32) == acc[0].view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------------
# fill_unvoiced, the .f0 file, params
# ------------------------------------------------------------------------------------------------------------------------
def test_fill_unvoiced():
    f32 = np.float32
    f0 = np.array([0, 0, 100.5, 0, 0, 0, 130.25, 131, 0, 0], dtype=f32)
    out = f0track.fill_unvoiced(f0)
    assert out.dtype == f32 and np.all(out[:2] == f32(100.5)) and np.all(out[7:] == f32(131))          # both ends
    for t in (3, 4, 5):                                                  # the inner gap, in the contract's float32 operations
        want = f32(f32(100.5) + f32(f32(130.25) - f32(100.5)) * f32(f32(t - 2) / f32(4)))
        assert out[t].view(np.uint32) == want.view(np.uint32)
    assert np.array_equal(out[[2, 6, 7]].view(np.uint32), f0[[2, 6, 7]].view(np.uint32))                # voiced: bits kept
    voiced = np.array([101.3, 99.9, 250.0], dtype=f32)
    assert np.array_equal(f0track.fill_unvoiced(voiced).view(np.uint32), voiced.view(np.uint32))
    assert f0track.fill_unvoiced(np.zeros(5, f32)) is None and f0track.fill_unvoiced(np.zeros(0, f32)) is None
    assert np.all(f0track.fill_unvoiced(np.array([0, 0, 80], f32)) == 80)
    for bad in ([1, np.nan], [1, -2], [[1, 2]]):
        with pytest.raises(ValueError):
            f0track.fill_unvoiced(np.array(bad, f32))


def test_f0_file_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    f0 = (rng.uniform(50, 1000, 40)).astype(np.float32)
    f0[[0, 7, 8, 39]] = 0
    per = rng.uniform(0, 1.2, 40).astype(np.float32)
    per[3] = np.float32(1e-39)                                           # a subnormal survives too
    times = f0track.frame_times(40, HOP, SR)
    assert times[0] == 0 and times[1] == HOP / SR
    path = str(tmp_path / "a.f0")
    f0track.write_f0(path, times, f0, per)
    lines = open(path).read().splitlines()
    assert len(lines) == 40 and all(len(ll.split()) == 3 for ll in lines) and lines[0].split()[1] == "0"
    tt, ff, pp = f0track.read_f0(path, n_frames=40)
    assert np.array_equal(ff.view(np.uint32), f0.view(np.uint32)) and np.array_equal(pp.view(np.uint32), per.view(np.uint32))
    assert np.allclose(tt, times, rtol=1e-8)
    with pytest.raises(ValueError, match="40 rows.*41 frames"):
        f0track.read_f0(path, n_frames=41)
    from mbexwn_vocoder_amd.batched import f0_path, load_contour
    assert f0_path("x/y/a.mell", str(tmp_path)) == path and f0_path("a.wav", str(tmp_path)) == path
    assert np.array_equal(load_contour("q/a.mell", str(tmp_path), 40), f0track.fill_unvoiced(f0))
    with pytest.raises(ValueError, match="one row per frame"):
        load_contour("a.mell", str(tmp_path), 39)
    with pytest.raises(OSError):
        load_contour("b.mell", str(tmp_path), 40)
    for text in ("0 100\n", "0 100 0.1 7\n", "0 x 0.1\n", "0 -5 0.1\n", "0 nan 0.1\n"):
        open(path, "w").write("# a comment\n0 100 0.1\n" + text)
        with pytest.raises(ValueError):
            f0track.read_f0(path)
    with pytest.raises(ValueError):
        f0track.write_f0(path, times, f0, per[:-1])


def test_params():
    prm = f0track.params(24000)
    assert (prm["sample_rate"], prm["window"], prm["tau_min"], prm["tau_max"]) == (24000, 1024, 24, 437)
    assert prm["window"] + prm["tau_max"] == 1461
    assert np.float32(prm["threshold"]) == np.float32(0.15) and np.float32(prm["e_min"]) == np.float32(1024 * 1e-4 ** 2)
    assert sorted(prm) == sorted(f0track.PARAM_KEYS)
    prm = f0track.params(16000, f0_min=80, f0_max=400, window=512, threshold=0.1, rms_floor=0)
    assert (prm["tau_min"], prm["tau_max"], prm["window"], prm["e_min"]) == (40, 200, 512, 0.0)
    for kw in ({"f0_min": 0}, {"f0_min": -5}, {"f0_min": 1000, "f0_max": 500}, {"f0_max": float("inf")}, {"f0_min": float("nan")},
               {"window": 100}, {"window": 32}, {"window": 4096}, {"window": 2048, "f0_min": 10}, {"f0_min": 5},
               {"f0_max": 20000, "f0_min": 13000}, {"rms_floor": -1}, {"threshold": float("nan")}):
        with pytest.raises(ValueError):
            f0track.params(24000, **kw)
    for rate in (0, -1, 24000.5):
        with pytest.raises(ValueError):
            f0track.params(rate)
    good = f0track.params(24000)
    for kw in ({"window": 96}, {"tau_max": 1}, {"tau_min": 437}, {"tau_min": -1}, {"window": 2048, "tau_max": 2049}, {"sample_rate": 0}):
        with pytest.raises(ValueError):
            f0track.check_params(dict(good, **kw))
    with pytest.raises(ValueError):
        f0track.check_params({"window": 64})
    from mbexwn_vocoder_amd.analysis import generate_mels
    cfg = {"sample_rate": 24000, "hop_size": 300, "fft_size": 2048, "win_size": 1200, "mel_channels": 80, "fmin": 0, "fmax": 8000,
           "lin_amp_off": 1e-5, "lin_amp_scale": 1, "mel_amp_scale": 1}
    with pytest.raises(ValueError, match="model rate"):
        generate_mels([np.zeros(100, np.float32)], [24000], cfg, on_device=False, f0_out=[], f0_params=f0track.params(16000))


def test_generate_mels_host_tracks_on_the_mel_frames():
    """f0_out on the host path: one (f0, periodicity) per item, one value per .mell column, on timemap.centres -- the regular
    frames and the warped ones --, the dictionaries with exactly their keys, and nothing changed without the argument."""
    from mbexwn_vocoder_amd import timemap
    from mbexwn_vocoder_amd.analysis import generate_mels, mell_header
    cfg = {"sample_rate": 24000, "hop_size": 300, "fft_size": 2048, "win_size": 1200, "mel_channels": 80, "fmin": 0, "fmax": 8000,
           "lin_amp_off": 1e-5, "lin_amp_scale": 1, "mel_amp_scale": 1}
    tt = np.arange(7000) / SR
    snd = (0.5 * np.sin(2 * np.pi * 150 * tt) + 0.2 * np.sin(2 * np.pi * 300 * tt)).astype(np.float32)
    plain = generate_mels([snd, snd], [SR, SR], cfg, on_device=False, time_maps=[None, 1.5])
    tracked = []
    dicts = generate_mels([snd, snd], [SR, SR], cfg, on_device=False, time_maps=[None, 1.5], f0_out=tracked)
    prm = f0track.params(SR)
    for ii, spec in enumerate((None, 1.5)):
        assert sorted(dicts[ii]) == sorted(dict(mell_header(cfg), mell=0)) and np.array_equal(dicts[ii]["mell"], plain[ii]["mell"])
        want = f0track.track_f0_host(snd, timemap.centres(snd.size, 300, SR, spec), prm)
        assert tracked[ii][0].shape == (dicts[ii]["mell"].shape[1],)
        assert np.array_equal(tracked[ii][0].view(np.uint32), want[0].view(np.uint32))
        assert np.array_equal(tracked[ii][1].view(np.uint32), want[1].view(np.uint32))
    assert tracked[1][0].size == int(np.floor(7000 * 1.5 / 300)) + 1
    mid = tracked[0][0][4:-4]
    assert np.all(np.abs(cents(mid, 150.0)) < 5.0)


# ------------------------------------------------------------------------------------------------------------------------
# header, symbol list, build lists
# ------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_point_and_the_library_exports_it(tmp_path):
    """(that the header declares exactly these names, no other header does and the library exports them: test_abi_headers.py)"""
    from mbexwn_vocoder_amd import abi
    from mbexwn_vocoder_amd.build import HEADERS, SOURCES
    text = open(os.path.join(ROOT, "include", "mbexwn_pitch.h")).read()
    assert "THE DEFINITION" in text and "Refused" in text and '"track f0:"' in text
    assert abi.symbols("mbexwn_pitch.h") == ["mbxp_track_f0"]
    assert any(hh.endswith("mbexwn_pitch.h") for hh in HEADERS) and "f0_track.hip" in SOURCES
    assert abi.MBX_ABI_VERSION == 11
    src = tmp_path / "use.c"
    src.write_text('#include "mbexwn_pitch.h"\nint main(void){ (void)mbxp_track_f0; return 0; }\n')
    res = subprocess.run(["cc", "-std=c99", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr                               # the header is plain C
    kernel = open(os.path.join(ROOT, "mbexwn_vocoder_amd", "csrc", "f0_track.hip")).read()
    assert "#pragma clang fp contract(off)" in kernel and "fmaf" not in kernel and "getenv" not in kernel and "hipMalloc" not in kernel


def test_the_c_entry_point_refuses_on_the_host():
    """mbxp_track_f0 checks every argument before it touches the device: the refusals need no GPU."""
    import ctypes
    lib = engine.load_library()
    buf = (ctypes.c_float * 64)()
    ptr = ctypes.addressof(buf)
    good = dict(audio=ptr, stride=16, batch=1, n_samples=ptr, centres=ptr, n_frames=ptr, max_frames=1, sample_rate=24000, window=1024,
                tau_min=24, tau_max=437, threshold=0.15, e_min=0.0, f0=ptr, periodicity=ptr)

    def call(**kw):
        aa = dict(good, **kw)
        return lib.mbxp_track_f0(aa["audio"], aa["stride"], aa["batch"], aa["n_samples"], aa["centres"], aa["n_frames"],
                                 aa["max_frames"], aa["sample_rate"], aa["window"], aa["tau_min"], aa["tau_max"],
                                 ctypes.c_float(aa["threshold"]), ctypes.c_float(aa["e_min"]), aa["f0"], aa["periodicity"], None)

    cases = [{name: None} for name in ("audio", "n_samples", "centres", "n_frames", "f0", "periodicity")]
    cases += [{"window": 0}, {"window": 96}, {"window": 2112}, {"tau_max": 1}, {"tau_min": 437}, {"window": 2048, "tau_max": 2049},
              {"sample_rate": 0}, {"max_frames": 0}, {"stride": 0}, {"batch": -1}, {"batch": 65536}]
    for kw in cases:
        assert call(**kw) == 1, kw                                       # MBX_ERR_INVALID_ARGUMENT
        assert lib.mbx_last_error().decode().startswith("track f0:"), kw
    assert call(batch=0) == 0                                            # nothing to do


# ------------------------------------------------------------------------------------------------------------------------
# the tools
# ------------------------------------------------------------------------------------------------------------------------
def test_transform_audio_flags(tmp_path, capsys, monkeypatch):
    tool = load_script("transform_audio")
    args = tool.make_parser().parse_args(["a.wav", "-o", "out"])
    assert (args.f0_source, args.f0_min, args.f0_max, args.write_f0) == ("net", 55.0, 1000.0, False)
    args = tool.make_parser().parse_args(["a.wav", "-o", "out", "--f0-source", "audio", "--f0-min", "70", "--f0-max", "500.5", "--write-f0"])
    assert (args.f0_source, args.f0_min, args.f0_max, args.write_f0) == ("audio", 70.0, 500.5, True)
    assert set(vars(args)) == set(inspect.signature(tool.main).parameters)            # every parsed name is an argument of main
    for flag, value in (("--f0-source", "file"), ("--f0-min", "0"), ("--f0-min", "nan"), ("--f0-max", "-3"), ("--f0-max", "x")):
        with pytest.raises(SystemExit) as exc:
            tool.make_parser().parse_args(["a.wav", "-o", "out", flag, value])
        assert exc.value.code == 2 and flag in capsys.readouterr().err
    from scipy.io import wavfile
    from mbexwn_vocoder_amd import batched
    from mbexwn_vocoder_amd.mel_inverter import create_synthetic_model_dir
    model = create_synthetic_model_dir(str(tmp_path / "model"), "SPEECH")
    snd = tmp_path / "a.wav"
    wavfile.write(str(snd), 24000, np.zeros(100, dtype=np.float32))
    res = run_script("transform_audio", [str(snd), "-o", str(tmp_path / "no"), "--f0-min", "600", "--f0-max", "500"])
    assert res.returncode == 1 and "--f0-min" in res.stderr and not os.path.exists(tmp_path / "no")
    seen = []

    def fake_ranks(script, argv, *rest, **kw):
        seen.append(list(argv))
        return 0

    monkeypatch.setattr(batched, "run_ranks", fake_ranks)
    for extra, want in (({"f0_source": "audio"}, ["--f0-source", "audio", "--f0-min", "55.0", "--f0-max", "1000.0"]),
                        ({"f0_source": "audio", "f0_min": 80.0, "f0_max": 400.0, "write_f0": True},
                         ["--f0-source", "audio", "--f0-min", "80.0", "--f0-max", "400.0", "--write-f0"]),
                        ({"write_f0": True, "f0_max": 600.0}, ["--f0-min", "55.0", "--f0-max", "600.0", "--write-f0"]), ({}, [])):
        with pytest.raises(SystemExit) as exc:
            tool.main([str(snd)], str(tmp_path / "out"), model_id=model, gpus=2, **extra)
        assert exc.value.code == 0
        argv = seen.pop()
        got = [aa for ii, aa in enumerate(argv) if "-f0" in aa or (ii and "--f0" in argv[ii - 1])]
        assert got == want
        rank = tool.make_parser().parse_args(argv)                       # and the rank's parser takes what the parent sends
        assert rank.f0_source == extra.get("f0_source", "net") and rank.write_f0 == extra.get("write_f0", False)


def test_resynth_mel_and_generate_mel_flags(tmp_path):
    res = run_script("resynth_mel", ["--help"])
    assert res.returncode == 0 and "--f0-dir" in res.stdout
    params = inspect.signature(load_script("resynth_mel").main).parameters
    assert params["f0_dir"].default is None
    source = open(os.path.join(BIN, "resynth_mel.py")).read()
    assert "f0_dir=f0_dir" in source and "load_contour(" in source                                        # run_job, single
    from mbexwn_vocoder_amd import batched
    tool, seen = load_script("resynth_mel"), []
    with pytest.MonkeyPatch.context() as patch:                          # ranks: what the parent of a --gpus job sends
        patch.setattr(batched, "run_ranks", lambda script, argv, *rest, **kw: seen.append(list(argv)) or 0)
        with pytest.raises(SystemExit) as exc:
            tool.main("model", ["a.mell"], "out", gpus=2, quiet=True, f0_dir="contours")
    assert exc.value.code == 0 and seen[0][seen[0].index("--f0-dir"):][:2] == ["--f0-dir", "contours"]
    assert tool.make_parser().parse_args(seen[0]).f0_dir == "contours"
    res = run_script("generate_mel", ["--help"])
    assert res.returncode == 0 and all(flag in res.stdout for flag in ("--write-f0", "--f0-min", "--f0-max"))
    params = inspect.signature(load_script("generate_mel").main).parameters
    assert (params["write_f0"].default, params["f0_min"].default, params["f0_max"].default) == (False, 55.0, 1000.0)
    res = run_script("generate_mel", ["a.wav", "-o", "o", "--f0-min", "x"])
    assert res.returncode == 2 and "--f0-min" in res.stderr
    # the host path of the tool writes NAME.f0 next to NAME.mell: one row per column, the definition's values
    from scipy.io import wavfile
    from mbexwn_vocoder_amd.fileio import load_var
    from mbexwn_vocoder_amd.mel_inverter import create_synthetic_model_dir
    model = create_synthetic_model_dir(str(tmp_path / "model"), "SPEECH")
    tt = np.arange(6000) / SR
    snd = (0.5 * np.sin(2 * np.pi * 200 * tt)).astype(np.float32)
    wavfile.write(str(tmp_path / "tone.wav"), SR, snd)
    out = str(tmp_path / "mel")
    res = run_script("generate_mel", [str(tmp_path / "tone.wav"), "-o", out, "--model_id", model, "--host", "--write-f0", "-q"])
    assert res.returncode == 0, res.stderr[-2000:]
    mell = load_var(os.path.join(out, "tone.mell"))["mell"]
    times, f0, per = f0track.read_f0(os.path.join(out, "tone.f0"), n_frames=mell.shape[1])
    want = f0track.track_f0_host(snd, np.arange(mell.shape[1]) * HOP, f0track.params(SR))
    assert np.array_equal(f0.view(np.uint32), want[0].view(np.uint32)) and np.array_equal(per.view(np.uint32), want[1].view(np.uint32))
    assert np.all(np.abs(cents(f0[4:-4], 200.0)) < 5.0)
    res = run_script("generate_mel", [str(tmp_path / "tone.wav"), "-o", out, "--model_id", model, "--host", "--write-f0", "--f0-min",
                                      "900", "--f0-max", "100"])
    assert res.returncode == 1 and "f0_min" in res.stderr
    res = run_script("generate_mel", [str(tmp_path / "tone.wav"), "-o", str(tmp_path / "plain"), "--model_id", model, "--host", "-q"])
    assert res.returncode == 0 and os.listdir(tmp_path / "plain") == ["tone.mell"]                      # without the flag: no .f0


# ------------------------------------------------------------------------------------------------------------------------
# the f0s argument
# ------------------------------------------------------------------------------------------------------------------------
def test_f0s_are_checked_before_anything_runs(tmp_path):
    from mbexwn_vocoder_amd.batched import check_f0s, run_micro_batches
    from mbexwn_vocoder_amd.mel_inverter import F0_SOURCES, MELInverter, create_synthetic_model_dir
    good = np.full(4, 100.0, np.float32)
    assert check_f0s(None, [4, 5]) is None and check_f0s([None, None], [4, 5]) is None
    out = check_f0s([good.astype(np.float64), None], [4, 5])
    assert out[0].dtype == np.float32 and out[1] is None
    for bad, what in (([good], "one entry per item"), ([good[:3], None], "one value per mel frame"),
                      ([np.array([100, 0, 100, 100.0]), None], "finite and positive"),
                      ([np.array([100, -1, 100, 100.0]), None], "finite and positive"),
                      ([np.array([100, np.nan, 100, 100.0]), None], "finite and positive"),
                      ([np.array([100, np.inf, 100, 100.0]), None], "finite and positive"),
                      ([None, np.full((1, 5), 100.0)], "one value per mel frame")):
        with pytest.raises(ValueError, match=what):
            check_f0s(bad, [4, 5])

    class Engine:                                                        # anything run_micro_batches touched would raise
        @property
        def dims(self):
            raise AssertionError("the engine was used before the check")

    mels = [np.zeros((4, 80), np.float32), np.zeros((5, 80), np.float32)]
    with pytest.raises(ValueError, match="one value per mel frame"):
        next(run_micro_batches(Engine(), mels, f0s=[good, np.full(4, 100.0)]))
    model = create_synthetic_model_dir(str(tmp_path / "model"), "SPEECH")
    inv = MELInverter.host_only(model)
    scaled = [mm[np.newaxis] for mm in mels]
    with pytest.raises(ValueError, match="finite and positive"):
        inv.synth_from_mels(scaled, f0s=[good, np.zeros(5)])
    with pytest.raises(ValueError, match="one value per mel frame"):
        inv.synth_from_mels(scaled, f0s=[good[:2], None])
    assert F0_SOURCES == ("net", "audio")
    with pytest.raises(ValueError, match="f0_source"):
        inv.transform_audio([np.zeros(10, np.float32)], [24000], ["a.wav"], f0_source="file")
    with pytest.raises(ValueError, match="f0_min"):
        inv.transform_audio([np.zeros(10, np.float32)], [24000], ["a.wav"], f0_source="audio", f0_params={"f0_min": 0})
    assert inspect.signature(inv.track_f0).parameters["on_device"].default is False
    assert inspect.signature(inv.transform_audio).parameters["f0_source"].default == "net"
