"""Time stretching on the host (no GPU needed): the time map (mbexwn_vocoder_amd/timemap.py), the host definition of the mel
analysis at arbitrary frame positions (analysis.compute_log_mel_at), the header and export of mbxw_mel_frames_at and its
refusals, and the tools' new arguments."""
import ctypes
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import frontend_reference as fr
from mbexwn_vocoder_amd import timemap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mbexwn_vocoder_amd", "bin")
H, R = 300, 24000
HOST_GEOMETRIES = ("12_4_16_5", "1200_300_2048_80")


def run_script(name, args):
    return subprocess.run([sys.executable, os.path.join(BIN, name + ".py"), *args], capture_output=True, text=True, timeout=600)


def load_script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(BIN, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------------------------------------
# timemap.centres
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, H - 1, H, H + 1, 7 * H, 7 * H + 5])
def test_factor_one_is_the_regular_frames(n):
    want = np.arange(n // H + 1) * H
    for spec in (1.0, None, 1, np.float32(1.0)):
        got = timemap.centres(n, H, R, spec)
        assert got.dtype == np.int64 and np.array_equal(got, want), spec
    assert timemap.frame_count(n, H, R, 1.0) == n // H + 1


@pytest.mark.parametrize("n", [1, H - 1, H, H + 1, 7 * H, 7 * H + 5])
def test_factor_two_holds_every_regular_centre_on_its_even_frames(n):
    cc = timemap.centres(n, H, R, 2.0)
    assert cc.size == 2 * n // H + 1
    for tt in range(n // H + 1):
        assert cc[2 * tt] == tt * H
    assert np.all(np.diff(cc) >= 0) and cc[0] == 0 and cc[-1] <= n


@pytest.mark.parametrize("factor", [0.5, 1.37])
@pytest.mark.parametrize("n", [1, H - 1, H + 1, 7 * H + 5, 24000])
def test_other_factors_follow_the_definition(factor, n):
    cc = timemap.centres(n, H, R, factor)
    frames = int(np.floor(np.float64(n) * np.float64(factor) / H)) + 1
    assert cc.dtype == np.int64 and cc.size == frames == timemap.frame_count(n, H, R, factor)
    assert np.all(np.diff(cc) >= 0) and cc.min() >= 0 and cc.max() <= n
    want = [min(max(int(np.rint(np.float64(kk * H) / np.float64(factor))), 0), n) for kk in range(frames)]
    assert cc.tolist() == want


def test_breakpoint_map_with_a_held_and_a_fast_segment():
    """1 s of sound: [0, 0.5] s at speed 1, held for 0.25 s of output, then the second half three times as fast."""
    n = R
    bp = np.array([[0.0, 0.0], [0.5, 0.5], [0.75, 0.5], [0.75 + 0.5 / 3, 1.0]])
    cc = timemap.centres(n, H, R, bp)
    frames = int(np.floor(bp[-1, 0] * R / H)) + 1
    assert cc.dtype == np.int64 and cc.size == frames == timemap.frame_count(n, H, R, bp)
    want = [min(max(int(np.rint(np.interp(kk * H / R, bp[:, 0], bp[:, 1]) * R)), 0), n) for kk in range(frames)]
    assert cc.tolist() == want
    assert np.array_equal(cc[:41], np.arange(41) * H)                         # speed 1: the regular frames
    assert np.all(cc[40:61] == 12000)                                         # held: one frame, repeated
    assert np.all(np.diff(cc[60:73]) == 3 * H)                                # three hops of the sound per frame
    assert np.all(np.diff(cc) >= 0) and cc.max() <= n
    # lists are taken as arrays; a map may end anywhere inside the sound
    assert np.array_equal(timemap.centres(n, H, R, [[0, 0], [2, 0.5]]), np.rint(np.arange(161) * H / 4).astype(np.int64))


def test_refusals():
    for bad in (0, -1.0, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="finite positive"):
            timemap.centres(1000, H, R, bad)
    n = R
    for bad, what in (([[0.1, 0.0], [1.0, 1.0]], "from 0"),                   # t_out does not start at 0
                      ([[0.0, 0.0], [0.5, 0.2], [0.5, 0.4]], "strictly increasing"),
                      ([[0.0, 0.0], [0.5, 0.4], [0.4, 0.5]], "strictly increasing"),
                      ([[0.0, 0.0], [0.5, 0.4], [1.0, 0.3]], "non-decreasing"),
                      ([[0.0, -0.1], [1.0, 0.5]], "non-decreasing within"),
                      ([[0.0, 0.0], [1.0, 1.0 + 1e-3]], "non-decreasing within"),   # behind the sound's end
                      ([[0.0, 0.0], [1.0, float("nan")]], "finite"),
                      ([[0.0, 0.0, 0.0]], r"\(m, 2\)"), ([0.0, 1.0], r"\(m, 2\)"), (np.zeros((0, 2)), r"\(m, 2\)")):
        with pytest.raises(ValueError, match=what):
            timemap.centres(n, H, R, bad)
    # the engine's limit of 2^24 - 1 sub-band rows an item, named in frames
    limit = ((1 << 24) - 1) // 20
    with pytest.raises(ValueError, match=f"limit of {limit} frames"):
        timemap.centres(R, H, R, 1e9, rows_per_frame=20)
    with pytest.raises(ValueError, match=f"limit of {limit} frames"):
        timemap.centres(limit * H, H, R, 1.0, rows_per_frame=20)              # limit + 1 frames
    assert timemap.frame_count(limit * H - 1, H, R, 1.0, rows_per_frame=20) == limit
    with pytest.raises(ValueError, match=f"limit of {limit} frames"):
        timemap.centres(R, H, R, [[0.0, 0.0], [1e9, 1.0]], rows_per_frame=20)
    with pytest.raises(ValueError, match=f"limit of {(1 << 24) - 1} frames"):
        timemap.centres(R, H, R, 1e300)
    assert timemap.per_item(2.0, 3) == [2.0] * 3 and timemap.per_item(None, 2) == [None, None]
    assert timemap.per_item([1.0, None], 2) == [1.0, None]
    with pytest.raises(ValueError, match="one entry per item"):
        timemap.per_item([1.0], 2)


# ------------------------------------------------------------------------------------------------------------------------
# analysis.compute_log_mel_at
# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=HOST_GEOMETRIES)
def geometry(request):
    cfg = fr.MEL_GEOMETRIES[request.param]
    hop = int(cfg["hop_size"])
    nn = 9 * hop + hop // 2 + 1
    return cfg, np.random.default_rng(41).normal(size=(2, nn)).astype(np.float32)


def test_regular_centres_give_the_bits_of_compute_log_mel(geometry):
    from mbexwn_vocoder_amd.analysis import compute_log_mel, compute_log_mel_at
    cfg, snd = geometry
    want, rate = compute_log_mel(snd, cfg)
    cc = timemap.centres(snd.shape[1], cfg["hop_size"], cfg["sample_rate"], None)
    got, got_rate = compute_log_mel_at(snd, cc, cfg)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape and got_rate == rate
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # one row of centres per item, a 1-D sound, and clipping of what lies outside [0, n]
    both, _ = compute_log_mel_at(snd, np.stack((cc, cc)), cfg)
    one, _ = compute_log_mel_at(snd[1], cc, cfg)
    assert np.array_equal(both, want) and np.array_equal(one[0], want[1])
    edge, _ = compute_log_mel_at(snd, np.array([-5, 0, snd.shape[1], snd.shape[1] + 1000]), cfg)
    assert np.array_equal(edge[:, 0], edge[:, 1]) and np.array_equal(edge[:, 2], edge[:, 3])
    with pytest.raises(ValueError, match="integer"):
        compute_log_mel_at(snd, cc.astype(np.float64), cfg)


def test_a_shifted_centre_is_the_regular_frame_of_the_shifted_sound(geometry):
    """Centre t * hop + d: row t of compute_log_mel(x[d:]), for the frames the padding does not reach on either side."""
    from mbexwn_vocoder_amd.analysis import compute_log_mel, compute_log_mel_at
    cfg, snd = geometry
    win, hop = int(cfg["win_size"]), int(cfg["hop_size"])
    for dd in (1, hop - 1):
        want, _ = compute_log_mel(snd[:, dd:], cfg)
        frames = want.shape[1]
        got, _ = compute_log_mel_at(snd, np.arange(frames) * hop + dd, cfg)
        inner = [tt for tt in range(frames) if tt * hop - win // 2 >= 0 and tt * hop - win // 2 + win <= snd.shape[1] - dd]
        assert len(inner) >= 4
        assert np.array_equal(got[:, inner].view(np.uint32), want[:, inner].view(np.uint32)), dd
        assert not np.array_equal(got[:, inner], compute_log_mel(snd, cfg)[0][:, inner])        # and not the unshifted frame


# ------------------------------------------------------------------------------------------------------------------------
# header, symbol list, refusals
# ------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_point_and_the_library_exports_it(tmp_path):
    """(that the header declares exactly these names, no other header does and the library exports them: test_abi_headers.py)"""
    from mbexwn_vocoder_amd import abi
    from mbexwn_vocoder_amd.build import HEADERS, SOURCES
    text = open(os.path.join(ROOT, "include", "mbexwn_warp.h")).read()
    assert "THE PROMISE" in text and "bit for bit" in text and "Refused" in text and "centres" in text
    assert abi.symbols("mbexwn_warp.h") == ["mbxw_mel_frames_at"]
    assert any(hh.endswith("mbexwn_warp.h") for hh in HEADERS) and "mel_warp.hip" in SOURCES
    assert abi.MBX_ABI_VERSION == 11
    src = tmp_path / "use.c"
    src.write_text('#include "mbexwn_warp.h"\nint main(void){ (void)mbxw_mel_frames_at; return 0; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)
    # mel_frame.h stays the one place of a frame's arithmetic: the new kernel calls its body and has no transform of its own
    kernel = open(os.path.join(ROOT, "mbexwn_vocoder_amd", "csrc", "mel_warp.hip")).read()
    assert "mel_frame_body(" in kernel and "fft_lds<" not in kernel and "logf(" not in kernel


def test_entry_point_refuses_bad_arguments_before_touching_the_device():
    """mbxw_mel_frames_at checks every argument on the host and returns MBX_ERR_INVALID_ARGUMENT without a launch."""
    from mbexwn_vocoder_amd import engine
    from mbexwn_vocoder_amd.build import build_library
    build_library()
    lib = engine.load_library()
    fake = ctypes.c_void_p(256)                              # never dereferenced: the checks fail first
    pointers = ("audio", "n_samples", "centres", "n_frames", "window", "twiddle", "basis", "bin_lo", "bin_hi", "out")

    def call(stride=4096, batch=2, max_frames=8, win=1200, fft_size=2048, n_mels=80, **kw):
        pp = {name: kw.get(name, fake) for name in pointers}
        return lib.mbxw_mel_frames_at(pp["audio"], stride, batch, pp["n_samples"], pp["centres"], pp["n_frames"], max_frames,
                                      win, fft_size, n_mels, pp["window"], pp["twiddle"], pp["basis"], pp["bin_lo"],
                                      pp["bin_hi"], ctypes.c_float(1e-7), pp["out"], None)

    def why():
        return lib.mbx_last_error().decode()

    for name in pointers:
        assert call(**{name: None}) == 1 and why().startswith("mel frames at:") and "null" in why(), name
    for kw, what in (({"fft_size": 4}, "fft_size"), ({"fft_size": 4096}, "fft_size"), ({"fft_size": 1536}, "fft_size"),
                     ({"fft_size": 0}, "fft_size"), ({"win": 1}, "win"), ({"win": 2049}, "win"),
                     ({"win": 600, "fft_size": 512}, "win"), ({"n_mels": 0}, "n_mels"), ({"max_frames": 0}, "max_frames"),
                     ({"stride": 0}, "stride"), ({"stride": -4}, "stride"), ({"batch": 65536}, "batch"), ({"batch": -1}, "batch")):
        assert call(**kw) == 1 and why().startswith("mel frames at:") and what in why(), kw
    assert call(batch=0) == 0                                # an empty batch is nothing to do


# ------------------------------------------------------------------------------------------------------------------------
# the tools
# ------------------------------------------------------------------------------------------------------------------------
def test_transform_audio_arguments(tmp_path, capsys):
    tool = load_script("transform_audio")
    args = tool.make_parser().parse_args(["a.wav", "-o", "out"])
    assert args.time_stretch == 1.0 and args.time_stretch_file is None
    args = tool.make_parser().parse_args(["a.wav", "-o", "out", "--time-stretch", "1.5", "--time-stretch-file", "s.txt"])
    assert args.time_stretch == 1.5 and args.time_stretch_file == "s.txt"
    import inspect
    assert set(vars(args)) == set(inspect.signature(tool.main).parameters)
    for value in ("0", "-2", "nan", "inf", "x"):
        with pytest.raises(SystemExit) as exc:
            tool.make_parser().parse_args(["a.wav", "-o", "out", "--time-stretch", value])
        assert exc.value.code == 2 and "--time-stretch" in capsys.readouterr().err
    # the list: the format and the parser of --transposition-file; a bad line ends the tool before torch, named by its number
    from scipy.io import wavfile
    from mbexwn_vocoder_amd.batched import file_stretches, read_transposition_file
    snd = tmp_path / "a.wav"
    wavfile.write(str(snd), 24000, np.zeros(100, dtype=np.float32))
    listing = tmp_path / "stretch.txt"
    listing.write_text("# per file\na.wav 1.5\nsub/b.wav 0.5  # twice as fast\n")
    assert file_stretches(["x/a.wav", "b.wav", "c.wav"], 2.0, read_transposition_file(str(listing))) == [1.5, 0.5, 2.0]
    assert file_stretches(["a.wav"]) == [1.0]
    with pytest.raises(ValueError, match="finite and positive"):
        file_stretches(["a.wav"], 0.0)
    out = str(tmp_path / "out")
    for text, what in (("a.wav 1\nb.wav 0\n", "finite and positive"), ("a.wav 1\nb.wav\n", "basename factor"),
                       ("a.wav 1\nb.wav fast\n", "float")):
        listing.write_text(text)
        res = run_script("transform_audio", [str(snd), "-o", out, "--time-stretch-file", str(listing)])
        assert res.returncode == 1 and what in res.stderr and "stretch.txt:2:" in res.stderr, res.stderr[-2000:]
    res = run_script("transform_audio", [str(snd), "-o", out, "--time-stretch-file", str(tmp_path / "none.txt")])
    assert res.returncode == 1 and "none.txt" in res.stderr
    assert not os.path.exists(out)
    res = run_script("generate_mel", ["--help"])
    assert res.returncode == 0 and "--time-stretch" in res.stdout


def test_rank_plan_weighs_a_file_by_its_stretched_duration(tmp_path):
    """A 1 s file at factor 4 outweighs a 3 s file at factor 1; without factors the plan is the one by duration.  A file
    whose stretched length exceeds the engine's limit is skipped by the parent."""
    from scipy.io import wavfile
    from mbexwn_vocoder_amd.batched import plan_audio_ranks
    names = []
    for name, seconds in (("three.wav", 3.0), ("one.wav", 1.0), ("two.wav", 2.0), ("half.wav", 0.5)):
        names.append(str(tmp_path / name))
        wavfile.write(names[-1], 8000, np.zeros(int(seconds * 8000), np.float32))
    plain = plan_audio_ranks(names, 2)
    assert plain["shards"] == [[0, 3], [2, 1]] and plain["skipped"] == []        # 3 + 0.5 | 2 + 1
    assert plan_audio_ranks(names, 2, stretches=[1.0] * 4) == plain
    warped = plan_audio_ranks(names, 2, stretches=[1.0, 4.0, 1.0, 1.0])
    assert warped["shards"] == [[1, 3], [0, 2]]                                  # 4 + 0.5 | 3 + 2
    assert warped["files"] == names
    limited = plan_audio_ranks(names, 2, stretches=[1.0, 1e9, 1.0, 1.0], frame_limit=(300, 24000, 20))
    assert limited["files"] == [names[0], names[2], names[3]]
    assert [os.path.basename(ff) for ff, _ in limited["skipped"]] == ["one.wav"] and "frames" in limited["skipped"][0][1]


def test_generate_mels_on_the_host_with_time_maps(tmp_path):
    """generate_mels(on_device=False, time_maps=[2.0]): every second column is the unstretched file's column; the None item
    is today's; generate_mel.py --host --time-stretch 2 writes that dictionary."""
    from mbexwn_vocoder_amd.analysis import generate_mels, resampled_length
    from mbexwn_vocoder_amd.config import read_config
    from mbexwn_vocoder_amd.fileio import load_var
    from mbexwn_vocoder_amd.mel_inverter import create_synthetic_model_dir
    from scipy.io import wavfile
    model = create_synthetic_model_dir(str(tmp_path / "model"), "SPEECH")
    pre = read_config(config_file=os.path.join(model, "config.yaml"))["preprocess_config"]
    rng = np.random.default_rng(5)
    snd, other = (0.1 * rng.normal(size=4000)).astype(np.float32), (0.1 * rng.normal(size=3000)).astype(np.float32)
    plain = generate_mels([snd, other], [24000, 16000], pre, on_device=False)
    assert [dd["mell"].tobytes() for dd in generate_mels([snd, other], [24000, 16000], pre, on_device=False,
                                                         time_maps=[None, None])] == [dd["mell"].tobytes() for dd in plain]
    got = generate_mels([snd, other], [24000, 16000], pre, on_device=False, time_maps=[2.0, None])
    frames = plain[0]["mell"].shape[1]
    assert frames == 4000 // 300 + 1 and got[0]["mell"].shape == (80, 2 * 4000 // 300 + 1)
    assert np.array_equal(got[0]["mell"][:, 0:2 * frames:2].view(np.uint32), plain[0]["mell"].view(np.uint32))
    assert not np.array_equal(got[0]["mell"][:, 1], plain[0]["mell"][:, 0])
    assert got[1]["mell"].tobytes() == plain[1]["mell"].tobytes()
    assert set(got[0]) == set(plain[0]) and all(np.array_equal(got[0][kk], plain[0][kk]) for kk in plain[0] if kk != "mell")
    # a resampled item: its centres come from the resampled length
    fast = generate_mels([other], [16000], pre, on_device=False, time_maps=[0.5])[0]["mell"]
    n_model = resampled_length(3000, 16000, 24000)
    assert n_model == 4500 and fast.shape[1] == int(n_model * 0.5 // 300) + 1
    assert np.array_equal(fast, plain[1]["mell"][:, 0:2 * fast.shape[1]:2])
    with pytest.raises(ValueError, match="finite positive"):
        generate_mels([snd], [24000], pre, on_device=False, time_maps=[0.0])
    with pytest.raises(ValueError, match="one entry per item"):
        generate_mels([snd], [24000], pre, on_device=False, time_maps=[1.0, 2.0])
    wav = tmp_path / "snd.wav"
    wavfile.write(str(wav), 24000, snd)
    out = str(tmp_path / "mells")
    res = run_script("generate_mel", [str(wav), "-o", out, "--model_id", model, "--host", "--time-stretch", "2", "-q"])
    assert res.returncode == 0, res.stderr[-2000:]
    saved = load_var(os.path.join(out, "snd.mell"))
    assert list(saved) == list(got[0]) and np.array_equal(saved["mell"], got[0]["mell"])
    for bad in ("0", "nan", "1e9"):
        res = run_script("generate_mel", [str(wav), "-o", out, "--model_id", model, "--host", "--time-stretch", bad, "-q"])
        assert res.returncode == 1 and "generate_mel::error::" in res.stderr, (bad, res.stderr[-2000:])
