"""Formant shift on the host (no GPU): the numpy definition of the envelope warp (envelope.warp_envelope_host), the centre
table, the factor checks of MELInverter, the tools' flags and their way to the ranks of a --gpus job, the header and the
ctypes mirror of the extended mbx_forward_options, and the factor rows of the streaming driver."""
import ctypes
import importlib.util
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from mbexwn_vocoder_amd import engine
from mbexwn_vocoder_amd.envelope import channel_centres, warp_envelope_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mbexwn_vocoder_amd", "bin")
# (mel_channels, fmin, fmax) of the configurations the definition was stated for
TABLES = [(80, 0.0, 12000.0), (80, 0.0, 8000.0), (20, 50.0, 4000.0), (7, 0.0, 12000.0)]


def load_script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(BIN, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_script(name, args):
    return subprocess.run([sys.executable, os.path.join(BIN, name + ".py"), *args], capture_output=True, text=True, timeout=600)


def centres_of(n_mels, fmin, fmax):
    return channel_centres({"mel_channels": n_mels, "fmin": fmin, "fmax": fmax, "sample_rate": 24000})


def bits(array):
    return np.ascontiguousarray(array, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------------
# the definition
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", TABLES, ids=[f"{nn}_{int(lo)}_{int(hi)}" for nn, lo, hi in TABLES])
def test_centres_are_strictly_increasing(table):
    from mbexwn_vocoder_amd.analysis import mel_frequencies
    n_mels, fmin, fmax = table
    cc = centres_of(*table)
    assert cc.dtype == np.float32 and cc.shape == (n_mels,) and cc.flags["C_CONTIGUOUS"]
    assert np.all(np.diff(cc) > 0) and fmin < cc[0] and cc[-1] < fmax
    assert np.array_equal(cc, mel_frequencies(n_mels + 2, fmin, fmax)[1:-1].astype(np.float32))
    # fmax: null in a configuration means half the sample rate, as the mel basis reads it
    assert np.array_equal(channel_centres({"mel_channels": n_mels, "fmin": fmin, "fmax": None, "sample_rate": 2 * fmax}), cc)


def test_centres_refuse_a_single_channel():
    with pytest.raises(ValueError, match="at least two"):
        centres_of(1, 0.0, 12000.0)


def test_factor_one_copies_the_bits():
    cc = centres_of(*TABLES[0])
    rng = np.random.default_rng(1)
    mel = rng.normal(-5.0, 2.0, size=(2, 5, 80)).astype(np.float32)
    mel[0, 0, 0], mel[0, 0, -1], mel[1, 2, 40], mel[1, 4, -1] = -0.0, -0.0, -0.0, np.float32(1e-42)      # (a subnormal too)
    for factors in (1.0, np.ones((2, 5), dtype=np.float32), np.ones(5)):
        out = warp_envelope_host(mel, factors, cc)
        assert out.dtype == np.float32 and out.shape == mel.shape and np.array_equal(bits(out), bits(mel))
    # mixed per frame: the frames with 1 are copies, the others are not; n_frames leaves the rows behind an item's end alone
    factors = np.asarray([[1.0, 1.25, 1.0, 0.8, 1.0], [2.0, 1.0, 1.0 + 2.0 ** -23, 1.0, 0.5]], dtype=np.float32)
    out = warp_envelope_host(mel, factors, cc)
    same = factors == 1.0
    assert np.array_equal(bits(out[same]), bits(mel[same]))
    assert all(not np.array_equal(out[bb, tt], mel[bb, tt]) for bb, tt in zip(*np.nonzero(~same)))
    cut = warp_envelope_host(mel, factors, cc, n_frames=[3, 0])
    assert np.array_equal(bits(cut[0, :3]), bits(out[0, :3])) and np.array_equal(bits(cut[0, 3:]), bits(mel[0, 3:]))
    assert np.array_equal(bits(cut[1]), bits(mel[1]))
    for bad in (mel[..., :79], mel[0, 0, :]):
        with pytest.raises(ValueError):
            warp_envelope_host(bad, 1.5, cc)


@pytest.mark.parametrize("table", TABLES, ids=[f"{nn}_{int(lo)}_{int(hi)}" for nn, lo, hi in TABLES])
def test_edges_are_held(table):
    """phi = 2 reads at c[m] / 2: every channel whose half frequency lies below c[0] takes x[0]; phi = 0.5 reads at 2 c[m]:
    every channel at or above c[n-1] / 2 takes x[n-1] -- exactly, whatever lies between."""
    cc = centres_of(*table)
    n = cc.shape[0]
    rng = np.random.default_rng(2)
    row = rng.normal(-5.0, 2.0, size=(1, n)).astype(np.float32)
    up, down = warp_envelope_host(row, 2.0, cc)[0], warp_envelope_host(row, 0.5, cc)[0]
    low = cc / np.float32(2.0) < cc[0]
    high = cc / np.float32(0.5) >= cc[-1]
    assert low[0] and high[-1]
    assert np.all(bits(up[low]) == bits(row[0, 0])) and np.all(bits(down[high]) == bits(row[0, -1]))
    # between the edges the value lies between its two neighbours of the old row
    f = cc / np.float32(2.0)
    for m in np.nonzero(~low)[0]:
        i = np.searchsorted(cc, f[m], side="right") - 1
        assert min(row[0, i], row[0, i + 1]) <= up[m] <= max(row[0, i], row[0, i + 1])
    # the last channel read at exactly c[n-1] (phi = 1 + 2^-23 rounds c / phi to the float32 below c: not this case), and
    # a frequency equal to a centre reads that centre's value
    pair = np.asarray([[3.0, 7.0]], dtype=np.float32)
    assert np.array_equal(warp_envelope_host(pair, 0.5, np.asarray([100.0, 200.0], dtype=np.float32))[0], [7.0, 7.0])
    assert np.array_equal(warp_envelope_host(pair, 2.0, np.asarray([100.0, 200.0], dtype=np.float32))[0], [3.0, 3.0])
    assert np.array_equal(warp_envelope_host(pair, 1.25, np.asarray([100.0, 200.0], dtype=np.float32))[0],
                          [3.0, np.float32(3.0) + np.float32(0.6) * np.float32(4.0)])         # f = 160: w = 0.6


@pytest.mark.parametrize("table", [TABLES[0], TABLES[2]], ids=["80_0_12000", "20_50_4000"])
def test_a_row_linear_in_hz_is_reproduced(table):
    """x[m] = a + b c[m] warped by any factor is a + b f inside the table.  The tolerance, derived for u = 2^-24 (float32
    unit roundoff), M = max |x| and D = max |x[i+1] - x[i]|, against the line evaluated in float64 at the float32 f:
      - x[i] and x[i+1] are float32 roundings of the line, u M each, combined with weights 1 - w and w: u M;
      - w = (f - c[i]) / (c[i+1] - c[i]) carries three relative roundings and w <= 1: 3 u D on w (x[i+1] - x[i]);
      - the difference and the product round once each: 2 u D;   - the sum rounds once: u M.
    Together 2 u M + 5 u D, which is at most 3 u M -- three roundings on values of the row's magnitude -- when D <= M / 5
    (asserted; terms in u^2 are 1e-7 of that)."""
    cc = centres_of(*table)
    a, b = -8.0, 6.0 / float(cc[-1])
    line = lambda f: a + b * np.asarray(f, dtype=np.float64)                                         # noqa: E731
    row = line(cc).astype(np.float32)[None]
    big, step = float(np.max(np.abs(row))), float(np.max(np.abs(np.diff(row[0].astype(np.float64)))))
    assert step <= big / 5
    tol = 3 * 2.0 ** -24 * big
    checked = 0
    for phi in (0.5, 0.8, 0.9, 1.1, 1.25, 2.0, 1.0 + 2.0 ** -23, 1.37):
        f = cc / np.float32(phi)
        inside = (f >= cc[0]) & (f <= cc[-1])
        out = warp_envelope_host(row, phi, cc)[0]
        err = np.max(np.abs(out[inside].astype(np.float64) - line(f[inside])))
        assert err <= tol, (phi, err, tol)
        checked += int(inside.sum())
    assert checked > 4 * cc.shape[0]


# ------------------------------------------------------------------------------------------------------------------------
# MELInverter
# ------------------------------------------------------------------------------------------------------------------------
def test_check_factors_and_the_inverter_arguments(tmp_path):
    from mbexwn_vocoder_amd.mel_inverter import MELInverter, check_factors, create_synthetic_model_dir
    assert check_factors(1.2, 3, "formant") == [1.2] * 3 and check_factors([1, 2], 2, "formant") == [1.0, 2.0]
    for bad in (0, -1.5, float("nan"), float("inf"), [1.0, 0.0], [1.0, -2.0], [1.0, float("nan")], [1.0, float("inf")]):
        with pytest.raises(ValueError, match="formant must be finite and positive"):
            check_factors(bad, 2, "formant")
    for bad in ([1.0], [1.0, 1.0, 1.0], [[1.0, 1.0]]):
        with pytest.raises(ValueError, match="formant must be one factor or one per item"):
            check_factors(bad, 2, "formant")
    with pytest.raises(ValueError, match="transposition must be finite"):
        check_factors(0, 2)                                              # the name it had stays the default
    inv = MELInverter.host_only(create_synthetic_model_dir(str(tmp_path / "model"), "SPEECH"))
    mel = np.zeros((1, 4, 80), dtype=np.float32)
    for bad in (0.0, -1.0, float("nan"), np.ones(3), np.asarray([1.0, 1.0, 0.0, 1.0])):
        with pytest.raises(ValueError, match="formant"):
            inv.synth_from_mel(mel, formant=bad)
        with pytest.raises(ValueError, match="formant"):
            inv.synth_from_mels([mel], formants=[bad])
    with pytest.raises(ValueError, match="one formants entry per mel"):
        inv.synth_from_mels([mel], formants=[1.2, 1.2])
    for bad in (1.2, [1.2, 1.2]):
        with pytest.raises(ValueError, match="formant takes one entry per sound"):
            inv.transform_audio([np.zeros(10, np.float32)], [24000], ["a.wav"], formant=bad)
    for name in ("synth_from_mel", "transform_audio"):
        assert inspect.signature(getattr(MELInverter, name)).parameters["formant"].default is None
    assert inspect.signature(MELInverter.synth_from_mels).parameters["formants"].default is None
    # the model's centre table is the one of its analysis
    cc = channel_centres(inv.preprocess_config)
    assert cc.shape == (80,) and np.array_equal(cc, centres_of(80, inv.preprocess_config["fmin"], inv.preprocess_config["fmax"]))


# ------------------------------------------------------------------------------------------------------------------------
# the tools
# ------------------------------------------------------------------------------------------------------------------------
def test_transform_audio_flags(tmp_path, capsys, monkeypatch):
    tool = load_script("transform_audio")
    args = tool.make_parser().parse_args(["a.wav", "-o", "out"])
    assert args.formant_shift == 1.0 and args.formant_shift_file is None
    args = tool.make_parser().parse_args(["a.wav", "-o", "out", "--formant-shift", "1.2", "--formant-shift-file", "f.txt"])
    assert args.formant_shift == 1.2 and args.formant_shift_file == "f.txt"
    assert set(vars(args)) == set(inspect.signature(tool.main).parameters)
    for value in ("0", "-2", "nan", "inf", "x"):
        with pytest.raises(SystemExit) as exc:
            tool.make_parser().parse_args(["a.wav", "-o", "out", "--formant-shift", value])
        assert exc.value.code == 2 and "--formant-shift" in capsys.readouterr().err
    # forwarded to the ranks of a --gpus job: the factor when it is not 1, the list whenever it is given
    from scipy.io import wavfile
    from mbexwn_vocoder_amd import batched
    from mbexwn_vocoder_amd.mel_inverter import create_synthetic_model_dir
    model = create_synthetic_model_dir(str(tmp_path / "model"), "SPEECH")
    snd = tmp_path / "a.wav"
    wavfile.write(str(snd), 24000, np.zeros(100, dtype=np.float32))
    listing = tmp_path / "shift.txt"
    listing.write_text("a.wav 0.9\n")
    seen = []

    def fake_ranks(script, argv, *rest, **kw):
        seen.append(list(argv))
        return 0

    monkeypatch.setattr(batched, "run_ranks", fake_ranks)
    for extra, want in (({"formant_shift": 1.2}, ["--formant-shift", "1.2"]),
                        ({"formant_shift_file": str(listing)}, ["--formant-shift-file", str(listing)]), ({}, [])):
        with pytest.raises(SystemExit) as exc:
            tool.main([str(snd)], str(tmp_path / "out"), model_id=model, gpus=2, **extra)
        assert exc.value.code == 0
        argv = seen.pop()
        got = [aa for ii, aa in enumerate(argv) if aa.startswith("--formant") or (ii and argv[ii - 1].startswith("--formant"))]
        assert got == want
        tool.make_parser().parse_args(argv)                              # and the rank's parser takes what the parent sends


def test_formant_shift_file_rejects_what_the_transposition_file_rejects(tmp_path):
    from scipy.io import wavfile
    from mbexwn_vocoder_amd.batched import file_factors, read_transposition_file
    snd = tmp_path / "a.wav"
    wavfile.write(str(snd), 24000, np.zeros(100, dtype=np.float32))
    listing = tmp_path / "shift.txt"
    listing.write_text("# per file\na.wav 1.2\nsub/b.wav 0.8  # down\n")
    table = read_transposition_file(str(listing))
    assert file_factors(["x/a.wav", "b.wav", "c.wav"], 1.1, table, what="formant shift") == [1.2, 0.8, 1.1]
    with pytest.raises(ValueError, match="formant shift must be finite and positive"):
        file_factors(["a.wav"], 0.0, what="formant shift")
    out = str(tmp_path / "out")
    for text, what in (("a.wav 1\nb.wav 0\n", "finite and positive"), ("a.wav 1\nb.wav -1.5\n", "finite and positive"),
                       ("a.wav 1\nb.wav nan\n", "finite"), ("a.wav 1\nb.wav\n", "basename factor"),
                       ("a.wav 1\nb.wav 1 2\n", "basename factor"), ("a.wav 1\nb.wav fast\n", "float"),
                       ("a.wav 1\nx/a.wav 2\n", "twice")):
        listing.write_text(text)
        res = run_script("transform_audio", [str(snd), "-o", out, "--formant-shift-file", str(listing)])
        assert res.returncode == 1 and what in res.stderr and "shift.txt:2:" in res.stderr, res.stderr[-2000:]
    res = run_script("transform_audio", [str(snd), "-o", out, "--formant-shift-file", str(tmp_path / "none.txt")])
    assert res.returncode == 1 and "none.txt" in res.stderr
    assert not os.path.exists(out)


def test_resynth_mel_and_stream_transpose_flags():
    res = run_script("resynth_mel", ["--help"])
    assert res.returncode == 0 and "--formant-shift" in res.stdout
    for value in ("0", "-1", "nan", "x"):
        res = run_script("resynth_mel", ["model", "-i", "a.mell", "--formant-shift", value])
        assert res.returncode == 2 and "--formant-shift" in res.stderr, value
    params = inspect.signature(load_script("resynth_mel").main).parameters
    assert params["formant_shift"].default is None
    source = open(os.path.join(BIN, "resynth_mel.py")).read()
    assert "formant=formant_shift" in source                                                            # run_job
    from mbexwn_vocoder_amd import batched
    tool, seen = load_script("resynth_mel"), []
    with pytest.MonkeyPatch.context() as patch:                          # ranks: what the parent of a --gpus job sends
        patch.setattr(batched, "run_ranks", lambda script, argv, *rest, **kw: seen.append(list(argv)) or 0)
        with pytest.raises(SystemExit) as exc:
            tool.main("model", ["a.mell"], "out", gpus=2, quiet=True, formant_shift=1.2)
    assert exc.value.code == 0 and seen[0][seen[0].index("--formant-shift"):][:2] == ["--formant-shift", repr(1.2)]
    assert tool.make_parser().parse_args(seen[0]).formant_shift == 1.2
    res = run_script("stream_transpose", ["--help"])
    assert res.returncode == 0 and "--formant-shift" in res.stdout
    tool = load_script("stream_transpose")
    assert inspect.signature(tool.main).parameters["formant_shift"].default == 1.0
    assert inspect.signature(tool.stream_file).parameters["formant"].default is None
    res = run_script("stream_transpose", ["missing.wav", "-o", "o.wav", "--formant-shift", "x"])
    assert res.returncode == 2 and "--formant-shift" in res.stderr

    class Live:
        """records what stream_file hands to push_audio"""
        def __init__(self):
            self.pushes, self.left = [], 2

        def open(self, *args, **kw):
            pass

        def push_audio(self, sid, samples, **kw):
            self.pushes.append(kw)

        def tick(self):
            return {}

        def finished(self, sid):
            return True

        def close(self, sid):
            pass

    live = Live()
    tool.stream_file(live, np.zeros(250, dtype=np.float32), 100, 1.5, formant=1.3)
    assert [kw["formant"] for kw in live.pushes] == [1.3] * 3 and live.pushes[-1]["last"]
    live = Live()
    tool.stream_file(live, np.zeros(250, dtype=np.float32), 100, 1.5)
    assert all("formant" not in kw for kw in live.pushes)               # without the flag: the calls of before


# ------------------------------------------------------------------------------------------------------------------------
# header, symbol list, struct mirror, refusals
# ------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_point_and_the_library_exports_it(tmp_path):
    """(that the header declares exactly these names, no other header does and the library exports them: test_abi_headers.py)"""
    from mbexwn_vocoder_amd import abi
    from mbexwn_vocoder_amd.build import HEADERS, SOURCES
    text = open(os.path.join(ROOT, "include", "mbexwn_envelope.h")).read()
    assert "THE DEFINITION" in text and "Refused" in text and "not compensated" in text
    assert abi.symbols("mbexwn_envelope.h") == ["mbxe_warp_envelope", "mbxe_forward"]
    assert any(hh.endswith("mbexwn_envelope.h") for hh in HEADERS) and "mel_envelope.hip" in SOURCES
    assert abi.MBX_ABI_VERSION == 11
    src = tmp_path / "use.c"
    src.write_text('#include "mbexwn_envelope.h"\nint main(void){ (void)mbxe_warp_envelope; (void)mbxe_forward; return 0; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)
    # every operation separately rounded: contraction is off for the file, and it calls no fused multiply-add, log or exp
    kernel = open(os.path.join(ROOT, "mbexwn_vocoder_amd", "csrc", "mel_envelope.hip")).read()
    body = re.sub(r"//[^\n]*", "", kernel)
    assert "#pragma clang fp contract(off)" in body
    assert not re.search(r"\b(fmaf?|__fmaf_rn|logf?|expf?|exp2f|log2f)\s*\(", body)


def test_entry_point_refuses_bad_arguments_before_touching_the_device():
    from mbexwn_vocoder_amd.build import build_library
    build_library()
    lib = engine.load_library()
    fake = 1 << 20                                                       # never dereferenced: the checks fail first
    pointers = ("mel", "centres", "factors", "out")

    def call(stride=8 * 80, batch=2, max_frames=8, n_mels=80, n_frames=fake, **kw):
        pp = {name: kw.get(name, fake * (2 + ii * 16)) for ii, name in enumerate(pointers)}
        return lib.mbxe_warp_envelope(pp["mel"], stride, batch, n_frames, max_frames, n_mels, pp["centres"], pp["factors"],
                                      pp["out"], None)

    def why():
        return lib.mbx_last_error().decode()

    for name in pointers:
        assert call(**{name: None}) == 1 and why().startswith("warp envelope:") and "null" in why(), name
    for kw, what in (({"n_mels": 1}, "n_mels"), ({"n_mels": 0}, "n_mels"), ({"n_mels": 4097, "stride": 8 * 4097}, "n_mels"),
                     ({"max_frames": 0}, "max_frames"), ({"max_frames": -3}, "max_frames"), ({"batch": -1}, "batch"),
                     ({"batch": 65536}, "batch"), ({"stride": 8 * 80 - 1}, "stride"),
                     ({"out": 2 * fake}, "alias"), ({"out": 2 * fake + 4 * (8 * 80 + 7 * 80)}, "alias"),
                     ({"out": 2 * fake - 4 * (8 * 80 + 8 * 80) + 4}, "alias")):
        assert call(**kw) == 1 and why().startswith("warp envelope:") and what in why(), (kw, why())
    assert call(batch=0) == 0 and call(batch=0, n_frames=None) == 0      # an empty batch is nothing to do


def test_forward_options_mirror_matches_c(tmp_path):
    """sizeof(mbx_forward_options) and every field offset as gcc lays the header out, against the ctypes mirror.  The formant
    shift adds nothing to the struct (its three pointers are arguments of mbxe_forward): f0_item_mask stays its last field."""
    opt = engine.mbx_forward_options
    names = [name for name, _ in opt._fields_]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mbexwn_envelope.h"\nint main(void){\n'
                   'printf("%zu %d\\n", sizeof(mbx_forward_options), MBX_ABI_VERSION);\n'
                   + "".join(f'printf("%zu\\n", offsetof(mbx_forward_options, {name}));\n' for name in names)
                   + 'return 0;}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    size, abi = (int(vv) for vv in lines[0].split())
    assert size == ctypes.sizeof(opt) and abi == 11
    assert [int(vv) for vv in lines[1:1 + len(names)]] == [getattr(opt, name).offset for name in names]
    assert names[-3:] == ["f0_frames", "f0_scale", "f0_item_mask"]
    assert ctypes.sizeof(opt) == opt.f0_item_mask.offset + ctypes.sizeof(ctypes.c_void_p)


def test_forward_checks_the_factor_rows_on_the_host():
    """MBExWNEngine.forward without a library handle: malformed factor rows are refused before any call, and the options of
    a call are those it has without the shift (the three pointers are arguments of mbxe_forward, not fields)."""
    import torch
    from test_forward_options_host import B, T, _HostEngine
    eng = _HostEngine()
    mel = torch.zeros((B, T, 80), dtype=torch.float32)
    noise = torch.zeros((B, T * eng.dims.wn_in_rows_per_frame), dtype=torch.float32)
    rows = torch.ones((B, T), dtype=torch.float32)
    for bad in (rows[:, :-1], rows.reshape(-1), rows.double(), rows.numpy()):
        with pytest.raises(ValueError, match="formant must be a float32 tensor"):
            eng.forward(mel, noise=noise, formant=bad)
    assert "formant" not in inspect.signature(eng._forward_options).parameters
    assert engine.load_library().mbxe_forward.argtypes[9]._type_ is engine.mbx_forward_options


# ------------------------------------------------------------------------------------------------------------------------
# the streaming driver: the factor travels with its frame
# ------------------------------------------------------------------------------------------------------------------------
class _FormantFakeEngine:
    """CPU test double of the engine surface the streaming driver uses: the audio of frame t is (sum(mel[t]) + noise[t * spf])
    * formant[t] on every sample of the frame (formant[t] = 1 without the argument).  Records the keywords of every call."""

    def __init__(self):
        import torch
        from mbexwn_vocoder_amd.config import ModelDims, canonical_config
        cfg = canonical_config("SPEECH")
        self.config, self.dims, self.device = cfg, ModelDims(cfg), torch.device("cpu")
        self.calls = []

    def layer_state_info(self):
        return 0, 0, 0

    def conv_form_info(self):
        return {"split_f16_layers": 0, "split_f16_gate_layers": 0}

    def forward(self, mel, n_frames=None, noise=None, stream_state=None, **kw):
        import torch
        self.calls.append(tuple(kk for kk in ("f0_frames", "f0_scale", "f0_item_mask", "formant") if kw.get(kk) is not None))
        hop, spf = self.dims.hop_size, self.dims.steps_per_frame
        val = mel.sum(dim=2) + noise[:, ::spf]
        if kw.get("formant") is not None:
            assert kw["formant"].shape == val.shape and kw["formant"].dtype == torch.float32
            val = val * kw["formant"]
        return val.repeat_interleave(hop, dim=1), torch.zeros_like(stream_state)


def test_stream_factor_rows_travel_with_their_frames():
    """Two streams pushed in irregular packets -- one with per-frame formant factors, one without -- through rows that drop
    and grow: the streamed output is the closed form of the test double.  Tolerance as in
    test_pitch_control_host.test_control_rows_travel_with_their_frames: values below 1024 (spacing 6.1e-5), 80-term sums that
    differ by at most 2e-5, doubled by the largest factor, one rounding of the product: 4e-5 + 3.1e-5 < 2e-4."""
    from mbexwn_vocoder_amd.streaming import StreamingSynthesizer
    fake = _FormantFakeEngine()
    syn = StreamingSynthesizer(fake, chunk_frames=8)
    syn.use_graph = False
    rng = np.random.default_rng(5)
    lengths = {"a": 600, "b": 130}
    data = {sid: (rng.normal(size=(ll, 80)).astype(np.float32), rng.normal(size=(ll * 20,)).astype(np.float32))
            for sid, ll in lengths.items()}
    shift = {"a": rng.uniform(0.5, 2.0, size=600).astype(np.float32)}
    got, pos = {sid: [] for sid in lengths}, {sid: 0 for sid in lengths}
    for sid in lengths:
        syn.open(sid)
    for tick in range(400):
        for sid, ll in lengths.items():
            if pos[sid] < ll:
                nn = min(int(rng.integers(1, 13)) if tick else 300, ll - pos[sid])
                lo, hi = pos[sid], pos[sid] + nn
                extra = {"formant": shift[sid][lo:hi]} if sid in shift else {}
                syn.push(sid, data[sid][0][lo:hi], data[sid][1][lo * 20:hi * 20], last=hi >= ll, **extra)
                pos[sid] = hi
        for sid, audio in syn.tick().items():
            got[sid].append(audio)
        if all(syn.finished(sid) for sid in lengths):
            break
    assert syn._rows.formant.shape[1] == syn._in_cap >= 300 and syn.streams["a"].base > 0
    for sid, ll in lengths.items():
        mel, noise = data[sid]
        want = (mel.sum(axis=1) + noise[::20]) * shift.get(sid, np.float32(1.0))
        out = np.concatenate(got[sid])
        assert out.shape == (ll * 300,)
        np.testing.assert_allclose(out, np.repeat(want.astype(np.float32), 300), rtol=0, atol=2e-4)


def test_stream_factor_is_sticky_and_refused_when_malformed():
    """A synthesizer that never saw a factor other than 1 calls forward without the argument; from the first other factor on
    every call carries it, next to (and independent of) the pitch control."""
    from mbexwn_vocoder_amd.streaming import StreamingSynthesizer, _stage_layout
    rng = np.random.default_rng(6)
    mel, noise = rng.normal(size=(120, 80)).astype(np.float32), rng.normal(size=(120 * 20,)).astype(np.float32)

    def serve(syn, lo, hi, **extra):
        for pp in range(lo, hi, 8):
            more = {kk: vv[pp:pp + 8] if np.ndim(vv) else vv for kk, vv in extra.items()}
            syn.push(0, mel[pp:pp + 8], noise[pp * 20:(pp + 8) * 20], last=pp + 8 >= 120, **more)
            syn.tick()

    fake = _FormantFakeEngine()
    syn = StreamingSynthesizer(fake, chunk_frames=8)
    syn.open(0)
    serve(syn, 0, 64, formant=1.0)                                       # a factor of 1 is no factor
    serve(syn, 64, 72, formant=np.ones(120, dtype=np.float32))
    before = len(fake.calls)
    assert before >= 4 and set(fake.calls) == {()}
    serve(syn, 72, 96, formant=np.full(120, 1.25, dtype=np.float32))
    serve(syn, 96, 104)                                                  # the flag is sticky
    assert set(fake.calls[before:]) == {("formant",)}
    mid = len(fake.calls)
    serve(syn, 104, 120, transposition=1.5)                              # the pitch control arrives next to it
    assert set(fake.calls[mid:]) == {("f0_frames", "f0_scale", "f0_item_mask", "formant")}
    syn = StreamingSynthesizer(_FormantFakeEngine(), chunk_frames=8)
    syn.open(0)
    for bad in (0.0, -2.0, float("nan"), float("inf"), np.ones(3), np.asarray([1.0, 0.0, 1.0, 1.0])):
        with pytest.raises(ValueError, match="formant"):
            syn.push(0, mel[:4], noise[:80], formant=bad)
    assert syn.streams[0].have == 0                                      # a refused push appends nothing
    # the stage buffer of a replayed tick: the factor rows of the whole window, only once the synthesizer has seen a factor
    plain, shifted = _stage_layout(2, 6, 40, 80, 20, True, False), _stage_layout(2, 6, 40, 80, 20, True, False, True)
    assert shifted.size == plain.size + 2 * 40
    assert plain.views(np.zeros(plain.size, np.float32)).formant is None
    assert shifted.views(np.zeros(shifted.size, np.float32)).formant.shape == (2, 40)


def test_live_factors_follow_the_transposition_rule():
    """LiveResynthesizer.push_audio(formant=) through FrameFactors: the frames centred in a push take its factor; pushes in
    front of the first factor count as 1."""
    from mbexwn_vocoder_amd.live import LiveResynthesizer, _LStream
    from mbexwn_vocoder_amd.live_plan import frame_factors
    assert inspect.signature(LiveResynthesizer.push_audio).parameters["formant"].default is None
    st = _LStream(300, None, None)
    assert st.formants is None

    class Analyzer:
        def __init__(self):
            self.streams = {0: type("S", (), {"in_have": 0})()}

        def push(self, sid, samples, last=False, sample_rate=None):
            self.streams[sid].in_have += len(samples)

    live = LiveResynthesizer.__new__(LiveResynthesizer)
    live.analyzer, live.streams = Analyzer(), {0: st}
    pushes = [(700, None), (500, 1.3), (450, None), (650, 0.9)]
    for ii, (count, factor) in enumerate(pushes):
        live.push_audio(0, np.zeros(count, dtype=np.float32), last=ii == len(pushes) - 1, formant=factor,
                        transposition=2.0 if ii == 1 else None)
    total = st.factors.frames
    assert st.formants.frames == total == 2300 // 300 + 1
    assert np.array_equal(st.formants.take(0, total), frame_factors(pushes, 300))
    assert np.array_equal(st.factors.take(0, total), frame_factors([(700, None), (500, 2.0), (450, None), (650, None)], 300))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="formant must be finite and positive"):
            live.push_audio(0, np.zeros(10, dtype=np.float32), formant=bad)
