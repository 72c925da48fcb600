"""The definition of the level stage, mbexwn_vocoder_amd/level.py, on the CPU: the K-weighting
against the standard's table, the hop energies against a filter over the whole signal, the calibration point, the gates, the
gain, the true peak; the argument checks and the header of the device entry points (no GPU needed); the options of the tools."""
import ctypes
import importlib.util
import os
import subprocess

import numpy as np
import pytest

from mbexwn_vocoder_amd import level

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mbexwn_vocoder_amd", "bin")


def load_tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(BIN, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_coefficients_at_48_khz_are_the_standards_table():
    got = level.k_weighting(48000)
    want = [1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
            1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621]
    assert got.dtype == np.float64 and got.shape == (10,)
    assert np.max(np.abs(got - np.asarray(want))) < 1e-12
    with pytest.raises(ValueError):
        level.k_weighting(0)


def test_hop_rounding():
    assert [level.hop_samples(rr) for rr in (24000, 11025, 48000)] == [2400, 1103, 4800]
    assert level.hop_samples(44100) == 4410 and level.hop_samples(22050) == 2205


@pytest.mark.parametrize("rate", [24000, 11025, 48000])
def test_hop_energies_against_a_filter_over_the_whole_signal(rate):
    from scipy.signal import lfilter
    xx = (0.1 * np.random.default_rng(rate).standard_normal(int(1.35 * rate)) + 0.05).astype(np.float32)
    coef, hop = level.k_weighting(rate), level.hop_samples(rate)
    yy = lfilter(coef[5:8], [1.0, coef[8], coef[9]], lfilter(coef[:3], [1.0, coef[3], coef[4]], xx.astype(np.float64)))
    hops = xx.size // hop
    want = (yy[:hops * hop] ** 2).reshape(hops, hop).sum(axis=1)
    got = level.hop_energies_host(xx, rate)
    assert got.shape == (hops,) and hops == 13
    assert np.max(np.abs(got - want) / want) < 1e-10


def test_the_calibration_point():
    """A full-scale 997 Hz sine reads -3.01 LUFS."""
    xx = np.sin(2 * np.pi * 997.0 * np.arange(5 * 48000) / 48000.0)
    mm = level.measure_host(xx, 48000)
    assert abs(mm.lufs + 3.01) <= 0.005 and mm.count == mm.n_abs == 47
    assert abs(level.lufs(level.target_power(-23.0)) + 23.0) < 1e-12 and level.lufs(0.0) == float("-inf")


def test_gates():
    rate, hop = 24000, 2400
    nn = int(6.03 * rate)
    xx = 0.1 * np.random.default_rng(0).standard_normal(nn)
    xx[nn // 2:] *= 10 ** (-30 / 20)
    mm = level.measure_host(xx, rate)
    assert mm.blocks.size == 57 and mm.n_abs == 57 and mm.count == 30
    loud = mm.blocks[mm.blocks > level.ABS_GATE]
    threshold = 0.1 * np.mean(loud)
    assert np.min(np.abs(10 * np.log10(mm.blocks / threshold))) >= 0.1      # no block sits on the relative gate
    assert abs(mm.power / np.mean(mm.blocks[mm.blocks > threshold]) - 1) < 1e-14
    # a half below -70 LUFS falls to the absolute gate
    quiet = 0.1 * np.random.default_rng(1).standard_normal(nn)
    quiet[nn // 2:] *= 10 ** (-80 / 20)
    mq = level.measure_host(quiet, rate)
    # the quiet half begins inside hop 30: blocks 31 .. 56 lie wholly in it and every one of them is dropped, blocks 0 .. 30
    # hold some of the loud half and stay
    assert mq.blocks.size == 57 and nn // 2 // hop == 30
    assert np.all(mq.blocks[31:] <= level.ABS_GATE) and np.all(level.lufs(mq.blocks[31:]) < -70)
    assert np.all(mq.blocks[:31] > level.ABS_GATE) and mq.n_abs == 31 and 0 < mq.count <= 31
    # the shortest measurable item
    short = level.measure_host(xx[:4 * hop - 1], rate)
    assert short.count == 0 and short.blocks.size == 0 and short.power == 0.0 and short.lufs == float("-inf")
    assert level.gain_host(short.power, short.count, short.sample_peak, level.target_power(-23.0)) == (np.float32(1.0), False)
    one = level.measure_host(xx[:4 * hop], rate)
    assert one.blocks.size == 1 and one.count == 1
    assert level.measure_host(np.zeros(8 * hop), rate).count == 0            # silence


def test_gain():
    mm = level.measure_host(0.1 * np.random.default_rng(2).standard_normal(24000), 24000)
    target = level.target_power(-23.0)
    gain, limited = level.gain_host(mm.power, mm.count, mm.sample_peak, target, 10.0)
    assert gain.dtype == np.float32 and not limited
    assert abs(level.lufs(mm.power * float(gain) ** 2) + 23.0) < 1e-5         # the target, the ceiling slack
    assert level.gain_host(mm.power, mm.count, mm.sample_peak, target)[0] == gain
    ceiling = level.ceiling_linear(-1.0)
    bound, limited = level.gain_host(mm.power, mm.count, mm.sample_peak, level.target_power(-3.0), ceiling)
    assert limited and float(bound) * float(mm.sample_peak) <= ceiling * (1 + 2.0 ** -23)
    assert float(bound) * float(mm.sample_peak) >= ceiling * (1 - 2.0 ** -23)
    # a ceiling alone never scales up
    assert level.gain_host(mm.power, mm.count, mm.sample_peak, None, 10.0) == (np.float32(1.0), False)
    down, limited = level.gain_host(mm.power, mm.count, mm.sample_peak, None, 0.05)
    assert limited and down < 1
    for peak in (np.float32("nan"), np.float32(0.0)):
        assert level.gain_host(mm.power, mm.count, peak, target, 0.05) == (np.float32(1.0), False)
    assert np.isnan(level.bits_peak(np.asarray([0.1, np.nan, -0.7], dtype=np.float32)))
    assert level.bits_peak(np.asarray([0.1, -0.7], dtype=np.float32)) == np.float32(0.7) and level.bits_peak([]) == 0


def test_true_peak_of_the_quarter_rate_sine():
    rate = 24000
    xx = 0.5 * np.sin(2 * np.pi * (rate / 4) * np.arange(rate) / rate + np.pi / 4)
    mm = level.measure_host(xx, rate, true_peak=True)
    assert abs(float(mm.sample_peak) - 0.35355) < 1e-4
    assert 1.35 * float(mm.sample_peak) <= float(mm.true_peak) <= 0.5 * 1.01
    assert level.measure_host(xx, rate).true_peak == mm.sample_peak


def test_level_control_and_the_defaults():
    assert level.level_control() is None
    both = level.level_control(-23.0)
    assert both.target == -23.0 and both.peak_limit == -1.0 and not both.true_peak
    assert level.level_control(peak_limit=-3.0, true_peak=True).target is None
    assert both.powers([4, 5]) == [level.target_power(-23.0)] * 2
    assert level.level_control([0.5, None, 0.0]).powers([2, 0, 1]) == [None, 0.5, None]
    with pytest.raises(ValueError):
        level.level_control(true_peak=True)
    with pytest.raises(ValueError):
        level.level_control(float("nan"))
    with pytest.raises(ValueError):
        level.level_control(-23.0, float("inf"))
    with pytest.raises(ValueError, match="input"):
        level.level_control("input")                          # only a caller with source sounds takes the word
    # the one validation of the tools and the methods: the default of the peak limit, true_peak without a peak to limit
    assert level.check_options(-23.0, None, False) == (-23.0, -1.0, False)
    assert level.check_options("input", None, True, allow_input=True) == ("input", -1.0, True)
    assert level.check_options(None, None, False) == (None, None, False)
    assert level.check_options(None, -3.0, True) == (None, -3.0, True)
    assert level.check_options([0.5, None], None, False) == ([0.5, None], -1.0, False)
    with pytest.raises(ValueError, match="--true-peak"):
        level.check_options(None, None, True)
    with pytest.raises(ValueError, match="LUFS"):
        level.check_options("loud", None, False, allow_input=True)


def test_entry_points_refuse_bad_arguments_before_touching_the_device():
    from mbexwn_vocoder_amd import abi
    from mbexwn_vocoder_amd.build import build_library
    build_library()
    lib = abi.load_library()
    fake = ctypes.c_void_p(256)                              # never dereferenced: the checks fail first
    gate = ctypes.c_double(level.ABS_GATE)

    def why():
        return lib.mbx_last_error().decode()

    rows = (ctypes.c_double * 20)(*([1.0] * 20))               # host rows, as n_samples and hops are host arrays

    def measure(counts, hops, stride=10000, cap=4, audio=fake, coefs=rows, gate_p=ctypes.byref(gate), taps=None, n_taps=0,
                work=fake, records=fake):
        nn = (ctypes.c_int64 * max(1, len(counts)))(*counts)
        hh = (ctypes.c_int32 * max(1, len(hops)))(*hops)
        return lib.mbxl_measure(audio, stride, len(counts), nn, hh, coefs, gate_p, taps, n_taps, work, cap, records, None)

    assert measure([9600], [2400], audio=None) == 1 and "null" in why() and why().startswith("level measure")
    for name in ("work", "records"):
        assert measure([9600], [2400], **{name: None}) == 1 and "null" in why(), name
    assert measure([9600], [2400], coefs=None) == 1 and "coefficient" in why()
    assert measure([9600], [2400], gate_p=None) == 1 and "null" in why()
    assert measure([-1], [2400]) == 1 and "n_samples" in why()
    assert measure([10001], [2400]) == 1 and "stride" in why()
    assert measure([9600], [0]) == 1 and "hop" in why()
    assert measure([9600, 12000], [2400, 2400], stride=12000) == 1 and "workspace" in why()    # 5 hops, room for 4
    assert measure([9600], [2400], cap=0) == 1 and "hops_cap" in why()
    assert measure([9600], [2400], stride=-1) == 1
    assert measure([9600], [2400], taps=fake, n_taps=0) == 1 and "n_taps" in why()
    assert measure([9600], [2400], taps=fake, n_taps=8193) == 1
    assert lib.mbxl_measure(fake, 10000, -1, None, None, rows, ctypes.byref(gate), None, 0, fake, 4, fake, None) == 1
    assert lib.mbxl_measure(fake, 10000, 1, None, None, rows, ctypes.byref(gate), None, 0, fake, 4, fake, None) == 1
    assert measure([], []) == 0                              # an empty batch is nothing to do

    limit = ctypes.c_double(0.5)
    powers = (ctypes.c_double * 2)(0.0, 0.01)
    assert lib.mbxl_gains(None, 2, powers, None, ctypes.byref(limit), 0, fake, None) == 1 and "null" in why()
    assert lib.mbxl_gains(fake, 2, None, None, None, 0, fake, None) == 1 and "target" in why()
    assert lib.mbxl_gains(fake, 2, powers, None, None, 0, None, None) == 1
    assert lib.mbxl_gains(fake, -1, powers, None, None, 0, fake, None) == 1 and why().startswith("level gains")
    assert lib.mbxl_gains(fake, 2, powers, None, ctypes.byref(ctypes.c_double(0.0)), 0, fake, None) == 1 and "ceiling" in why()
    assert lib.mbxl_gains(fake, 0, None, None, None, 0, None, None) == 0

    def apply(counts, stride=100, out_stride=100, audio=fake, gains=fake, out=ctypes.c_void_p(4096)):
        nn = (ctypes.c_int64 * max(1, len(counts)))(*counts)
        return lib.mbxl_apply(audio, stride, len(counts), nn, gains, out, out_stride, None)

    for name in ("audio", "gains", "out"):
        assert apply([10], **{name: None}) == 1 and "null" in why(), name
    assert apply([101]) == 1 and apply([60], out_stride=50) == 1 and "stride" in why()
    assert apply([-1]) == 1 and apply([10], stride=-5) == 1
    assert apply([10], out=fake, out_stride=120) == 1 and "in place" in why()
    assert lib.mbxl_apply(fake, 100, -1, None, fake, fake, 100, None) == 1
    assert apply([]) == 0


def test_header_declares_the_entry_points_and_the_library_exports_them(tmp_path):
    """(that the header declares exactly these names, no other header does and the library exports them: test_abi_headers.py)"""
    from mbexwn_vocoder_amd import abi
    from mbexwn_vocoder_amd.build import HEADERS, SOURCES
    text = open(os.path.join(ROOT, "include", "mbexwn_level.h")).read()
    assert "workspace" in text and "Refused" in text and "HOST" in text and "MBXL_RECORD_BYTES 24" in text
    assert abi.symbols("mbexwn_level.h") == ["mbxl_measure", "mbxl_gains", "mbxl_apply"]
    assert any(hh.endswith("mbexwn_level.h") for hh in HEADERS) and "level.hip" in SOURCES
    assert abi.MBX_ABI_VERSION == 11
    assert level.RECORD_WORDS * 4 == 24
    src = tmp_path / "use.c"
    src.write_text('#include "mbexwn_level.h"\nint main(void){ (void)mbxl_measure; (void)mbxl_gains; (void)mbxl_apply; return 0; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                   check=True)


def test_options_of_the_tools(capsys):
    from mbexwn_vocoder_amd import cli
    transform, resynth = load_tool("transform_audio"), load_tool("resynth_mel")
    args = transform.make_parser().parse_args(["a.wav", "-o", "out"])
    assert args.loudness is None and args.peak_limit is None and args.true_peak is False
    args = transform.make_parser().parse_args(["a.wav", "-o", "out", "--loudness", "-23", "--peak-limit", "-2.5", "--true-peak"])
    assert args.loudness == -23.0 and args.peak_limit == -2.5 and args.true_peak is True
    assert transform.make_parser().parse_args(["a.wav", "-o", "out", "--loudness", "input"]).loudness == "input"
    args = resynth.make_parser().parse_args(["SPEECH", "-i", "a.mell", "--loudness", "-16", "--batch", "4"])
    assert args.loudness == -16.0 and args.peak_limit is None and args.true_peak is False
    for tool, argv, word in ((resynth, ["SPEECH", "-i", "a.mell", "--loudness", "input"], "input"),
                             (resynth, ["SPEECH", "-i", "a.mell", "--loudness", "loud"], "LUFS"),
                             (transform, ["a.wav", "-o", "out", "--loudness", "inf"], "LUFS"),
                             (transform, ["a.wav", "-o", "out", "--peak-limit", "nan"], "dBFS")):
        with pytest.raises(SystemExit) as exc:
            tool.make_parser().parse_args(argv)
        assert exc.value.code == 2 and word in capsys.readouterr().err
    # the ranks of a --gpus job get the options
    parser = transform.make_parser()
    values = vars(parser.parse_args(["a.wav", "-o", "out", "--loudness", "input", "--peak-limit", "-2", "--true-peak", "--gpus", "2"]))
    argv = cli.rank_argv(parser, values, ["a.wav"])
    assert argv[argv.index("--loudness") + 1] == "input" and argv[argv.index("--peak-limit") + 1] == "-2.0" and "--true-peak" in argv
    assert parser.parse_args(argv).loudness == "input"
    parser = resynth.make_parser()
    values = vars(parser.parse_args(["SPEECH", "-i", "a.mell", "--loudness", "-23", "--gpus", "2"]))
    argv = cli.rank_argv(parser, values, ["SPEECH"])
    assert parser.parse_args(argv).loudness == -23.0 and "--peak-limit" not in argv


def test_the_writers_line():
    from mbexwn_vocoder_amd.batched import level_line
    report = {"loudness_in": -18.04, "loudness_out": -23.0, "gain": 0.565, "gain_db": -4.96, "peak_in": 0.9, "peak_out": 0.5085,
              "limited": False}
    line = level_line("syn_a.flac", report)
    assert "-18.04 -> -23.00 LUFS" in line and "gain -4.96 dB" in line and "peak -5.87 dBFS" in line and "limit" not in line
    assert "the peak limit" in level_line("syn_a.flac", dict(report, limited=True))
    silent = dict(report, loudness_in=float("-inf"), loudness_out=float("-inf"), gain=1.0, gain_db=0.0, peak_out=0.0)
    assert "not measurable" in level_line("syn_a.flac", silent) and "peak -inf dBFS" in level_line("syn_a.flac", silent)
