"""The decoded F0 contour's host side (no GPU needed): the definition f0decode.py on a sound the greedy tracker gets wrong, on
the sounds it gets right, on a frame with more candidates than slots and on hand-made tables; decode_params' refusals; the
header and exports of mbxc_f0_candidates and mbxc_decode_f0 and their refusals on the host; the new flags of the tools.

The bounds: 5 cents on steady tones and 10 on the vibrato glide are those test_f0track_host.py holds the greedy tracker to
(measured with the decoder: 0.12 cents on the adversarial sound); "at least 20" and "at least 10" wrong frames are about half
of what the greedy pick (38) and the decoder without its jump weight (30) showed when the definition was fixed."""
import ctypes
import importlib.util
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

from mbexwn_vocoder_amd import engine, f0decode, f0track

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mbexwn_vocoder_amd", "bin")
SR, HOP = 24000, 300
TONES = [60, 82.4, 110, 146.8, 220, 330, 440, 523.25, 700, 880]
f32 = np.float32


def load_script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(BIN, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_script(name, args):
    return subprocess.run([sys.executable, os.path.join(BIN, name + ".py"), *args], capture_output=True, text=True, timeout=600)


def bits(arr):
    return np.ascontiguousarray(arr, dtype=np.float32).view(np.uint32)


def inside(centres, n, prm):
    L = prm["window"] + prm["tau_max"]
    first = centres - (L >> 1)
    return (first >= 0) & (first + L <= n)


def cents(f0, true):
    return 1200.0 * np.log2(np.maximum(np.asarray(f0, np.float64), 1e-9) / true)


def adversarial(seed=1):
    n = 48000
    t = np.arange(n) / SR
    am = 0.3 + 0.2 * np.sin(2 * np.pi * 3 * t)
    x = 0.3 * sum(((1 if h % 2 == 0 else am) / h) * np.sin(2 * np.pi * h * 110 * t + h) for h in range(1, 13))
    return (x + 1e-3 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


@pytest.fixture(scope="module")
def adversarial_halves():
    """difference_host of the adversarial sound, computed once: everything that does not depend on the decoder."""
    prm = f0track.params(SR)
    return prm, f0track.difference_host(adversarial(), np.arange(161) * HOP, prm)


# ------------------------------------------------------------------------------------------------------------------------
# the definition on signals with a known pitch
# ------------------------------------------------------------------------------------------------------------------------
def test_the_greedy_pick_jumps_on_the_adversarial_sound_and_the_decoder_does_not(adversarial_halves):
    prm, halves = adversarial_halves
    greedy, _ = f0track.pick_host(*halves, prm)
    wrong = int(np.count_nonzero(np.abs(cents(greedy[4:-4], 110.0)) > 50))
    print(f"greedy: {wrong} of {greedy.size - 8} frames more than 50 cents off")
    assert wrong >= 20                                                   # the control: the input is adversarial
    dec = f0decode.decode_params()
    tables = f0decode.candidates_host(*halves, prm, dec)
    f0, per = f0decode.viterbi_host(*tables, SR, dec)
    assert f0.dtype == per.dtype == np.float32 and f0.shape == per.shape == (161,)
    err = np.abs(cents(f0[4:-4], 110.0))
    print(f"viterbi: worst {err.max():.3f} cents")
    assert np.all(f0[4:-4] > 0) and err.max() <= 5.0
    whole = f0decode.track_f0_viterbi_host(adversarial(), np.arange(161) * HOP, prm, dec)
    assert np.array_equal(bits(whole[0]), bits(f0)) and np.array_equal(bits(whole[1]), bits(per))
    # the transition term does the work: without it the candidates alone do not decide
    loose = f0decode.decode_params(w_jump=0)
    f0, _ = f0decode.viterbi_host(*tables, SR, loose)
    wrong = int(np.count_nonzero(np.abs(cents(f0[4:-4], 110.0)) > 50))
    print(f"viterbi with w_jump = 0: {wrong} frames more than 50 cents off")
    assert wrong >= 10


def test_steady_tones_stay_within_five_cents():
    prm, dec = f0track.params(SR), f0decode.decode_params()
    rng = np.random.default_rng(0)
    n = 12000
    tt = np.arange(n) / SR
    centres = np.arange(n // HOP + 1) * HOP
    keep = inside(centres, n, prm)
    for f in TONES:
        x = sum((0.5 / h) * np.sin(2 * np.pi * f * h * tt + h) for h in range(1, 9) if f * h < 11000)
        x = (x + 1e-3 * rng.standard_normal(n)).astype(np.float32)
        f0, per = f0decode.track_f0_viterbi_host(x, centres, prm, dec)
        assert np.all(f0[keep] > 0), f
        err = float(np.abs(cents(f0[keep], f)).max())
        print(f"{f} Hz: worst {err:.2f} cents")
        assert err <= 5.0, (f, err)


def test_vibrato_glide_stays_within_ten_cents():
    prm, dec = f0track.params(SR), f0decode.decode_params()
    n = 24000
    tt = np.arange(n) / SR
    fi = 200 * 2 ** (0.5 * np.sin(2 * np.pi * 5.5 * tt) / 12) * (1 + 0.2 * tt)
    ph = 2 * np.pi * np.cumsum(fi) / SR
    x = sum((0.5 / h) * np.sin(h * ph) for h in range(1, 9)).astype(np.float32)
    centres = np.arange(n // HOP + 1) * HOP
    keep = inside(centres, n, prm)
    f0, _ = f0decode.track_f0_viterbi_host(x, centres, prm, dec)
    assert np.all(f0[keep] > 0)
    err = cents(f0[keep], fi[centres[keep]])
    print(f"glide: worst {np.abs(err).max():.2f} cents")
    assert np.abs(err).max() <= 10.0


def test_noise_silence_and_a_gap():
    prm, dec = f0track.params(SR), f0decode.decode_params()
    centres = np.arange(41) * HOP
    noise = (0.1 * np.random.default_rng(1).standard_normal(12000)).astype(np.float32)
    assert np.all(f0decode.track_f0_viterbi_host(noise, centres, prm, dec)[0] == 0)
    f0, per = f0decode.track_f0_viterbi_host(np.zeros(12000, np.float32), centres, prm, dec)
    assert np.all(f0 == 0) and np.all(per == 1)
    # a 220 Hz tone with a silent gap from 0.7 s to 1.1 s: the greedy tracker's voiced / unvoiced pattern
    n = 43200
    tt = np.arange(n) / SR
    x = sum((0.5 / h) * np.sin(2 * np.pi * 220 * h * tt + h) for h in range(1, 9))
    x = (x + 1e-3 * np.random.default_rng(2).standard_normal(n)).astype(np.float32)
    x[int(0.7 * SR):int(1.1 * SR)] = 0
    centres = np.arange(n // HOP + 1) * HOP
    greedy, _ = f0track.track_f0_host(x, centres, prm)
    f0, _ = f0decode.track_f0_viterbi_host(x, centres, prm, dec)
    assert np.array_equal(greedy > 0, f0 > 0) and 20 < np.count_nonzero(f0 == 0) < 60
    assert np.all(np.abs(cents(f0[f0 > 0][4:-4], 220.0)) < 50)
    # empty sounds and empty tables
    f0, per = f0decode.track_f0_viterbi_host(np.zeros(0, np.float32), np.arange(3), prm, dec)
    assert np.all(f0 == 0) and np.all(per == 1)
    assert f0decode.track_f0_viterbi_host(noise, np.zeros(0, np.int64), prm, dec)[0].shape == (0,)


def test_the_number_of_candidates_is_capped():
    """A chain of sub-harmonics: periodic noise of periods 3 * 2^k gives one frame six picks."""
    prm = {"sample_rate": SR, "window": 1024, "tau_min": 2, "tau_max": 2047, "threshold": 0.15, "e_min": 0.0}
    rng = np.random.default_rng(5)
    y = np.zeros(8000)
    for k in range(10):
        period = 3 * 2 ** k
        tab = rng.standard_normal(period)
        tab = (tab - tab.mean()) / tab.std()
        y += np.sqrt(0.46 if k == 0 else 0.06) * np.tile(tab, 8000 // period + 1)[:8000]
    halves = f0track.difference_host((0.2 * y).astype(np.float32), np.array([4000]), prm)
    period, cost, dprime = (tt[0] for tt in f0decode.candidates_host(*halves, prm, f0decode.decode_params(n_cand=7)))
    count = int(np.count_nonzero(period))
    print(f"{count} candidates: periods {period[:count]}, costs {cost[:count]}")
    assert count > 3 and np.all(np.diff(period[:count]) > 0) and np.all(cost[count:7] == np.inf) and np.all(period[count:] == 0)
    assert len(set(cost[:count])) == count                              # no tie decides what follows
    p3, c3, d3 = (tt[0] for tt in f0decode.candidates_host(*halves, prm, f0decode.decode_params(n_cand=3)))
    best = np.sort(np.argsort(cost[:count], kind="stable")[:3])          # the three largest P are the three smallest costs
    assert np.array_equal(bits(p3[:3]), bits(period[best])) and np.array_equal(bits(c3[:3]), bits(cost[best]))
    assert np.array_equal(bits(d3[:3]), bits(dprime[best])) and np.all(p3[3:] == 0) and np.all(c3[3:7] == np.inf)
    assert c3[7] == cost[7] and d3[7] == dprime[7]                       # the unvoiced slot does not depend on the cap


def test_candidates_on_a_hand_made_difference_function():
    """d' with two dips: which thresholds pick which, the weight sums in ascending n, ties, slots and the unvoiced slot."""
    prm = {"sample_rate": 1000, "window": 64, "tau_min": 2, "tau_max": 12, "threshold": 0.15, "e_min": 1.0}
    row = np.ones(13, f32)
    row[4:7] = [0.30, 0.20, 0.28]                                        # a dip to 0.20 at lag 5
    row[9:12] = [0.12, 0.05, 0.09]                                       # and one to 0.05 at lag 10
    dec = f0decode.decode_params(thresholds=[0.1, 0.25, 0.5], weights=[0.25, 0.5, 0.125])
    period, cost, dprime = f0decode.candidates_host(row[None], np.array([2.0], f32), np.array([False]), prm, dec)
    # theta 0.1: first lag below is 10 -> 10; theta 0.25: lag 5; theta 0.5: lag 4, walked on to 5.  P[5] = 0.5 + 0.125, P[10] = 0.25
    assert np.array_equal(cost[0], f32([1 - 0.625, 1 - 0.25, np.inf, np.inf, np.inf, np.inf, np.inf, 1.0]))
    assert abs(period[0, 0] - 5) < 1 and abs(period[0, 1] - 10) < 1 and np.all(period[0, 2:] == 0)
    assert np.array_equal(dprime[0], f32([0.20, 0.05, 1, 1, 1, 1, 1, 0.05]))
    want = f32(5) + min(max(f32(f32(f32(0.30) - f32(0.28)) / f32(f32(f32(0.30) - f32(0.20)) + f32(f32(0.28) - f32(0.20)))) * f32(0.5), f32(-1)), f32(1))
    assert period[0, 0] == want
    # equal P: the smaller lag wins the only slot
    tie = f0decode.decode_params(n_cand=1, thresholds=[0.1, 0.25], weights=[0.5, 0.5])
    period, cost, _ = f0decode.candidates_host(row[None], np.array([2.0], f32), np.array([False]), prm, tie)
    assert abs(period[0, 0] - 5) < 1 and np.all(period[0, 1:] == 0) and cost[0, 0] == 0.5
    # below the energy floor, or bad: no pick at all, U is the sum of all weights
    for energy, bad, d7 in ((0.5, False, 0.05), (2.0, True, 1.0)):
        period, cost, dprime = f0decode.candidates_host(row[None], np.array([energy], f32), np.array([bad]), prm, dec)
        assert np.all(period == 0) and np.all(cost[0, :7] == np.inf) and cost[0, 7] == f32(1) - f32(f32(f32(0.25) + f32(0.5)) + f32(0.125))
        assert dprime[0, 7] == f32(d7)


# ------------------------------------------------------------------------------------------------------------------------
# the decoder on hand-made tables
# ------------------------------------------------------------------------------------------------------------------------
def tables(frames):
    """(T, 8) tables from per-frame lists of (period, cost) and the unvoiced cost; dprime numbers the entries."""
    T = len(frames)
    period, cost = np.zeros((T, 8), f32), np.full((T, 8), np.inf, f32)
    for t, (slots, unvoiced) in enumerate(frames):
        for k, (pp, cc) in enumerate(slots):
            period[t, k], cost[t, k] = pp, cc
        cost[t, 7] = unvoiced
    dprime = (np.arange(T * 8, dtype=f32).reshape(T, 8) + 1) / 1024
    return period, cost, dprime


def test_ties_resolve_to_the_smaller_index():
    dec = f0decode.decode_params()
    # equal costs and equal periods in slots 0 and 1: slot 0 at every frame; then the unvoiced slot as cheap as they are
    period, cost, dprime = tables([([(100, 0.25), (100, 0.25)], 1.0)] * 4)
    f0, per = f0decode.viterbi_host(period, cost, dprime, SR, dec)
    assert np.all(f0 == f32(SR) / f32(100)) and np.array_equal(per, dprime[:, 0])
    period, cost, dprime = tables([([(100, 0.25), (100, 0.25)], 0.25)] * 4)
    f0, per = f0decode.viterbi_host(period, cost, dprime, SR, dec)
    assert np.all(f0 > 0) and np.array_equal(per, dprime[:, 0])          # index 0 < 7 at the end, and 0 -> 0 costs nothing
    # two paths of equal total cost: the back pointer takes the smaller i
    period, cost, dprime = tables([([(100, 0.5), (200, 0.5)], 1.0), ([(150, 0.0)], 1.0)])
    one = f0decode.decode_params(w_jump=0)
    f0, per = f0decode.viterbi_host(period, cost, dprime, SR, one)
    assert np.array_equal(per, [dprime[0, 0], dprime[1, 0]])
    # T = 0 and T = 1
    f0, per = f0decode.viterbi_host(period[:0], cost[:0], dprime[:0], SR, dec)
    assert f0.shape == per.shape == (0,) and f0.dtype == per.dtype == np.float32
    f0, per = f0decode.viterbi_host(*tables([([(100, 0.75), (50, 0.5)], 0.625)]), SR, dec)
    assert f0[0] == f32(SR) / f32(50) and per[0] == f32(2) / 1024         # the cheapest slot
    f0, per = f0decode.viterbi_host(*tables([([(100, 0.75), (50, 0.5)], 0.25)]), SR, dec)
    assert f0[0] == 0 and per[0] == f32(8) / 1024


def test_unavailable_slots_never_reach_the_output():
    dec = f0decode.decode_params()
    frames = [([(100, 0.1)], 1.0)] * 9
    period, cost, dprime = tables(frames)
    cost[4, 0] = np.inf                                                  # frame 4: no voiced slot at all -> through slot 7
    f0, per = f0decode.viterbi_host(period, cost, dprime, SR, dec)
    assert f0[4] == 0 and per[4] == dprime[4, 7] and np.all(np.delete(f0, 4) == 240)
    for field, value in (("cost", np.nan), ("cost", np.inf), ("cost", -0.5), ("cost", 1e7), ("period", np.nan), ("period", np.inf),
                         ("period", -100.0), ("period", 1e7), ("period", 0.5)):
        period, cost, dprime = tables([([(100, 0.5), (101, 0.0)], 1.0)] * 5)
        (cost if field == "cost" else period)[:, 1] = value              # the cheap slot is the broken one
        f0, per = f0decode.viterbi_host(period, cost, dprime, SR, dec)
        assert np.all(f0 == 240) and np.array_equal(per, dprime[:, 0]), (field, value)
    # slot 7 is always available: a broken cost counts as 0
    for value in (np.nan, np.inf, -1.0, 1e7):
        period, cost, dprime = tables([([(100, 0.5)], value)] * 3)
        f0, per = f0decode.viterbi_host(period, cost, dprime, SR, dec)
        assert np.all(f0 == 0) and np.array_equal(per, dprime[:, 7]), value


def test_renormalisation_keeps_delta_finite():
    T = 5000
    grow = 1e6 * (np.arange(T) + 1) / T
    period, cost, dprime = tables([([(100, gg), (300, gg * 0.5)], gg) for gg in grow])
    trace = []
    f0, per = f0decode.viterbi_host(period, cost, dprime, SR, f0decode.decode_params(w_jump=1e6, w_switch=1e6), trace=trace)
    trace = np.asarray(trace)
    assert trace.shape == (T, 8) and np.all(np.isfinite(trace[:, [0, 1, 7]])) and np.all(np.isinf(trace[:, 2:7]))
    assert trace[1:].min(axis=1).max() == 0 and trace[:, [0, 1, 7]].max() <= 4e6      # the minimum is taken off after every frame
    assert np.all(np.isfinite(f0)) and np.all(f0 == 80)                  # 300 samples: half the cost, never worth a switch


# ------------------------------------------------------------------------------------------------------------------------
# parameters, header, symbol list, refusals
# ------------------------------------------------------------------------------------------------------------------------
def test_decode_params():
    dec = f0decode.decode_params()
    assert sorted(dec) == sorted(f0decode.DECODE_KEYS) and (dec["n_cand"], dec["w_jump"], dec["w_switch"]) == (7, 4.0, 0.5)
    th, ww = dec["thresholds"], dec["weights"]
    assert th.dtype == ww.dtype == np.float32 and th.shape == ww.shape == (16,)
    assert np.array_equal(th, [f32((n + 1) / 32) for n in range(16)])
    t64 = th.astype(np.float64)
    beta = t64 * (1 - t64) ** 11
    assert np.array_equal(ww, (beta / beta.sum()).astype(f32)) and abs(float(ww.sum()) - 1) < 1e-6
    good = dict(thresholds=[0.1, 0.2], weights=[0.5, 0.5])
    assert f0decode.decode_params(n_cand=1, w_jump=0, w_switch=1e6, **good)["weights"].dtype == np.float32
    for kw in ({"thresholds": []}, {"thresholds": np.linspace(0.01, 0.5, 17)}, {"thresholds": [0.2, 0.1]}, {"thresholds": [0.1, 0.1]},
               {"thresholds": [0.1, np.nan]}, {"thresholds": [0.1, np.inf]}, {"thresholds": [[0.1, 0.2]]},
               {"weights": [0.5]}, {"weights": [0.5, -0.1]}, {"weights": [0.5, np.nan]}, {"weights": [np.inf, 0.5]},
               {"n_cand": 0}, {"n_cand": 8}, {"n_cand": 2.5}, {"w_jump": -1}, {"w_jump": np.nan}, {"w_jump": 2e6}, {"w_jump": np.inf},
               {"w_switch": -0.5}, {"w_switch": np.nan}, {"w_switch": 1.5e6}):
        with pytest.raises(ValueError, match="f0 decode"):
            f0decode.decode_params(**dict(good, **kw))
    with pytest.raises(ValueError, match="f0 decode"):
        f0decode.check_decode({"n_cand": 3})
    from mbexwn_vocoder_amd.analysis import generate_mels
    cfg = {"sample_rate": 24000, "hop_size": 300, "fft_size": 2048, "win_size": 1200, "mel_channels": 80, "fmin": 0, "fmax": 8000,
           "lin_amp_off": 1e-5, "lin_amp_scale": 1, "mel_amp_scale": 1}
    with pytest.raises(ValueError, match="f0_out"):
        generate_mels([np.zeros(100, np.float32)], [24000], cfg, on_device=False, f0_decode=dec)
    with pytest.raises(ValueError, match="f0 decode"):
        generate_mels([np.zeros(100, np.float32)], [24000], cfg, on_device=False, f0_out=[], f0_decode={"n_cand": 3})


def test_header_declares_the_entry_points_and_the_library_exports_them(tmp_path):
    """(that the header declares exactly these names, no other header does and the library exports them: test_abi_headers.py)"""
    from mbexwn_vocoder_amd import abi
    from mbexwn_vocoder_amd.build import HEADERS, SOURCES
    text = open(os.path.join(ROOT, "include", "mbexwn_contour.h")).read()
    assert "THE DEFINITION" in text and "Refused" in text and '"f0 candidates:"' in text and '"decode f0:"' in text
    assert "HOST pointers" in text
    assert abi.symbols("mbexwn_contour.h") == ["mbxc_f0_candidates", "mbxc_decode_f0"]
    assert abi.symbols("mbexwn_pitch.h") == ["mbxp_track_f0"] and abi.MBX_ABI_VERSION == 11
    assert any(hh.endswith("mbexwn_contour.h") for hh in HEADERS) and "f0_frame.h" in HEADERS and "f0_decode.hip" in SOURCES
    src = tmp_path / "use.c"
    src.write_text('#include "mbexwn_contour.h"\nint main(void){ (void)mbxc_f0_candidates; (void)mbxc_decode_f0; return 0; }\n')
    res = subprocess.run(["cc", "-std=c99", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr                               # the header is plain C
    csrc = os.path.join(ROOT, "mbexwn_vocoder_amd", "csrc")
    kernel = open(os.path.join(csrc, "f0_decode.hip")).read()
    assert "#pragma clang fp contract(off)" in kernel and "fmaf" not in kernel and "getenv" not in kernel and "hipMalloc" not in kernel
    # the frame code is shared, not copied: both kernels call the one function of f0_frame.h
    shared = open(os.path.join(csrc, "f0_frame.h")).read()
    tracker = open(os.path.join(csrc, "f0_track.hip")).read()
    assert "f0_frame_dprime(" in shared and "#pragma clang fp contract(off)" in shared and "fmaf" not in shared
    for text in (kernel, tracker):
        assert '#include "f0_frame.h"' in text and text.count("f0_frame_dprime(") == 1 and "f0_lane_sum(" not in text


def test_the_c_entry_points_refuse_on_the_host():
    """Both entry points check every argument before they touch the device: the refusals need no GPU."""
    lib = engine.load_library()
    buf = (ctypes.c_float * 64)()
    ptr = ctypes.addressof(buf)
    fpp = ctypes.POINTER(ctypes.c_float)

    def host(values):
        arr = np.asarray(values, np.float32)
        return arr, arr.ctypes.data_as(fpp)

    th, ww = host([0.1, 0.2]), host([0.5, 0.5])
    good = dict(audio=ptr, stride=16, batch=1, n_samples=ptr, centres=ptr, n_frames=ptr, max_frames=1, sample_rate=24000, window=1024,
                tau_min=24, tau_max=437, e_min=0.0, thresholds=th[1], weights=ww[1], n_thresholds=2, n_cand=7, period=ptr, cost=ptr,
                dprime=ptr)

    def call(**kw):
        aa = dict(good, **kw)
        return lib.mbxc_f0_candidates(aa["audio"], aa["stride"], aa["batch"], aa["n_samples"], aa["centres"], aa["n_frames"],
                                      aa["max_frames"], aa["sample_rate"], aa["window"], aa["tau_min"], aa["tau_max"],
                                      ctypes.c_float(aa["e_min"]), aa["thresholds"], aa["weights"], aa["n_thresholds"], aa["n_cand"],
                                      aa["period"], aa["cost"], aa["dprime"], None)

    broken = [host(vv) for vv in ([0.1, np.nan], [0.2, 0.1], [0.1, 0.1], [0.5, -1.0], [np.inf, 0.5])]
    cases = [{name: None} for name in ("audio", "n_samples", "centres", "n_frames", "thresholds", "weights", "period", "cost", "dprime")]
    cases += [{"window": 0}, {"window": 96}, {"window": 2112}, {"tau_max": 1}, {"tau_min": 437}, {"window": 2048, "tau_max": 2049},
              {"sample_rate": 0}, {"max_frames": 0}, {"stride": 0}, {"batch": -1}, {"batch": 65536}, {"e_min": float("nan")},
              {"n_thresholds": 0}, {"n_thresholds": 17}, {"n_cand": 0}, {"n_cand": 8}]
    cases += [{"thresholds": bb[1]} for bb in broken[:3]] + [{"weights": bb[1]} for bb in broken[3:]]
    for kw in cases:
        assert call(**kw) == 1, kw                                       # MBX_ERR_INVALID_ARGUMENT
        assert lib.mbx_last_error().decode().startswith("f0 candidates:"), kw
    assert call(batch=0) == 0                                            # nothing to do

    good = dict(period=ptr, cost=ptr, dprime=ptr, n_frames=ptr, max_frames=1, batch=1, sample_rate=24000, w_jump=4.0, w_switch=0.5,
                f0=ptr, periodicity=ptr)

    def decode(**kw):
        aa = dict(good, **kw)
        return lib.mbxc_decode_f0(aa["period"], aa["cost"], aa["dprime"], aa["n_frames"], aa["max_frames"], aa["batch"],
                                  aa["sample_rate"], ctypes.c_float(aa["w_jump"]), ctypes.c_float(aa["w_switch"]), aa["f0"],
                                  aa["periodicity"], None)

    cases = [{name: None} for name in ("period", "cost", "dprime", "n_frames", "f0", "periodicity")]
    cases += [{"max_frames": 0}, {"max_frames": 16001}, {"batch": -1}, {"batch": 65536}, {"sample_rate": 0}]
    cases += [{key: vv} for key in ("w_jump", "w_switch") for vv in (float("nan"), -0.5, 1.5e6, float("inf"))]
    for kw in cases:
        assert decode(**kw) == 1, kw
        assert lib.mbx_last_error().decode().startswith("decode f0:"), kw
    assert decode(batch=0) == 0


# ------------------------------------------------------------------------------------------------------------------------
# the tools
# ------------------------------------------------------------------------------------------------------------------------
def test_transform_audio_flags(tmp_path, capsys, monkeypatch):
    tool = load_script("transform_audio")
    args = tool.make_parser().parse_args(["a.wav", "-o", "out"])
    assert (args.pitch_decode, args.pitch_jump, args.pitch_switch) == ("greedy", 4.0, 0.5)
    args = tool.make_parser().parse_args(["a.wav", "-o", "out", "--pitch-decode", "viterbi", "--pitch-jump", "2.5", "--pitch-switch", "0"])
    assert (args.pitch_decode, args.pitch_jump, args.pitch_switch) == ("viterbi", 2.5, 0.0)
    assert set(vars(args)) == set(inspect.signature(tool.main).parameters)            # every parsed name is an argument of main
    for flag, value in (("--pitch-decode", "pyin"), ("--pitch-jump", "-1"), ("--pitch-jump", "nan"), ("--pitch-switch", "2e6"),
                        ("--pitch-switch", "x")):
        with pytest.raises(SystemExit) as exc:
            tool.make_parser().parse_args(["a.wav", "-o", "out", flag, value])
        assert exc.value.code == 2 and flag in capsys.readouterr().err
    assert tool.pitch_decode_params("greedy", 4.0, 0.5) is None
    dec = tool.pitch_decode_params("viterbi", 2.0, 0.25)
    assert (dec["w_jump"], dec["w_switch"], dec["n_cand"]) == (2.0, 0.25, 7)
    from scipy.io import wavfile
    from mbexwn_vocoder_amd import batched
    from mbexwn_vocoder_amd.mel_inverter import create_synthetic_model_dir
    model = create_synthetic_model_dir(str(tmp_path / "model"), "SPEECH")
    snd = tmp_path / "a.wav"
    wavfile.write(str(snd), 24000, np.zeros(100, dtype=np.float32))
    res = run_script("transform_audio", [str(snd), "-o", str(tmp_path / "no"), "--pitch-decode", "viterbi"])
    assert res.returncode == 1 and "--pitch-decode" in res.stderr and not os.path.exists(tmp_path / "no")     # nothing to decode
    seen = []

    def fake_ranks(script, argv, *rest, **kw):
        seen.append(list(argv))
        return 0

    monkeypatch.setattr(batched, "run_ranks", fake_ranks)
    for extra, want in (({"f0_source": "audio"}, []), ({"f0_source": "audio", "pitch_decode": "greedy", "pitch_jump": 4.0, "pitch_switch": 0.5}, []),
                        ({"f0_source": "audio", "pitch_decode": "viterbi"}, ["--pitch-decode", "viterbi"]),
                        ({"write_f0": True, "pitch_decode": "viterbi", "pitch_jump": 2.0, "pitch_switch": 0.0},
                         ["--pitch-decode", "viterbi", "--pitch-jump", "2.0", "--pitch-switch", "0.0"]), ({}, [])):
        with pytest.raises(SystemExit) as exc:
            tool.main([str(snd)], str(tmp_path / "out"), model_id=model, gpus=2, **extra)
        assert exc.value.code == 0
        argv = seen.pop()
        got = [aa for ii, aa in enumerate(argv) if "--pitch" in aa or (ii and "--pitch" in argv[ii - 1])]
        assert got == want
        rank = tool.make_parser().parse_args(argv)                       # and the rank's parser takes what the parent sends
        assert rank.pitch_decode == extra.get("pitch_decode", "greedy") and rank.pitch_jump == extra.get("pitch_jump", 4.0)
    for name in ("transform_audio", "run_audio_job"):
        from mbexwn_vocoder_amd.mel_inverter import MELInverter
        func = MELInverter.transform_audio if name == "transform_audio" else batched.run_audio_job
        assert inspect.signature(func).parameters["f0_decode"].default is None
    assert inspect.signature(MELInverter.track_f0).parameters["decode"].default is None
    inv = MELInverter.host_only(model)
    with pytest.raises(ValueError, match="f0_decode"):
        inv.transform_audio([np.zeros(10, np.float32)], [24000], ["a.wav"], f0_decode=f0decode.decode_params())


def test_generate_mel_writes_the_decoded_contour(tmp_path):
    res = run_script("generate_mel", ["--help"])
    assert res.returncode == 0 and all(flag in res.stdout for flag in ("--pitch-decode", "--pitch-jump", "--pitch-switch"))
    params = inspect.signature(load_script("generate_mel").main).parameters
    assert (params["pitch_decode"].default, params["pitch_jump"].default, params["pitch_switch"].default) == ("greedy", 4.0, 0.5)
    res = run_script("generate_mel", ["a.wav", "-o", "o", "--pitch-decode", "pyin"])
    assert res.returncode == 2 and "--pitch-decode" in res.stderr
    from scipy.io import wavfile
    from mbexwn_vocoder_amd.fileio import load_var
    from mbexwn_vocoder_amd.mel_inverter import create_synthetic_model_dir
    model = create_synthetic_model_dir(str(tmp_path / "model"), "SPEECH")
    snd = adversarial()[:12000]
    wav = str(tmp_path / "adv.wav")
    wavfile.write(wav, SR, snd)
    prm = f0track.params(SR)
    for tag, extra, dec in (("default", [], f0decode.decode_params()),
                            ("weights", ["--pitch-jump", "1.5", "--pitch-switch", "0.25"], f0decode.decode_params(w_jump=1.5, w_switch=0.25))):
        out = str(tmp_path / tag)
        res = run_script("generate_mel", [wav, "-o", out, "--model_id", model, "--host", "--write-f0", "--pitch-decode", "viterbi", "-q",
                                          *extra])
        assert res.returncode == 0, res.stderr[-2000:]
        mell = load_var(os.path.join(out, "adv.mell"))["mell"]
        _, f0, per = f0track.read_f0(os.path.join(out, "adv.f0"), n_frames=mell.shape[1])
        want = f0decode.track_f0_viterbi_host(snd, np.arange(mell.shape[1]) * HOP, prm, dec)
        assert np.array_equal(bits(f0), bits(want[0])) and np.array_equal(bits(per), bits(want[1])), tag
        if tag == "default":
            assert np.all(np.abs(cents(f0[4:-4], 110.0)) < 5.0)
    res = run_script("generate_mel", [wav, "-o", str(tmp_path / "no"), "--model_id", model, "--host", "--pitch-decode", "viterbi"])
    assert res.returncode == 1 and "--write-f0" in res.stderr
    res = run_script("generate_mel", [wav, "-o", str(tmp_path / "no"), "--model_id", model, "--host", "--write-f0", "--pitch-decode",
                                      "viterbi", "--pitch-jump", "-3"])
    assert res.returncode == 1 and "w_jump" in res.stderr
