"""The decoded F0 contour on the GPU: mbxc_f0_candidates and mbxc_decode_f0 (csrc/f0_decode.hip) against their definitions
f0decode.candidates_host and f0decode.viterbi_host, bit for bit -- no tolerance: both sides make the same separately rounded
float32 operations in the same order --, their memory contract (outputs between guard bands, rows at or behind n_frames keep
the fill), their refusals, and the path through the package and the tools."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from guarded import Guarded
from helpers import build_case
from mbexwn_vocoder_amd import analysis, f0decode, f0track, timemap

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mbexwn_vocoder_amd", "bin")
SR, HOP, STRIDE, SEED = 24000, 300, 6100, 11
# (window, tau_min, tau_max): one partial sum per lane and the smallest frame; a middle one; the defaults at 24 kHz; L = 4095
SETS = [(64, 2, 5), (128, 3, 64), (1024, 24, 437), (2048, 2, 2047)]
E_DEFAULT = float(f0track.params(SR)["e_min"])
WORD = {"nan": -1, "huge": int(np.float32(1e30).view(np.int32))}
FPP = ctypes.POINTER(ctypes.c_float)


@pytest.fixture(scope="module")
def torch():
    import torch as tt
    return tt


def dev(torch, arr):
    return torch.as_tensor(np.ascontiguousarray(arr)).cuda()


def bits(arr):
    return np.ascontiguousarray(arr, dtype=np.float32).view(np.uint32)


def harmonic(n, f0, rng, noise=1e-3, amp=0.5):
    tt = np.arange(n) / SR
    x = sum((amp / h) * np.sin(2 * np.pi * f0 * h * tt + h) for h in range(1, 9))
    return (x + noise * rng.standard_normal(n)).astype(np.float32)


def adversarial(n=48000):
    """The sound of tests/test_f0decode_host.py that the greedy pick gets wrong: 110 Hz, strong even harmonics, the odd ones
    swelling and fading at 3 Hz."""
    t = np.arange(n) / SR
    am = 0.3 + 0.2 * np.sin(2 * np.pi * 3 * t)
    x = 0.3 * sum(((1 if h % 2 == 0 else am) / h) * np.sin(2 * np.pi * h * 110 * t + h) for h in range(1, 13))
    return (x + 1e-3 * np.random.default_rng(1).standard_normal(n)).astype(np.float32)


def chain_sound():
    """Periodic noise tables of periods 3 * 2^k: a frame with six candidates."""
    rng = np.random.default_rng(5)
    y = np.zeros(8000)
    for k in range(10):
        period = 3 * 2 ** k
        tab = rng.standard_normal(period)
        tab = (tab - tab.mean()) / tab.std()
        y += np.sqrt(0.46 if k == 0 else 0.06) * np.tile(tab, 8000 // period + 1)[:8000]
    return (0.2 * y).astype(np.float32)


def decode_sets():
    """(label, decode_params, e_min): n_cand 1, 2, 3, 7; N = 1, 3 and 16; weights with zeros; e_min 0 and the default; and
    thresholds that every frame with a signal gets below, also with lags 2 .. 4 only."""
    zeros = f0decode.default_weights(f0decode.default_thresholds())
    zeros[[0, 3, 4, 9]] = 0
    return [("defaults", f0decode.decode_params(), 0.0), ("n_cand 3", f0decode.decode_params(n_cand=3), E_DEFAULT),
            ("N = 1", f0decode.decode_params(n_cand=1, thresholds=[0.15], weights=[0.75]), 0.0),
            ("zero weights", f0decode.decode_params(n_cand=7, weights=zeros), E_DEFAULT),
            ("thresholds above 1", f0decode.decode_params(n_cand=2, thresholds=[0.5, 1.5, 3.0], weights=[0.25, 0.5, 0.25]), 0.0)]


@pytest.fixture(scope="module")
def items():
    """The ragged batch: (label, samples).  n = 0, 1, 37, 700 (shorter than the default L) and 6000, stride above them."""
    rng = np.random.default_rng(21)
    n = 6000
    tiny = (1e-17 * np.sin(2 * np.pi * 200.0 * np.arange(n) / SR)).astype(np.float32)
    broken = harmonic(n, 180.0, rng)
    broken[[900, 2400, 4000]] = [np.nan, np.inf, 1e20]
    return [("tone+noise", harmonic(n, 220.0, rng)), ("adversarial", adversarial()[:n]),
            ("noise", (0.1 * rng.standard_normal(n)).astype(np.float32)), ("silence", np.zeros(n, np.float32)), ("tone 1e-17", tiny),
            ("n=700", harmonic(700, 440.0, rng)), ("n=37", (0.1 * rng.standard_normal(37)).astype(np.float32)),
            ("n=1", np.ones(1, np.float32)), ("n=0", np.zeros(0, np.float32)), ("not finite", broken),
            ("no frames", harmonic(n, 110.0, rng))]


def centre_tables(items, regular):
    rows = []
    for _, x in items:
        n = x.size
        if regular == "one":
            rows.append([n // 2])
        elif regular:
            rows.append(list(range(0, n + 1, HOP)))
        else:                                   # repeats, descending, 0, n, below 0 and above n
            rows.append([n // 2, n // 2, n, 0, -7, n + 1000, n // 3, 1, 2 * n // 3, n // 3])
    counts = [len(rr) for rr in rows]
    counts[-1] = 0                                                       # the last item: no frames
    table = np.full((len(rows), max(counts)), 123, dtype=np.int64)       # entries behind a count: valid, and unused
    for ii, rr in enumerate(rows):
        table[ii, :len(rr)] = rr
    return table, counts


def padded(items, pad):
    sound = np.full((len(items), STRIDE), pad, dtype=np.float32)         # behind every item's end: never read
    for ii, (_, x) in enumerate(items):
        sound[ii, :x.size] = x
    return sound, [x.size for _, x in items]


class Candidates:
    """One raw call of mbxc_f0_candidates with its own buffers: the three tables between guard bands, pre-filled."""

    def __init__(self, torch, sound, lengths, centres, counts, fill="nan"):
        from mbexwn_vocoder_amd.engine import load_library
        self.torch, self.lib = torch, load_library()
        self.sound = dev(torch, np.asarray(sound, np.float32))
        self.lengths, self.counts = dev(torch, np.asarray(lengths, np.int32)), dev(torch, np.asarray(counts, np.int32))
        self.centres = dev(torch, np.asarray(centres, np.int64))
        self.batch, self.frames = int(self.sound.shape[0]), int(self.centres.shape[1])
        self.out = [Guarded(name, 4 * self.batch * self.frames * 8, fill, device="cuda") for name in ("period", "cost", "dprime")]

    def run(self, dec=None, **kw):
        dec = dec or f0decode.decode_params()
        th = np.ascontiguousarray(dec["thresholds"], np.float32)
        ww = np.ascontiguousarray(dec["weights"], np.float32)
        args = dict(audio=self.sound.data_ptr(), stride=int(self.sound.shape[1]), batch=self.batch, n_samples=self.lengths.data_ptr(),
                    centres=self.centres.data_ptr(), n_frames=self.counts.data_ptr(), max_frames=self.frames, sample_rate=SR,
                    window=1024, tau_min=24, tau_max=437, e_min=0.0, thresholds=th.ctypes.data_as(FPP),
                    weights=ww.ctypes.data_as(FPP), n_thresholds=int(th.size), n_cand=int(dec["n_cand"]),
                    period=self.out[0].ptr, cost=self.out[1].ptr, dprime=self.out[2].ptr)
        args.update(kw)
        status = self.lib.mbxc_f0_candidates(args["audio"], args["stride"], args["batch"], args["n_samples"], args["centres"],
                                             args["n_frames"], args["max_frames"], args["sample_rate"], args["window"],
                                             args["tau_min"], args["tau_max"], ctypes.c_float(args["e_min"]), args["thresholds"],
                                             args["weights"], args["n_thresholds"], args["n_cand"], args["period"], args["cost"],
                                             args["dprime"], None)
        self.torch.cuda.synchronize()
        return status

    def refill(self):
        for gg in self.out:
            gg.refill()

    def results(self, dtype=None):
        dtype = dtype or self.torch.float32
        return tuple(gg.view(dtype, self.batch, self.frames, 8).cpu().numpy() for gg in self.out)

    def untouched(self):
        return all(gg.payload_untouched() for gg in self.out)

    def check(self):
        for gg in self.out:
            gg.check()


class Decode:
    """One raw call of mbxc_decode_f0: the two outputs between guard bands, pre-filled."""

    def __init__(self, torch, tables, counts, fill="nan"):
        from mbexwn_vocoder_amd.engine import load_library
        self.torch, self.lib = torch, load_library()
        self.tables = [dev(torch, np.asarray(tt, np.float32)) for tt in tables]
        self.counts = dev(torch, np.asarray(counts, np.int32))
        self.batch, self.frames = int(self.tables[0].shape[0]), int(self.tables[0].shape[1])
        self.f0 = Guarded("f0", 4 * self.batch * self.frames, fill, device="cuda")
        self.per = Guarded("periodicity", 4 * self.batch * self.frames, fill, device="cuda")

    def run(self, **kw):
        args = dict(period=self.tables[0].data_ptr(), cost=self.tables[1].data_ptr(), dprime=self.tables[2].data_ptr(),
                    n_frames=self.counts.data_ptr(), max_frames=self.frames, batch=self.batch, sample_rate=SR, w_jump=4.0,
                    w_switch=0.5, f0=self.f0.ptr, periodicity=self.per.ptr)
        args.update(kw)
        status = self.lib.mbxc_decode_f0(args["period"], args["cost"], args["dprime"], args["n_frames"], args["max_frames"],
                                         args["batch"], args["sample_rate"], ctypes.c_float(args["w_jump"]),
                                         ctypes.c_float(args["w_switch"]), args["f0"], args["periodicity"], None)
        self.torch.cuda.synchronize()
        return status

    def results(self, dtype=None):
        dtype = dtype or self.torch.float32
        return tuple(gg.view(dtype, self.batch, self.frames).cpu().numpy() for gg in (self.f0, self.per))

    def untouched(self):
        return self.f0.payload_untouched() and self.per.payload_untouched()

    def check(self):
        self.f0.check()
        self.per.check()


@pytest.mark.parametrize("window,tau_min,tau_max", SETS)
def test_candidates_kernel_equals_the_host_definition_bit_for_bit(torch, items, window, tau_min, tau_max):
    modes = ["one"] if window == 2048 else [True, False]
    used = 0
    for mode, fill, pad in zip(modes, ("nan", "huge"), (np.nan, 1e30)):
        table, counts = centre_tables(items, mode)
        sound, lengths = padded(items, pad)
        base = {"sample_rate": SR, "window": window, "tau_min": tau_min, "tau_max": tau_max, "threshold": 0.15, "e_min": 0.0}
        halves = [f0track.difference_host(x, table[ii, :counts[ii]], base) for ii, (_, x) in enumerate(items)]
        call = Candidates(torch, sound, lengths, table, counts, fill=fill)
        for label_d, dec, e_min in decode_sets():
            prm = dict(base, e_min=e_min)
            call.refill()
            assert call.run(dec, window=window, tau_min=tau_min, tau_max=tau_max, e_min=e_min) == 0
            call.check()                                                 # the guards around the three tables keep the pattern
            got, raw = call.results(), call.results(torch.int32)
            for ii, (label, x) in enumerate(items):
                want = f0decode.candidates_host(*halves[ii], prm, dec)
                for name, gg, rr, ww in zip(("period", "cost", "dprime"), got, raw, want):
                    what = (label, mode, label_d, name)
                    assert np.array_equal(bits(gg[ii, :counts[ii]]), bits(ww)), (what, gg[ii, :counts[ii]], ww)
                    assert np.all(rr[ii, counts[ii]:] == WORD[fill]), what
                assert np.all(want[0][:, 7] == 0) and np.all(want[1][:, :7][want[0][:, :7] == 0] == np.inf)
                assert np.all(np.count_nonzero(want[0], axis=1) <= dec["n_cand"])
                if label == "not finite":                                # the frames over the three samples offer no lag
                    assert halves[ii][2].any() and np.all(want[0][halves[ii][2]] == 0) and np.all(want[2][halves[ii][2], 7] == 1)
                used += int(np.count_nonzero(want[0]))
        # and the module's wrapper gives the same tensors
        dec = f0decode.decode_params()
        tabs = f0decode.candidates_device(dev(torch, sound), dev(torch, np.asarray(lengths, np.int32)), dev(torch, table),
                                          dev(torch, np.asarray(counts, np.int32)), base, dec)
        for ii, (label, x) in enumerate(items):
            for gg, ww in zip(tabs, f0decode.candidates_host(*halves[ii], base, dec)):
                assert np.array_equal(bits(gg[ii, :counts[ii]].cpu().numpy()), bits(ww)), label
    assert used > 0                                                      # the comparison saw candidates, not only empty slots


def test_candidates_of_the_subharmonic_chain_are_capped(torch):
    x = chain_sound()
    prm = {"sample_rate": SR, "window": 1024, "tau_min": 2, "tau_max": 2047, "threshold": 0.15, "e_min": 0.0}
    half = f0track.difference_host(x, np.array([4000]), prm)
    call = Candidates(torch, x[None], [x.size], np.array([[4000]], np.int64), [1])
    for n_cand in (7, 3):
        dec = f0decode.decode_params(n_cand=n_cand)
        want = f0decode.candidates_host(*half, prm, dec)
        call.refill()
        assert call.run(dec, window=1024, tau_min=2, tau_max=2047) == 0
        call.check()
        for gg, ww in zip(call.results(), want):
            assert np.array_equal(bits(gg[0]), bits(ww)), (n_cand, gg[0], ww)
        used = np.count_nonzero(want[0][0])
        assert used == 3 if n_cand == 3 else used > 3


def random_tables(rng, batch, frames):
    """Costs from {0, 0.25, 0.5, 1} and periods from {50, 100, 200}, so that ties occur; 0 .. 7 used slots per frame; NaN,
    inf, negative and 1e7 entries sprinkled over both tables."""
    period = rng.choice(np.array([50, 100, 200], np.float32), size=(batch, frames, 8))
    cost = rng.choice(np.array([0, 0.25, 0.5, 1], np.float32), size=(batch, frames, 8))
    dprime = rng.random((batch, frames, 8)).astype(np.float32)
    count = rng.integers(0, 8, size=(batch, frames))
    unused = np.arange(7)[None, None, :] >= count[:, :, None]
    period[:, :, :7][unused] = 0
    cost[:, :, :7][unused] = np.inf
    period[:, :, 7] = 0
    for tab in (period, cost):
        where = rng.random(tab.shape) < 0.03
        tab[where] = rng.choice(np.array([np.nan, np.inf, -0.5, 1e7], np.float32), size=int(where.sum()))
    return period, cost, dprime


def test_decode_kernel_equals_the_host_definition_bit_for_bit(torch):
    rng = np.random.default_rng(31)
    counts = [0, 1, 2, 37, 300, 300]
    tables = random_tables(rng, len(counts), 300)
    voiced = 0
    for fill in ("nan", "huge"):
        call = Decode(torch, tables, counts, fill=fill)
        for w_jump in (0.0, 4.0):
            for w_switch in (0.0, 0.5):
                dec = f0decode.decode_params(w_jump=w_jump, w_switch=w_switch)
                call.f0.refill()
                call.per.refill()
                assert call.run(w_jump=w_jump, w_switch=w_switch) == 0
                call.check()
                got, raw = call.results(), call.results(torch.int32)
                for ii, kk in enumerate(counts):
                    want = f0decode.viterbi_host(*(tt[ii, :kk] for tt in tables), SR, dec)
                    for gg, rr, ww in zip(got, raw, want):
                        assert np.array_equal(bits(gg[ii, :kk]), bits(ww)), (fill, w_jump, w_switch, ii)
                        assert np.all(rr[ii, kk:] == WORD[fill]), (fill, w_jump, w_switch, ii)
                    assert np.all(np.isin(want[0], [0, SR / 50, SR / 100, SR / 200]))    # no sprinkled entry reaches f0
                    voiced += int(np.count_nonzero(want[0]))
        if fill == "huge":
            continue
        # the wrapper; a count above max_frames and a negative one are clamped
        dec = f0decode.decode_params()
        f0, per = f0decode.decode_device(*call.tables, dev(torch, np.asarray([-4, 1, 2, 37, 300, 900], np.int32)), SR, dec)
        assert np.all(f0[0].cpu().numpy() == 0) and np.all(per[0].cpu().numpy() == 0)
        for ii, kk in list(enumerate(counts))[1:]:
            want = f0decode.viterbi_host(*(tt[ii, :kk] for tt in tables), SR, dec)
            assert np.array_equal(bits(f0[ii, :kk].cpu().numpy()), bits(want[0])), ii
            assert np.array_equal(bits(per[ii, :kk].cpu().numpy()), bits(want[1])), ii
    assert voiced > 0


def test_decode_kernel_at_its_frame_limit(torch):
    tables = random_tables(np.random.default_rng(32), 1, 16000)
    call = Decode(torch, tables, [16000])
    assert call.run() == 0
    call.check()
    want = f0decode.viterbi_host(*(tt[0] for tt in tables), SR, f0decode.decode_params())
    for gg, ww in zip(call.results(), want):
        assert np.array_equal(bits(gg[0]), bits(ww))
    assert np.count_nonzero(want[0]) > 1000


def test_both_kernels_decode_the_adversarial_sound(torch):
    x = adversarial()
    cc = np.arange(161, dtype=np.int64) * HOP
    prm, dec = f0track.params(SR), f0decode.decode_params()
    want = f0decode.track_f0_viterbi_host(x, cc, prm, dec)
    args = (dev(torch, x[None]), dev(torch, np.asarray([x.size], np.int32)), dev(torch, cc[None]), dev(torch, np.asarray([161], np.int32)))
    f0, per = f0decode.track_f0_viterbi_device(*args, prm, dec)
    assert np.array_equal(bits(f0[0].cpu().numpy()), bits(want[0])) and np.array_equal(bits(per[0].cpu().numpy()), bits(want[1]))
    greedy = f0track.track_f0_device(*args, prm)[0][0].cpu().numpy()
    assert np.count_nonzero(np.abs(1200 * np.log2(np.maximum(greedy[4:-4], 1e-9) / 110)) > 50) >= 20
    assert np.all(want[0][4:-4] > 0) and np.max(np.abs(1200 * np.log2(want[0][4:-4] / 110))) < 5.0


def test_refusals_leave_the_outputs_untouched(torch, items):
    sound, lengths = padded(items[:2], 0.0)
    table = np.tile(np.arange(0, 6001, HOP, dtype=np.int64), (2, 1))
    call = Candidates(torch, sound, lengths, table, [table.shape[1]] * 2, fill="huge")

    def why():
        return call.lib.mbx_last_error().decode()

    def host(values):
        arr = np.asarray(values, np.float32)
        return arr, arr.ctypes.data_as(FPP)

    keep = [host(vv) for vv in ([0.1, np.nan], [0.1, np.inf], [0.2, 0.2], [0.2, 0.1], [0.5, -0.1], [0.5, np.nan], [0.5, np.inf])]
    cases = [({name: None}, "null") for name in ("audio", "n_samples", "centres", "n_frames", "thresholds", "weights", "period",
                                                 "cost", "dprime")]
    cases += [({"window": 0}, "window"), ({"window": 32}, "window"), ({"window": 96}, "window"), ({"window": 2112}, "window"),
              ({"tau_max": 1}, "tau_max"), ({"tau_min": 437}, "tau_min"), ({"tau_min": -1}, "tau_min"),
              ({"tau_min": 2, "tau_max": 2}, "tau_min"), ({"window": 2048, "tau_max": 2049}, "4096"),
              ({"sample_rate": 0}, "sample_rate"), ({"e_min": float("nan")}, "e_min"),
              ({"max_frames": 0}, "max_frames"), ({"stride": 0}, "stride"), ({"batch": -1}, "batch"), ({"batch": 65536}, "batch"),
              ({"n_thresholds": 0}, "n_thresholds"), ({"n_thresholds": 17}, "n_thresholds"), ({"n_cand": 0}, "n_cand"),
              ({"n_cand": 8}, "n_cand")]
    cases += [({"thresholds": keep[ii][1], "n_thresholds": 2}, "thresholds") for ii in range(4)]
    cases += [({"weights": keep[ii][1], "n_thresholds": 2}, "weights") for ii in range(4, 7)]
    for kw, what in cases:
        assert call.run(**kw) == 1, kw                                   # MBX_ERR_INVALID_ARGUMENT
        assert why().startswith("f0 candidates:") and what in why(), (kw, why())
        assert call.untouched(), kw
        call.check()
    assert call.run(batch=0) == 0 and call.untouched()                   # nothing to do
    assert call.run() == 0 and not call.untouched()                      # and the same buffers do run

    tables = random_tables(np.random.default_rng(33), 2, 40)
    dcall = Decode(torch, tables, [40, 7], fill="huge")
    cases = [({name: None}, "null") for name in ("period", "cost", "dprime", "n_frames", "f0", "periodicity")]
    cases += [({"max_frames": 0}, "max_frames"), ({"max_frames": 16001}, "16000"), ({"batch": -1}, "batch"), ({"batch": 65536}, "batch"),
              ({"w_jump": float("nan")}, "w_jump"), ({"w_jump": -1.0}, "w_jump"), ({"w_jump": 2e6}, "w_jump"),
              ({"w_switch": float("nan")}, "w_switch"), ({"w_switch": -0.5}, "w_switch"), ({"w_switch": float("inf")}, "w_switch"),
              ({"sample_rate": 0}, "sample_rate")]
    for kw, what in cases:
        assert dcall.run(**kw) == 1, kw
        assert why().startswith("decode f0:") and what in why(), (kw, why())
        assert dcall.untouched(), kw
        dcall.check()
    assert dcall.run(batch=0) == 0 and dcall.untouched()
    empty = Decode(torch, tables, [0, 0], fill="huge")
    assert empty.run() == 0 and empty.untouched()                        # items without frames write nothing
    assert dcall.run() == 0 and not dcall.untouched()


# ---------------------------------------------------------------------------------------------------------------------------
# through the package: the synthetic canonical model, batch_invariant kernels

def run_script(name, args):
    return subprocess.run([sys.executable, os.path.join(BIN, name + ".py"), *args], capture_output=True, text=True, timeout=600)


def voiced(freq, rate):
    ph = 2 * np.pi * np.cumsum(freq) / rate
    return sum((0.5 / h) * np.sin(h * ph) for h in range(1, 9) if h * freq.max() < 0.45 * rate).astype(np.float32)


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    from mbexwn_vocoder_amd.config import dump_config
    from mbexwn_vocoder_amd.weights import save_weights
    cfg, raw, _ = build_case("SPEECH", {})
    path = str(tmp_path_factory.mktemp("model") / "speech")
    os.makedirs(path)
    dump_config(os.path.join(path, "config.yaml"), cfg)
    save_weights(os.path.join(path, "weights.npz"), raw)
    return path


@pytest.fixture(scope="module")
def inv(model_dir):
    from mbexwn_vocoder_amd.mel_inverter import MELInverter
    return MELInverter(model_dir, batch_invariant=True)


@pytest.fixture(scope="module")
def sounds():
    """(names, sounds, rates): the adversarial sound (0.5 s), the vibrato glide, silence, and a 200 Hz tone at 16 kHz."""
    tt = np.arange(12000) / SR
    glide = 200 * 2 ** (0.5 * np.sin(2 * np.pi * 5.5 * tt) / 12) * (1 + 0.2 * tt)
    return (["adv.wav", "glide.wav", "silence.wav", "tone16.wav"],
            [adversarial(12000), voiced(glide, SR), np.zeros(7000, np.float32), voiced(np.full(6400, 200.0), 16000)],
            [SR, SR, SR, 16000])


@pytest.fixture(scope="module")
def host_decoded(inv, sounds):
    """The definition on every sound at the model rate (the 16 kHz one through the device resampler, as generate_mels does)."""
    import torch
    from mbexwn_vocoder_amd import resample
    _, snds, rates = sounds
    prm, dec = f0track.params(SR), f0decode.decode_params()
    out = []
    for snd, rate in zip(snds, rates):
        if rate != SR:
            res, n_dev = resample.resample_device(torch.as_tensor(snd[None]).cuda(), torch.as_tensor(np.asarray([snd.size], np.int32)).cuda(),
                                                  rate, SR)
            snd = res[0, :int(n_dev[0])].cpu().numpy()
        out.append(f0decode.track_f0_viterbi_host(snd, timemap.centres(snd.size, inv.hop_size, SR, None), prm, dec))
    return out


def test_generate_mels_decodes_what_the_host_decodes(inv, sounds, host_decoded):
    _, snds, rates = sounds
    dec = f0decode.decode_params()
    plain = analysis.generate_mels(snds, rates, inv.preprocess_config, batch=3)
    got = []
    dicts = analysis.generate_mels(snds, rates, inv.preprocess_config, batch=3, f0_out=got, f0_decode=dec)
    on_host = []
    analysis.generate_mels(snds[:3], rates[:3], inv.preprocess_config, on_device=False, f0_out=on_host, f0_decode=dec)
    for ii, want in enumerate(host_decoded):
        assert np.array_equal(bits(dicts[ii]["mell"]), bits(plain[ii]["mell"]))
        assert got[ii][0].shape == got[ii][1].shape == (dicts[ii]["mell"].shape[1],)
        assert np.array_equal(bits(got[ii][0]), bits(want[0])) and np.array_equal(bits(got[ii][1]), bits(want[1])), ii
        if ii < 3:
            assert np.array_equal(bits(on_host[ii][0]), bits(want[0])) and np.array_equal(bits(on_host[ii][1]), bits(want[1])), ii
    assert np.all(got[2][0] == 0)                                        # silence
    # the greedy contour of the adversarial sound jumps; the decoded one does not
    greedy = []
    analysis.generate_mels(snds[:1], rates[:1], inv.preprocess_config, f0_out=greedy)
    assert np.count_nonzero(np.abs(1200 * np.log2(np.maximum(greedy[0][0][4:-4], 1e-9) / 110)) > 50) > 0
    assert np.max(np.abs(1200 * np.log2(got[0][0][4:-4] / 110))) < 5.0
    with pytest.raises(ValueError, match="f0_out"):
        analysis.generate_mels(snds[:1], rates[:1], inv.preprocess_config, f0_decode=dec)
    times, f0, per = inv.track_f0(snds[0], SR, on_device=True, decode=dec)
    assert np.array_equal(bits(f0), bits(host_decoded[0][0])) and np.array_equal(bits(per), bits(host_decoded[0][1]))


def test_transform_audio_runs_on_the_decoded_contour(inv, sounds, host_decoded):
    from mbexwn_vocoder_amd.noise import item_key
    names, snds, rates = sounds
    factors = [1.0, 1.25, 1.0, 0.8]
    dec = f0decode.decode_params()
    decoded = inv.transform_audio(snds, rates, names, transposition=factors, noise_seed=SEED, f0_source="audio", f0_decode=dec)
    scaled = [inv.scale_mel(dd) for dd in analysis.generate_mels(snds, rates, inv.preprocess_config)]
    rows = [np.full(int(mm.shape[1]), ff, dtype=np.float32) for mm, ff in zip(scaled, factors)]
    contours = [f0track.fill_unvoiced(ff) for ff, _ in host_decoded]
    routed = inv.synth_from_mels(scaled, noise_seed=SEED, noise_keys=[item_key(nn) for nn in names], transpositions=rows, f0s=contours)
    assert contours[2] is None
    for ii in range(4):
        assert np.array_equal(bits(decoded[ii]), bits(routed[ii])), ii
    greedy = inv.transform_audio(snds, rates, names, transposition=factors, noise_seed=SEED, f0_source="audio")
    assert not np.array_equal(bits(greedy[0]), bits(decoded[0]))          # the adversarial item: another contour, another audio
    with pytest.raises(ValueError, match="f0_decode"):
        inv.transform_audio(snds, rates, names, f0_decode=dec)


def test_no_decode_keeps_the_bits_and_the_launches(inv, sounds, monkeypatch):
    """Every entry point of the two headers makes one launch: the calls of the three are counted on the loaded library."""
    from mbexwn_vocoder_amd.engine import load_library
    names, snds, rates = sounds
    lib, calls = load_library(), []
    for symbol in ("mbxp_track_f0", "mbxc_f0_candidates", "mbxc_decode_f0"):
        def spy(*args, _real=getattr(lib, symbol), _name=symbol):
            calls.append(_name)
            return _real(*args)
        monkeypatch.setattr(lib, symbol, spy)

    def run(**kw):
        del calls[:]
        out = inv.transform_audio(snds, rates, names, noise_seed=SEED, f0_source="audio", max_batch=2, **kw)
        return out, list(calls)

    without, made = run()
    given, made_none = run(f0_decode=None)
    assert made == made_none == ["mbxp_track_f0"] * 3                    # two micro-batches at 24 kHz, one at 16 kHz
    for aa, bb in zip(without, given):
        assert np.array_equal(bits(aa), bits(bb))
    _, made_dec = run(f0_decode=f0decode.decode_params())
    assert made_dec == ["mbxc_f0_candidates", "mbxc_decode_f0"] * 3      # two launches in place of the tracker's


@pytest.mark.timeout(600)
def test_cli_decoded_f0_file_then_f0_dir(inv, model_dir, sounds, host_decoded, tmp_path):
    """generate_mel.py --write-f0 --pitch-decode viterbi, then resynth_mel.py --f0-dir: the 16-bit samples of
    synth_from_mel(f0=filled decoded contour) with the file's keyed noise."""
    from scipy.io import wavfile
    from mbexwn_vocoder_amd import flac
    from mbexwn_vocoder_amd.audioio import read_audio
    from mbexwn_vocoder_amd.fileio import load_var
    from mbexwn_vocoder_amd.noise import item_key
    _, snds, _ = sounds
    wav = str(tmp_path / "adv.wav")
    wavfile.write(wav, SR, snds[0])
    mells = str(tmp_path / "mells")
    res = run_script("generate_mel", [wav, "-o", mells, "--model_id", model_dir, "--write-f0", "--pitch-decode", "viterbi", "-q"])
    assert res.returncode == 0, res.stderr[-3000:]
    saved = load_var(os.path.join(mells, "adv.mell"))
    _, f0, per = f0track.read_f0(os.path.join(mells, "adv.f0"), n_frames=saved["mell"].shape[1])
    assert np.array_equal(bits(f0), bits(host_decoded[0][0])) and np.array_equal(bits(per), bits(host_decoded[0][1]))
    mell = os.path.join(mells, "adv.mell")
    want = inv.synth_from_mel(inv.scale_mel(saved), f0=f0track.fill_unvoiced(f0), noise_seed=SEED, noise_key=item_key(mell))
    want16 = flac.to_pcm16(want).astype(np.float32) / np.float32(32768.0)
    out = str(tmp_path / "out")
    res = run_script("resynth_mel", [model_dir, "-i", mell, "-o", out, "--f0-dir", mells, "--noise-seed", str(SEED),
                                     "--batch-invariant", "-q"])
    assert res.returncode == 0, res.stderr[-3000:]
    got, rate = read_audio(os.path.join(out, "syn_adv.flac"))
    assert rate == SR and np.array_equal(got, want16)
