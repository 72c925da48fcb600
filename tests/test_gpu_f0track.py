"""The F0 tracker on the GPU: mbxp_track_f0 (csrc/f0_track.hip) against its definition f0track.track_f0_host, bit for bit on
f0 and periodicity -- no tolerance: both sides make the same separately rounded float32 operations in the same order --, its
memory contract (outputs between guard bands, rows at or behind n_frames keep the fill) and its refusals."""
import ctypes

import numpy as np
import pytest

from guarded import Guarded
from mbexwn_vocoder_amd import f0track

pytestmark = pytest.mark.gpu
SR, HOP, STRIDE = 24000, 300, 6100
# (window, tau_min, tau_max): one partial sum per lane and the smallest frame; a middle one; the defaults at 24 kHz; L = 4095
SETS = [(64, 2, 5), (128, 3, 64), (1024, 24, 437), (2048, 2, 2047)]
E_DEFAULT = float(f0track.params(SR)["e_min"])
COMBOS = [(thr, e_min) for thr in (0.15, 1.5, 0.0) for e_min in (0.0, E_DEFAULT)]


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


@pytest.fixture(scope="module")
def items():
    """The ragged batch: (label, samples).  n = 0, 1, 37, 700 (shorter than the default L) and 6000, stride above them."""
    rng = np.random.default_rng(20)
    n = 6000
    tiny = (1e-17 * np.sin(2 * np.pi * 200.0 * np.arange(n) / SR)).astype(np.float32)
    dc = (0.5 + 0.3 * np.sin(2 * np.pi * 330.0 * np.arange(n) / SR)).astype(np.float32)
    broken = harmonic(n, 180.0, rng)
    broken[[900, 2400, 4000]] = [np.nan, np.inf, 1e20]
    return [("tone+noise", harmonic(n, 220.0, rng)), ("noise", (0.1 * rng.standard_normal(n)).astype(np.float32)),
            ("silence", np.zeros(n, np.float32)), ("tone 1e-17", tiny), ("tone + dc", dc), ("n=700", harmonic(700, 440.0, rng)),
            ("n=37", (0.1 * rng.standard_normal(37)).astype(np.float32)), ("n=1", np.ones(1, np.float32)),
            ("n=0", np.zeros(0, np.float32)), ("high tone", harmonic(n, 6000.0, rng, amp=0.5)), ("not finite", broken),
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


class Call:
    """One raw call of mbxp_track_f0 with its own buffers: the two outputs between guard bands, pre-filled."""

    def __init__(self, torch, sound, lengths, centres, counts, fill="nan"):
        from mbexwn_vocoder_amd.engine import load_library
        self.torch, self.lib = torch, load_library()
        self.sound = dev(torch, np.asarray(sound, np.float32))
        self.lengths, self.counts = dev(torch, np.asarray(lengths, np.int32)), dev(torch, np.asarray(counts, np.int32))
        self.centres = dev(torch, np.asarray(centres, np.int64))
        self.batch, self.frames = int(self.sound.shape[0]), int(self.centres.shape[1])
        self.f0 = Guarded("f0", 4 * self.batch * self.frames, fill, device="cuda")
        self.per = Guarded("periodicity", 4 * self.batch * self.frames, fill, device="cuda")

    def run(self, **kw):
        args = dict(audio=self.sound.data_ptr(), stride=int(self.sound.shape[1]), batch=self.batch, n_samples=self.lengths.data_ptr(),
                    centres=self.centres.data_ptr(), n_frames=self.counts.data_ptr(), max_frames=self.frames, sample_rate=SR,
                    window=1024, tau_min=24, tau_max=437, threshold=0.15, e_min=0.0, f0=self.f0.ptr, periodicity=self.per.ptr)
        args.update(kw)
        status = self.lib.mbxp_track_f0(args["audio"], args["stride"], args["batch"], args["n_samples"], args["centres"],
                                        args["n_frames"], args["max_frames"], args["sample_rate"], args["window"], args["tau_min"],
                                        args["tau_max"], ctypes.c_float(args["threshold"]), ctypes.c_float(args["e_min"]),
                                        args["f0"], args["periodicity"], None)
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


def padded(items, pad):
    sound = np.full((len(items), STRIDE), pad, dtype=np.float32)         # behind every item's end: never read
    for ii, (_, x) in enumerate(items):
        sound[ii, :x.size] = x
    return sound, [x.size for _, x in items]


@pytest.mark.parametrize("window,tau_min,tau_max", SETS)
def test_kernel_equals_the_host_definition_bit_for_bit(torch, items, window, tau_min, tau_max):
    word = {"nan": -1, "huge": int(np.float32(1e30).view(np.int32))}
    modes = ["one"] if window == 2048 else [True, False]
    voiced = 0
    for mode, fill, pad in zip(modes, ("nan", "huge"), (np.nan, 1e30)):
        table, counts = centre_tables(items, mode)
        sound, lengths = padded(items, pad)
        base = {"sample_rate": SR, "window": window, "tau_min": tau_min, "tau_max": tau_max, "threshold": 0.15, "e_min": 0.0}
        halves = [f0track.difference_host(x, table[ii, :counts[ii]], base) for ii, (_, x) in enumerate(items)]
        call = Call(torch, sound, lengths, table, counts, fill=fill)
        for thr, e_min in COMBOS:
            prm = dict(base, threshold=float(np.float32(thr)), e_min=e_min)
            call.f0.refill()
            call.per.refill()
            assert call.run(window=window, tau_min=tau_min, tau_max=tau_max, threshold=thr, e_min=e_min) == 0
            call.check()                                                 # the guards around both outputs keep the pattern
            got_f0, got_per = call.results()
            raw_f0, raw_per = call.results(torch.int32)
            for ii, (label, x) in enumerate(items):
                want_f0, want_per = f0track.pick_host(*halves[ii], prm)
                what = (label, mode, thr, e_min)
                assert np.array_equal(bits(got_f0[ii, :counts[ii]]), bits(want_f0)), (what, got_f0[ii, :counts[ii]], want_f0)
                assert np.array_equal(bits(got_per[ii, :counts[ii]]), bits(want_per)), (what, got_per[ii, :counts[ii]], want_per)
                assert np.all(raw_f0[ii, counts[ii]:] == word[fill]) and np.all(raw_per[ii, counts[ii]:] == word[fill]), what
                if label == "not finite":                                # the frames over the three samples: unvoiced
                    assert halves[ii][2].any() and np.all(want_f0[halves[ii][2]] == 0)
                if thr == 0.0:
                    assert np.all(want_f0 == 0)                          # the arg-min path: never a pick
                voiced += int(np.count_nonzero(want_f0))
        # the whole path through the module's wrapper gives the same tensors
        f0_dev, per_dev = f0track.track_f0_device(dev(torch, sound), dev(torch, np.asarray(lengths, np.int32)), dev(torch, table),
                                                  dev(torch, np.asarray(counts, np.int32)), dict(base, threshold=float(np.float32(0.15))))
        for ii, (label, x) in enumerate(items):
            want_f0, want_per = f0track.pick_host(*halves[ii], dict(base, threshold=float(np.float32(0.15))))
            assert np.array_equal(bits(f0_dev[ii, :counts[ii]].cpu().numpy()), bits(want_f0)), label
            assert np.array_equal(bits(per_dev[ii, :counts[ii]].cpu().numpy()), bits(want_per)), label
    assert voiced > 0                                                    # the comparison saw picks, not only zeros


def test_wrong_table_entries_are_clamped(torch, items):
    """n_samples of -3 and stride + 10 behave as 0 and stride; a count above max_frames and a negative one write max_frames
    rows and none."""
    x = items[0][1]
    sound = np.zeros((3, STRIDE), np.float32)
    sound[:, :x.size] = x
    cc = np.array([[300, 3000, 5700, 6099]] * 3, dtype=np.int64)
    call = Call(torch, sound, [-3, STRIDE + 10, x.size], cc, [4, 4 + 3, -2])
    assert call.run() == 0
    call.check()
    f0, per = call.results()
    assert np.all(f0[0] == 0) and np.all(per[0] == 1)                    # an empty item: silence
    want = f0track.track_f0_host(sound[1], cc[1], dict(f0track.params(SR), e_min=0.0))
    assert np.array_equal(bits(f0[1]), bits(want[0])) and np.array_equal(bits(per[1]), bits(want[1]))
    raw = call.results(torch.int32)
    assert np.all(raw[0][2] == -1) and np.all(raw[1][2] == -1)           # a negative count: nothing written


def test_refusals_leave_the_outputs_untouched(torch, items):
    sound, lengths = padded(items[:2], 0.0)
    table = np.tile(np.arange(0, 6001, HOP, dtype=np.int64), (2, 1))
    call = Call(torch, sound, lengths, table, [table.shape[1]] * 2, fill="huge")

    def why():
        return call.lib.mbx_last_error().decode()

    cases = [({name: None}, "null") for name in ("audio", "n_samples", "centres", "n_frames", "f0", "periodicity")]
    cases += [({"window": 0}, "window"), ({"window": 32}, "window"), ({"window": 96}, "window"), ({"window": 2112}, "window"),
              ({"tau_max": 1}, "tau_max"), ({"tau_min": 437}, "tau_min"), ({"tau_min": -1}, "tau_min"),
              ({"tau_min": 2, "tau_max": 2}, "tau_min"), ({"window": 2048, "tau_max": 2049}, "4096"),
              ({"sample_rate": 0}, "sample_rate"), ({"threshold": float("nan")}, "threshold"),
              ({"max_frames": 0}, "max_frames"), ({"stride": 0}, "stride"), ({"batch": -1}, "batch"), ({"batch": 65536}, "batch")]
    for kw, what in cases:
        assert call.run(**kw) == 1, kw                                   # MBX_ERR_INVALID_ARGUMENT
        assert why().startswith("track f0:") and what in why(), (kw, why())
        assert call.untouched(), kw
        call.check()
    assert call.run(batch=0) == 0 and call.untouched()                   # nothing to do
    assert call.run() == 0 and not call.untouched()                      # and the same buffers do run
