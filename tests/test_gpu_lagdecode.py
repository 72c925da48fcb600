"""The fixed-lag F0 decoder on the GPU (csrc/f0_lag.hip through include/mbexwn_live_contour.h, live.py):
mbxv_f0_candidate_frames on rings against f0decode.candidates_host on the whole sound; mbxv_decode_f0_frames against
f0decode.viterbi_lag_host however the frames are cut into calls; both entry points between guard bands and their refusals; a
decoding StreamingAnalyzer; the live pipeline with f0_lag against transform_audio(f0_lag=, f0_fill="hold"); the tool.  Every
comparison is on bits: both sides make the same separately rounded float32 operations in the same order."""
import ctypes
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

from guarded import FILLS, GuardSet, fill_word
from mbexwn_vocoder_amd import f0decode, f0track
from mbexwn_vocoder_amd.live_plan import f0_frames_ready, frames_total

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "mbexwn_vocoder_amd", "bin", "stream_transpose.py")
BIN = os.path.join(ROOT, "mbexwn_vocoder_amd", "bin")
SMALL_MODEL = {"mbexwn_config:pp_mod_subnet:n_channels": 32, "mbexwn_config:pp_mod_subnet:n_layers": 5}
SR, SEED = 24000, 7
# (window, tau_min, tau_max, hop) of tests/test_gpu_live_pitch.py: the smallest frame with an odd L = 69; the defaults at 24 kHz
SETS = {"small": (64, 2, 5, 16), "default": (1024, 24, 437, 300)}
TINY16 = {"sample_rate": SR, "hop_size": 16, "win_size": 48, "fft_size": 64, "mel_channels": 8, "fmin": 0.0, "fmax": None,
          "lin_amp_off": 1e-5, "lin_amp_scale": 1, "mel_amp_scale": 1}
FPP = ctypes.POINTER(ctypes.c_float)
LAGS = (0, 1, 8, 63, 128)


def bits(arr):
    return np.ascontiguousarray(arr, dtype=np.float32).view(np.uint32)


def same(one, other):
    return all(aa.shape == bb.shape and np.array_equal(bits(aa), bits(bb)) for aa, bb in zip(one, other))


def harmonic(n, f0, rng, noise=1e-3, amp=0.5):
    tt = np.arange(n) / SR
    x = sum((amp / h) * np.sin(2 * np.pi * f0 * h * tt + h) for h in range(1, 9))
    return (x + noise * rng.standard_normal(n)).astype(np.float32)


def adversarial(n=24000):
    """The sound of tests/test_f0decode_host.py that the greedy pick gets wrong, one second of it."""
    t = np.arange(n) / SR
    am = 0.3 + 0.2 * np.sin(2 * np.pi * 3 * t)
    x = 0.3 * sum(((1 if h % 2 == 0 else am) / h) * np.sin(2 * np.pi * h * 110 * t + h) for h in range(1, 13))
    return (x + 1e-3 * np.random.default_rng(1).standard_normal(n)).astype(np.float32)


def config_of(name):
    from mbexwn_vocoder_amd.config import canonical_config
    return TINY16 if name == "small" else canonical_config("SPEECH")["preprocess_config"]


def params_of(name, e_min=None):
    window, tau_min, tau_max, _ = SETS[name]
    default = float(f0track.params(SR, window=window)["e_min"])
    return {"sample_rate": SR, "window": window, "tau_min": tau_min, "tau_max": tau_max, "threshold": float(np.float32(0.15)),
            "e_min": default if e_min is None else e_min}


def random_cuts(rng, n, hop):
    cuts, left = [], n
    while left:
        kind = int(rng.integers(0, 3))
        cc = 1 if kind == 0 else int(rng.integers(2, hop + 1)) if kind == 1 else int(rng.integers(hop, 3 * hop + 1))
        cc = min(cc, left)
        cuts.append(cc)
        left -= cc
    return cuts


def random_tables(rng, batch, frames):
    """The hand-made tables of tests/test_gpu_f0decode.py: costs from {0, 0.25, 0.5, 1} and periods from {50, 100, 200}, so
    that ties occur; 0 .. 7 used slots per frame; NaN, inf, negative and 1e7 entries sprinkled over both tables."""
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


def decode_sets(name):
    """(label, decode_params, e_min): n_cand 1 and 7, N = 1 and 16, e_min 0 and the default."""
    default = params_of(name)["e_min"]
    return [("defaults", f0decode.decode_params(), 0.0), ("n_cand 1", f0decode.decode_params(n_cand=1), default),
            ("N = 1", f0decode.decode_params(n_cand=7, thresholds=[0.15], weights=[0.75]), default),
            ("N = 1, n_cand 1", f0decode.decode_params(n_cand=1, thresholds=[0.3], weights=[1.0]), 0.0)]


@pytest.fixture(scope="module")
def lib():
    from mbexwn_vocoder_amd.engine import load_library
    return load_library()


def candidate_frames(lib, rings, ring_samples, desc, max_new, hop, prm, dec, out, n_streams=None):
    import torch
    th, ww = np.ascontiguousarray(dec["thresholds"], np.float32), np.ascontiguousarray(dec["weights"], np.float32)
    return lib.mbxv_f0_candidate_frames(rings.data_ptr(), int(rings.shape[0]), ring_samples, desc.data_ptr(),
                                        int(desc.shape[0]) if n_streams is None else n_streams, max_new, hop, SR, prm["window"],
                                        prm["tau_min"], prm["tau_max"], ctypes.c_float(prm["e_min"]), th.ctypes.data_as(FPP),
                                        ww.ctypes.data_as(FPP), int(th.size), int(dec["n_cand"]), *(tt.data_ptr() for tt in out),
                                        torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------------------------------
# the candidates of a stream's frames, from its ring
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SETS))
def test_candidate_frames_equal_the_host_definition_under_random_cuts(lib, name):
    """Tracking streams of a StreamingAnalyzer keep the rings (one of them resampled on the device from 44.1 kHz); behind every
    tick the entry point runs on those rings for the frames the tick handed out -- of open streams and, at the end, of closed
    ones.  Concatenated, the tables of a stream are candidates_host on its whole model-rate sound."""
    import torch
    from mbexwn_vocoder_amd import resample
    from mbexwn_vocoder_amd.live import StreamingAnalyzer
    cfg, hop = config_of(name), SETS[name][3]
    rng = np.random.default_rng(51)
    tone = 6000.0 if name == "small" else 196.0                      # a pitch the parameter set can find
    broken = harmonic(3000, 180.0, rng)
    broken[[900, 2400]] = [np.nan, 1e20]
    tt = np.arange(3000) / 44100.0
    sounds = {"tone": (harmonic(4000, tone, rng), SR), "not finite": (broken, SR), "n=37": ((0.1 * rng.standard_normal(37)).astype(np.float32), SR),
              "n=1": (np.ones(1, np.float32), SR),
              "resampled": ((0.4 * np.sin(2 * np.pi * tone * tt) + 1e-3 * rng.standard_normal(3000)).astype(np.float32), 44100)}
    whole = {}
    for kk, (x, rate) in sounds.items():
        if rate != SR:
            res, n_dev = resample.resample_device(torch.as_tensor(x[None]).cuda(), torch.as_tensor(np.asarray([x.size], np.int32)).cuda(), rate, SR)
            x = res[0, :int(n_dev[0])].cpu().numpy()
        whole[kk] = x
    sets = decode_sets(name) if name == "small" else decode_sets(name)[:1]
    an = StreamingAnalyzer(cfg, slots=2)
    for kk, (x, rate) in sounds.items():
        an.open(kk, sample_rate=rate, f0_params=params_of(name))
    cuts = {kk: random_cuts(rng, x.size, (8 if name == "small" else 1) * hop * rate // SR) for kk, (x, rate) in sounds.items()}
    got = {kk: [[] for _ in sets] for kk in sounds}
    pos, step = dict.fromkeys(sounds, 0), dict.fromkeys(sounds, 0)
    was_open = set()
    while not all(an.finished(kk) for kk in sounds):
        for kk, (x, _) in sounds.items():
            if step[kk] < len(cuts[kk]):
                end = pos[kk] + cuts[kk][step[kk]]
                an.push(kk, x[pos[kk]:end], last=end == x.size)
                pos[kk], step[kk] = end, step[kk] + 1
        before = {kk: an.streams[kk].emitted for kk in sounds}
        rows = an.tick()
        work = [(kk, before[kk], mel.shape[0]) for kk, mel in rows.items()]
        if not work:
            continue
        was_open.update(kk for kk, _, _ in work if not an.streams[kk].closed)
        desc = torch.as_tensor(np.asarray([[an.streams[kk].slot, first, nn, an.streams[kk].have if an.streams[kk].closed else -1]
                                           for kk, first, nn in work], np.int64)).cuda()
        max_new = max(nn for _, _, nn in work)
        for si, (_, dec, e_min) in enumerate(sets):
            out = [torch.full((len(work), max_new, 8), np.nan, dtype=torch.float32, device="cuda") for _ in range(3)]
            assert candidate_frames(lib, an.rings, an.ring_samples, desc, max_new, hop, params_of(name, e_min), dec, out) == 0
            host = [tt.cpu().numpy() for tt in out]
            for row, (kk, _, nn) in enumerate(work):
                got[kk][si].append([tt[row, :nn] for tt in host])
                assert all(np.all(np.isnan(tt[row, nn:])) for tt in host)            # rows behind n_frames are not written
    assert {"tone", "resampled"} <= was_open                              # frames of open streams were compared, and closed ones
    used = 0
    for kk, x in whole.items():
        centres = np.arange(0, x.size + 1, hop)
        for si, (label, dec, e_min) in enumerate(sets):
            prm = params_of(name, e_min)
            want = f0decode.candidates_host(*f0track.difference_host(x, centres, prm), prm, dec)
            tables = [np.concatenate([part[ii] for part in got[kk][si]]) for ii in range(3)]
            assert same(tables, want), (kk, label)
            used += int(np.count_nonzero(want[0]))
    assert used > 0                                                      # the comparison saw candidates, not only empty slots


RING, HOP = 128, 16
DESC = [[0, 7, 4, -1], [1, 0, 4, 60], [2, 0, 0, -1], [3, 0, 1, 60], [-1, 0, 1, 60], [1, -1, 1, 60]]
SMALL_PRM = {"sample_rate": SR, "window": 64, "tau_min": 2, "tau_max": 5, "threshold": float(np.float32(0.15)), "e_min": 0.0}


def raw_buffers(fill):
    """The buffers of tests/test_gpu_live_pitch.py: three rings of 128 samples, the small parameter set (L = 69, hop 16).
    Slot 0: a running stream that holds its samples [72, 200).  Slot 1: a closed stream of 60 samples, frames 0 .. 3.  Slot 2:
    nothing to do.  Then three rows to skip: a slot outside the store, a negative slot, a negative first frame."""
    import torch
    rng = np.random.default_rng(9)
    running, closed = harmonic(200, 6000.0, rng, amp=0.3), harmonic(60, 8000.0, rng, amp=0.3)
    gs = GuardSet(fill, device="cuda")
    rings = gs.new("rings", 3 * RING * 4)
    view = rings.view(torch.float32, 3, RING)
    idx = np.arange(72, 200)
    view[0, torch.as_tensor(idx & (RING - 1)).cuda()] = torch.as_tensor(running[idx]).cuda()
    view[1, :60] = torch.as_tensor(closed).cuda()
    tables = [gs.new(label, len(DESC) * 5 * 8 * 4) for label in ("period", "cost", "dprime")]
    return dict(gs=gs, running=running, closed=closed, rings=rings, desc=gs.put("desc", np.asarray(DESC, dtype=np.int64)), tables=tables)


def call_candidates(lib, buf, **change):
    import torch
    dec = f0decode.decode_params()
    th, ww = np.ascontiguousarray(dec["thresholds"], np.float32), np.ascontiguousarray(dec["weights"], np.float32)
    args = dict(rings=buf["rings"].ptr, n_slots=3, ring_samples=RING, desc=buf["desc"].ptr, n_streams=len(DESC), max_new_frames=5,
                hop=HOP, sample_rate=SR, window=64, tau_min=2, tau_max=5, e_min=0.0, thresholds=th.ctypes.data_as(FPP),
                weights=ww.ctypes.data_as(FPP), n_thresholds=int(th.size), n_cand=7, period=buf["tables"][0].ptr,
                cost=buf["tables"][1].ptr, dprime=buf["tables"][2].ptr)
    args.update(change)
    return lib.mbxv_f0_candidate_frames(args["rings"], args["n_slots"], args["ring_samples"], args["desc"], args["n_streams"],
                                        args["max_new_frames"], args["hop"], args["sample_rate"], args["window"], args["tau_min"],
                                        args["tau_max"], ctypes.c_float(args["e_min"]), args["thresholds"], args["weights"],
                                        args["n_thresholds"], args["n_cand"], args["period"], args["cost"], args["dprime"],
                                        torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("fill", FILLS)
def test_candidate_frames_between_guard_bands(lib, fill):
    import torch
    buf = raw_buffers(fill)
    word = fill_word(fill)
    before = buf["rings"].view(torch.int32).clone()
    assert call_candidates(lib, buf) == 0, lib.mbx_last_error()
    torch.cuda.synchronize()
    buf["gs"].check()
    dec = f0decode.decode_params()
    x = np.concatenate((buf["running"], np.zeros(100, np.float32)))     # any sound that continues the 200 samples
    want_running = f0decode.candidates_host(*f0track.difference_host(x, HOP * np.arange(7, 11), SMALL_PRM), SMALL_PRM, dec)
    want_closed = f0decode.candidates_host(*f0track.difference_host(buf["closed"], HOP * np.arange(4), SMALL_PRM), SMALL_PRM, dec)
    for got, want_r, want_c in zip(buf["tables"], want_running, want_closed):
        out = got.view(torch.float32, len(DESC), 5, 8).cpu().numpy()
        assert np.array_equal(bits(out[0, :4]), bits(want_r)) and np.array_equal(bits(out[1, :4]), bits(want_c)), got.name
        raw = out.view(np.int32)
        assert np.all(raw[0, 4:] == word) and np.all(raw[1, 4:] == word)             # rows behind n_frames keep the fill
        assert np.all(raw[2:] == word)                                               # no frames; the three skipped rows
    assert np.count_nonzero(want_running[0]) and np.all(np.isfinite(want_closed[2]))
    assert torch.equal(buf["rings"].view(torch.int32), before)                       # the input is an input


def test_candidate_frames_refusals_leave_the_tables_untouched(lib):
    import torch
    buf = raw_buffers("huge")

    def host(values):
        arr = np.asarray(values, np.float32)
        return arr, arr.ctypes.data_as(FPP)

    broken = [host(vv) for vv in ([0.1, np.nan], [0.2, 0.1], [0.1, 0.1], [0.5, -1.0], [np.inf, 0.5])]
    cases = [dict(rings=None), dict(desc=None), dict(period=None), dict(cost=None), dict(dprime=None), dict(thresholds=None),
             dict(weights=None), dict(n_streams=-1), dict(n_streams=65536), dict(max_new_frames=-1), dict(n_slots=0), dict(hop=0),
             dict(sample_rate=0), dict(window=0), dict(window=32), dict(window=96), dict(window=2112), dict(tau_max=1), dict(tau_min=-1),
             dict(tau_min=5), dict(window=2048, tau_max=2049, ring_samples=8192), dict(e_min=float("nan")), dict(ring_samples=0),
             dict(ring_samples=96), dict(ring_samples=64), dict(ring_samples=1024, window=1024, tau_max=437),
             dict(n_thresholds=0), dict(n_thresholds=17), dict(n_cand=0), dict(n_cand=8)]
    cases += [dict(thresholds=bb[1], n_thresholds=2) for bb in broken[:3]] + [dict(weights=bb[1], n_thresholds=2) for bb in broken[3:]]
    for change in cases:
        status = call_candidates(lib, buf, **change)
        message = lib.mbx_last_error().decode()
        assert status == 1 and message.startswith("f0 candidate frames:") and len(message) > 24, (change, status, message)
    torch.cuda.synchronize()
    assert all(tt.payload_untouched() for tt in buf["tables"])
    buf["gs"].check()
    assert call_candidates(lib, buf, n_streams=0) == 0 and call_candidates(lib, buf, max_new_frames=0) == 0      # nothing to do
    torch.cuda.synchronize()
    assert all(tt.payload_untouched() for tt in buf["tables"])
    assert call_candidates(lib, buf) == 0                                             # and the same buffers do run
    torch.cuda.synchronize()
    assert not any(tt.payload_untouched() for tt in buf["tables"])
    buf["gs"].check()


# ---------------------------------------------------------------------------------------------------------------------
# the recursion, continued call by call
# ---------------------------------------------------------------------------------------------------------------------
class LagCalls:
    """The streams of one launch: their whole tables on the host, a state store of `n_slots` rows and the outputs between
    guard bands; `feed` uploads the next frames of every stream, calls the entry point once and collects what was decided."""

    def __init__(self, lib, tables, counts, lag, fill="nan", n_slots=None, slots=None):
        import torch
        self.torch, self.lib, self.tables, self.counts, self.lag = torch, lib, tables, list(counts), lag
        self.batch = len(self.counts)
        self.slots = list(range(self.batch)) if slots is None else list(slots)
        self.n_slots = n_slots or max(self.slots) + 1
        self.words = int(lib.mbxv_lag_state_words())
        self.gs = GuardSet(fill, device="cuda")
        self.state = self.gs.new("state", self.n_slots * self.words * 4)
        for slot in self.slots:
            self.state.view(torch.int32, self.n_slots, self.words)[slot].zero_()     # a fresh stream: a zero-filled row
        self.done = [0] * self.batch
        self.decided = [0] * self.batch
        self.got = [([], []) for _ in range(self.batch)]
        self.word = fill_word(fill)

    def feed(self, chunk, w_jump=4.0, w_switch=0.5, max_new=None, close=True):
        torch = self.torch
        n = [min(chunk, kk - dd) for kk, dd in zip(self.counts, self.done)]
        max_new = max(max(n), 1) if max_new is None else max_new
        parts = [np.full((self.batch, max_new, 8), 7.0, np.float32) for _ in range(3)]
        for bb in range(self.batch):
            for part, tab in zip(parts, self.tables):
                part[bb, :n[bb]] = tab[bb, self.done[bb]:self.done[bb] + n[bb]]
        final = [close and dd + nn >= kk for dd, nn, kk in zip(self.done, n, self.counts)]
        # hop 1: a closed stream of T frames has n_total = T - 1
        desc = np.asarray([[self.slots[bb], self.done[bb], n[bb], self.counts[bb] - 1 if final[bb] else -1] for bb in range(self.batch)],
                          np.int64)
        max_out = max_new + self.lag
        dev = [self.gs.put(label, part) for label, part in zip(("period", "cost", "dprime"), parts)]
        desc_dev = self.gs.put("desc", desc)
        f0, per = self.gs.new("f0", self.batch * max_out * 4), self.gs.new("periodicity", self.batch * max_out * 4)
        status = self.lib.mbxv_decode_f0_frames(dev[0].ptr, dev[1].ptr, dev[2].ptr, desc_dev.ptr, self.batch, max_new, 1, self.state.ptr,
                                                self.n_slots, self.lag, SR, ctypes.c_float(w_jump), ctypes.c_float(w_switch), f0.ptr,
                                                per.ptr, max_out, torch.cuda.current_stream().cuda_stream)
        assert status == 0, self.lib.mbx_last_error()
        torch.cuda.synchronize()
        self.gs.check()
        out = [gg.view(torch.float32, self.batch, max_out).cpu().numpy() for gg in (f0, per)]
        for bb in range(self.batch):
            self.done[bb] += n[bb]
            target = max(self.decided[bb], f0decode.lag_frames_decided(self.done[bb], self.lag, final[bb]))
            count = target - self.decided[bb]
            assert count <= n[bb] + self.lag
            for kk in (0, 1):
                self.got[bb][kk].append(out[kk][bb, :count].copy())
                assert np.all(out[kk].view(np.int32)[bb, count:] == self.word), bb   # entries behind the decided count are untouched
            self.decided[bb] = target
        del self.gs.buffers[1:]                                          # the state stays; the call's own buffers go

    def results(self, bb):
        return tuple(np.concatenate(self.got[bb][kk]) for kk in (0, 1))


@pytest.mark.parametrize("lag", LAGS)
def test_decode_frames_equal_the_host_definition_for_every_cut(lib, lag):
    """One launch holds streams of T in {1, 2, lag, lag + 1, 37, 300} frames, fed in chunks of 1, 7, 64, 65 and 150 frames, each
    with the four weight pairs: 65 crosses the 64-frame sub-chunk, 300 frames wrap the 256-frame ring."""
    rng = np.random.default_rng(61 + lag)
    counts = [1, 2, max(lag, 1), lag + 1, 37, 300]
    tables = random_tables(rng, len(counts), 300)
    voiced, fills = 0, iter(FILLS * 7)
    for w_jump in (0.0, 4.0):
        for w_switch in (0.0, 0.5):
            dec = f0decode.decode_params(w_jump=w_jump, w_switch=w_switch)
            wants = [f0decode.viterbi_lag_host(*(tt[bb, :kk] for tt in tables), SR, dec, lag) for bb, kk in enumerate(counts)]
            for want in wants:
                assert np.all(np.isin(want[0], [0, SR / 50, SR / 100, SR / 200]))    # no sprinkled entry reaches f0
                voiced += int(np.count_nonzero(want[0]))
            for chunk in (1, 7, 64, 65, 150):
                calls = LagCalls(lib, tables, counts, lag, fill=next(fills))
                while any(dd < kk for dd, kk in zip(calls.done, counts)):
                    calls.feed(chunk, w_jump, w_switch)
                for bb, want in enumerate(wants):
                    assert same(calls.results(bb), want), (lag, w_jump, w_switch, chunk, bb)
    assert voiced > 0
    # the end told by a call of its own with no frame in it
    short = [1, 2, 37]
    calls = LagCalls(lib, tuple(tt[:3] for tt in tables), short, lag)
    dec = f0decode.decode_params()
    while any(dd < kk for dd, kk in zip(calls.done, short)):
        calls.feed(5, close=False)
    calls.feed(5, close=True)
    for bb, kk in enumerate(short):
        assert same(calls.results(bb), f0decode.viterbi_lag_host(*(tt[bb, :kk] for tt in tables), SR, dec, lag)), (lag, bb)


def test_decode_frames_have_no_frame_limit(lib):
    """20000 frames in a single call, and through decode_lag_device: nothing but the ring is kept."""
    import torch
    tables = random_tables(np.random.default_rng(62), 1, 20000)
    dec = f0decode.decode_params()
    want = f0decode.viterbi_lag_host(*(tt[0] for tt in tables), SR, dec, 8)
    calls = LagCalls(lib, tables, [20000], 8)
    calls.feed(20000)
    assert same(calls.results(0), want) and np.count_nonzero(want[0]) > 1000
    dev = [torch.as_tensor(tt).cuda() for tt in tables]
    f0, per = f0decode.decode_lag_device(*dev, torch.as_tensor(np.asarray([20000], np.int32)).cuda(), SR, dec, 8)
    assert same((f0[0].cpu().numpy(), per[0].cpu().numpy()), want)
    # a ragged batch through the wrapper: counts below 0 and above max_frames are clamped, rows behind a count stay zero
    ragged = random_tables(np.random.default_rng(63), 4, 90)
    counts = [-4, 1, 37, 900]
    for lag in (0, 8, 128):
        f0, per = f0decode.decode_lag_device(*(torch.as_tensor(tt).cuda() for tt in ragged), torch.as_tensor(np.asarray(counts, np.int32)).cuda(),
                                             SR, dec, lag)
        assert f0.shape == per.shape == (4, 90)
        for bb, kk in enumerate(np.clip(counts, 0, 90)):
            want = f0decode.viterbi_lag_host(*(tt[bb, :kk] for tt in ragged), SR, dec, lag)
            assert same((f0[bb, :kk].cpu().numpy(), per[bb, :kk].cpu().numpy()), want), (lag, bb)
            assert not f0[bb, kk:].any() and not per[bb, kk:].any()
    assert same(tuple(tt.cpu().numpy() for tt in f0decode.decode_lag_device(*(torch.as_tensor(tt).cuda() for tt in ragged),
                                                                          torch.as_tensor(np.asarray([90] * 4, np.int32)).cuda(), SR, dec, 128)),
                tuple(tt.cpu().numpy() for tt in f0decode.decode_device(*(torch.as_tensor(tt).cuda() for tt in ragged),
                                                                      torch.as_tensor(np.asarray([90] * 4, np.int32)).cuda(), SR, dec)))


@pytest.mark.parametrize("fill", FILLS)
def test_decode_frames_memory_contract(lib, fill):
    """A state store of six rows between guard bands; streams in slots 4 and 1; rows to skip: a slot outside the store, a
    negative slot, a negative first frame and a first frame that is not the state's `done`; and a row with nothing to do.  The
    skipped rows' outputs and states, and the state rows of no stream, keep every bit."""
    import torch
    rng = np.random.default_rng(64)
    tables = random_tables(rng, 6, 40)
    words = int(lib.mbxv_lag_state_words())
    calls = LagCalls(lib, tuple(tt[:2] for tt in tables), [40, 23], 8, fill=fill, n_slots=6, slots=[4, 1])
    calls.feed(15)                                                        # both streams have seen 15 frames
    state = calls.state.view(torch.int32, 6, words)
    before = state.clone()
    word = fill_word(fill)
    for slot in (0, 2, 3, 5):
        assert torch.all(before[slot] == word)                            # the rows of no stream: the call above left them
    assert int(before[4, 0]) == int(before[1, 0]) == 15 and int(before[4, 1]) == int(before[1, 1]) == 7
    desc = np.asarray([[4, 15, 10, -1], [6, 15, 10, -1], [-1, 15, 10, -1], [1, -1, 10, -1], [1, 14, 10, -1], [1, 16, 10, 22], [2, 0, 0, 5]],
                      np.int64)
    gs = GuardSet(fill, device="cuda")
    parts = [np.ascontiguousarray(np.broadcast_to(tt[0, 15:25], (len(desc), 10, 8))) for tt in tables]
    dev = [gs.put(label, part) for label, part in zip(("period", "cost", "dprime"), parts)]
    desc_dev = gs.put("desc", desc)
    f0, per = gs.new("f0", len(desc) * 18 * 4), gs.new("periodicity", len(desc) * 18 * 4)
    status = lib.mbxv_decode_f0_frames(dev[0].ptr, dev[1].ptr, dev[2].ptr, desc_dev.ptr, len(desc), 10, 1, calls.state.ptr, 6, 8, SR,
                                       ctypes.c_float(4.0), ctypes.c_float(0.5), f0.ptr, per.ptr, 18, torch.cuda.current_stream().cuda_stream)
    assert status == 0, lib.mbx_last_error()
    torch.cuda.synchronize()
    gs.check()
    calls.gs.check()
    after = calls.state.view(torch.int32, 6, words)
    # no stream's row, and the skipped stream's, keep every bit.  So does row 2, named by the last descriptor with first frame
    # 0 and no frame to see: under the nan and huge fills its `done` word is not 0 and the row is skipped; under the zero fill
    # it is a stream without a frame that stays open (0 frames are not the n_total / hop + 1 = 6 of its end), and writing its
    # head back leaves 4384 zeros.
    for slot in (0, 1, 2, 3, 5):
        assert torch.equal(after[slot], before[slot]), (fill, slot)
    assert int(after[4, 0]) == 25 and int(after[4, 1]) == 17 and not torch.equal(after[4], before[4])
    assert torch.all(after[2] == word)
    want = f0decode.viterbi_lag_host(*(tt[0, :25] for tt in tables), SR, f0decode.decode_params(), 8)
    raw = [gg.view(torch.float32, len(desc), 18).cpu().numpy() for gg in (f0, per)]
    for kk in (0, 1):
        assert np.array_equal(bits(raw[kk][0, :10]), bits(want[kk][7:17]))
        assert np.all(raw[kk].view(np.int32)[0, 10:] == word) and np.all(raw[kk].view(np.int32)[1:] == word)


def test_decode_frames_refusals_leave_outputs_and_state_untouched(lib):
    import torch
    words = int(lib.mbxv_lag_state_words())
    gs = GuardSet("huge", device="cuda")
    tables = [gs.put(label, part[0]) for label, part in zip(("period", "cost", "dprime"), random_tables(np.random.default_rng(65), 1, 4))]
    desc = gs.put("desc", np.asarray([[0, 0, 4, -1]], np.int64))
    state, f0, per = gs.new("state", words * 4), gs.new("f0", 12 * 4), gs.new("periodicity", 12 * 4)
    good = dict(period=tables[0].ptr, cost=tables[1].ptr, dprime=tables[2].ptr, desc=desc.ptr, n_streams=1, max_new_frames=4, hop=300,
                state=state.ptr, n_slots=1, lag=8, sample_rate=SR, w_jump=4.0, w_switch=0.5, f0=f0.ptr, periodicity=per.ptr, max_out=12)

    def call(**kw):
        aa = dict(good, **kw)
        return lib.mbxv_decode_f0_frames(aa["period"], aa["cost"], aa["dprime"], aa["desc"], aa["n_streams"], aa["max_new_frames"],
                                         aa["hop"], aa["state"], aa["n_slots"], aa["lag"], aa["sample_rate"], ctypes.c_float(aa["w_jump"]),
                                         ctypes.c_float(aa["w_switch"]), aa["f0"], aa["periodicity"], aa["max_out"],
                                         torch.cuda.current_stream().cuda_stream)

    cases = [{name: None} for name in ("period", "cost", "dprime", "desc", "state", "f0", "periodicity")]
    cases += [{"n_streams": -1}, {"n_streams": 65536}, {"max_new_frames": -1}, {"hop": 0}, {"n_slots": 0}, {"lag": -1}, {"lag": 129},
              {"max_out": 11}, {"lag": 128, "max_out": 131}, {"sample_rate": 0}]
    cases += [{key: vv} for key in ("w_jump", "w_switch") for vv in (float("nan"), -0.5, 1.5e6, float("inf"))]
    for kw in cases:
        status = call(**kw)
        message = lib.mbx_last_error().decode()
        assert status == 1 and message.startswith("decode f0 frames:") and len(message) > 20, (kw, status, message)
    assert call(n_streams=0) == 0
    torch.cuda.synchronize()
    assert state.payload_untouched() and f0.payload_untouched() and per.payload_untouched()
    gs.check()
    # a state row of the fill is no stream at frame 0: the row is skipped; zeroed, the same buffers do run
    assert call() == 0
    torch.cuda.synchronize()
    assert state.payload_untouched() and f0.payload_untouched()
    state.view(torch.int32).zero_()
    assert call() == 0
    torch.cuda.synchronize()
    assert int(state.view(torch.int32)[0]) == 4 and f0.payload_untouched()            # 4 frames seen, none decided at lag 8
    assert call(desc=gs.put("closing", np.asarray([[0, 4, 0, 3 * 300]], np.int64)).ptr) == 0
    torch.cuda.synchronize()
    assert not f0.payload_untouched() and not per.payload_untouched()
    gs.check()


# ---------------------------------------------------------------------------------------------------------------------
# the analyzer with decoding streams
# ---------------------------------------------------------------------------------------------------------------------
def serve(an, open_kw, sounds, cuts, pushes_per_tick=1):
    """Push every sound in its cuts, `pushes_per_tick[stream]` pushes between two ticks; returns per stream the concatenated
    (mel rows, f0, periodicity)."""
    got = {kk: ([], [], []) for kk in sounds}
    pos, step = dict.fromkeys(sounds, 0), dict.fromkeys(sounds, 0)
    per_tick = pushes_per_tick if isinstance(pushes_per_tick, dict) else dict.fromkeys(sounds, pushes_per_tick)
    for kk in sounds:
        an.open(kk, **open_kw)
    rounds = 0
    while not all(an.finished(kk) for kk in sounds):
        for kk, ss in sounds.items():
            for _ in range(per_tick[kk]):
                if step[kk] < len(cuts[kk]):
                    end = pos[kk] + cuts[kk][step[kk]]
                    an.push(kk, ss[pos[kk]:end], last=end == ss.size)
                    pos[kk], step[kk] = end, step[kk] + 1
        rows = an.tick()
        for sid, mel in rows.items():
            got[sid][0].append(mel)
        for sid, (f0, per) in an.last_f0.items():
            assert f0.dtype == per.dtype == np.float32 and f0.shape == per.shape and f0.size > 0
            got[sid][1].append(f0)
            got[sid][2].append(per)
        rounds += 1
        assert rounds < 100000
    empty = np.zeros(0, np.float32)
    return {kk: (np.concatenate(parts[0]), np.concatenate(parts[1] or [empty]), np.concatenate(parts[2] or [empty])) for kk, parts in got.items()}


@pytest.mark.parametrize("name,lag", [("small", 0), ("small", 8), ("small", 128), ("default", 8)])
def test_decoding_analyzer_equals_the_host_definition(name, lag):
    """Several streams with different cuts and pushes per tick: the concatenated last_f0 is viterbi_lag_host of the whole
    sound's candidates, it trails the mel rows by `lag` frames until the end, the mel rows are those of streams that do not
    decode, and steady ticks allocate nothing."""
    from mbexwn_vocoder_amd.live import StreamingAnalyzer
    cfg, prm, hop = config_of(name), params_of(name), SETS[name][3]
    rng = np.random.default_rng(71)
    n = 6000 if name == "small" else 12000
    tone = 6000.0 if name == "small" else 220.0
    broken = harmonic(n, 180.0, rng)
    broken[[900, 2400, 4000]] = [np.nan, np.inf, 1e20]
    sounds = {"tone": harmonic(n, tone, rng), "adversarial": adversarial(n), "noise": (0.1 * rng.standard_normal(n)).astype(np.float32),
              "not finite": broken, "n=700": harmonic(700, 440.0, rng), "n=37": (0.1 * rng.standard_normal(37)).astype(np.float32),
              "n=1": np.ones(1, np.float32)}
    step = hop if name == "default" else 8 * hop
    cuts = {kk: random_cuts(rng, ss.size, step) for kk, ss in sounds.items()}
    cuts["noise"] = [sounds["noise"].size]                               # one push: max_new is the whole sound's frames
    per_tick = dict.fromkeys(sounds, 1)
    per_tick.update({"adversarial": 3, "n=700": 7})
    dec = f0decode.decode_params(w_jump=2.0) if name == "small" else f0decode.decode_params()
    an = StreamingAnalyzer(cfg, slots=4)
    got = serve(an, dict(f0_params=prm, f0_lag=lag, f0_decode=dec), sounds, cuts, per_tick)
    plain = serve(StreamingAnalyzer(cfg, slots=4), dict(f0_params=prm), sounds, cuts, per_tick)
    voiced = 0
    for kk, ss in sounds.items():
        centres = np.arange(0, ss.size + 1, hop)
        tables = f0decode.candidates_host(*f0track.difference_host(ss, centres, prm), prm, dec)
        want = f0decode.viterbi_lag_host(*tables, SR, dec, lag)
        assert same(got[kk][1:], want), (kk, lag)
        nan = np.isnan(plain[kk][0])
        assert got[kk][0].shape == plain[kk][0].shape and np.array_equal(np.isnan(got[kk][0]), nan), kk
        assert np.array_equal(bits(got[kk][0])[~nan], bits(plain[kk][0])[~nan]), kk              # the mel promise is untouched
        voiced += int(np.count_nonzero(want[0]))
    assert voiced > 0
    # steady ticks allocate nothing: a second pass of streams over the stores the first one sized
    allocations = an.device_allocations
    for kk in list(sounds):
        an.close(kk)
    again = serve(an, dict(f0_params=prm, f0_lag=lag, f0_decode=dec), sounds, cuts, per_tick)
    assert an.device_allocations == allocations
    for kk in sounds:
        assert same(again[kk], got[kk]), kk                               # and a reused slot's state starts from nothing


def test_decided_frames_trail_by_the_lag_and_no_lag_keeps_the_calls(monkeypatch, lib):
    from mbexwn_vocoder_amd.live import StreamingAnalyzer
    cfg, prm, hop = config_of("small"), params_of("small"), 16
    calls = []
    for symbol in ("mbxl_ring_append", "mbxl_mel_frames", "mbxt_f0_frames", "mbxv_f0_candidate_frames", "mbxv_decode_f0_frames"):
        def spy(*args, _real=getattr(lib, symbol), _name=symbol):
            calls.append(_name)
            return _real(*args)
        monkeypatch.setattr(lib, symbol, spy)
    x = harmonic(2000, 6000.0, np.random.default_rng(72))
    an = StreamingAnalyzer(cfg)
    an.open("s", f0_params=prm, f0_lag=8)
    an.open("plain")
    emitted = decided = 0
    for start in range(0, 2000, 100):
        an.push("s", x[start:start + 100], last=start + 100 == 2000)
        an.push("plain", x[start:start + 100], last=start + 100 == 2000)
        del calls[:]
        rows = an.tick()
        assert calls == ["mbxl_ring_append", "mbxl_mel_frames", "mbxv_f0_candidate_frames", "mbxv_decode_f0_frames"]
        emitted += rows["s"].shape[0] if "s" in rows else 0
        decided += an.last_f0["s"][0].size if "s" in an.last_f0 else 0
        assert "plain" not in an.last_f0
        assert decided == f0decode.lag_frames_decided(emitted, 8, start + 100 == 2000) == an.streams["s"].f0_decided
        if 0 < emitted <= 8:
            assert "s" in rows and "s" not in an.last_f0                 # rows handed out, nothing decided yet: absent
    assert emitted == decided == frames_total(2000, hop)
    # streams without a lag: the entry points of before, and no others
    an = StreamingAnalyzer(cfg)
    an.open("t", f0_params=prm)
    an.open("plain")
    for start in range(0, 2000, 500):
        an.push("t", x[start:start + 500], last=start + 500 == 2000)
        an.push("plain", x[start:start + 500], last=start + 500 == 2000)
        del calls[:]
        an.tick()
        assert calls == ["mbxl_ring_append", "mbxl_mel_frames", "mbxt_f0_frames"]
    an = StreamingAnalyzer(cfg)
    an.open("plain")
    an.push("plain", x, last=True)
    del calls[:]
    an.tick()
    assert calls == ["mbxl_ring_append", "mbxl_mel_frames"] and an._lag_state is None and an._cand is None
    assert f0_frames_ready(2000, hop, 69, closed=True) == frames_total(2000, hop)


@pytest.mark.parametrize("lag", [0, 8])
def test_a_reused_slot_starts_from_a_fresh_decoder_whatever_its_first_tick_does(lag):
    """One slot.  A decoding stream runs to its end and leaves its `done` in the slot's state row; the next stream in that slot
    starts with a push too small for a frame.  At lag 0 such a tick has no plane and launches no decoder -- the row must be
    zeroed all the same, beside the ring, or every later launch would skip the stream (its first frame is not that `done`)."""
    from mbexwn_vocoder_amd.live import StreamingAnalyzer
    cfg, prm, hop = config_of("small"), params_of("small"), 16
    rng = np.random.default_rng(73)
    dec = f0decode.decode_params()
    an = StreamingAnalyzer(cfg, slots=1)
    first = serve(an, dict(f0_params=prm, f0_lag=lag), {"first": harmonic(1500, 6000.0, rng)}, {"first": [700, 800]})["first"]
    assert first[1].size == frames_total(1500, hop)
    slot = an.streams["first"].slot
    assert int(an._lag_state[slot, 0]) == frames_total(1500, hop)         # what the closed stream leaves behind
    an.close("first")
    x = harmonic(2000, 6000.0, rng)
    an.open("second", f0_params=prm, f0_lag=lag)
    assert an.streams["second"].slot == slot
    an.push("second", x[:10])
    assert an.tick() == {} and an.last_f0 == {}                           # 10 samples: appended, no frame yet
    assert not an.streams["second"].fresh and not an._lag_state[slot].any()
    parts = ([], [])
    for start in range(10, 2000, 199):
        an.push("second", x[start:start + 199], last=start + 199 >= 2000)
        an.tick()
        if "second" in an.last_f0:
            for part, value in zip(parts, an.last_f0["second"]):
                part.append(value)
    assert an.finished("second")
    tables = f0decode.candidates_host(*f0track.difference_host(x, np.arange(0, 2001, hop), prm), prm, dec)
    want = f0decode.viterbi_lag_host(*tables, SR, dec, lag)
    assert same(tuple(np.concatenate(part) for part in parts), want) and np.count_nonzero(want[0]) > 3


# ---------------------------------------------------------------------------------------------------------------------
# audio in, audio out, with the decoded pitch of the audio
# ---------------------------------------------------------------------------------------------------------------------
NAME = "lag.wav"


def pipeline_sound():
    """0.1 s of silence, 0.5 s of the adversarial 110 Hz voice, 0.1 s of noise at 0.05, 0.2 s of a 260 Hz tone."""
    rng = np.random.default_rng(31)
    return np.concatenate((np.zeros(2400, np.float32), adversarial(12000), (0.05 * rng.standard_normal(2400)).astype(np.float32),
                           harmonic(4800, 260.0, rng)))


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    from mbexwn_vocoder_amd.mel_inverter import create_synthetic_model_dir
    return create_synthetic_model_dir(str(tmp_path_factory.mktemp("model") / "speech_small"), "SPEECH", **SMALL_MODEL)


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("stream_transpose", TOOL)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


@pytest.fixture(scope="module")
def pipeline(model_dir):
    """The engine (pinned to the convolution form the streams run, as in tests/test_gpu_live_pitch.py), the sound, and the
    host definition's lagged contour of it -- the references of the tests below, computed once."""
    from mbexwn_vocoder_amd.mel_inverter import MELInverter
    inv = MELInverter(model_dir, conv_form="f23")
    snd = pipeline_sound()
    prm, dec = f0track.params(SR), f0decode.decode_params()
    tables = f0decode.candidates_host(*f0track.difference_host(snd, np.arange(0, snd.size + 1, inv.hop_size), prm), prm, dec)
    return inv, snd, dec, {lag: f0decode.viterbi_lag_host(*tables, SR, dec, lag) for lag in (0, 8)}


def test_live_pipeline_with_a_lag_equals_transform_audio(pipeline, tool):
    from mbexwn_vocoder_amd.live import LiveResynthesizer, keyed_noise_fn
    inv, snd, dec, contours = pipeline
    hop = inv.hop_size
    live = LiveResynthesizer(inv)
    noise = keyed_noise_fn(inv.model, SEED)
    tracked = []
    audio = tool.stream_file(live, snd, 1920, 1.5, stream_id=NAME, noise_fn=noise, f0_source="audio", f0_out=tracked, f0_decode=dec, f0_lag=8)
    got = tuple(np.concatenate([pair[kk] for pair in tracked]) for kk in (0, 1))
    assert same(got, contours[8])
    assert not same(got, contours[0])                                    # the lag decides something on this sound
    want = inv.transform_audio([snd], [SR], [NAME], transposition=1.5, noise_seed=SEED, f0_source="audio", f0_decode=dec, f0_lag=8,
                               f0_fill="hold")[0]
    assert audio.shape == want.shape == ((snd.size // hop + 1) * hop,)
    assert np.array_equal(bits(audio), bits(want))                       # sample for sample
    # a transposition and a formant factor given per push: they reach exactly the frames they were given for
    live.open(NAME, noise_fn=noise, f0_source="audio", f0_decode=dec, f0_lag=8)
    pieces, factors, shifts = [], [], []
    for ii, start in enumerate(range(0, snd.size, 1700)):
        end = min(start + 1700, snd.size)
        factors.append((end - start, 1.0 + 0.1 * (ii % 4)))
        shifts.append((end - start, 1.0 if ii < 3 else 0.9 + 0.05 * (ii % 5)))
        live.push_audio(NAME, snd[start:end], last=end == snd.size, transposition=factors[-1][1],
                        **({} if ii < 3 else {"formant": shifts[-1][1]}))
        pieces += [aa for aa in [live.tick().get(NAME)] if aa is not None]
    while not live.finished(NAME):
        pieces.append(live.tick()[NAME])
    live.close(NAME)
    from mbexwn_vocoder_amd.live_plan import frame_factors
    from mbexwn_vocoder_amd.noise import item_key
    from mbexwn_vocoder_amd import analysis
    scaled = [inv.scale_mel(dd) for dd in analysis.generate_mels([snd], [SR], inv.preprocess_config)]
    routed = inv.synth_from_mels(scaled, noise_seed=SEED, noise_keys=[item_key(NAME)], transpositions=[frame_factors(factors, hop)],
                                 formants=[frame_factors(shifts, hop)], f0s=[f0track.fill_hold(contours[8][0], 150.0)])[0]
    assert np.array_equal(bits(np.concatenate(pieces)), bits(routed))
    assert live.lookahead_ms_for(f0_source="audio", f0_lag=8) == live.lookahead_ms_for(f0_source="audio") + 100.0


def test_no_lag_keeps_the_bits_and_the_launches(pipeline, monkeypatch, lib):
    inv, snd, dec, contours = pipeline
    calls = []
    for symbol in ("mbxp_track_f0", "mbxc_f0_candidates", "mbxc_decode_f0", "mbxv_f0_candidate_frames", "mbxv_decode_f0_frames"):
        def spy(*args, _real=getattr(lib, symbol), _name=symbol):
            calls.append(_name)
            return _real(*args)
        monkeypatch.setattr(lib, symbol, spy)

    def run(**kw):
        del calls[:]
        out = inv.transform_audio([snd], [SR], [NAME], noise_seed=SEED, f0_source="audio", f0_decode=dec, **kw)[0]
        return out, list(calls)

    without, made = run()
    given, made_none = run(f0_lag=None)
    assert made == made_none == ["mbxc_f0_candidates", "mbxc_decode_f0"]
    assert np.array_equal(bits(without), bits(given))
    lagged, made_lag = run(f0_lag=8)
    assert made_lag == ["mbxc_f0_candidates", "mbxv_decode_f0_frames"]   # one launch in place of the whole-item decoder's
    _, f0, per = inv.track_f0(snd, SR, on_device=True, decode=dec, f0_lag=8)
    assert same((f0, per), contours[8])
    _, f0, per = inv.track_f0(snd, SR, on_device=True, decode=dec, f0_lag=0)
    assert same((f0, per), contours[0])
    with pytest.raises(ValueError, match="f0_lag"):
        inv.transform_audio([snd], [SR], [NAME], f0_source="audio", f0_lag=8)


@pytest.mark.timeout(600)
def test_stream_transpose_tool_decodes_and_equals_the_file_tool(pipeline, model_dir, tmp_path):
    from scipy.io import wavfile
    from mbexwn_vocoder_amd.audioio import read_audio
    inv, snd, dec, contours = pipeline
    src, dst = str(tmp_path / NAME), str(tmp_path / "out" / "out.wav")
    wavfile.write(src, SR, snd)
    res = subprocess.run([sys.executable, TOOL, src, "-o", dst, "--model_id", model_dir, "--transposition", "1.5", "--noise-seed",
                          str(SEED), "--f0-source", "audio", "--pitch-decode", "viterbi", "--pitch-lag", "8", "--write-f0"],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    got, rate = read_audio(dst)
    _, f0, per = f0track.read_f0(str(tmp_path / "out" / "out.f0"), n_frames=contours[8][0].size)
    assert same((f0, per), contours[8])
    assert "look-ahead" in res.stderr
    files = str(tmp_path / "files")
    res = subprocess.run([sys.executable, os.path.join(BIN, "transform_audio.py"), src, "-o", files, "--model_id", model_dir,
                          "--transposition", "1.5", "--noise-seed", str(SEED), "--f0-source", "audio", "--pitch-decode", "viterbi",
                          "--pitch-lag", "8", "--f0-fill", "hold", "--conv-form", "f23", "-q"],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    from mbexwn_vocoder_amd import flac
    want, want_rate = read_audio(os.path.join(files, "syn_lag.flac"))    # the file tool writes 16 bits: the stream's samples, rounded
    assert rate == want_rate == SR and got.shape == want.shape
    assert np.array_equal(want, flac.to_pcm16(got).astype(np.float32) / np.float32(32768.0))
