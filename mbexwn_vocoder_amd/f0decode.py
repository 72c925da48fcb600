"""A decoded F0 contour: Viterbi over YIN candidates, the opt-in second way from the tracker's
difference function to a contour.  The greedy pick of f0track.py decides every frame on its own; here every frame offers up
to seven lags and an "unvoiced" state, and one path over the whole item is chosen, so that a frame whose d' at half the
period dips below the threshold no longer jumps an octave.

The functions ending in ``_host`` are THE DEFINITION, in numpy float32; ``csrc/f0_decode.hip`` (``mbxc_f0_candidates`` and
``mbxc_decode_f0``, include/mbexwn_contour.h) gives their bits -- the arrangement f0track.py has with ``csrc/f0_track.hip``.
It works like pYIN, but with linear costs instead of log-probabilities: every operation is one rounded float32 operation
(no logarithm, no fused multiply-add), every sum has one fixed order.

Stage 1, :func:`candidates_host`, per frame, from ``f0track.difference_host``'s d', energy and bad flags, with ``lo =
max(tau_min, 2)``, ``hi = tau_max - 1``.  A frame is usable if it is not bad and its energy is at least ``e_min``.  For each
threshold ``theta_n`` (ascending) ``pick_n`` is f0track's pick rule with that threshold: the smallest lag in [lo, hi] with
``d' < theta_n``, moved on while ``tau + 1 <= hi`` and ``d'[tau + 1] < d'[tau]``; none if the frame is not usable or no lag
is below.  ``P[tau]`` is the float32 sum of ``weights[n]`` over the n with ``pick_n == tau``, in ascending n, and ``U`` that
over the n without a pick.  Every lag that is some ``pick_n`` is a candidate (also with P = 0, when its weights are); the
``n_cand`` with the largest P are kept, the smaller lag winning a tie, and listed by ascending lag in slots 0 .. count - 1
of three (K, 8) tables: ``period = float(tau) + off`` (f0track's parabola and clamp), ``cost = max(1 - P, 0)``, ``dprime =
d'[tau]``.  An unused slot below 7 holds (0, +inf, 1).  Slot 7 is "unvoiced": period 0, ``cost = max(1 - U, 0)``, dprime =
d' at the first index of its minimum over [lo, hi], 1 for a bad frame.

Stage 2, :func:`viterbi_host`, per item of T frames.  Slot k < 7 of a frame is available iff ``0 <= cost <= 1e6`` and ``1 <=
period <= 1e6`` (false for NaN); slot 7 always is, with local cost ``cost`` if ``0 <= cost <= 1e6``, else 0.  Frame 0:
``delta[j] = loc[j]``.  Frame t > 0, every available j: over the available i of frame t - 1 in ascending order ``v = delta[i]
+ tr(i, j)``, the smallest kept with strict ``<`` (the smallest i wins a tie); ``new[j] = best + loc[j]``; then ``m =
min(new)`` over the available slots and ``delta[j] = new[j] - m``.  ``tr(i, j)`` is ``w_jump * (|p_j - p_i| / (p_j + p_i))``
between voiced slots, 0 between unvoiced ones, ``w_switch`` otherwise.  The last state is the smallest index of the minimum
of delta; the back pointers give the path.  ``f0 = float(sample_rate) / period`` (0 for slot 7), periodicity the slot's
dprime.
"""
import math

import numpy as np

from . import f0track

f32 = np.float32

SLOTS = 8                    # seven lags and "unvoiced"
MAX_THRESHOLDS = 16
LIMIT = f32(1e6)             # costs, periods and the two weights lie in [0, 1e6]: no sum of the recursion overflows
MAX_DEVICE_FRAMES = 16000    # mbxc_decode_f0 keeps 4 bytes of back pointers per frame in 64 000 bytes of LDS

DECODE_KEYS = ("n_cand", "w_jump", "w_switch", "thresholds", "weights")


def default_thresholds():
    return np.asarray([f32((n + 1) / 32) for n in range(16)], dtype=f32)


def default_weights(thresholds):
    """Beta(2, 12) weights at the thresholds: ``theta (1 - theta)^11`` in float64, normalised to sum 1, as float32."""
    th = np.asarray(thresholds, dtype=np.float64)
    with np.errstate(all="ignore"):
        w = th ** (2 - 1) * (1.0 - th) ** (12 - 1)
    total = w.sum()
    if not (np.all(np.isfinite(w)) and np.all(w >= 0) and total > 0):
        raise ValueError("f0 decode: the default weights need thresholds in (0, 1); give weights")
    return (w / total).astype(f32)


def check_decode(dec):
    """Raise ValueError unless the dictionary is one the definition and ``mbxc_f0_candidates`` / ``mbxc_decode_f0`` accept."""
    if not isinstance(dec, dict) or sorted(dec) != sorted(DECODE_KEYS):
        raise ValueError(f"f0 decode: the parameters must be a dictionary with the keys {DECODE_KEYS}")
    th, ww = np.asarray(dec["thresholds"]), np.asarray(dec["weights"])
    if th.ndim != 1 or not 1 <= th.size <= MAX_THRESHOLDS:
        raise ValueError(f"f0 decode: need 1 .. {MAX_THRESHOLDS} thresholds in a 1-D array, got shape {th.shape}")
    th = th.astype(f32)
    if not np.all(np.isfinite(th)) or np.any(th[1:] <= th[:-1]):
        raise ValueError("f0 decode: the thresholds must be finite and strictly ascending")
    if ww.ndim != 1 or ww.size != th.size:
        raise ValueError(f"f0 decode: need one weight per threshold, got {ww.shape} for {th.size}")
    ww = ww.astype(f32)
    if not np.all(np.isfinite(ww)) or np.any(ww < 0):
        raise ValueError("f0 decode: the weights must be finite and not negative")
    nc = dec["n_cand"]
    if isinstance(nc, bool) or nc != int(nc) or not 1 <= int(nc) <= SLOTS - 1:
        raise ValueError(f"f0 decode: n_cand must be an integer in 1 .. {SLOTS - 1}, got {nc!r}")
    for key in ("w_jump", "w_switch"):
        vv = float(dec[key])
        if not (math.isfinite(vv) and 0.0 <= vv <= float(LIMIT)):
            raise ValueError(f"f0 decode: {key} must be finite and in [0, 1e6], got {dec[key]!r}")
    return dec


def decode_params(n_cand=7, w_jump=4.0, w_switch=0.5, thresholds=None, weights=None):
    """The checked dictionary both stages take.  ``thresholds``: default ``float32((n + 1) / 32)``, n = 0 .. 15; ``weights``:
    default :func:`default_weights` of the thresholds.  Refused: fewer than 1 or more than 16 thresholds, thresholds that
    are not finite and strictly ascending, another number of weights, weights that are not finite or negative, ``n_cand``
    outside 1 .. 7, ``w_jump`` or ``w_switch`` not finite or outside [0, 1e6]."""
    th = default_thresholds() if thresholds is None else np.array(thresholds, dtype=f32)
    dec = {"n_cand": n_cand, "w_jump": w_jump, "w_switch": w_switch, "thresholds": th,
           "weights": th if weights is None else np.array(weights, dtype=f32)}
    if weights is None:
        dec["weights"] = np.zeros(th.shape, dtype=f32)
        check_decode(dec)                                            # the thresholds, before the weights are made from them
        dec["weights"] = default_weights(th)
    check_decode(dec)
    dec["n_cand"], dec["w_jump"], dec["w_switch"] = int(n_cand), float(f32(w_jump)), float(f32(w_switch))
    return dec


def _period(row, tau):
    """f0track.pick_host's refinement: ``float(tau)`` plus the clamped vertex of the parabola through d'[tau - 1 .. tau + 1]."""
    a, b, g = row[tau - 1], row[tau], row[tau + 1]
    den = f32(f32(a - b) + f32(g - b))
    off = f32(0)
    if den > 0:
        with np.errstate(all="ignore"):
            off = f32(f32(f32(a - g) / den) * f32(0.5))
        off = min(max(off, f32(-1)), f32(1))
    return f32(f32(tau) + off)


def candidates_host(dp, energy, bad, prm, dec):
    """Stage 1 (the module's docstring) on ``f0track.difference_host``'s results: ``period``, ``cost``, ``dprime``, each
    (K, 8) float32."""
    f0track.check_params(prm)
    check_decode(dec)
    tau_min, tau_max, e_min = int(prm["tau_min"]), int(prm["tau_max"]), f32(prm["e_min"])
    th, ww, n_cand = np.asarray(dec["thresholds"], dtype=f32), np.asarray(dec["weights"], dtype=f32), int(dec["n_cand"])
    dp = np.asarray(dp, dtype=f32)
    K = dp.shape[0]
    lo, hi = max(tau_min, 2), tau_max - 1
    period = np.zeros((K, SLOTS), dtype=f32)
    cost = np.full((K, SLOTS), np.inf, dtype=f32)
    dprime = np.ones((K, SLOTS), dtype=f32)
    for t in range(K):
        row = dp[t]
        usable = (not bad[t]) and bool(energy[t] >= e_min)
        P, U = {}, f32(0)
        for n in range(th.size):
            below = row[lo:hi + 1] < th[n]
            if not (usable and below.any()):
                U = f32(U + ww[n])
                continue
            tau = lo + int(np.argmax(below))
            while tau + 1 <= hi and row[tau + 1] < row[tau]:
                tau += 1
            P[tau] = f32(P.get(tau, f32(0)) + ww[n])
        keep = sorted(sorted(P, key=lambda tau: (-float(P[tau]), tau))[:n_cand])
        for kk, tau in enumerate(keep):
            period[t, kk] = _period(row, tau)
            cost[t, kk] = max(f32(f32(1) - P[tau]), f32(0))
            dprime[t, kk] = row[tau]
        cost[t, SLOTS - 1] = max(f32(f32(1) - U), f32(0))
        if not bad[t]:
            dprime[t, SLOTS - 1] = row[lo + int(np.argmin(row[lo:hi + 1]))]
    return period, cost, dprime


def _checked_tables(name, period, cost, dprime, sample_rate):
    period, cost, dprime = (np.ascontiguousarray(aa, dtype=f32) for aa in (period, cost, dprime))
    if not (period.ndim == 2 and period.shape[1] == SLOTS and period.shape == cost.shape == dprime.shape):
        raise ValueError(f"{name}: three tables of shape (T, {SLOTS}), got {period.shape}, {cost.shape}, {dprime.shape}")
    if int(sample_rate) < 1:
        raise ValueError(f"{name}: sample_rate must be at least 1, got {sample_rate!r}")
    return period, cost, dprime


def _forward(period, cost, dec, trace=None):
    """The forward recursion of stage 2 on T >= 1 frames: the back pointers (T, 8) and every frame's best state -- the smallest
    index of the minimum of its delta.  Frame t of both depends on the frames 0 .. t only."""
    T = period.shape[0]
    w_jump, w_switch, inf = f32(dec["w_jump"]), f32(dec["w_switch"]), f32(np.inf)
    with np.errstate(all="ignore"):
        # what does not depend on the path, for all frames at once: availability, local costs, tr[t, i, j] from t - 1 to t
        c_ok = (cost >= 0) & (cost <= LIMIT)
        avail = c_ok & (period >= 1) & (period <= LIMIT)
        avail[:, SLOTS - 1] = True
        loc = np.where(c_ok, cost, f32(0)).astype(f32)
        pi, pj = period[:-1, :, None], period[1:, None, :]
        tr = (w_jump * (np.abs(pj - pi) / (pj + pi))).astype(f32)
        tr[:, SLOTS - 1, :] = w_switch
        tr[:, :, SLOTS - 1] = w_switch
        tr[:, SLOTS - 1, SLOTS - 1] = f32(0)
    back = np.zeros((T, SLOTS), dtype=np.int64)
    best = np.zeros(T, dtype=np.int64)
    delta = np.where(avail[0], loc[0], inf).astype(f32)
    best[0] = int(np.argmin(delta))
    if trace is not None:
        trace.append(delta.copy())
    with np.errstate(all="ignore"):
        for t in range(1, T):
            v = np.where(avail[t - 1][:, None], delta[:, None] + np.where(avail[t - 1][:, None], tr[t - 1], f32(0)), inf)
            back[t] = np.argmin(v, axis=0)                              # the first index of the minimum: strict <, ascending i
            new = np.where(avail[t], v.min(axis=0) + loc[t], inf).astype(f32)
            delta = new - new.min()
            best[t] = int(np.argmin(delta))
            if trace is not None:
                trace.append(delta.copy())
    return back, best


def viterbi_host(period, cost, dprime, sample_rate, dec, trace=None):
    """Stage 2 (the module's docstring) on the (T, 8) tables of one item: ``(f0, periodicity)``, each (T,) float32.
    ``trace``: a list that receives every frame's delta (8,), +inf at unavailable slots."""
    check_decode(dec)
    period, cost, dprime = _checked_tables("viterbi_host", period, cost, dprime, sample_rate)
    T = period.shape[0]
    f0, per = np.zeros(T, dtype=f32), np.zeros(T, dtype=f32)
    if T == 0:
        return f0, per
    back, best = _forward(period, cost, dec, trace)
    state = best[T - 1]
    sr = f32(int(sample_rate))
    with np.errstate(all="ignore"):
        for t in range(T - 1, -1, -1):
            if state < SLOTS - 1:
                f0[t] = sr / period[t, state]
            per[t] = dprime[t, state]
            state = int(back[t, state])
    return f0, per


def track_f0_viterbi_host(x, centres, prm, dec):
    """The decoded contour of a 1-D sound: ``f0track.difference_host``, :func:`candidates_host`, :func:`viterbi_host`.
    Arguments and results as ``f0track.track_f0_host``, plus ``dec``: :func:`decode_params`."""
    dp, energy, bad = f0track.difference_host(x, centres, prm)
    return viterbi_host(*candidates_host(dp, energy, bad, prm, dec), int(prm["sample_rate"]), dec)


# ------------------------------------------------------------------------------------------------------------------------
# the fixed-lag decision: a stream decides frame t once frame t + lag has been seen
# ------------------------------------------------------------------------------------------------------------------------
MAX_LAG = 128                # mbxv_decode_f0_frames keeps a ring of 256 frames: lag + 1 behind a sub-chunk of 64


def check_lag(lag):
    """The look-ahead of the fixed-lag decoder in frames, as an int: ValueError for a bool, a non-integer or a value outside
    0 .. 128."""
    if isinstance(lag, (bool, np.bool_)) or not isinstance(lag, (int, np.integer)) or not 0 <= int(lag) <= MAX_LAG:
        raise ValueError(f"f0 decode: the lag must be an integer in 0 .. {MAX_LAG} frames, got {lag!r}")
    return int(lag)


def lag_frames_decided(done, lag, closed=False):
    """Frames of a stream the fixed-lag decoder has decided once it has seen ``done`` of them: frame t waits for frame t +
    lag while the stream is open; a closed stream has all of them (the rule beside ``live_plan.f0_frames_ready``)."""
    return int(done) if closed else max(0, int(done) - int(lag))


def viterbi_lag_host(period, cost, dprime, sample_rate, dec, lag):
    """Stage 2 with a fixed lag, on the (T, 8) tables of one item: the forward recursion is :func:`viterbi_host`'s; frame t
    takes the state the back pointers lead to from the best state of frame ``e = min(t + lag, T - 1)`` (the smallest index
    of the minimum of delta_e), so it depends on the frames 0 .. t + lag only.  ``lag >= T - 1`` is :func:`viterbi_host`.
    Returns ``(f0, periodicity)``, each (T,) float32."""
    check_decode(dec)
    lag = check_lag(lag)
    period, cost, dprime = _checked_tables("viterbi_lag_host", period, cost, dprime, sample_rate)
    T = period.shape[0]
    f0, per = np.zeros(T, dtype=f32), np.zeros(T, dtype=f32)
    if T == 0:
        return f0, per
    back, best = _forward(period, cost, dec)
    sr = f32(int(sample_rate))
    with np.errstate(all="ignore"):
        for t in range(T):
            e = min(t + lag, T - 1)
            state = int(best[e])
            for u in range(e, t, -1):
                state = int(back[u, state])
            if state < SLOTS - 1:
                f0[t] = sr / period[t, state]
            per[t] = dprime[t, state]
    return f0, per


class LagDecoder:
    """:func:`viterbi_lag_host` as a state machine, and the definition of the state ``mbxv_decode_f0_frames`` keeps per
    stream: ``done`` frames seen, ``decided`` of them handed out, ``delta`` (8) of the last frame, that frame's periods and
    costs, and of the last ``lag + 1`` frames the pointer word (eight 3-bit back pointers and, from bit 24, the frame's best
    state), the periods and the dprimes.  The concatenated results of ``push`` are ``viterbi_lag_host`` of the concatenated
    tables, however they were cut."""

    def __init__(self, sample_rate, dec, lag):
        check_decode(dec)
        if int(sample_rate) < 1:
            raise ValueError(f"LagDecoder: sample_rate must be at least 1, got {sample_rate!r}")
        self.lag, self.sample_rate = check_lag(lag), int(sample_rate)
        self.w_jump, self.w_switch = f32(dec["w_jump"]), f32(dec["w_switch"])
        self.done = self.decided = 0
        self.delta = np.zeros(SLOTS, dtype=f32)
        self.prev_period, self.prev_cost = np.zeros(SLOTS, dtype=f32), np.zeros(SLOTS, dtype=f32)
        self.words, self.periods, self.dprimes = {}, {}, {}      # frame -> word, (8,), (8,): the last lag + 1 frames

    @staticmethod
    def _available(period, cost):
        c_ok = (cost >= 0) & (cost <= LIMIT)
        avail = c_ok & (period >= 1) & (period <= LIMIT)
        avail[SLOTS - 1] = True
        return avail, np.where(c_ok, cost, f32(0)).astype(f32)

    def _step(self, period, cost):
        inf = f32(np.inf)
        avail, loc = self._available(period, cost)
        word = 0
        if self.done == 0:
            delta = np.where(avail, loc, inf).astype(f32)
        else:
            before, _ = self._available(self.prev_period, self.prev_cost)
            pi, pj = self.prev_period[:, None], period[None, :]
            tr = (self.w_jump * (np.abs(pj - pi) / (pj + pi))).astype(f32)
            tr[SLOTS - 1, :] = self.w_switch
            tr[:, SLOTS - 1] = self.w_switch
            tr[SLOTS - 1, SLOTS - 1] = f32(0)
            v = np.where(before[:, None], self.delta[:, None] + np.where(before[:, None], tr, f32(0)), inf)
            arg = np.argmin(v, axis=0)
            new = np.where(avail, v.min(axis=0) + loc, inf).astype(f32)
            delta = new - new.min()
            word = sum(int(arg[j]) << (3 * j) for j in range(SLOTS) if avail[j])
        self.delta, self.prev_period, self.prev_cost = delta, period.copy(), cost.copy()
        return word | int(np.argmin(delta)) << 24

    def push(self, period, cost, dprime, last=False):
        """The tables (n, 8) of the next n >= 0 frames; ``last``: no frame follows.  Returns ``(f0, periodicity)`` of the
        frames that became decided: those below ``lag_frames_decided(done, lag, last)``."""
        period, cost, dprime = _checked_tables("LagDecoder.push", period, cost, dprime, self.sample_rate)
        with np.errstate(all="ignore"):
            for row in range(period.shape[0]):
                t = self.done
                self.words[t], self.periods[t], self.dprimes[t] = self._step(period[row], cost[row]), period[row].copy(), dprime[row].copy()
                self.done = t + 1
            target = max(self.decided, lag_frames_decided(self.done, self.lag, last))
            f0, per = np.zeros(target - self.decided, dtype=f32), np.zeros(target - self.decided, dtype=f32)
            sr = f32(self.sample_rate)
            for t in range(self.decided, target):
                e = min(t + self.lag, self.done - 1)
                state = self.words[e] >> 24
                for u in range(e, t, -1):
                    state = (self.words[u] >> (3 * state)) & 7
                if state < SLOTS - 1:
                    f0[t - self.decided] = sr / self.periods[t][state]
                per[t - self.decided] = self.dprimes[t][state]
        self.decided = target
        for store in (self.words, self.periods, self.dprimes):          # what no later frame reads
            for t in [t for t in store if t < self.done - self.lag - 1]:
                del store[t]
        return f0, per


def decode_lag_device(period, cost, dprime, n_frames, sample_rate, dec, lag):
    """:func:`viterbi_lag_host` on the GPU for a ragged batch (``mbxv_decode_f0_frames``, include/mbexwn_live_contour.h, on
    fresh zero states: every item is a stream that is pushed once and closed): tensors as for :func:`decode_device`, of any
    length -- the kernel keeps a ring of frames, not the item.  Returns two cuda tensors (batch, max_frames), f0 and
    periodicity; rows from ``n_frames[b]`` on stay zero.  No engine, current stream."""
    import ctypes
    import torch
    from .abi import _check, load_library
    check_decode(dec)
    lag = check_lag(lag)
    if not torch.is_tensor(period) or period.dim() != 3 or int(period.shape[2]) != SLOTS or period.dtype != torch.float32 or not period.is_cuda:
        raise ValueError(f"period must be a float32 cuda tensor of shape (batch, max_frames, {SLOTS})")
    dev = period.device
    for name, tt in (("cost", cost), ("dprime", dprime)):
        if not torch.is_tensor(tt) or tt.dtype != torch.float32 or tt.shape != period.shape or tt.device != dev:
            raise ValueError(f"{name} must be a float32 tensor with the shape and device of period")
    B, frames = int(period.shape[0]), int(period.shape[1])
    if not torch.is_tensor(n_frames) or n_frames.dtype != torch.int32 or tuple(n_frames.shape) != (B,) or n_frames.device != dev:
        raise ValueError("n_frames must be an int32 tensor of shape (batch,) on the device of period")
    if int(sample_rate) < 1:
        raise ValueError(f"decode_lag_device: sample_rate must be at least 1, got {sample_rate!r}")
    period, cost, dprime = period.contiguous(), cost.contiguous(), dprime.contiguous()
    f0 = torch.zeros((B, frames + lag), dtype=torch.float32, device=dev)
    per = torch.zeros((B, frames + lag), dtype=torch.float32, device=dev)
    if B == 0 or frames == 0:
        return f0[:, :frames].contiguous(), per[:, :frames].contiguous()
    lib = load_library()
    counts = n_frames.to(torch.int64).clamp(0, frames)
    # every item is its own stream: slot b, first frame 0, all its frames, and n_total = T - 1 with hop 1 closes it
    desc = torch.stack([torch.arange(B, device=dev), torch.zeros_like(counts), counts, counts - 1], dim=1).contiguous()
    state = torch.zeros((B, int(lib.mbxv_lag_state_words())), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _check(lib.mbxv_decode_f0_frames(period.data_ptr(), cost.data_ptr(), dprime.data_ptr(), desc.data_ptr(), B, frames, 1,
                                         state.data_ptr(), B, lag, int(sample_rate), ctypes.c_float(float(dec["w_jump"])),
                                         ctypes.c_float(float(dec["w_switch"])), f0.data_ptr(), per.data_ptr(), frames + lag,
                                         torch.cuda.current_stream(dev).cuda_stream))
    return f0[:, :frames].contiguous(), per[:, :frames].contiguous()


def _host_tables(dec):
    th = np.ascontiguousarray(dec["thresholds"], dtype=f32)
    ww = np.ascontiguousarray(dec["weights"], dtype=f32)
    return th, ww


def candidates_device(audio, n_samples, centres, n_frames, prm, dec):
    """:func:`candidates_host` behind ``difference_host`` on the GPU (csrc/f0_decode.hip through ``mbxc_f0_candidates``,
    include/mbexwn_contour.h), for a ragged batch: the tensors of ``f0track.track_f0_device``.  Returns three cuda tensors
    (batch, max_frames, 8): period, cost, dprime; rows of item b from ``n_frames[b]`` on are not written (they stay zero).
    No engine: the launch goes to the current stream of the buffers' device."""
    import ctypes
    import torch
    from .abi import _check, load_library
    f0track.check_params(prm)
    check_decode(dec)
    if not torch.is_tensor(audio) or audio.dim() != 2 or audio.dtype != torch.float32 or not audio.is_cuda:
        raise ValueError("audio must be a float32 cuda tensor of shape (batch, stride)")
    dev = audio.device
    audio = audio.contiguous()
    B, N = int(audio.shape[0]), int(audio.shape[1])
    for name, tt in (("n_samples", n_samples), ("n_frames", n_frames)):
        if not torch.is_tensor(tt) or tt.dtype != torch.int32 or tuple(tt.shape) != (B,) or tt.device != dev:
            raise ValueError(f"{name} must be an int32 tensor of shape (batch,) on the device of audio")
    if not torch.is_tensor(centres) or centres.dtype != torch.int64 or centres.dim() != 2 or int(centres.shape[0]) != B or centres.device != dev:
        raise ValueError("centres must be an int64 tensor of shape (batch, max_frames) on the device of audio")
    n_samples, n_frames, centres = n_samples.contiguous(), n_frames.contiguous(), centres.contiguous()
    frames = int(centres.shape[1])
    tables = [torch.zeros((B, frames, SLOTS), dtype=torch.float32, device=dev) for _ in range(3)]
    if B == 0 or frames == 0:
        return tuple(tables)
    th, ww = _host_tables(dec)
    fpp = ctypes.POINTER(ctypes.c_float)
    with torch.cuda.device(dev):
        _check(load_library().mbxc_f0_candidates(audio.data_ptr(), N, B, n_samples.data_ptr(), centres.data_ptr(),
                                                 n_frames.data_ptr(), frames, int(prm["sample_rate"]), int(prm["window"]),
                                                 int(prm["tau_min"]), int(prm["tau_max"]), ctypes.c_float(float(prm["e_min"])),
                                                 th.ctypes.data_as(fpp), ww.ctypes.data_as(fpp), int(th.size), int(dec["n_cand"]),
                                                 tables[0].data_ptr(), tables[1].data_ptr(), tables[2].data_ptr(),
                                                 torch.cuda.current_stream(dev).cuda_stream))
    return tuple(tables)


def decode_device(period, cost, dprime, n_frames, sample_rate, dec):
    """:func:`viterbi_host` on the GPU for a ragged batch (``mbxc_decode_f0``): three float32 cuda tables (batch,
    max_frames, 8) and ``n_frames`` int32 cuda (batch,), clamped to [0, max_frames].  Returns two cuda tensors (batch,
    max_frames), f0 and periodicity; rows from ``n_frames[b]`` on stay zero.  No engine, current stream.

    The kernel keeps its back pointers in LDS and takes at most :data:`MAX_DEVICE_FRAMES` frames.  A longer table goes,
    item by item, through :func:`viterbi_host` (with a copy to the host and back): the bits are the same by construction,
    since the kernel gives the definition's bits."""
    import ctypes
    import torch
    from .abi import _check, load_library
    check_decode(dec)
    if not torch.is_tensor(period) or period.dim() != 3 or int(period.shape[2]) != SLOTS or period.dtype != torch.float32 or not period.is_cuda:
        raise ValueError(f"period must be a float32 cuda tensor of shape (batch, max_frames, {SLOTS})")
    dev = period.device
    for name, tt in (("cost", cost), ("dprime", dprime)):
        if not torch.is_tensor(tt) or tt.dtype != torch.float32 or tt.shape != period.shape or tt.device != dev:
            raise ValueError(f"{name} must be a float32 tensor with the shape and device of period")
    B, frames = int(period.shape[0]), int(period.shape[1])
    if not torch.is_tensor(n_frames) or n_frames.dtype != torch.int32 or tuple(n_frames.shape) != (B,) or n_frames.device != dev:
        raise ValueError("n_frames must be an int32 tensor of shape (batch,) on the device of period")
    if int(sample_rate) < 1:
        raise ValueError(f"decode_device: sample_rate must be at least 1, got {sample_rate!r}")
    period, cost, dprime, n_frames = period.contiguous(), cost.contiguous(), dprime.contiguous(), n_frames.contiguous()
    f0 = torch.zeros((B, frames), dtype=torch.float32, device=dev)
    per = torch.zeros((B, frames), dtype=torch.float32, device=dev)
    if B == 0 or frames == 0:
        return f0, per
    if frames > MAX_DEVICE_FRAMES:
        counts = np.clip(n_frames.cpu().numpy(), 0, frames)
        tabs = [tt.cpu().numpy() for tt in (period, cost, dprime)]
        f0_h, per_h = np.zeros((B, frames), dtype=f32), np.zeros((B, frames), dtype=f32)
        for bb in range(B):
            kk = int(counts[bb])
            f0_h[bb, :kk], per_h[bb, :kk] = viterbi_host(*(tt[bb, :kk] for tt in tabs), int(sample_rate), dec)
        return torch.as_tensor(f0_h).to(dev), torch.as_tensor(per_h).to(dev)
    with torch.cuda.device(dev):
        _check(load_library().mbxc_decode_f0(period.data_ptr(), cost.data_ptr(), dprime.data_ptr(), n_frames.data_ptr(), frames, B,
                                             int(sample_rate), ctypes.c_float(float(dec["w_jump"])),
                                             ctypes.c_float(float(dec["w_switch"])), f0.data_ptr(), per.data_ptr(),
                                             torch.cuda.current_stream(dev).cuda_stream))
    return f0, per


def track_f0_viterbi_device(audio, n_samples, centres, n_frames, prm, dec):
    """:func:`track_f0_viterbi_host` on the GPU, for a ragged batch: :func:`candidates_device`, then :func:`decode_device`
    -- two launches.  Arguments and results as ``f0track.track_f0_device``."""
    tables = candidates_device(audio, n_samples, centres, n_frames, prm, dec)
    return decode_device(*tables, n_frames, int(prm["sample_rate"]), dec)
