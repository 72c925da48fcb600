"""Look-ahead peak limiter: the definition on the host (numpy) and the device stage (csrc/limiter.hip through ``mbxd_limit``
and ``mbxd_limit_emit`` of include/mbexwn_limiter.h).  DESIGN.md section 6n.

THE DEFINITION.  Everything is float32, every product and every sum rounded on its own (no fused multiply-add).  At ``rate``

    h = max(1, round(lookahead_ms * rate / 2000))     the look-ahead is 2 h samples
    H = round(hold_ms * rate / 1000) >= h             the hold
    W = H + h + 1
    w[j] ~ sin^2(pi (j + 1) / (2 h + 2)), j = 0 .. 2 h, normalised to sum 1 in float64, then rounded to float32

and for an item x[0 .. n), a gain g0 and a ceiling c > 0

    u[k]    = x[k] * g0
    need[k] = c / d[k] where d[k] is finite and > c, else exactly 1; 1 outside [0, n).  d[k] = |u[k]|, or -- true peak,
              whole items only -- the maximum (of bit patterns) of |u[k]| and |v[q]|, q in [4 k - 3, 4 k + 3] inside
              [0, 4 n), v = u at four times the rate (``resample.resample_device``)
    m[i]    = min(need[k], k in [i - H, i + h])
    g[i]    = 1 - acc, acc from 0, for j = -h .. h ascending acc = acc + w[j + h] * (1 - m[i + j])
    y[i]    = u[i] * g[i], then y > c gives c and y < -c gives -c (comparisons: a NaN stays a NaN)

There is no recurrence: output i is a function of the samples [i - h - H, i + 2 h] alone, a minimum of non-negative floats
is exact and associative and the sum has a fixed order, so any tiling gives the same bits, and a stream (output i once
sample i + 2 h is there, or the stream is closed) gives the bits of the whole item.  Where no sample of the window is over
the ceiling every term is 0 and g is exactly 1.  In exact arithmetic g[i] <= need[i]; in float32 the product can exceed c
by (2 h + 4) * 2^-24 relative, which the clamp takes off.

STATISTICS of an item, 4 int32 words: the smallest bit pattern (as a signed integer) of g, from that of 1.0; the number of
samples with g < 1; the number of samples the clamp changed; 0.
"""
from dataclasses import dataclass

import numpy as np

DEFAULT_LOOKAHEAD_MS = 1.5
DEFAULT_HOLD_MS = 20.0
TILE = 2048                 # outputs per block of the device kernels (MBXD_TILE of include/mbexwn_limiter.h)
LDS_WORDS = 16000           # what a block may use (MBXD_LDS_WORDS)
STAT_WORDS = 4
ONE_BITS = 0x3F800000       # the bit pattern of 1.0f: where the smallest gain starts


def window(rate, lookahead_ms=None, hold_ms=None):
    """(h, H) of the definition at ``rate``; None is the default, 1.5 ms and 20 ms -- THE place where the numbers are filled
    in.  ValueError for values that are not finite and positive, and for H < h."""
    lookahead_ms = DEFAULT_LOOKAHEAD_MS if lookahead_ms is None else lookahead_ms
    hold_ms = DEFAULT_HOLD_MS if hold_ms is None else hold_ms
    rate, lookahead_ms, hold_ms = float(rate), float(lookahead_ms), float(hold_ms)
    if not (np.isfinite(rate) and rate > 0):
        raise ValueError(f"limiter: the rate must be positive, got {rate!r}")
    if not (np.isfinite(lookahead_ms) and lookahead_ms > 0):
        raise ValueError(f"limiter: the look-ahead must be a positive number of ms, got {lookahead_ms!r}")
    if not (np.isfinite(hold_ms) and hold_ms > 0):
        raise ValueError(f"limiter: the hold must be a positive number of ms, got {hold_ms!r}")
    h = max(1, int(np.floor(lookahead_ms * rate / 2000.0 + 0.5)))
    H = int(np.floor(hold_ms * rate / 1000.0 + 0.5))
    if H < h:
        raise ValueError(f"limiter: the hold ({hold_ms} ms, {H} samples at {rate:g} Hz) must not be shorter than half the "
                         f"look-ahead ({lookahead_ms} ms, h = {h})")
    return h, H


def weights(h):
    """w of the definition: float32 (2 h + 1,)."""
    h = int(h)
    if h < 1:
        raise ValueError(f"limiter: h must be at least 1, got {h}")
    j = np.arange(2 * h + 1, dtype=np.float64)
    w = np.sin(np.pi * (j + 1.0) / (2.0 * h + 2.0)) ** 2
    return (w / w.sum()).astype(np.float32)


def lds_words(h, H, n_taps=0):
    """The LDS words a block of the device kernels needs for the window (h, H), with ``n_taps`` true-peak taps."""
    span = TILE + 3 * h + H
    return 2 * span + 1 + (2 * h + 1) + int(n_taps) + 16


def check_window(h, H, n_taps=0):
    """ValueError for a window the device kernels refuse."""
    if h < 1 or H < h:
        raise ValueError(f"limiter: need 1 <= h <= H, got h = {h}, H = {H}")
    if lds_words(h, H, n_taps) > LDS_WORDS:
        raise ValueError(f"limiter: the window (h = {h}, H = {H}) is too long for the device: "
                         f"{lds_words(h, H, n_taps)} LDS words of {LDS_WORDS}")


@dataclass
class LimitStats:
    """``min_gain``: the smallest g (float32; 1 where nothing was limited); ``limited``: samples with g < 1; ``clamped``:
    samples the clamp changed."""
    min_gain: np.float32
    limited: int
    clamped: int

    @classmethod
    def from_words(cls, words):
        words = np.ascontiguousarray(words, dtype=np.int32).reshape(STAT_WORDS)
        return cls(words[:1].view(np.float32)[0], int(words[1]), int(words[2]))

    def words(self):
        return np.asarray([np.float32(self.min_gain).view(np.int32), self.limited, self.clamped, 0], dtype=np.int32)

    @property
    def reduction_db(self):
        """The deepest gain reduction in dB (>= 0)."""
        gain = float(self.min_gain)
        return float("inf") if not gain > 0 else float(-20.0 * np.log10(gain))

    def merged(self, other):
        low = min(np.float32(self.min_gain).view(np.int32), np.float32(other.min_gain).view(np.int32))
        return LimitStats(np.int32(low).view(np.float32), self.limited + other.limited, self.clamped + other.clamped)


TRUE_PEAK_TAPS = 180        # of the 4x filter (``resample.reference_filter(r, 4 r)``: the design depends on the ratio alone)


def check_rates(rates, lookahead_ms=None, hold_ms=None, true_peak=False):
    """ValueError when the window is refused at one of ``rates`` -- a hold shorter than half the look-ahead, a window too
    long for the device: what a job asks before anything runs."""
    for rate in sorted(set(int(round(rr)) for rr in rates)):
        check_window(*window(rate, lookahead_ms, hold_ms), TRUE_PEAK_TAPS if true_peak else 0)


def abs_bits(x):
    return np.abs(np.ascontiguousarray(x, dtype=np.float32)).view(np.uint32)


def needs_host(u, ceiling, v=None):
    """need of the definition for the float32 item ``u`` (already x * g0); ``v``: u at four times the rate (4 n,), or None."""
    u = np.ascontiguousarray(u, dtype=np.float32)
    c = np.float32(ceiling)
    d = abs_bits(u).copy()
    if v is not None:
        v = abs_bits(v)
        n = u.size
        if v.size != 4 * n:
            raise ValueError(f"limiter: v must hold 4 n = {4 * n} samples, got {v.size}")
        padded = np.zeros(4 * n + 6, dtype=np.uint32)
        padded[3:3 + 4 * n] = v
        for off in range(7):                                # q = 4 k - 3 + off
            d = np.maximum(d, padded[off:off + 4 * n:4])
    d = d.view(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        over = np.isfinite(d) & (d > c)
        need = np.where(over, c / np.where(over, d, np.float32(1.0)), np.float32(1.0)).astype(np.float32)
    return need


def _sliding_min(a, width):
    """min(a[i .. i + width)) for 0 <= i <= a.size - width, by doubling."""
    size = 1
    tab = a
    while 2 * size <= width:
        tab = np.minimum(tab[:tab.size - size], tab[size:])
        size *= 2
    count = a.size - width + 1
    return np.minimum(tab[:count], tab[width - size:width - size + count])


def gain_span_host(need_span, h, H, w=None):
    """g over [a, b) from ``need_span``, the needs over [a - h - H, b + 2 h) (1 where the index is outside the item): THE
    evaluation, which the whole item and every cut of a stream go through."""
    need_span = np.ascontiguousarray(need_span, dtype=np.float32)
    w = weights(h) if w is None else np.asarray(w, dtype=np.float32)
    count = need_span.size - (3 * h + H)
    if count < 0:
        raise ValueError("limiter: the span of needs is shorter than its margins")
    one = np.float32(1.0)
    slack = one - _sliding_min(need_span, H + h + 1)        # 1 - m over [a - h, b + h)
    acc = np.zeros(count, dtype=np.float32)
    for j in range(2 * h + 1):
        acc = acc + w[j] * slack[j:j + count]
    return one - acc


def finish_host(u, g, ceiling):
    """(y, LimitStats) from u and g."""
    c = np.float32(ceiling)
    with np.errstate(invalid="ignore", over="ignore"):
        y = (np.asarray(u, dtype=np.float32) * g).astype(np.float32)
        out = np.where(y > c, c, y)
        out = np.where(out < -c, -c, out).astype(np.float32)
        clamped = int(np.count_nonzero((y > c) | (y < -c)))
    low = int(min([ONE_BITS] + ([int(g.view(np.int32).min())] if g.size else [])))
    return out, LimitStats(np.int32(low).view(np.float32), int(np.count_nonzero(g < np.float32(1.0))), clamped)


def limit_host(x, g0, ceiling, h, H, v=None, details=False):
    """The definition on a 1-D item: ``(y, LimitStats)``, with ``details`` also (u, need, g).  ``v``: true peak (above)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim != 1:
        raise ValueError("limit_host: a 1-D signal is expected")
    if not np.float32(ceiling) > 0:
        raise ValueError(f"limit_host: the ceiling must be positive, got {ceiling!r}")
    window_check = (int(h) >= 1 and int(H) >= int(h))
    if not window_check:
        raise ValueError(f"limiter: need 1 <= h <= H, got h = {h}, H = {H}")
    with np.errstate(invalid="ignore", over="ignore"):
        u = (x * np.float32(g0)).astype(np.float32)
    need = needs_host(u, ceiling, v)
    span = np.concatenate((np.ones(h + H, dtype=np.float32), need, np.ones(2 * h, dtype=np.float32)))
    g = gain_span_host(span, h, H)
    y, stats = finish_host(u, g, ceiling)
    return (y, stats, u, need, g) if details else (y, stats)


# ------------------------------------------------------------------------------------------------
# streams: which outputs are final, which samples are still to be read
# ------------------------------------------------------------------------------------------------
def trim_ceiling(ceiling):
    """The ceiling the static stage behind a true-peak limiter is given (``level.gains_device``): c (1 - 2^-16).  The gain
    c' / peak is rounded to float32, every sample's product is, and the true peak of the trimmed audio is the resampler's
    chain over those products, not the measured peak times the gain: 45 terms and as many sums, each off by 2^-24 of a sum of
    magnitudes that is up to 2.5 times the result (the L1 norm of a phase of the 4x filter), 7e-6 relative at the most.  With
    twice that taken off (0.00013 dB) the trimmed true peak is <= c and not just close to it."""
    # an estimate, not a proof for every item: the bound above is derived, the factor of two on it is a choice
    return float(ceiling) * (1.0 - 2.0 ** -16)


def ready_outputs(have, h, final=None):
    """The number of final outputs of a stream with ``have`` samples: every one once it is closed at ``final`` samples,
    else output i once have >= i + 2 h + 1."""
    return int(final) if final is not None and final >= 0 else max(0, int(have) - 2 * int(h))


def keep_from(next_out, h, H):
    """The first sample the outputs from ``next_out`` on still read: max(0, next_out - h - H)."""
    return max(0, int(next_out) - int(h) - int(H))


class StreamLimiterHost:
    """The stream restatement on the host: ``push`` samples in any cuts, get the outputs that became final.  Their
    concatenation has the bits of :func:`limit_host` on the whole item."""

    def __init__(self, g0, ceiling, h, H):
        self.g0, self.ceiling, self.h, self.H = np.float32(g0), np.float32(ceiling), int(h), int(H)
        self.kept = np.zeros(0, dtype=np.float32)           # the samples from `base` on
        self.base = self.have = self.done = 0
        self.stats = LimitStats(np.float32(1.0), 0, 0)

    def push(self, samples, last=False):
        samples = np.ascontiguousarray(samples, dtype=np.float32)
        self.kept = np.concatenate((self.kept, samples))
        self.have += samples.size
        a, b = self.done, ready_outputs(self.have, self.h, self.have if last else None)
        if b <= a:
            return np.zeros(0, dtype=np.float32)
        h, H = self.h, self.H
        lo, hi = a - h - H, b + 2 * h                       # the span of needs
        end = self.have if last else hi                     # an open stream has hi <= have
        inside = self.kept[max(lo, 0) - self.base:min(hi, end) - self.base]
        with np.errstate(invalid="ignore", over="ignore"):
            u = (inside * self.g0).astype(np.float32)
        span = np.concatenate((np.ones(max(0, -lo), dtype=np.float32), needs_host(u, self.ceiling),
                               np.ones(max(0, hi - end), dtype=np.float32)))
        g = gain_span_host(span, h, H)
        first = a - max(lo, 0)
        y, stats = finish_host(u[first:first + (b - a)], g, self.ceiling)
        self.stats = self.stats.merged(stats)
        self.done = b
        keep = keep_from(b, h, H)
        self.kept, self.base = self.kept[keep - self.base:], keep
        return y


# ------------------------------------------------------------------------------------------------
# the device stage
# ------------------------------------------------------------------------------------------------
_device_weights = {}


def device_weights(h, device):
    """w on the device, made and uploaded once per (h, device)."""
    import torch
    key = (int(h), str(device))
    if key not in _device_weights:
        _device_weights[key] = torch.as_tensor(weights(h), device=device)
    return _device_weights[key]


def new_stats(count, device):
    """int32 (count, 4) statistics of items nothing has been limited in yet."""
    import torch
    stats = torch.zeros((int(count), STAT_WORDS), dtype=torch.int32, device=device)
    stats[:, 0] = ONE_BITS
    return stats


def workspace_floats(stride, batch, h, H, n_taps=0):
    """The floats of the workspace of ``mbxd_limit`` in place (``mbxd_limit_workspace_floats``)."""
    reach = n_taps // 4 + 2 if n_taps else 0
    return int(batch) * (-(-int(stride) // TILE)) * (3 * int(h) + int(H) + 2 * reach)


def limit_device(audio, n_samples, gains, ceiling, h, H, rate=None, true_peak=False, out=None, workspace=None):
    """The definition on every item audio[b, :n_samples[b]] of a float32 cuda batch (B, stride), enqueued on the current
    stream: ``(out, stats)`` with ``out`` (B, stride) float32 -- a new tensor, or ``out``; ``out=audio`` is in place, with the
    same bits, through ``workspace`` (a float32 tensor of ``workspace_floats`` elements, allocated when None: the samples
    every tile reads outside itself are saved there first) -- and ``stats`` int32 (B, 4) on the device.  ``gains``: float32 (B,) on the device
    (g0 per item), or one number.  ``true_peak``: needs from the 4x true peak, with the taps of ``resample.device_taps``."""
    import ctypes
    import torch
    from .abi import _check, load_library
    from .level import _check_audio
    counts = _check_audio(audio, n_samples, "limit_device")
    B, dev = int(audio.shape[0]), audio.device
    if np.isscalar(gains):
        gains = torch.full((B,), float(gains), dtype=torch.float32, device=dev)
    if gains.dtype != torch.float32 or tuple(gains.shape) != (B,) or gains.device != dev or not gains.is_contiguous():
        raise ValueError("limit_device: gains must be a contiguous float32 tensor (batch,) on the device of audio")
    if out is None:
        out = torch.empty_like(audio)
    _check_audio(out, n_samples, "limit_device (out)")
    if out.device != dev:
        raise ValueError("limit_device: out must be on the device of audio")
    taps, n_taps = None, 0
    if true_peak:
        from .resample import device_taps
        rate = 48000 if rate is None else int(round(rate))  # the design depends on the ratio alone
        taps, up, down = device_taps(rate, 4 * rate, dev)
        assert (up, down) == (4, 1)
        n_taps = int(taps.numel())
    check_window(int(h), int(H), n_taps)
    stats = torch.empty((B, STAT_WORDS), dtype=torch.int32, device=dev)
    if B == 0:
        return out, stats
    if out.data_ptr() == audio.data_ptr():
        need = workspace_floats(audio.shape[1], B, h, H, n_taps)
        if workspace is None:
            workspace = torch.empty((max(need, 1),), dtype=torch.float32, device=dev)
        if workspace.dtype != torch.float32 or workspace.device != dev or not workspace.is_contiguous() or workspace.numel() < need:
            raise ValueError(f"limit_device: in place needs a contiguous float32 workspace of {need} elements on the device of audio")
    w = device_weights(h, dev)
    counts_c = (ctypes.c_int64 * B)(*counts)
    with torch.cuda.device(dev):
        _check(load_library().mbxd_limit(audio.data_ptr(), int(audio.shape[1]), B, counts_c, gains.data_ptr(), float(ceiling),
                                         int(h), int(H), w.data_ptr(), taps.data_ptr() if taps is not None else None, n_taps,
                                         out.data_ptr(), int(out.shape[1]), stats.data_ptr(),
                                         workspace.data_ptr() if workspace is not None else None,
                                         int(workspace.numel()) if workspace is not None else 0,
                                         torch.cuda.current_stream(dev).cuda_stream))
    return out, stats


def limit_emit_device(rings, desc, n_rows, max_new, ceiling, h, H, out, stats=None):
    """``mbxd_limit_emit``: the new outputs of every stream of a tick from the rings (n_slots, ring_samples) into the packed
    rows ``out``; ``desc`` int64 (n_rows, 6) on the device; ``stats`` None or int32 (n_slots, 4) from :func:`new_stats`."""
    import torch
    from .abi import _check, load_library
    dev = rings.device
    check_window(int(h), int(H))
    w = device_weights(h, dev)
    with torch.cuda.device(dev):
        _check(load_library().mbxd_limit_emit(rings.data_ptr(), int(rings.shape[0]), int(rings.shape[1]), desc.data_ptr(),
                                              int(n_rows), int(max_new), float(ceiling), int(h), int(H), w.data_ptr(),
                                              out.data_ptr(), int(out.numel()),
                                              stats.data_ptr() if stats is not None else None,
                                              torch.cuda.current_stream(dev).cuda_stream))
    return out


def gain_bits(g0):
    """The sixth word of a descriptor row of ``mbxd_limit_emit``: the bit pattern of the float32 gain."""
    return int(np.float32(g0).view(np.uint32))


def emit_row(slot, first_out, count, final, out_offset, g0):
    """One descriptor row of ``mbxd_limit_emit``; ``final``: the stream's length once it is known, else None."""
    return [int(slot), int(first_out), int(count), -1 if final is None else int(final), int(out_offset), gain_bits(g0)]
