"""The time map of a change of duration, defined once, on the host, in numpy.

A sound of ``n`` samples at the model rate ``R`` with hop ``H`` becomes K output frames; their integer centre samples
``c[0..K)`` lie in ``[0, n]``.  The analysis (``analysis.compute_log_mel_at`` on the host, ``mbxw_mel_frames_at`` on the
device) takes one frame around every centre, and the synthesizer emits ``H`` samples per frame at the pitch the frame carries:
K frames are K * H samples of the sound, slower or faster, at the original pitch.  Host and device cannot disagree about where
a frame lies, because the device only ever sees the integers.

Constant factor ``s`` (finite, > 0; the output lasts ``s`` times as long):
    K = int(floor(float64(n) * float64(s) / H)) + 1
    c[k] = clip(int(rint(float64(k * H) / float64(s))), 0, n)
  For s == 1.0 this is exactly K = n // H + 1, c[k] = k * H: the frames of the regular analysis.

Breakpoints, ``(m, 2)`` float64 rows ``(t_out, t_in)`` in seconds: ``t_out`` strictly increasing from 0, ``t_in``
non-decreasing within ``[0, n / R]`` (equal neighbours hold a frame):
    K = int(floor(t_out[-1] * R / H)) + 1
    c[k] = clip(int(rint(np.interp(k * H / R, t_out, t_in) * R)), 0, n)

Explicit centres, :class:`Centres` around an int64 array: K = its size, c = the array, which must be non-decreasing and lie
within ``[0, n]``.  This is how a map that was computed in frames (align.py) reaches the analysis
without a trip through float seconds, where ``floor(t_out[-1] * R / H) + 1`` could lose the last frame to rounding.
"""
import numpy as np

# the engine's limit: an item has at most 2^24 - 1 sub-band rows (32-bit row indices inside the kernels)
MAX_ROWS = (1 << 24) - 1


def check_factor(factor, what="time stretch"):
    """``factor`` as a float, or ValueError unless it is finite and positive."""
    try:
        value = float(factor)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: a finite positive factor is expected, got {factor!r}") from None
    if not (np.isfinite(value) and value > 0):
        raise ValueError(f"{what}: a finite positive factor is expected, got {factor!r}")
    return value


class Centres:
    """A time map given as the centre samples themselves: a 1-D array of at least one integer (kept as int64).  Whether they
    fit a sound -- non-decreasing, within [0, n], no more frames than the engine takes -- is checked where the sound's
    length is known (:func:`centres`, :func:`frame_count`).  A bare 1-D list is NOT this kind of spec: wrap it."""

    def __init__(self, values):
        arr = np.asarray(values)
        if arr.ndim != 1 or arr.size < 1 or arr.dtype.kind not in "iu":
            raise ValueError(f"time stretch: explicit centres are a 1-D integer array with at least one entry, got "
                             f"shape {arr.shape} of {arr.dtype}")
        self.values = arr.astype(np.int64)


def is_factor(spec):
    """True for a spec that is one number (a constant factor), False for None, a breakpoint array or :class:`Centres`."""
    return spec is not None and not isinstance(spec, Centres) and np.ndim(spec) == 0


def _check_frames(frames, rows_per_frame):
    limit = MAX_ROWS // max(1, int(rows_per_frame))
    if not frames <= limit:                                   # also an infinite or NaN count
        raise ValueError(f"time stretch: the stretched item would have {frames:.0f} frames, more than the engine's limit of "
                         f"{limit} frames (2^24 - 1 sub-band rows, {int(rows_per_frame)} per frame); split the recording")


def _plan(n, hop, rate, spec, rows_per_frame):
    """(K, factor or None, breakpoints or None) of a checked spec; for :class:`Centres` (K, None, the checked int64 array)."""
    n, hop = int(n), int(hop)
    if n < 0 or hop < 1 or not (np.isfinite(rate) and rate > 0):
        raise ValueError(f"time stretch: need n >= 0, hop >= 1 and a positive rate, got n={n}, hop={hop}, rate={rate}")
    if isinstance(spec, Centres):
        cc = spec.values
        if np.any(np.diff(cc) < 0):
            raise ValueError("time stretch: explicit centres must be non-decreasing")
        if cc[0] < 0 or cc[-1] > n:
            raise ValueError(f"time stretch: explicit centres must lie within [0, {n}], got {int(cc[0])} .. {int(cc[-1])}")
        _check_frames(float(cc.size), rows_per_frame)
        return int(cc.size), None, cc
    if spec is None or is_factor(spec):
        factor = np.float64(1.0 if spec is None else check_factor(spec))
        frames = np.floor(np.float64(n) * factor / hop) + 1
        _check_frames(frames, rows_per_frame)
        return int(frames), factor, None
    bp = np.asarray(spec, dtype=np.float64)
    if bp.ndim != 2 or bp.shape[1] != 2 or bp.shape[0] < 1:
        raise ValueError(f"time stretch: a breakpoint map is an (m, 2) array of (t_out, t_in) rows, got shape {bp.shape}")
    t_out, t_in = bp[:, 0], bp[:, 1]
    if not np.all(np.isfinite(bp)):
        raise ValueError("time stretch: a breakpoint map must be finite")
    if t_out[0] != 0 or np.any(np.diff(t_out) <= 0):
        raise ValueError("time stretch: t_out of a breakpoint map must be strictly increasing from 0")
    if np.any(np.diff(t_in) < 0) or t_in[0] < 0 or t_in[-1] > n / float(rate):
        raise ValueError(f"time stretch: t_in of a breakpoint map must be non-decreasing within [0, {n / float(rate)!r}] s")
    frames = np.floor(t_out[-1] * float(rate) / hop) + 1
    _check_frames(frames, rows_per_frame)
    return int(frames), None, bp


def frame_count(n, hop, rate, spec, rows_per_frame=1):
    """K of :func:`centres`, with its checks, without building the centres."""
    return _plan(n, hop, rate, spec, rows_per_frame)[0]


def centres(n, hop, rate, spec, rows_per_frame=1):
    """The int64 centre samples ``c[0..K)`` of the output frames of a sound of ``n`` samples at ``rate`` with hop ``hop``.

    ``spec``: None (the regular frames, factor 1), a factor, a breakpoint array or :class:`Centres` (the module's text gives
    the definitions).  ``rows_per_frame``: the sub-band rows the engine makes of one frame (``ModelDims.steps_per_frame``); K
    may not exceed ``(2^24 - 1) // rows_per_frame`` frames.  ValueError for a factor that is not finite or not positive, a
    malformed or non-monotone map, and a K above that limit (the message names the limit in frames)."""
    frames, factor, bp = _plan(n, hop, rate, spec, rows_per_frame)
    if isinstance(spec, Centres):
        return bp.copy()
    kk = np.arange(frames, dtype=np.int64)
    if bp is None:
        pos = np.rint((kk * int(hop)).astype(np.float64) / factor)
    else:
        pos = np.rint(np.interp(kk * int(hop) / float(rate), bp[:, 0], bp[:, 1]) * float(rate))
    return np.clip(pos.astype(np.int64), 0, int(n))


def per_item(spec, count, what="time_stretch"):
    """One spec per item out of ``spec``: None, one factor or one breakpoint array for all, or a list / tuple of ``count``
    specs.  (A 2-D array is one map; a list is one spec per item.)"""
    if isinstance(spec, (list, tuple)):
        if len(spec) != count:
            raise ValueError(f"{what}: one entry per item ({count}) is expected, got {len(spec)}")
        return list(spec)
    return [spec] * count
