"""F0 from the audio itself: a YIN-type tracker on the frame grid of the mel analysis.

:func:`track_f0_host` is THE DEFINITION, in numpy float32; ``csrc/f0_track.hip`` (``mbxp_track_f0``, include/mbexwn_pitch.h)
gives its bits.  Every operation is one separately rounded float32 operation, every sum has one fixed order, the division is
the correctly rounded one -- the arrangement ``envelope.warp_envelope_host`` has with ``csrc/mel_envelope.hip``.

With ``L = W + tau_max`` the frame with centre ``c`` (clipped to [0, n]) is ``y[i] = x[c - L // 2 + i]``, zero outside the
sound: no reflection, which would manufacture periodicity.  For every lag ``1 <= tau <= tau_max``

    s = (tau_max - tau) >> 1                        both windows lie symmetrically about the frame's centre
    d[tau]  = S((y[s + j] - y[s + tau + j])^2)      0 <= j < W, S = :func:`lane_sum`
    d'[tau] = d[tau] * tau / (d[1] + ... + d[tau])  the running sum sequential; 1 where it is not positive

and ``E = S(y[h + j]^2)`` with ``h = tau_max >> 1`` is the energy of the W samples about the centre.  The pick is the smallest
``tau`` in ``[max(tau_min, 2), tau_max - 1]`` with ``d'[tau] < threshold``, moved on while the next ``d'`` is smaller; the
periodicity is ``d'`` there (without a pick: at the first index of its minimum over that range, and ``f0 = 0``).  A pick with
``E >= e_min`` gives ``f0 = sr / (tau + off)`` with the vertex ``off`` of the parabola through ``d'[tau - 1 .. tau + 1]``,
clamped to [-1, 1]; one without gives ``f0 = 0``.  ``f0 == 0`` means unvoiced.  A frame that touches a sample which is not
finite, or larger in magnitude than :data:`SAMPLE_LIMIT` (the sums could overflow), is unvoiced with periodicity 1.
"""
import math

import numpy as np

f32 = np.float32

# |x| above this (or not finite) makes a frame unvoiced: below it no sum of the definition overflows
# (2048 lags * 2048 terms * (2e15)^2 * 2048 < 3.4e38), so d' is never NaN and the searches need no rule for one
SAMPLE_LIMIT = f32(1e15)

PARAM_KEYS = ("sample_rate", "window", "tau_min", "tau_max", "threshold", "e_min")


def check_params(prm):
    """Raise ValueError unless the dictionary is one :func:`track_f0_host` and ``mbxp_track_f0`` accept."""
    if sorted(prm) != sorted(PARAM_KEYS):
        raise ValueError(f"f0 parameters must have the keys {PARAM_KEYS}, got {sorted(prm)}")
    sr, W, t0, t1 = (int(prm[kk]) for kk in PARAM_KEYS[:4])
    if sr < 1:
        raise ValueError(f"f0 parameters: sample_rate must be at least 1, got {sr}")
    if W < 64 or W > 2048 or W % 64:
        raise ValueError(f"f0 parameters: window must be a multiple of 64 in 64 .. 2048, got {W}")
    if t1 < 2 or t0 < 0 or max(t0, 2) > t1 - 1:
        raise ValueError(f"f0 parameters: need 0 <= tau_min, 2 <= tau_max and max(tau_min, 2) <= tau_max - 1, got {t0}, {t1}")
    if W + t1 > 4096:
        raise ValueError(f"f0 parameters: window + tau_max must be at most 4096, got {W} + {t1}")
    if math.isnan(float(prm["threshold"])) or math.isnan(float(prm["e_min"])):
        raise ValueError("f0 parameters: threshold and e_min must be numbers")
    return prm


def params(sample_rate, f0_min=55.0, f0_max=1000.0, window=1024, threshold=0.15, rms_floor=1e-4):
    """The tracker's integers and floor from a frequency range: ``tau_max = ceil(sr / f0_min)``, ``tau_min = floor(sr /
    f0_max)``, ``e_min = float32(window * rms_floor^2)``.  24 kHz and the defaults: tau_min 24, tau_max 437, L = 1461."""
    sr = int(sample_rate)
    f0_min, f0_max = float(f0_min), float(f0_max)
    if sr < 1 or sr != sample_rate:
        raise ValueError(f"f0 parameters: sample_rate must be a positive integer, got {sample_rate!r}")
    if not (math.isfinite(f0_min) and math.isfinite(f0_max) and 0.0 < f0_min < f0_max):
        raise ValueError(f"f0 parameters: need 0 < f0_min < f0_max, got {f0_min}, {f0_max}")
    if not (math.isfinite(float(rms_floor)) and float(rms_floor) >= 0.0):
        raise ValueError(f"f0 parameters: rms_floor must not be negative, got {rms_floor!r}")
    if window != int(window):
        raise ValueError(f"f0 parameters: window must be an integer, got {window!r}")
    if sr / f0_min > 4096 or sr / f0_max > 4096:
        raise ValueError(f"f0 parameters: f0_min {f0_min} Hz needs lags above 4096 samples at {sr} Hz")
    return check_params({"sample_rate": sr, "window": int(window), "tau_min": int(math.floor(sr / f0_max)),
                         "tau_max": int(math.ceil(sr / f0_min)), "threshold": float(f32(threshold)),
                         "e_min": float(f32(int(window) * float(rms_floor) ** 2))})


def lane_sum(p):
    """The definition's sum of W = 64 m values, over the last axis: 64 partial sums ``a[l] = p[l] + p[l + 64] + ...`` in that
    order, then halved six times, ``a[l] = a[l] + a[l + m]`` for ``l < m``, m = 32 .. 1.  (An xor butterfly over a 64-lane wave
    gives the same bits: float addition commutes.)"""
    p = np.asarray(p, dtype=f32)
    q = p.reshape(p.shape[:-1] + (p.shape[-1] // 64, 64))
    acc = q[..., 0, :].copy()
    for kk in range(1, q.shape[-2]):
        acc = acc + q[..., kk, :]
    m = 32
    while m >= 1:
        acc = acc[..., :m] + acc[..., m:2 * m]
        m >>= 1
    return acc[..., 0]


def difference_host(x, centres, prm):
    """The first half of :func:`track_f0_host`: ``d'`` (K, tau_max + 1; column 0 unused), the energy (K,) and which frames
    touch a sample that is not finite or above :data:`SAMPLE_LIMIT` (K,) -- everything that does not depend on the
    threshold, the energy floor and tau_min."""
    check_params(prm)
    x = np.ascontiguousarray(x, dtype=f32)
    if x.ndim != 1:
        raise ValueError(f"track_f0_host: the sound must be 1-D, got shape {x.shape}")
    cc = np.asarray(centres)
    if cc.ndim != 1 or (cc.size and cc.dtype.kind not in "iu"):
        raise ValueError("track_f0_host: centres must be a 1-D integer array")
    n, K = x.size, cc.size
    W, tau_max = int(prm["window"]), int(prm["tau_max"])
    L = W + tau_max
    cc = np.clip(cc.astype(np.int64), 0, n)
    idx = cc[:, None] - (L >> 1) + np.arange(L, dtype=np.int64)[None, :]
    inside = (idx >= 0) & (idx < n)
    y = np.where(inside, x[np.clip(idx, 0, max(n - 1, 0))] if n else f32(0), f32(0)).astype(f32)
    with np.errstate(all="ignore"):
        bad = ~(np.abs(y) <= SAMPLE_LIMIT).all(axis=1)
        y[bad] = f32(0)                                          # their result is fixed in pick_host; keep the arithmetic quiet
        d = np.zeros((K, tau_max + 1), dtype=f32)
        for tau in range(1, tau_max + 1):
            s = (tau_max - tau) >> 1
            e = y[:, s:s + W] - y[:, s + tau:s + tau + W]
            d[:, tau] = lane_sum(e * e)
        h = tau_max >> 1
        energy = lane_sum(y[:, h:h + W] * y[:, h:h + W])
        dp = np.ones((K, tau_max + 1), dtype=f32)
        run = np.zeros(K, dtype=f32)
        for tau in range(1, tau_max + 1):
            run = run + d[:, tau]
            num = d[:, tau] * f32(tau)
            dp[:, tau] = np.where(run > 0, num / np.where(run > 0, run, f32(1)), f32(1))
    return dp, energy, bad


def pick_host(dp, energy, bad, prm):
    """The second half of :func:`track_f0_host`: (f0, periodicity) from :func:`difference_host`'s results."""
    check_params(prm)
    sr, tau_min, tau_max = int(prm["sample_rate"]), int(prm["tau_min"]), int(prm["tau_max"])
    thr, e_min = f32(prm["threshold"]), f32(prm["e_min"])
    K = dp.shape[0]
    f0, per = np.zeros(K, dtype=f32), np.ones(K, dtype=f32)
    lo, hi = max(tau_min, 2), tau_max - 1
    below = dp[:, lo:hi + 1] < thr
    for t in range(K):
        if bad[t]:
            continue
        if not below[t].any():
            per[t] = dp[t, lo + int(np.argmin(dp[t, lo:hi + 1]))]
            continue
        tau = lo + int(np.argmax(below[t]))
        while tau + 1 <= hi and dp[t, tau + 1] < dp[t, tau]:
            tau += 1
        per[t] = dp[t, tau]
        if not energy[t] >= e_min:
            continue
        a, b, g = dp[t, tau - 1], dp[t, tau], dp[t, tau + 1]
        den = f32(f32(a - b) + f32(g - b))
        off = f32(0)
        if den > 0:
            with np.errstate(all="ignore"):
                off = f32(f32(f32(a - g) / den) * f32(0.5))
            off = min(max(off, f32(-1)), f32(1))
        f0[t] = f32(sr) / f32(f32(tau) + off)
    return f0, per


def track_f0_host(x, centres, prm):
    """F0 (Hz, 0 = unvoiced) and periodicity of the frames of the 1-D sound ``x`` centred on the integer samples ``centres``
    (clipped to [0, len(x)]): two float32 arrays (K,).  ``prm``: :func:`params`.  The module's docstring is the definition;
    :func:`difference_host` and :func:`pick_host` are its two halves."""
    return pick_host(*difference_host(x, centres, prm), prm)


def track_f0_device(audio, n_samples, centres, n_frames, prm):
    """:func:`track_f0_host` on the GPU (csrc/f0_track.hip through ``mbxp_track_f0``, include/mbexwn_pitch.h), for a ragged
    batch: ``audio`` float32 cuda (batch, stride), ``n_samples`` int32 cuda (batch,), ``centres`` int64 cuda (batch,
    max_frames), ``n_frames`` int32 cuda (batch,).  Returns two cuda tensors (batch, max_frames), f0 and periodicity; rows of
    item b from ``n_frames[b]`` on are not written (they stay zero).  No engine: the launch goes to the current stream of the
    buffers' device."""
    import ctypes
    import torch
    from .abi import _check, load_library
    check_params(prm)
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
    f0 = torch.zeros((B, frames), dtype=torch.float32, device=dev)
    per = torch.zeros((B, frames), dtype=torch.float32, device=dev)
    if B == 0 or frames == 0:
        return f0, per
    with torch.cuda.device(dev):
        _check(load_library().mbxp_track_f0(audio.data_ptr(), N, B, n_samples.data_ptr(), centres.data_ptr(), n_frames.data_ptr(),
                                            frames, int(prm["sample_rate"]), int(prm["window"]), int(prm["tau_min"]),
                                            int(prm["tau_max"]), ctypes.c_float(float(prm["threshold"])),
                                            ctypes.c_float(float(prm["e_min"])), f0.data_ptr(), per.data_ptr(),
                                            torch.cuda.current_stream(dev).cuda_stream))
    return f0, per


def fill_unvoiced(f0):
    """A contour the oscillator can take (``f0_frames`` must be positive everywhere) from a tracked one, in float32: voiced
    frames keep their bits; a gap between voiced frames ``i < k`` gets ``f0[i] + (f0[k] - f0[i]) * (float(t - i) / float(k -
    i))``; frames in front of the first voiced one take its value, frames behind the last one the last's.  No voiced frame
    (or no frame) at all: None -- the item then keeps the model's own F0."""
    f0 = np.asarray(f0, dtype=f32)
    if f0.ndim != 1:
        raise ValueError(f"fill_unvoiced: the contour must be 1-D, got shape {f0.shape}")
    if not np.all(np.isfinite(f0)) or np.any(f0 < 0):
        raise ValueError("fill_unvoiced: the contour must be finite and not negative (0 = unvoiced)")
    voiced = np.flatnonzero(f0 > 0)
    if voiced.size == 0:
        return None
    out = f0.copy()
    out[:voiced[0]] = f0[voiced[0]]
    out[voiced[-1] + 1:] = f0[voiced[-1]]
    for i, k in zip(voiced[:-1], voiced[1:]):
        if k - i > 1:
            t = np.arange(i + 1, k)
            w = (t - i).astype(f32) / f32(k - i)
            out[i + 1:k] = f0[i] + f32(f0[k] - f0[i]) * w
    return out


F0_FILLS = ("interpolate", "hold")


def check_fill(f0_fill, f0_source, what):
    """Raise ValueError unless ``f0_fill`` is a fill and goes with ``f0_source``: "hold" fills a tracked contour."""
    if f0_fill not in F0_FILLS:
        raise ValueError(f"{what}: f0_fill must be one of {F0_FILLS}, got {f0_fill!r}")
    if f0_fill == "hold" and f0_source != "audio":
        raise ValueError(f"{what}: f0_fill='hold' fills the tracked contour and needs f0_source='audio'")


def fill_tracked(f0, f0_fill="interpolate", f0_initial=150.0):
    """The oscillator's contour from a tracked one: :func:`fill_unvoiced` (None without a voiced frame) or, "hold",
    :func:`fill_hold`."""
    return fill_hold(f0, f0_initial) if f0_fill == "hold" else fill_unvoiced(f0)


def fill_hold(f0, initial=150.0):
    """The causal fill, what a stream can do: voiced frames keep their bits, an unvoiced frame takes
    the last voiced value in front of it, frames in front of the first voiced one take ``float32(initial)``.  Always an
    array (float32, the shape of ``f0``).  Chunk by chunk with the last value of a chunk's result as the next chunk's
    ``initial`` it gives what it gives on the whole contour."""
    f0 = np.asarray(f0, dtype=f32)
    if f0.ndim != 1:
        raise ValueError(f"fill_hold: the contour must be 1-D, got shape {f0.shape}")
    if not np.all(np.isfinite(f0)) or np.any(f0 < 0):
        raise ValueError("fill_hold: the contour must be finite and not negative (0 = unvoiced)")
    try:
        with np.errstate(over="ignore"):
            start = f32(initial)
    except (TypeError, ValueError):
        raise ValueError(f"fill_hold: initial must be a finite positive frequency in Hz, got {initial!r}") from None
    if start.ndim != 0 or not (np.isfinite(start) and start > 0):
        raise ValueError(f"fill_hold: initial must be a finite positive frequency in Hz, got {initial!r}")
    # the index of the last voiced frame at or in front of every frame, -1 in front of the first
    last = np.maximum.accumulate(np.where(f0 > 0, np.arange(f0.size), -1)) if f0.size else np.zeros(0, dtype=np.int64)
    return np.where(last >= 0, f0[np.maximum(last, 0)], start).astype(f32)


def frame_times(n_frames, hop, sample_rate):
    """The time in seconds of every frame on the synthesis grid: frame k drives the hop samples from ``k * hop`` on."""
    return np.arange(int(n_frames), dtype=np.float64) * (int(hop) / float(sample_rate))


def write_f0(path, times, f0, periodicity):
    """A ``.f0`` file: one text row ``time_s f0_hz periodicity`` per frame, ``%.9g`` (a float32 survives it), 0 = unvoiced."""
    f0, periodicity = np.asarray(f0, dtype=f32), np.asarray(periodicity, dtype=f32)
    times = np.asarray(times, dtype=np.float64)
    if not (f0.ndim == 1 and f0.shape == periodicity.shape == times.shape):
        raise ValueError("write_f0: times, f0 and periodicity must be 1-D and equally long")
    with open(path, "w") as fh:
        for tt, ff, pp in zip(times, f0, periodicity):
            fh.write("%.9g %.9g %.9g\n" % (tt, ff, pp))


def read_f0(path, n_frames=None):
    """(times float64, f0 float32, periodicity float32) of a ``.f0`` file; blank lines and lines starting with # are skipped.
    ``n_frames``: the row count it must have (one per mel frame) -- another is refused."""
    rows = []
    with open(path) as fh:
        for ln, line in enumerate(fh, 1):
            line = line.strip()
            if not line or line.startswith("#"):
                continue
            parts = line.split()
            if len(parts) != 3:
                raise ValueError(f"{path}:{ln}: expected 'time_s f0_hz periodicity', got {line!r}")
            try:
                rows.append([float(pp) for pp in parts])
            except ValueError:
                raise ValueError(f"{path}:{ln}: not three numbers: {line!r}") from None
    arr = np.asarray(rows, dtype=np.float64).reshape(-1, 3)
    if n_frames is not None and arr.shape[0] != int(n_frames):
        raise ValueError(f"{path}: {arr.shape[0]} rows, but the mel has {int(n_frames)} frames (one row per frame)")
    f0 = arr[:, 1].astype(f32)
    if not np.all(np.isfinite(f0)) or np.any(f0 < 0):
        raise ValueError(f"{path}: f0 must be finite and not negative (0 = unvoiced)")
    return arr[:, 0], f0, arr[:, 2].astype(f32)
