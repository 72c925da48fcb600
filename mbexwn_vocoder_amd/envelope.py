"""Formant shift: the mel envelope of a frame read at ``f / phi`` -- the host definition of
``mbxe_warp_envelope`` (include/mbexwn_envelope.h, csrc/mel_envelope.hip), in numpy float32.

A log-mel row ``x[0..n)`` is log amplitude at the channel centre frequencies ``c[0..n)``.  Between the centres the envelope is
linear in Hz, outside ``[c[0], c[n-1]]`` it is held.  The warped row is that envelope read at ``c[m] / phi``: ``phi > 1``
moves the formants up.  Every step is one separately rounded float32 operation (numpy has no fused multiply-add), which the
device repeats with contraction switched off, so host and device give the same bits.  The overall level is not compensated.
"""
import numpy as np

from .analysis import mel_frequencies


def channel_centres(preprocess_config):
    """The float32 roundings of the mel channels' centre frequencies in Hz, (mel_channels,), strictly increasing: the
    inner points of the mel filter bank's edge frequencies, computed in float64."""
    cfg = preprocess_config
    n_mels = int(cfg["mel_channels"])
    fmax = cfg["sample_rate"] / 2.0 if cfg.get("fmax") is None else cfg["fmax"]
    centres = np.ascontiguousarray(mel_frequencies(n_mels + 2, cfg["fmin"], fmax)[1:-1].astype(np.float32))
    if n_mels < 2 or not np.all(np.diff(centres) > 0):
        raise ValueError("the formant shift needs at least two mel channels with strictly increasing centre frequencies")
    return centres


def warp_envelope_host(mel, factors, centres, n_frames=None):
    """``mel`` (..., frames, n) float32 rows, ``factors`` (..., frames) float32 (finite, > 0), ``centres`` (n,) float32 ->
    the warped rows, float32, same shape.  A factor of exactly 1 copies the row; ``n_frames`` (one count per item of a
    (batch, frames, n) input) leaves the rows at or behind an item's count as copies."""
    x = np.ascontiguousarray(mel, dtype=np.float32)
    c = np.ascontiguousarray(centres, dtype=np.float32)
    n = c.shape[0]
    if x.ndim < 2 or x.shape[-1] != n or n < 2:
        raise ValueError("warp_envelope_host: mel must be (..., frames, n) with n = len(centres) >= 2")
    phi = np.broadcast_to(np.asarray(factors, dtype=np.float32), x.shape[:-1]).reshape(-1)
    rows = x.reshape(-1, n)
    with np.errstate(all="ignore"):
        f = c[None, :] / phi[:, None]                                     # one correctly rounded float32 division
        k = np.searchsorted(c, f.reshape(-1), side="right").reshape(f.shape)     # centres <= f
        i = np.clip(k - 1, 0, n - 2)
        lo, hi = np.take_along_axis(rows, i, axis=1), np.take_along_axis(rows, i + 1, axis=1)
        w = (f - c[i]) / (c[i + 1] - c[i])
        val = lo + w * (hi - lo)
    out = np.where(k == 0, rows[:, :1], np.where(k == n, rows[:, -1:], val)).astype(np.float32)
    keep = phi == np.float32(1.0)
    if n_frames is not None:
        if x.ndim != 3:
            raise ValueError("warp_envelope_host: n_frames needs a (batch, frames, n) input")
        counts = np.asarray(n_frames).reshape(-1, 1)
        keep = keep | (np.arange(x.shape[1])[None, :] >= counts).reshape(-1)
    out[keep] = rows[keep]
    return out.reshape(x.shape)
