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


_device_centres = {}


def device_centres(preprocess_config, device):
    """``channel_centres`` of an analysis as a float32 tensor on the device, uploaded once per (analysis, device)."""
    import torch
    cfg = preprocess_config
    key = (int(cfg["mel_channels"]), float(cfg["fmin"]), cfg.get("fmax"), float(cfg["sample_rate"]), str(device))
    if key not in _device_centres:
        _device_centres[key] = torch.as_tensor(channel_centres(cfg), device=device)
    return _device_centres[key]


def warp_envelope_device(mel, factors, centres, n_frames=None):
    """The definition on the GPU (``mbxe_warp_envelope``, csrc/mel_envelope.hip): mel float32 cuda (B, T, n) -- a view with a
    batch stride of its own is passed as it is --, factors float32 (B, T), centres float32 (n,) (``device_centres``), n_frames
    optional int32 (B,), all on the device of mel -> the warped rows (B, T, n) with the batch stride of mel (the kernel has one
    item stride for both), bit-equal to :func:`warp_envelope_host`.
    Enqueued on the current stream of that device."""
    import torch
    from .abi import _check, load_library
    if not torch.is_tensor(mel) or mel.dim() != 3 or mel.dtype != torch.float32 or not mel.is_cuda:
        raise ValueError("mel must be a float32 cuda tensor (batch, frames, channels)")
    dev = mel.device
    B, T, n = (int(ss) for ss in mel.shape)
    if not torch.is_tensor(centres) or centres.dtype != torch.float32 or tuple(centres.shape) != (n,) or centres.device != dev:
        raise ValueError(f"centres must be a float32 tensor of shape ({n},) on the device of mel")
    if not torch.is_tensor(factors) or factors.dtype != torch.float32 or tuple(factors.shape) != (B, T) or factors.device != dev:
        raise ValueError(f"factors must be a float32 tensor of shape ({B}, {T}) on the device of mel")
    if n_frames is not None and (not torch.is_tensor(n_frames) or n_frames.dtype != torch.int32 or
                                 tuple(n_frames.shape) != (B,) or n_frames.device != dev):
        raise ValueError("n_frames must be an int32 tensor of shape (batch,) on the device of mel")
    if B == 0 or T == 0:
        return torch.empty((B, T, n), dtype=torch.float32, device=dev)
    if mel.stride(2) != 1 or mel.stride(1) != n or (B > 1 and mel.stride(0) < T * n):
        mel = mel.contiguous()
    factors, centres = factors.contiguous(), centres.contiguous()
    # row_stride_items is the item stride of mel AND of out: the result of a strided view is a view with the same batch stride
    stride = int(mel.stride(0)) if B > 1 else T * n
    out = torch.empty((B - 1) * stride + T * n, dtype=torch.float32, device=dev).as_strided((B, T, n), (stride, n, 1))
    # no handle, hence no device of its own: the launch goes to the CURRENT device, which must be the buffers'
    with torch.cuda.device(dev):
        _check(load_library().mbxe_warp_envelope(mel.data_ptr(), stride, B,
                                                 n_frames.contiguous().data_ptr() if n_frames is not None else None, T, n,
                                                 centres.data_ptr(), factors.data_ptr(), out.data_ptr(),
                                                 torch.cuda.current_stream(dev).cuda_stream))
    return out
