"""Sample-rate conversion in front of the mel analysis: the reference's resampler, on the host and on the device.

Restates
  resample (filter design)       reference MBExWN_NVoc/sig_proc/resample.py:31-63
  scipy.signal.resample_poly     the call the reference ends in (:64), as one closed formula

The definition everything here is tested against.  With ``taps, up, down = reference_filter(in_sr, out_sr)``,
``g = float32(taps * up)`` and ``half, pre, rem, n_out = plan(len(taps), up, down, n)``:

    y[k] = sum_j g[(k + rem) * down - j * up - pre] * x[j]            0 <= k < n_out

over 0 <= j < n with the tap index inside [0, n_taps).  ``half + pre`` is a multiple of ``down``, so the tap index is
``k * down + half - j * up``: that is what the device kernel (csrc/resample_poly.hip) evaluates, one float32 fmaf chain
per output over ascending j.  ``resample_host`` evaluates the same taps in float64 and rounds once.

Live streams at another rate than the model's (live.py, csrc/resample_stream.hip) evaluate the same chain from a ring as
the samples arrive -- output k once sample (k * down + half) // up is there -- through the one device function both kernels
share (csrc/resample_chain.h): ``resample_device`` on the whole sound is what a stream's outputs are tested against.
"""
from functools import lru_cache
from math import ceil, gcd, pi

import numpy as np

DEVICE_TILE = 1024          # outputs per block of the device kernel (MBXA_RESAMPLE_TILE of include/mbexwn_audio.h)


def positive_rate(rate, what="rate"):
    """A sample rate a caller handed in, as an int of Hz; anything that is not a finite positive number is refused."""
    if rate is None or isinstance(rate, (str, bytes)) or not np.isfinite(rate) or int(round(rate)) <= 0:
        raise ValueError(f"{what} must be a positive rate in Hz, got {rate!r}")
    return int(round(rate))


def reference_filter(in_sr, out_sr, stop_att=70, trans_width_normed=0.1, dtype=np.float32):
    """The reference's anti-aliasing FIR for in_sr -> out_sr: ``(taps, up, down)`` with integer up / down.

    Kept as the reference has it: the Kaiser beta comes from ``stop_att`` once, BEFORE the loop that lowers ``stop_att`` by
    6 dB while the filter would span more than 8000 input samples, and is not recomputed; the taps are designed in float64
    and cast to float32 for float32 input (``dtype``), any other dtype keeps float64."""
    from scipy.signal import firwin
    in_sr, out_sr = int(in_sr), int(out_sr)
    if in_sr <= 0 or out_sr <= 0:
        raise ValueError(f"resample: invalid sample rates {in_sr} -> {out_sr}")
    gg = gcd(in_sr, out_sr)
    up, down = out_sr // gg, in_sr // gg
    if stop_att >= 50:
        beta = 0.1102 * (stop_att - 8.7)
    elif stop_att >= 21:
        beta = 0.5842 * pow(stop_att - 21., 0.4) + 0.07886 * (stop_att - 21.)
    else:
        beta = 0.
    trans_width = 2 * pi * min(1., out_sr / in_sr) * trans_width_normed
    while True:
        radius = int(ceil((stop_att - 8.) / 2.285 / trans_width / 2))
        if 2 * radius > 8000 and stop_att > 10:
            stop_att -= 6
        else:
            break
    taps = firwin((2 * radius + 1) * up, cutoff=(1 - trans_width_normed) / max(up, down), window=("kaiser", beta))
    return taps.astype(np.float32 if np.dtype(dtype) == np.float32 else np.float64, copy=False), up, down


def plan(n_taps, up, down, n):
    """The indexing of scipy.signal.resample_poly for an n-sample signal: ``(half, pre, rem, n_out)`` -- the filter's
    centre, the zeros put in front of the taps so that the centre lands on an output, the outputs dropped in front, and
    the output length."""
    half = (int(n_taps) - 1) // 2
    pre = down - half % down
    rem = (half + pre) // down
    n_out = -(-int(n) * up // down)
    return half, pre, rem, n_out


def scaled_taps(taps, up):
    """``g`` of the definition: the taps times the gain ``up``, rounded to float32 (scipy: ``h = window * up`` in the
    window's dtype)."""
    return (np.asarray(taps, dtype=np.float32) * np.float32(up)).astype(np.float32)


@lru_cache(maxsize=16)
def _host_taps(in_sr, out_sr):
    taps, up, down = reference_filter(in_sr, out_sr)
    g = scaled_taps(taps, up).astype(np.float64)
    g.setflags(write=False)
    return g, up, down


def resample_host(x, in_sr, out_sr):
    """The definition evaluated in float64 on the float32 taps ``g`` (scipy.signal.upfirdn), rounded once to float32.
    ``x``: 1-D; a signal already at ``out_sr`` comes back as float32 unchanged."""
    from scipy.signal import upfirdn
    x = np.asarray(x)
    if x.ndim != 1:
        raise ValueError("resample_host: a 1-D signal is expected")
    if int(in_sr) == int(out_sr):
        return x.astype(np.float32, copy=False)
    g, up, down = _host_taps(int(in_sr), int(out_sr))
    half, pre, rem, n_out = plan(g.size, up, down, x.size)
    if n_out == 0:
        return np.zeros(0, dtype=np.float32)
    # upfirdn(h, x)[m] = sum_j h[m * down - j * up] x[j]: `pre` zeros in front of g shift the tap index as the definition
    # does; zeros behind make the output long enough for m = rem + n_out - 1
    post = max(0, (rem + n_out) * down - ((x.size - 1) * up + pre + g.size))
    h = np.concatenate((np.zeros(pre), g, np.zeros(post)))
    y = upfirdn(h, x.astype(np.float64), up, down)[rem:rem + n_out]
    assert y.size == n_out
    return y.astype(np.float32)


_device_taps = {}


def device_taps(in_sr, out_sr, device):
    """``(g on the device, up, down)``, designed and uploaded once per (rates, device)."""
    import torch
    key = (int(in_sr), int(out_sr), str(device))
    if key not in _device_taps:
        taps, up, down = reference_filter(in_sr, out_sr)
        _device_taps[key] = (torch.as_tensor(scaled_taps(taps, up), device=device), up, down)
    return _device_taps[key]


def resample_device(sound, n_samples, in_sr, out_sr):
    """The definition on the GPU (csrc/resample_poly.hip through ``mbxa_resample_poly``): ``sound`` is a float32 cuda tensor
    (batch, N), ``n_samples`` an optional int32 cuda tensor (batch,) of item lengths.  Returns ``(out, n_out)``: a float32
    cuda tensor (batch, ceil(N * up / down)) of which item b's first ``n_out[b]`` samples are written (the rest of a row is
    whatever the allocation held), and the int32 cuda tensor (batch,) of those lengths -- what ``compute_log_mel_device``
    takes as its ``n_samples``.  The row length comes from N by integer arithmetic on the host; the lengths stay on the
    device (integer tensor arithmetic, clamped as the kernel clamps them): no device-to-host copy, no synchronisation."""
    import torch
    from .abi import _check, load_library
    if sound.dim() != 2 or sound.dtype != torch.float32 or not sound.is_cuda:
        raise ValueError("sound must be a float32 cuda tensor of shape (batch, time)")
    dev = sound.device
    B, N = int(sound.shape[0]), int(sound.shape[1])
    if n_samples is not None:
        if n_samples.dtype != torch.int32 or tuple(n_samples.shape) != (B,) or n_samples.device != dev:
            raise ValueError("n_samples must be an int32 tensor of shape (batch,) on the device of sound")
        n_samples = n_samples.contiguous()
    g, up, down = device_taps(in_sr, out_sr, dev)
    max_out = -(-N * up // down)
    if max_out >= 2 ** 31:
        raise ValueError("resample_device: the resampled row does not fit 32-bit sample counts")
    sound = sound.contiguous()
    out = torch.empty((B, max_out), dtype=torch.float32, device=dev)
    if B == 0 or max_out == 0:
        return out, torch.zeros((B,), dtype=torch.int32, device=dev)
    if n_samples is None:
        n_out = torch.full((B,), max_out, dtype=torch.int32, device=dev)
    else:
        n_out = ((n_samples.clamp(0, N).to(torch.int64) * up + (down - 1)) // down).to(torch.int32)
    # no handle, hence no device of its own: the launch goes to the CURRENT device, which must be the buffers'
    with torch.cuda.device(dev):
        _check(load_library().mbxa_resample_poly(sound.data_ptr(), n_samples.data_ptr() if n_samples is not None else None,
                                                 B, N, up, down, g.data_ptr(), int(g.numel()), out.data_ptr(), max_out,
                                                 torch.cuda.current_stream(dev).cuda_stream))
    return out, n_out
