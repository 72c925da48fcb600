"""Keyed noise: the N(0,1) draw of the model's noise channel as a function of (seed, item key, absolute step) alone.

The device draws it (csrc/noise_keyed.hip through ``mbxn_fill_normal``: ``fill_normal_device``); the rest of this module is the
numpy mirror of the integer part of include/mbexwn_noise.h's definition, bit for bit, and a float64 evaluation of the float
part for the tests.  Value ``s`` of an item (``s >= 0``) belongs to quad ``q = s >> 2``, lane ``j = s & 3``:

1. ``(x0, x1, x2, x3) = philox4x32_10((q & 0xFFFFFFFF, q >> 32, 0, 0), (k0, k1))`` with ``k = seed ^ (item_key *
   0x9E3779B97F4A7C15 mod 2^64)``, ``k0`` its low and ``k1`` its high 32 bits;
2. ``u(x) = ((x >> 9) + 0.5) * 2^-23``: at most 24 significant bits, exact in float32, in [2^-24, 1 - 2^-24];
3. ``r = sqrt(-2 log u(x0))``, ``t = 2 pi u(x1)``: lanes 0 and 1 are ``r cos t`` and ``r sin t``; ``(x2, x3)`` give lanes 2 and
   3 the same way.  The device evaluates this in float32 (``2 pi`` is the float32 nearest to it).

Nothing here is on a hot path and nothing here stands in for the device: the forward's noise always comes from the kernel.
"""
import os
import zlib

import numpy as np

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
KEY_MIX = 0x9E3779B97F4A7C15
MASK32, MASK64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
TWO_PI_F32 = np.float32(6.283185307179586)


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11), vectorised over quads: ``counter`` (..., 4) and ``key`` (..., 2) hold 32-bit
    words (broadcast against each other); returns uint32 (..., 4)."""
    counter = np.asarray(counter, dtype=np.uint64) & np.uint64(MASK32)
    key = np.asarray(key, dtype=np.uint64) & np.uint64(MASK32)
    shape = np.broadcast_shapes(counter.shape[:-1], key.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(counter[..., ii], shape) for ii in range(4))
    k0, k1 = (np.broadcast_to(key[..., ii], shape) for ii in range(2))
    mask, m0, m1 = np.uint64(MASK32), np.uint64(PHILOX_M0), np.uint64(PHILOX_M1)
    shift = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2                        # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> shift) ^ c1 ^ k0, p1 & mask, (p0 >> shift) ^ c3 ^ k1, p0 & mask
        k0, k1 = (k0 + np.uint64(PHILOX_W0)) & mask, (k1 + np.uint64(PHILOX_W1)) & mask
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def item_key(name):
    """The key of a file: zlib.crc32 of its basename's UTF-8 bytes (an int is its own key)."""
    if isinstance(name, (int, np.integer)):
        return int(name) & MASK64
    return zlib.crc32(os.path.basename(os.fspath(name)).encode("utf-8")) & MASK32


def philox_key(seed, key):
    """(k0, k1) of an item: the low and high words of ``seed ^ (item_key * KEY_MIX mod 2^64)``."""
    kk = (int(seed) & MASK64) ^ ((int(key) & MASK64) * KEY_MIX & MASK64)
    return kk & MASK32, kk >> 32


def words(seed, key, first, count):
    """The uint32 words behind the values [first, first + count) of an item: (count,) word of value s is x[s & 3] of quad
    s >> 2."""
    first, count = int(first), int(count)
    if first < 0 or count < 0:
        raise ValueError("first and count must not be negative")
    if count == 0:
        return np.zeros(0, dtype=np.uint32)
    q0, q1 = first >> 2, (first + count + 3) >> 2
    quads = np.arange(q0, q1, dtype=np.uint64)
    counter = np.stack([quads & np.uint64(MASK32), quads >> np.uint64(32), np.zeros_like(quads), np.zeros_like(quads)], axis=-1)
    xx = philox4x32_10(counter, np.asarray(philox_key(seed, key), dtype=np.uint64))
    return xx.reshape(-1)[first - 4 * q0: first - 4 * q0 + count]


def unit_open(x):
    """u(x) of the definition as float64 (exact; it is exact in float32 too)."""
    return ((np.asarray(x, dtype=np.uint32) >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def uniforms(seed, key, first, count):
    """u of the words of the values [first, first + count): float64 (count,), strictly inside (0, 1).  The value at an even
    lane is the radius' uniform of its pair, the one at the odd lane behind it the angle's."""
    return unit_open(words(seed, key, first, count))


def _pairs(seed, key, first, count):
    first, count = int(first), int(count)
    lo = first & ~1                                      # whole pairs around the window
    hi = (first + count + 1) & ~1
    uu = uniforms(seed, key, lo, hi - lo)
    return uu[0::2], uu[1::2], first - lo


def normals_reference(seed, key, first, count):
    """The values [first, first + count) of an item in float64: the definition's formulas on the mirror's uniforms, with the
    angle scaled by the float32 ``2 pi`` the device multiplies with (its rounding is part of the definition, not an
    error)."""
    ua, ub, skip = _pairs(seed, key, first, count)
    rr, tt = np.sqrt(-2.0 * np.log(ua)), float(TWO_PI_F32) * ub
    return np.stack([rr * np.cos(tt), rr * np.sin(tt)], axis=-1).reshape(-1)[skip: skip + int(count)]


def normals_float32_port(seed, key, first, count):
    """The same three formulas in numpy float32: what a float32 evaluation with numpy's logf / sqrtf / sinf / cosf gives.
    Its distance from :func:`normals_reference` is the yardstick of the device's tolerance (tests/test_gpu_noise.py)."""
    ua, ub, skip = _pairs(seed, key, first, count)
    ua, ub = ua.astype(np.float32), ub.astype(np.float32)
    rr = np.sqrt(np.float32(-2.0) * np.log(ua))
    tt = TWO_PI_F32 * ub
    out = np.stack([rr * np.cos(tt), rr * np.sin(tt)], axis=-1).reshape(-1)[skip: skip + int(count)]
    assert out.dtype == np.float32
    return out


def fill_normal_device(seeds, item_keys, counts, first_step=None, out=None, device=None):
    """Keyed N(0,1) noise on the GPU (include/mbexwn_noise.h, ``mbxn_fill_normal``): row b holds the values ``first_step[b] ..
    first_step[b] + counts[b]`` of the item ``(seeds[b], item_keys[b])``, zeros behind them.  ``seeds`` / ``item_keys``:
    integers (taken mod 2^64), one per item, or one seed for all; ``counts`` / ``first_step``: host integers.  Returns a
    float32 tensor (B, max(counts)) on ``device`` (default: that of ``out``, else the current one); ``out``: a zeroed float32
    tensor (B, stride >= max(counts)) there to fill instead.  Enqueued on the current stream of that device."""
    import torch
    from .abi import _check, load_library
    counts = [int(nn) for nn in counts]
    B = len(counts)
    keys = [int(kk) for kk in item_keys]
    seeds = [int(seeds)] * B if np.ndim(seeds) == 0 else [int(ss) for ss in seeds]
    first = [0] * B if first_step is None else [int(ff) for ff in first_step]
    if not (len(keys) == len(seeds) == len(first) == B):
        raise ValueError(f"keyed_noise: one seed, item key and first step per count ({B})")
    if any(nn < 0 for nn in counts) or any(ff < 0 for ff in first):
        raise ValueError("keyed_noise: counts and first_step must not be negative")
    top = max(counts, default=0)
    if device is None:
        device = out.device if torch.is_tensor(out) else torch.device("cuda", torch.cuda.current_device())
    if out is None:
        out = torch.zeros((B, top), dtype=torch.float32, device=device)
    elif (not torch.is_tensor(out) or out.dim() != 2 or out.dtype != torch.float32 or out.device != device or not out.is_cuda
          or not out.is_contiguous() or int(out.shape[0]) != B or int(out.shape[1]) < top):
        raise ValueError(f"keyed_noise: out must be a contiguous float32 tensor ({B}, >= {top}) on the engine's device")
    if B == 0 or top == 0:
        return out
    table = np.empty((B, 4), dtype=np.uint64)            # one upload: seed, item key, first step, count
    table[:, 0] = [ss & MASK64 for ss in seeds]
    table[:, 1] = [kk & MASK64 for kk in keys]
    table[:, 2] = first
    table[:, 3] = counts
    dev = torch.as_tensor(table.view(np.int64)).to(device)
    keys_dev = dev[:, :2].contiguous()
    first_dev = dev[:, 2].contiguous()
    counts_dev = dev[:, 3].to(torch.int32)
    # no handle, hence no device of its own: the launch goes to the CURRENT device, which must be the buffers'
    with torch.cuda.device(device):
        _check(load_library().mbxn_fill_normal(out.data_ptr(), int(out.shape[1]), B, keys_dev.data_ptr(), first_dev.data_ptr(),
                                               counts_dev.data_ptr(), top, torch.cuda.current_stream(device).cuda_stream))
    return out
