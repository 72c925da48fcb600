"""Align a recording's timing to a guide: dynamic time warping of two log-mel sequences, the one
place in the package that PRODUCES a time map.  The result goes to the warped analysis as ``timemap.Centres``.

The functions ending in ``_host`` are THE DEFINITION, in numpy; ``csrc/mel_align.hip`` (``mbxg_local_cost`` and
``mbxg_align_path``, include/mbexwn_align.h) gives their bits -- the arrangement f0decode.py has with ``csrc/f0_decode.hip``.
Every float32 operation is one separately rounded operation (no fused multiply-add, no logarithm), every sum has the one
order stated here, and everything behind the quantised cost is integer.

Inputs: the guide's log-mel ``A`` (Ta, M) and the source's ``B`` (Tb, M), float32, both on the regular frame grid.

THE SUM of M float32 values x[0..M), used for the mean and for the cost alike: four interleaved partial sums ``s_r``, r = 0
.. 3, each starting at +0 and taking ``x[m]`` for m = r, r + 4, r + 8, ... in ascending m; the result is ``(s_0 + s_1) +
(s_2 + s_3)``.

Features (:func:`features_host`): ``F[t, m] = X[t, m] - mean_t`` with ``mean_t = SUM(X[t, :]) / float32(M)``: level is
removed, two takes at different gain align the same way.

Local cost (:func:`local_cost_host`): ``d(i, j) = SUM_m |FA[i, m] - FB[j, m]|``, then ``q(i, j) = int(rint((d if d < 2048
else 2048) * 8))``, so 0 <= q <= 16384 (a NaN cost is 16384).  Band: ``c(i) = (i * (Tb - 1) + (Ta - 1) // 2) // max(Ta - 1,
1)``; cell (i, j) is in the band iff ``|j - c(i)| <= W``.  The table is (Ta, 2 W + 1) uint16, column o of row i being j = c(i)
- W + o; a column whose j lies outside [0, Tb) holds :data:`NO_CELL`.

Recursion (:func:`path_host`), int32: steps (1, 1), (1, 2), (2, 1) in (guide, source) frames.  ``D[0, 0] = q[0, 0]``;
``D[i, j] = q[i, j] + min(D[i - 1, j - 1], D[i - 1, j - 2], D[i - 2, j - 1])`` over the predecessors that exist (in the band,
in the item, reachable), the first of that order winning a tie; a cell without one is unreachable.  At most 65 535 frames
per side (:data:`MAX_FRAMES`, checked in :func:`check_sizes`): a path has at most Ta nodes, and 65 535 * 16 384 < 2^31.
Backtracking from (Ta - 1, Tb - 1) to (0, 0) gives the nodes ``(i_k, j_k)`` in ascending order, their count and the total
cost ``D[Ta - 1, Tb - 1]``; an unreachable end gives count 0 and cost -1 (the length ratio is outside about [1/2, 2], or the
band is too narrow).

Centres (:func:`centres_from_path`), integers only: ``c[i_k] = j_k * hop``; a guide frame skipped by a (2, 1) step gets
``((j_k + j_{k+1}) * hop) // 2``; all clipped to [0, n_source].  Exactly Ta of them: the aligned sound has the guide's length.
"""
import numpy as np

f32 = np.float32

MAX_FRAMES = 65535           # per side: nodes * 16384 < 2^31 (the int32 sums), and i * (Tb - 1) + (Ta - 1) // 2 < 2^32
MAX_BAND = 511               # mbxg_align_path gives every band cell of a row its own thread: 2 W + 1 <= 1024
MAX_MELS = 240               # mbxg_local_cost keeps 64 source rows of M + 1 floats and the guide row in 64 KiB of LDS
NO_CELL = 65535              # a band column outside the item
Q_MAX = 16384
STEPS = ((1, 1), (1, 2), (2, 1))
_UNREACHED = np.int32(2 ** 31 - 1)


class AlignError(ValueError):
    """The two recordings cannot be aligned: no path of the allowed steps joins their ends inside the band."""


def check_sizes(n_a, n_b, band):
    """(Ta, Tb, W) as ints, or ValueError: an empty item, more than :data:`MAX_FRAMES` frames on a side (the bound that keeps
    ``nodes * 16384`` below 2^31), a band below 1 or above :data:`MAX_BAND`."""
    n_a, n_b = int(n_a), int(n_b)
    if isinstance(band, bool) or band != int(band):
        raise ValueError(f"align: the band must be a whole number of frames, got {band!r}")
    band = int(band)
    if n_a < 1 or n_b < 1:
        raise ValueError(f"align: an item without frames cannot be aligned (guide {n_a}, source {n_b} frames)")
    if n_a > MAX_FRAMES or n_b > MAX_FRAMES:
        raise ValueError(f"align: at most {MAX_FRAMES} frames per item (guide {n_a}, source {n_b}): the int32 path cost "
                         "could overflow; split the recording")
    if not 1 <= band <= MAX_BAND:
        raise ValueError(f"align: the band must be 1 .. {MAX_BAND} frames, got {band}")
    return n_a, n_b, band


def band_frames(align_band_s, rate, hop):
    """``--align-band SECONDS`` in frames: at least 1; ValueError unless finite and positive and at most :data:`MAX_BAND`."""
    try:
        value = float(align_band_s)
    except (TypeError, ValueError):
        value = float("nan")
    if not (np.isfinite(value) and value > 0):
        raise ValueError(f"align: the band must be a finite positive number of seconds, got {align_band_s!r}")
    frames = max(1, int(round(value * float(rate) / int(hop))))
    if frames > MAX_BAND:
        raise ValueError(f"align: a band of {value} s is {frames} frames, more than the limit of {MAX_BAND} frames "
                         f"({MAX_BAND * int(hop) / float(rate):.2f} s)")
    return frames


def band_centres(n_a, n_b):
    """``c(i)`` for i = 0 .. Ta - 1, int64."""
    ii = np.arange(int(n_a), dtype=np.int64)
    return (ii * (int(n_b) - 1) + (int(n_a) - 1) // 2) // max(int(n_a) - 1, 1)


def sum4_host(x):
    """THE SUM (the module's docstring) over the last axis of a float32 array."""
    x = np.asarray(x, dtype=f32)
    part = np.zeros(x.shape[:-1] + (4,), dtype=f32)
    with np.errstate(all="ignore"):
        for m in range(x.shape[-1]):
            part[..., m & 3] = part[..., m & 3] + x[..., m]
        return (part[..., 0] + part[..., 1]) + (part[..., 2] + part[..., 3])


def features_host(mel):
    """(T, M) float32 log-mel -> (T, M) float32 features: every row minus its mean over the channels."""
    mel = np.ascontiguousarray(mel, dtype=f32)
    if mel.ndim != 2 or mel.shape[1] < 1:
        raise ValueError(f"align: a log-mel of shape (frames, channels) is expected, got {mel.shape}")
    with np.errstate(all="ignore"):
        mean = sum4_host(mel) / f32(mel.shape[1])
        return (mel - mean[:, None]).astype(f32)


def local_cost_host(mel_a, mel_b, band, rows=256):
    """The quantised band cost table (Ta, 2 W + 1) uint16 of the guide ``mel_a`` (Ta, M) and the source ``mel_b`` (Tb, M);
    ``rows`` guide rows are worked on at a time (memory only)."""
    fa, fb = features_host(mel_a), features_host(mel_b)
    if fa.shape[1] != fb.shape[1]:
        raise ValueError(f"align: guide and source have {fa.shape[1]} and {fb.shape[1]} mel channels")
    n_a, n_b, band = check_sizes(fa.shape[0], fb.shape[0], band)
    cc = band_centres(n_a, n_b)
    out = np.full((n_a, 2 * band + 1), NO_CELL, dtype=np.uint16)
    offs = np.arange(-band, band + 1, dtype=np.int64)
    for start in range(0, n_a, max(1, int(rows))):
        jj = cc[start:start + rows, None] + offs[None, :]
        ok = (jj >= 0) & (jj < n_b)
        with np.errstate(all="ignore"):
            dd = sum4_host(np.abs(fa[start:start + rows, None, :] - fb[np.clip(jj, 0, n_b - 1)]))
            dd = np.where(dd < f32(2048), dd, f32(2048)).astype(f32)
            qq = np.rint(dd * f32(8)).astype(np.int32)
        out[start:start + rows][ok] = qq[ok].astype(np.uint16)
    return out


def band_table(q_full, band):
    """A full (Ta, Tb) table of quantised costs in the band layout of :func:`local_cost_host` (the tests' hand-made cases)."""
    q_full = np.asarray(q_full)
    n_a, n_b, band = check_sizes(q_full.shape[0], q_full.shape[1], band)
    if q_full.min() < 0 or q_full.max() > Q_MAX:
        raise ValueError(f"align: quantised costs lie in 0 .. {Q_MAX}")
    cc = band_centres(n_a, n_b)
    jj = cc[:, None] + np.arange(-band, band + 1, dtype=np.int64)[None, :]
    ok = (jj >= 0) & (jj < n_b)
    out = np.full(jj.shape, NO_CELL, dtype=np.uint16)
    out[ok] = q_full[np.nonzero(ok)[0], jj[ok]].astype(np.uint16)
    return out


def path_host(q_band, n_b, band):
    """The recursion and the backtrack (the module's docstring) on a band table (Ta, 2 W + 1) for a source of ``n_b`` frames:
    ``(nodes, cost)`` -- nodes (count, 2) int32 rows (i_k, j_k), ascending; count 0 and cost -1 for an unreachable end."""
    q_band = np.asarray(q_band)
    n_a, n_b, band = check_sizes(q_band.shape[0], n_b, band)
    nb = 2 * band + 1
    if q_band.shape != (n_a, nb):
        raise ValueError(f"align: a band table of shape ({n_a}, {nb}) is expected, got {q_band.shape}")
    qq = q_band.astype(np.int64)
    cc = band_centres(n_a, n_b)
    big = np.int64(_UNREACHED)
    dist = np.full((n_a, nb), big, dtype=np.int64)
    back = np.full((n_a, nb), 3, dtype=np.uint8)
    oo = np.arange(nb, dtype=np.int64)

    def shifted(row, shift):
        """row[o + shift] for every o, ``big`` outside the band."""
        idx = oo + shift
        ok = (idx >= 0) & (idx < nb)
        return np.where(ok, row[np.clip(idx, 0, nb - 1)], big)

    if qq[0, band] != NO_CELL:                               # j = 0 is column W of row 0 (c(0) = 0)
        dist[0, band] = qq[0, band]
    for ii in range(1, n_a):
        d1 = int(cc[ii] - cc[ii - 1])
        cands = [shifted(dist[ii - 1], d1 - 1), shifted(dist[ii - 1], d1 - 2),
                 shifted(dist[ii - 2], int(cc[ii] - cc[ii - 2]) - 1) if ii >= 2 else np.full(nb, big)]
        best, arg = cands[0].copy(), np.zeros(nb, dtype=np.uint8)
        for kk in (1, 2):
            take = cands[kk] < best                          # strict: the first of the order wins a tie
            best = np.where(take, cands[kk], best)
            arg = np.where(take, np.uint8(kk), arg)
        ok = (best != big) & (qq[ii] != NO_CELL)
        dist[ii] = np.where(ok, best + qq[ii], big)
        back[ii] = np.where(ok, arg, np.uint8(3))
    end = n_b - 1 - int(cc[n_a - 1]) + band
    if not 0 <= end < nb or dist[n_a - 1, end] == big:
        return np.zeros((0, 2), dtype=np.int32), -1
    nodes, ii, jj = [], n_a - 1, n_b - 1
    while True:
        nodes.append((ii, jj))
        if ii == 0 and jj == 0:
            break
        di, dj = STEPS[int(back[ii, jj - int(cc[ii]) + band])]
        ii, jj = ii - di, jj - dj
    return np.asarray(nodes[::-1], dtype=np.int32).reshape(-1, 2), int(dist[n_a - 1, end])


def align_host(mel_a, mel_b, band):
    """The whole definition on two arrays: :func:`local_cost_host`, then :func:`path_host`.  ``(nodes, cost)``."""
    return path_host(local_cost_host(mel_a, mel_b, band), np.shape(mel_b)[0], band)


def centres_from_path(nodes, hop, n_source):
    """The int64 centre samples ``c[0..Ta)`` in the source of the guide's frames (the module's docstring), from the nodes of
    a path that runs from (0, 0) to (Ta - 1, .)."""
    nodes = np.asarray(nodes, dtype=np.int64).reshape(-1, 2)
    if nodes.shape[0] < 1 or tuple(nodes[0]) != (0, 0):
        raise ValueError("align: a path starts at (0, 0) and has at least one node")
    step_i, step_j = np.diff(nodes[:, 0]), np.diff(nodes[:, 1])
    if not all((int(a), int(b)) in STEPS for a, b in zip(step_i, step_j)):
        raise ValueError("align: a path moves by (1, 1), (1, 2) or (2, 1)")
    hop, n_source = int(hop), int(n_source)
    out = np.zeros(int(nodes[-1, 0]) + 1, dtype=np.int64)
    out[nodes[:, 0]] = nodes[:, 1] * hop
    skip = np.nonzero(step_i == 2)[0]
    out[nodes[skip, 0] + 1] = ((nodes[skip, 1] + nodes[skip + 1, 1]) * hop) // 2
    return np.clip(out, 0, n_source)


def path_stats(nodes, cost, n_a, n_b, hop, rate):
    """What ``-v`` prints of a path: the mean cost per node (in summed |log-mel difference| over the channels, the quantum
    undone) and the largest offset of a node from the band's centre line, in ms."""
    nodes = np.asarray(nodes, dtype=np.int64).reshape(-1, 2)
    off = np.abs(nodes[:, 1] - band_centres(n_a, n_b)[nodes[:, 0]]).max() if nodes.shape[0] else 0
    return {"nodes": int(nodes.shape[0]), "cost": int(cost), "mean_cost": float(cost) / 8.0 / max(1, nodes.shape[0]),
            "max_offset_ms": 1000.0 * float(off) * int(hop) / float(rate)}


def cannot_align(n_a, n_b, band):
    return AlignError(f"cannot be aligned: no path with local slope in [1/2, 2] joins the ends of the guide ({n_a} frames) "
                      f"and the source ({n_b} frames) within a band of {band} frames")


# ------------------------------------------------------------------------------------------------------------------------
# the device
# ------------------------------------------------------------------------------------------------------------------------
def _check_batch(mel_a, n_a, mel_b, n_b, band):
    import torch
    for name, tt in (("mel_a", mel_a), ("mel_b", mel_b)):
        if not torch.is_tensor(tt) or tt.dim() != 3 or tt.dtype != torch.float32 or not tt.is_cuda:
            raise ValueError(f"{name} must be a float32 cuda tensor of shape (batch, max_frames, mel_channels)")
    dev, B = mel_a.device, int(mel_a.shape[0])
    if mel_b.device != dev or int(mel_b.shape[0]) != B or int(mel_b.shape[2]) != int(mel_a.shape[2]):
        raise ValueError("mel_a and mel_b must share device, batch and mel channels")
    for name, tt in (("n_a", n_a), ("n_b", n_b)):
        if not torch.is_tensor(tt) or tt.dtype != torch.int32 or tuple(tt.shape) != (B,) or tt.device != dev:
            raise ValueError(f"{name} must be an int32 tensor of shape (batch,) on the device of mel_a")
    if not 1 <= int(mel_a.shape[2]) <= MAX_MELS:
        raise ValueError(f"align: 1 .. {MAX_MELS} mel channels, got {int(mel_a.shape[2])}")
    check_sizes(max(1, int(mel_a.shape[1])), max(1, int(mel_b.shape[1])), band)
    return dev, B


def workspace_bytes(batch, max_frames_a, band):
    """``mbxg_align_workspace_size``: the bytes :func:`path_device` needs (back pointers and the reversed nodes)."""
    from .abi import load_library
    return int(load_library().mbxg_align_workspace_size(int(batch), int(max_frames_a), int(band)))


def local_cost_device(mel_a, n_a, mel_b, n_b, band):
    """:func:`local_cost_host` on the GPU for a ragged batch (``mbxg_local_cost``): ``mel_a`` (batch, max_a, M) and ``mel_b``
    (batch, max_b, M) float32 cuda, ``n_a`` / ``n_b`` int32 cuda (batch,).  Returns a uint16 cuda tensor (batch, max_a, 2 W +
    1); rows from ``n_a[b]`` on are not written (they stay zero).  No engine, current stream."""
    import torch
    from .abi import _check, load_library
    dev, B = _check_batch(mel_a, n_a, mel_b, n_b, band)
    mel_a, mel_b, n_a, n_b = mel_a.contiguous(), mel_b.contiguous(), n_a.contiguous(), n_b.contiguous()
    cost = torch.zeros((B, int(mel_a.shape[1]), 2 * int(band) + 1), dtype=torch.uint16, device=dev)
    if B == 0 or mel_a.shape[1] == 0 or mel_b.shape[1] == 0:
        return cost
    with torch.cuda.device(dev):
        _check(load_library().mbxg_local_cost(mel_a.data_ptr(), mel_b.data_ptr(), n_a.data_ptr(), n_b.data_ptr(), B,
                                              int(mel_a.shape[1]), int(mel_b.shape[1]), int(mel_a.shape[2]), int(band),
                                              cost.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    return cost


def path_device(cost, n_a, n_b, band):
    """:func:`path_host` on the GPU for a ragged batch (``mbxg_align_path``) on the table of :func:`local_cost_device`.
    Returns ``(nodes_i, nodes_j, count, total)``: int32 cuda (batch, max_a) twice -- entries from ``count[b]`` on are not
    written (they stay zero) -- and int32 cuda (batch,) twice; an item that cannot be aligned, or has no frames, has
    count 0 and total -1."""
    import torch
    from .abi import _check, load_library
    dev, B, frames = cost.device, int(cost.shape[0]), int(cost.shape[1])
    nodes_i = torch.zeros((B, frames), dtype=torch.int32, device=dev)
    nodes_j = torch.zeros((B, frames), dtype=torch.int32, device=dev)
    count = torch.zeros((B,), dtype=torch.int32, device=dev)
    total = torch.full((B,), -1, dtype=torch.int32, device=dev)
    if B == 0 or frames == 0:
        return nodes_i, nodes_j, count, total
    nbytes = workspace_bytes(B, frames, band)
    work = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _check(load_library().mbxg_align_path(cost.data_ptr(), n_a.data_ptr(), n_b.data_ptr(), B, frames, int(band),
                                              work.data_ptr(), nbytes, nodes_i.data_ptr(), nodes_j.data_ptr(), count.data_ptr(),
                                              total.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    return nodes_i, nodes_j, count, total


def align_device(mel_a, n_a, mel_b, n_b, band):
    """:func:`align_host` on the GPU for a ragged batch: :func:`local_cost_device`, then :func:`path_device` -- two
    launches, the node tensors stay on the device."""
    return path_device(local_cost_device(mel_a, n_a, mel_b, n_b, band), n_a, n_b, band)
