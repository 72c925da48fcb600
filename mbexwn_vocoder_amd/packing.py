"""The weight images of the specialised kernels and the tensor table of ``mbx_create``: numpy on the host, no binding, no GPU.

Every ``pack_*`` function lays one weight tensor out in the operand order of one kernel (the kernel copies the image of a tile
verbatim into LDS); ``fold_skip_weights`` / ``fold_start_weights`` form the products of the folded graph in float64;
``tensor_table`` is name -> float32 array of everything ``mbx_create`` takes.  tests/test_packing.py unpacks every image
against its definition.
"""
import numpy as np

from . import tables as tb
from .config import ModelDims
from .weights import block_prefix, fold_weight_norm_f64, fold_weights, merge_channel_groups

_WINOGRAD43_G = np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6],
                          [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]], dtype=np.float64)


def _padded(mat, rows, cols, dtype=np.float32):
    """mat (r, c) in the top left corner of a zero (rows, cols) matrix"""
    out = np.zeros((rows, cols), dtype=dtype)
    out[:mat.shape[0], :mat.shape[1]] = mat
    return out


def _gate_image(u, C, dtype=np.float32):
    """The products u (P, K, 2C) of a gate layer -- K input channels, the tanh columns in front of the sigmoid ones -- as the
    image (ceil(C/32) column tiles, ceil(K/8) channel slices, 512 P) of the 16x16x4 MFMA gate kernels: [product j]
    [channel parity e][lane = 16*kq + n][tanh step 0, tanh step 1, sigmoid step 0, sigmoid step 1] with input channel
    8*slice + 2*kq + step and output column (0 | C) + 32*tile + 2*n + e; out-of-range entries are zero."""
    P, K = u.shape[:2]
    nt, nk = (C + 31) // 32, (K + 7) // 8
    wp = np.zeros((P, nk * 8, 2, nt * 32))
    wp[:, :K, 0, :C] = u[:, :, :C]
    wp[:, :K, 1, :C] = u[:, :, C:]
    wp = wp.reshape(P, nk, 4, 2, 2, nt, 16, 2)                    # j, slice, kq, step, tanh|sigmoid, tile, n, e
    return np.ascontiguousarray(wp.transpose(5, 1, 0, 7, 2, 6, 4, 3).reshape(nt, nk, 512 * P), dtype=dtype)


def _gate_taps(w):
    w = np.asarray(w, dtype=np.float64)
    C = w.shape[1]
    assert w.shape == (3, C, 2 * C)
    return w, C


def pack_winograd4w_weights(w):
    """Winograd F(4,3) combinations U = G W of the three taps (3, C, 2C) of a dilated WaveNet convolution, packed for
    wn_gate_winograd4w_kernel (csrc/wn_winograd4w.hip, v_mfma_f32_16x16x4_f32); formed in float64, stored float32.

    Layout (ceil(C/32) column tiles, ceil(C/8) channel slices, 3072): the 12 KB image of one (tile, slice) is copied
    verbatim into LDS, ordered as _gate_image says with the six products."""
    w, C = _gate_taps(w)
    return _gate_image(np.einsum("ij,jcn->icn", _WINOGRAD43_G, w), C)


def pack_winograd2w_weights(w):
    """Winograd F(2,3) combinations W0, (W0+W1+W2)/2, (W0-W1+W2)/2, W2 of the three taps (3, C, 2C) of a dilated WaveNet
    convolution, packed for wn_gate_winograd2w_kernel (csrc/wn_winograd2w.hip, v_mfma_f32_16x16x4_f32); formed in
    float64, stored float32.

    Layout (ceil(C/32) column tiles, ceil(C/8) channel slices, 2048): the 8 KB image of one (tile, slice) is copied
    verbatim into LDS, ordered as _gate_image says with the four products."""
    w, C = _gate_taps(w)
    return _gate_image(np.stack((w[0], (w[0] + w[1] + w[2]) / 2, (w[0] - w[1] + w[2]) / 2, w[2])), C)


def _pointwise(w, widest=None):
    """(the (K, cout) matrix, K, cout) of the weights (1, K, cout) of a 1x1 convolution, float32"""
    w = np.asarray(w, dtype=np.float32)
    assert w.ndim == 3 and w.shape[0] == 1 and (widest is None or w.shape[2] <= widest)
    return w[0], w.shape[1], w.shape[2]


def pack_resskip_weights(w):
    """Weights (1, C, cout) of a WaveNet res/skip 1x1 convolution packed for wn_resskip_kernel (csrc/wn_resskip.hip).

    Layout (ceil(cout/128) column tiles, ceil(C/16) channel slices, 2048): the 8 KB image of one (tile, slice), ordered
    [channel half cc][column sub-tile jn][lane = 32*lk + n][k step st] with input channel 16*slice + 8*cc + 4*lk + st
    and output column 128*tile + 32*jn + n; out-of-range entries are zero.
    """
    mat, C, cout = _pointwise(w)
    nct, nk = (cout + 127) // 128, (C + 15) // 16
    wp = _padded(mat, nk * 16, nct * 128).reshape(nk, 2, 2, 4, nct, 4, 32)       # slice, cc, lk, st, tile, jn, n
    return np.ascontiguousarray(wp.transpose(4, 0, 1, 5, 2, 6, 3).reshape(nct, nk, 2048))


def pack_resskip_wide_weights(w):
    """Weights (1, K, cout) of a WaveNet res/skip 1x1 convolution packed for wn_resskip_wide_kernel
    (csrc/wn_resskip_wide.hip, v_mfma_f32_16x16x4_f32).

    Layout (ceil(K/8) channel slices, NP = ceil(cout/32) column tile pairs, 256): [pair p][lane = 16*kq + n][even tile
    step 0, even tile step 1, odd tile step 0, odd tile step 1] with input channel 8*slice + 2*kq + step and output
    column 32*p + 2*n + (0 even | 1 odd); out-of-range entries are zero.
    """
    mat, K, cout = _pointwise(w)
    nk, npair = (K + 7) // 8, (cout + 31) // 32
    wp = _padded(mat, nk * 8, npair * 32).reshape(nk, 4, 2, npair, 16, 2)        # slice, kq, step, pair, n, parity
    return np.ascontiguousarray(wp.transpose(0, 3, 1, 4, 5, 2).reshape(nk, npair, 256))


def pack_resskip_wave_weights(w):
    """Weights (1, K, cout <= 384) of a WaveNet res/skip 1x1 convolution packed for wn_resskip_wave_kernel
    (csrc/wn_resskip_wave.hip, v_mfma_f32_16x16x4_f32, 16-channel slices).

    Layout (ceil(K/16) channel slices, 12 column tile pairs, 512): [pair p][even tile | odd tile][lane = 16*kq + n][step]
    with input channel 16*slice + 4*kq + step and output column 32*p + 2*n + (0 even | 1 odd); out-of-range entries are
    zero (the image always has 12 pairs, so that every column split of the kernel finds its pairs).
    """
    mat, K, _ = _pointwise(w, widest=384)
    nk = (K + 15) // 16
    wp = _padded(mat, nk * 16, 12 * 32).reshape(nk, 4, 4, 12, 16, 2)             # slice, kq, step, pair, n, parity
    return np.ascontiguousarray(wp.transpose(0, 3, 5, 1, 4, 2).reshape(nk, 12, 512))


def _split_f16(wp, what):
    """(hi, lo') of zero-padded float32 weights, stacked in front: hi = fp16(w), lo' = fp16((w - hi) * 2^11)"""
    if not np.all(np.abs(wp) < 65000.0):
        raise ValueError(f"{what} weights outside fp16's range: split half precision is not available for this model")
    hi = wp.astype(np.float16)
    lo = ((wp - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    return np.stack((hi, lo))


def pack_resskip_f16_weights(w):
    """Weights (1, K, cout <= 384) of a folded WaveNet res/skip layer for wn_resskip_f16_kernel (csrc/wn_resskip_f16.hip,
    v_mfma_f32_16x16x32_f16; opt-in split half precision): every float32 weight is split into hi = fp16(w) and
    lo' = fp16((w - hi) * 2^11).

    Layout (ceil(K/32) steps, 12 column tile pairs, 1024 float32 words = 4 images x 64 lanes x 8 halves): images [even tile
    hi | even tile lo' | odd tile hi | odd tile lo'], lane = 16 kq + n holds the input channels 32 step + 4 kq .. + 3 and
    32 step + 16 + 4 kq .. + 3 of output column 32 p + 2 n + (0 even | 1 odd); out-of-range entries are zero.  Returned as
    float32 words (two halves each) because the tensor table of the C ABI is float32; the bits are what counts.
    """
    mat, K, _ = _pointwise(w, widest=384)
    nk = (K + 31) // 32
    both = _split_f16(_padded(mat, nk * 32, 384), "res/skip")      # (part, channel, column)
    both = both.reshape(2, nk, 2, 4, 4, 12, 16, 2)                 # part, step, half (0 | +16), kq, v, pair, n, parity
    img = both.transpose(1, 5, 7, 0, 3, 6, 2, 4)                   # step, pair, parity, part, kq, n, half, v
    img = np.ascontiguousarray(img).reshape(nk, 12, 4, 64, 8)      # image = 2 parity + part ; lane = 16 kq + n ; 8 halves
    return img.view(np.float32).reshape(nk, 12, 1024)


def pack_gate_f16_weights(w):
    """The three taps (3, C, 2C) of a dilated WaveNet convolution for wn_gate_f16_kernel (csrc/wn_gate_f16.hip,
    v_mfma_f32_16x16x32_f16; opt-in split half precision): hi = fp16(w), lo' = fp16((w - hi) * 2^11).

    Layout (ceil(C/32) column tiles, ceil(C/32) steps, 6144 float32 words): [tap][tile c = 2 e + (0 tanh | 1 sigmoid)]
    [hi | lo'][lane = 16 kq + n][8 halves], input channels 32 step + 8 kq .. + 7, output column (0 | C) + 32 tile block + 2 n
    + e; out-of-range entries are zero.  float32 words hold two halves each."""
    w = np.asarray(w, dtype=np.float32)
    C = w.shape[1]
    assert w.shape == (3, C, 2 * C)
    nt = nk = (C + 31) // 32
    wp = np.zeros((3, nk * 32, 2, nt * 32), dtype=np.float32)          # tap, channel, tanh|sigmoid, gate channel
    wp[:, :C, 0, :C] = w[:, :, :C]
    wp[:, :C, 1, :C] = w[:, :, C:]
    both = _split_f16(wp, "gate")                                      # part, tap, channel, s, gate channel
    both = both.reshape(2, 3, nk, 4, 8, 2, nt, 16, 2)                  # part, tap, step, kq, v, s, block, n, e
    img = both.transpose(6, 2, 1, 8, 5, 0, 3, 7, 4)                    # block, step, tap, e, s, part, kq, n, v
    return np.ascontiguousarray(img).view(np.float32).reshape(nt, nk, 6144)


def pack_end_weights(w):
    """Weights (1, C, n_out <= 32) of the WaveNet end convolution packed for wn_tail_kernel (csrc/wn_tail.hip):
    (ceil(C/8), 2, 32, 4) = [channel group c][lane half lk][column n][k step st] with input channel 8c + 4lk + st,
    zero padded to 32 columns and to a multiple of 8 channels."""
    mat, C, _ = _pointwise(w, widest=32)
    nc8 = (C + 7) // 8
    return np.ascontiguousarray(_padded(mat, nc8 * 8, 32).reshape(nc8, 2, 4, 32).transpose(0, 1, 3, 2))


# the res/skip images of a folded layer: (suffix of the name, packer, widest C + n_out it takes, only in split precision)
_FOLDED_IMAGES = (("", pack_resskip_weights, None, False), ("_wide", pack_resskip_wide_weights, None, False),
                  ("_wave", pack_resskip_wave_weights, 384, False), ("_f16", pack_resskip_f16_weights, 384, True))


def _folded_images(name, mat, split_f16):
    """{name + suffix: image} of the folded res/skip matrix mat (K, C + n_out) for every kernel that can take it"""
    return {name + suffix: pack(mat[None]) for suffix, pack, widest, split_only in _FOLDED_IMAGES
            if (widest is None or mat.shape[1] <= widest) and (split_f16 or not split_only)}


def fold_skip_weights(folded, n_layers, channels, split_f16=False):
    """Fold the skip path of the WaveNet into its end convolution (both are linear, reference
    MBExWN_NVoc/vocoder/model/custom_AE_layers.py:322-341: output += res_skip[:, C:]; ...; self.end(output)):

        end(sum_l (a_l Ws_l + bs_l)) = sum_l a_l (Ws_l We) + (sum_l bs_l We + be)

    so layer l < L-1 needs the C x (C + n_out) matrix [Wr_l | Ws_l We] instead of C x 2C, the last layer C x n_out
    instead of C x C, and the (rows, C) skip tensor never exists.  Products are formed in float64.  Returns the extra
    tensors {name: array} (packed for wn_resskip_kernel / wn_tail_kernel) or {} if the layout does not allow it.
    """
    we = np.asarray(folded["wn.end.w"], dtype=np.float64)
    if we.shape[0] != 1 or we.shape[2] > 32:
        return {}
    C, n_out = channels, we.shape[2]
    we = we[0]
    const = np.asarray(folded["wn.end.b"], dtype=np.float64).copy()
    out = {}
    biases = []
    for ll in range(n_layers):
        w = np.asarray(folded[f"wn.res_skip_{ll}.w"], dtype=np.float64)
        b = np.asarray(folded[f"wn.res_skip_{ll}.b"], dtype=np.float64)
        if w.shape[0] != 1:
            return {}
        last = ll == n_layers - 1
        ws, bs = (w[0], b) if last else (w[0][:, C:], b[C:])
        proj = ws @ we
        const += bs @ we
        if last:
            out["wn.tail.fold"] = pack_end_weights(proj[None])
        else:
            # (the split-precision image: behind the first layer only)
            out.update(_folded_images(f"wn.res_skip_{ll}.fold", np.concatenate((w[0][:, :C], proj), axis=1),
                                      split_f16 and ll >= 1))
            if ll == 0:
                out["__proj_0"] = proj                 # for fold_start_weights; not a device tensor
            biases.append(np.concatenate((b[:C], np.zeros(n_out))))
    if biases:
        biases[0][C:] = const                 # layer 0 initialises the accumulator
        for ll, bb in enumerate(biases):
            out[f"wn.res_skip_{ll}.fold_b"] = bb
        out["wn.tail.fold_b"] = np.zeros(n_out)
    else:
        out["wn.tail.fold_b"] = const
    return out


def fold_start_weights(folded, dims, fold_skip, split_f16=False):
    """Fold the WaveNet's start convolution (1x1, reference custom_AE_layers.py:177-182,280) into layer 0.

    With x' = [x | 1 | 0] (8 channels; x = pulse channels (+ noise), the constant channel carries the start bias) and
    Ws' = [Ws ; bs ; 0], h0 = x' Ws' and conv0(h0) = sum_tau x'[t + (tau-1) d] (Ws' W0_tau): the dilated convolution of
    layer 0 becomes a K = 24 contraction of the excitation itself (csrc/wn_gate0.hip), and its res/skip layer obtains
    h0 by contracting [a0 | x'] with [Wr ; Ws'] (csrc/wn_resskip.hip, h_init).  Products are formed in float64.
    Returns {name: array}: the (ceil(C/32), 3, 2, 64, 4) image of the tap products -- [tap][channel parity e][lane =
    16*kq + n][tanh step 0, tanh step 1, sigmoid step 0, sigmoid step 1], input channel 2*kq + step, output column
    (0 | C) + 32*tile + 2*n + e -- and the K-extended res/skip image; {} if the layout does not allow it.
    """
    C, L = dims.wn_channels, dims.wn_layers
    ws = np.asarray(folded["wn.start.w"], dtype=np.float64)
    w0 = np.asarray(folded["wn.conv1D_0.w"], dtype=np.float64)
    cin = dims.wn_in_channels
    if ws.shape != (1, cin, C) or w0.shape != (3, C, 2 * C) or cin + 1 > 8 or dims.pulse_channels_eff + 2 > 8:
        return {}
    wsp = _padded(ws[0], 8, C, dtype=np.float64)
    wsp[dims.pulse_channels_eff + 1] = np.asarray(folded["wn.start.b"], dtype=np.float64)   # the constant channel
    prod = np.einsum("kc,tcn->tkn", wsp, w0)                       # (3, 8, 2C): one channel slice of three products
    out = {"wn.conv1D_0.start_fold": _gate_image(prod, C, np.float64).reshape(-1, 3, 512)}
    if L > 1:
        if not fold_skip or "wn.res_skip_0.fold" not in fold_skip:
            return {}
        n_out = dims.wn_out_channels
        wr = np.asarray(folded["wn.res_skip_0.w"], dtype=np.float64)[0]
        ext = np.zeros((C + 16, C + n_out))
        ext[:C, :C] = wr[:, :C]
        ext[:C, C:] = np.asarray(fold_skip["__proj_0"], dtype=np.float64)    # Ws_0 We (C, n_out)
        ext[C:C + 8, :C] = wsp
        out.update(_folded_images("wn.res_skip_0.fold_start", ext, split_f16))
    return out


def tensor_table(config, raw_weights, wavetables, split_f16=False):
    """name -> float32 array of everything mbx_create needs: folded weights + constant tables (+ with ``split_f16`` the
    fp16-split images of the res/skip layers for the opt-in precision mode)."""
    dims = ModelDims(config)
    mb = config["mbexwn_config"]
    mbc = mb["multi_band_config"]
    wn_norm = mb.get("pp_mod_subnet", {}).get("use_weight_norm", None)
    out = dict(merge_channel_groups(fold_weights(raw_weights, wavenet_weight_norm=wn_norm,
                                                 wavenet_equalized_lr=dims.wn_equalized_lr), dims))
    # F0-net: the exact (float64) weight-norm fold of every layer, handed over as pairs of float32 words
    # (mbx_config.f0_accumulate = MBX_F0_ACC_F64: csrc/conv_mel.hip::conv1d_f64_tile reads them as doubles)
    for key in raw_weights:
        if key.startswith("PulsPar_Layer_") and key.endswith(".v") and key[:-2] + ".g" in raw_weights:
            w64 = np.ascontiguousarray(fold_weight_norm_f64(raw_weights[key], raw_weights[key[:-2] + ".g"]))
            out[key[:-2] + ".w64"] = w64.view(np.float32).reshape(w64.shape + (2,))
    _, syn = tb.pqmf_filters(int(mbc["subbands"]), int(mbc["taps"]), float(mbc["cutoff_ratio"]), float(mbc["beta"]),
                             mbc.get("max_band", None))
    out["table.pqmf_syn"] = syn
    if dims.pulse_pqmf:                                            # analysis bank in front of the WaveNet
        pq = dims.pulse_pqmf
        out["table.pulse_ana"] = tb.pqmf_filters(int(pq["subbands"]), int(pq["taps"]), float(pq["cutoff_ratio"]),
                                                 float(pq["beta"]), pq.get("max_band", None))[0]
    # (several WaveNet blocks / in-block upsampling run the library's generic kernels: no operand-order images)
    if not dims.wn_multi and out["wn.end.w"].shape[0] == 1 and out["wn.end.w"].shape[2] <= 32:
        out["wn.end.packed"] = pack_end_weights(out["wn.end.w"])
        fs = fold_skip_weights(out, dims.wn_layers, dims.wn_channels, split_f16=split_f16)
        if dims.wn_kernel_size == 3:
            out.update(fold_start_weights(out, dims, fs, split_f16=split_f16))
        fs.pop("__proj_0", None)
        out.update(fs)
    for ll in range(0 if dims.wn_multi else dims.wn_layers):
        out[f"wn.res_skip_{ll}.packed"] = pack_resskip_weights(out[f"wn.res_skip_{ll}.w"])
    if dims.wn_kernel_size == 3 and not dims.wn_multi:
        for ll in range(dims.wn_layers):
            out[f"wn.conv1D_{ll}.wino4w"] = pack_winograd4w_weights(out[f"wn.conv1D_{ll}.w"])
            out[f"wn.conv1D_{ll}.wino2w"] = pack_winograd2w_weights(out[f"wn.conv1D_{ll}.w"])
            if split_f16 and ll >= 1:
                out[f"wn.conv1D_{ll}.gate_f16"] = pack_gate_f16_weights(out[f"wn.conv1D_{ll}.w"])
    if dims.wn_multi:
        # several blocks: the library's block runner takes the packed res/skip weights and the F(4,3) images per block
        for bb in range(dims.n_wn_blocks):
            pre = block_prefix(bb)
            for ll in range(dims.wn_layers):
                out[f"{pre}res_skip_{ll}.packed"] = pack_resskip_weights(out[f"{pre}res_skip_{ll}.w"])
                if dims.wn_kernel_size == 3 and dims.wn_padding == "SAME":
                    out[f"{pre}conv1D_{ll}.wino4w"] = pack_winograd4w_weights(out[f"{pre}conv1D_{ll}.w"])
    out["table.hann"] = tb.hann_periodic_f32(dims.stft_win)
    out["table.inv_win"] = tb.inverse_stft_window_f32(dims.stft_win, dims.hop_size)
    out["table.wavetables"] = np.ascontiguousarray(wavetables.tables, dtype=np.float32)
    if dims.ps_env_order_scale and not mb.get("psns_use_cepstral_loss_constraint", False) and not dims.no_envelope:
        logs, rows = tb.cepstral_windows(dims.ps_env_order_scale, dims.sample_rate, dims.f0_min, dims.f0_max, dims.n_ceps)
        out["table.ceps_windows"] = rows
        out["table.ceps_log10f0"] = logs
        out["table.f0_smooth"] = tb.f0_smoothing_kernel(dims.hop_size)
    if mb.get("normalize_rms_from_mell", False):
        from .norm_mel import NormMel
        nm = NormMel(config)
        out["table.nm_inv_enorm"] = nm.inv_enorm
        out["table.nm_gwin"] = nm.gwin
        out["table.nm_smooth_win"] = nm.smooth_syn_win
        if nm.use_pinv:
            out["table.nm_pinv"] = nm.pinv
    return {kk: np.ascontiguousarray(vv, dtype=np.float32) for kk, vv in out.items()}
