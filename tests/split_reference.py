"""numpy emulation of the split-half-precision WaveNet path (csrc/wn_gate_f16.hip, csrc/wn_resskip_f16.hip): what the two
kernels are designed to compute, plugged into the float32 port of the graph through OracleModel.wavenet's taps and hook.

Operands: hi = fp16(x), lo' = fp16((x - hi) 2^11).
Res/skip (layers 0 .. L - 2, skip path folded into the end convolution, layer 0 with the folded start rows [a0 | x']):
    new = 2^-11 (2^11 (old + b) + (2^11 hi_a) hi_w + hi_a lo'_w + lo'_a hi_w)
Gate (layers >= 1): a main accumulator (bias + hi_h hi_w) and a cross accumulator (hi_h lo'_w + lo'_h hi_w) over the three taps,
    z = main + 2^-11 cross + conditioning.
All sums in float32 (numpy's float32 matrix product: another order than the MFMA's, the same arithmetic).  The hidden state is
carried between layers as fp16 planes, hi + 2^-11 lo', with ceil8(C) columns, the padding zero.  Layer 0's gate (the start
convolution folded in, float32) and the tail (the last layer's share of the end convolution, float32) are the port's / a float32
product.  The weights are UNPACKED from the images of packing.pack_resskip_f16_weights / pack_gate_f16_weights, not split again:
the packers' lane order is part of what the emulation checks.

``defects`` plants what only this path can get wrong (test_split_reference.py):
    "rs_act_lo_lost": (layer, c0, c1)    the res/skip layer loses lo' of its activation channels c0 .. c1 - 1
    "rs_w_lo_zero_pair": p               the lo' weight image of column pair p is zero in every res/skip layer
    "gate_cross_scale": (layer, tile, s) the cross accumulator of one 32-channel column tile enters with s instead of 2^-11
    "gate_last_tile_from": t             the last gate column tile takes the weight images of tile t (every layer)
    "plane_padding": v                   the plane columns C .. ceil8(C) - 1 hold v instead of 0
    "rs_last_pair_shifted": True         the last two output columns of every res/skip layer take the two columns before them
"""
import numpy as np

from mbexwn_vocoder_amd import packing
from mbexwn_vocoder_amd.config import ModelDims

F32 = np.float32
S = F32(2048.0)
SI = F32(1.0 / 2048.0)


def split(x):
    """float32 x -> (hi, lo') as fp16 arrays: hi = fp16(x), lo' = fp16(2^11 x - 2^11 hi) (exact in float32 before the rounding)."""
    x = np.asarray(x, dtype=F32)
    hi = x.astype(np.float16)
    lo = (x * S - hi.astype(F32) * S).astype(np.float16)
    return hi, lo


def unpack_resskip_f16(img):
    """Image of packing.pack_resskip_f16_weights (steps, 12, 1024 words) -> (hi, lo') fp16 arrays (32 steps, 384): channel, column."""
    nk = img.shape[0]
    halves = np.ascontiguousarray(img).view(np.float16).reshape(nk, 12, 2, 2, 4, 16, 2, 4)   # step, pair, parity, part, kq, n, half, v
    both = halves.transpose(3, 0, 6, 4, 7, 1, 5, 2)                                          # part, step, half, kq, v, pair, n, parity
    both = np.ascontiguousarray(both).reshape(2, nk * 32, 384)
    return both[0], both[1]


def unpack_gate_f16(img):
    """Image of packing.pack_gate_f16_weights (tiles, steps, 6144 words) -> fp16 array (part: hi | lo', tap, 32 steps channels,
    tanh | sigmoid, column tile, 32 gate channels of the tile)."""
    nt, nk = img.shape[:2]
    halves = np.ascontiguousarray(img).view(np.float16).reshape(nt, nk, 3, 2, 2, 2, 4, 16, 8)  # block, step, tap, e, s, part, kq, n, v
    both = halves.transpose(5, 2, 1, 6, 8, 4, 0, 7, 3)                                        # part, tap, step, kq, v, s, block, n, e
    return np.ascontiguousarray(both).reshape(2, 3, nk * 32, 2, nt, 32)


def unpack_end(img, C, n_out):
    """Image of packing.pack_end_weights (ceil(C/8), 2, 32, 4) -> (C, n_out) float32."""
    img = np.asarray(img, dtype=F32)
    return np.ascontiguousarray(img.transpose(0, 1, 3, 2)).reshape(-1, 32)[:C, :n_out]


class SplitEmulation:
    """The split path of one model (cfg, raw weights, wavetables as build_case gives them), run on the items of a
    WaveNetReference: result(ref) has the form of WaveNetReference.port_result."""

    def __init__(self, cfg, raw, wt, defects=None):
        self.dims = dims = ModelDims(cfg)
        self.C, self.L, self.n_out = dims.wn_channels, dims.wn_layers, dims.wn_out_channels
        self.C8 = (self.C + 7) // 8 * 8
        self.defects = dict(defects or {})
        tab = packing.tensor_table(cfg, raw, wt, split_f16=True)
        C, L = self.C, self.L
        assert "wn.res_skip_0.fold_start_f16" in tab and L >= 3
        self.rs = [unpack_resskip_f16(tab["wn.res_skip_0.fold_start_f16" if ll == 0 else f"wn.res_skip_{ll}.fold_f16"])
                   for ll in range(L - 1)]
        self.rs_b = [np.asarray(tab[f"wn.res_skip_{ll}.fold_b"]).astype(F32) for ll in range(L - 1)]
        self.gate = {ll: unpack_gate_f16(tab[f"wn.conv1D_{ll}.gate_f16"]) for ll in range(1, L)}
        self.gate_b = {ll: np.asarray(tab[f"wn.conv1D_{ll}.b"]).astype(F32) for ll in range(1, L)}
        self.tail_w = unpack_end(tab["wn.tail.fold"], C, self.n_out)
        self.tail_b = np.asarray(tab["wn.tail.fold_b"]).astype(F32)
        self.dil = [int(dims.wn_dilation(ll)) for ll in range(L)]
        self.const_channel = dims.pulse_channels_eff + 1          # x' = [x | 1 | 0]: the channel that carries the start bias
        pair = self.defects.get("rs_w_lo_zero_pair")
        if pair is not None:
            self.rs = [(hi, lo.copy()) for hi, lo in self.rs]
            for _, lo in self.rs:
                lo[:, 32 * pair:32 * pair + 32] = 0
        src = self.defects.get("gate_last_tile_from")
        if src is not None:
            for ll in self.gate:
                g = self.gate[ll] = self.gate[ll].copy()
                g[..., -1, :] = g[..., src, :]

    # ---- one layer's arithmetic -----------------------------------------------------------------------------------
    def resskip(self, ll, act, old):
        """act (rows, K) float32: the layer's input rows; old (rows, C + n_out) float32: hidden state and output accumulator
        (layer 0: zeros, the layer initialises both).  Returns the new (rows, C + n_out)."""
        hi_w, lo_w = self.rs[ll]
        K = hi_w.shape[0]
        a = np.zeros((act.shape[0], K), dtype=F32)
        a[:, :act.shape[1]] = act
        hi, lo = split(a)
        lost = self.defects.get("rs_act_lo_lost")
        if lost is not None and lost[0] == ll:
            lo[:, lost[1]:lost[2]] = 0
        cout = self.C + self.n_out
        hi32, lo32, whi, wlo = hi.astype(F32), lo.astype(F32), hi_w.astype(F32)[:, :cout], lo_w.astype(F32)[:, :cout]
        acc = S * (old + self.rs_b[ll])
        acc = acc + (hi32 * S) @ whi + hi32 @ wlo + lo32 @ whi
        new = acc * SI
        if self.defects.get("rs_last_pair_shifted"):
            new[:, cout - 2:] = new[:, cout - 4:cout - 2]
        return new

    def planes(self, h):
        """The hidden state (rows, C) as the planes hold it: (hi, lo') fp16 (rows, ceil8(C)), the padding zero."""
        hi = np.zeros((h.shape[0], self.C8), dtype=np.float16)
        lo = np.zeros_like(hi)
        hi[:, :self.C], lo[:, :self.C] = split(h)
        if "plane_padding" in self.defects:
            hi[:, self.C:] = lo[:, self.C:] = self.defects["plane_padding"]
        return hi, lo

    def gate_z(self, ll, planes, cond):
        """Pre-activation (rows, 2 C) of layer ll >= 1 from the planes and the interpolated conditioning (rows, 2 C)."""
        w = self.gate[ll].astype(F32)                                  # part, tap, channel, s, tile, 32
        K, nt = w.shape[2], w.shape[4]
        rows, d, C = planes[0].shape[0], self.dil[ll], self.C
        h = np.zeros((2, rows + 2 * d, K), dtype=F32)                   # the 8-channel chunks that start below C, zero rows around
        h[0, d:d + rows, :self.C8], h[1, d:d + rows, :self.C8] = planes[0], planes[1]
        main = np.zeros((rows, 2, nt * 32), dtype=F32)
        cross = np.zeros_like(main)
        main[:, 0, :C], main[:, 1, :C] = self.gate_b[ll][:C], self.gate_b[ll][C:]
        for tap in range(3):
            hh, hl = h[0, tap * d:tap * d + rows], h[1, tap * d:tap * d + rows]
            for s in range(2):
                whi, wlo = w[0, tap, :, s].reshape(K, nt * 32), w[1, tap, :, s].reshape(K, nt * 32)
                main[:, s] += hh @ whi
                cross[:, s] += hh @ wlo
                cross[:, s] += hl @ whi
        scale = np.full(nt * 32, SI, dtype=F32)
        bad = self.defects.get("gate_cross_scale")
        if bad is not None and bad[0] == ll:
            scale[32 * bad[1]:32 * bad[1] + 32] = F32(bad[2])
        y = main + cross * scale
        return np.concatenate((y[:, 0, :C], y[:, 1, :C]), axis=-1) + cond

    # ---- a whole item ---------------------------------------------------------------------------------------------
    def item(self, om32, x, mel):
        """{"wn_out", "wn_hidden", "wn_skip"} of one item (x (1, rows, cin), mel (1, frames, 80)); "wn_skip" is the port's (the
        folded path holds none)."""
        C, L = self.C, self.L
        st = {}
        xp = np.zeros((x.shape[1], 16), dtype=F32)
        xp[:, :x.shape[2]] = np.asarray(x[0]).astype(F32)
        xp[:, self.const_channel] = 1.0

        def gate_z(ll, hidden, cond, z):
            if ll == 0:
                return z
            return self.gate_z(ll, st["planes"], np.asarray(cond[0], dtype=F32))[None].astype(z.dtype)

        def gate_out(ll, a):
            st["a"] = np.asarray(a[0], dtype=F32)
            if ll == L - 1:
                st["out"] = st["acc"] + st["a"] @ self.tail_w + self.tail_b
            return a

        def hook(ll, hidden):
            if ll == 0:
                new = self.resskip(0, np.concatenate((st["a"], xp), axis=-1), np.zeros((xp.shape[0], C + self.n_out), dtype=F32))
            else:
                hi, lo = st["planes"]
                old_h = hi[:, :C].astype(F32) + lo[:, :C].astype(F32) * SI
                new = self.resskip(ll, st["a"], np.concatenate((old_h, st["acc"]), axis=-1))
            st["planes"], st["acc"] = self.planes(new[:, :C]), new[:, C:]
            hi, lo = st["planes"]
            st["h"] = hi[:, :C].astype(F32) + lo[:, :C].astype(F32) * SI
            return st["h"][None].astype(hidden.dtype)

        out, h, skip, _, _ = om32.wavenet(np.asarray(x).astype(F32), np.asarray(mel).astype(F32), return_layers=True, hook=hook,
                                          taps={"gate_z": gate_z, "gate_out": gate_out})
        assert np.array_equal(h[0], st["h"])
        return {"wn_out": st["out"], "wn_hidden": st["h"], "wn_skip": skip[0]}

    def result(self, ref):
        per = {ii: self.item(ref.om32, ref.xs[ii], ref.mels[ii]) for ii in ref.items}
        B, R = len(ref.lengths), max(ref.lengths) * ref.rpf
        out = {}
        for name in ("wn_out", "wn_hidden", "wn_skip"):
            arr = np.full((B, R, per[ref.items[0]][name].shape[-1]), np.nan, dtype=np.float64)
            for ii in ref.items:
                arr[ii, :ref.rows(ii)] = per[ii][name]
            out[name] = arr
        return out
