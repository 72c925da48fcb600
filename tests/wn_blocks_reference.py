"""Stage reference and comparator for the WaveNet of any model -- several blocks with in-block up-sampling, the generic
kernels of a handle without weight images, pulse-PQMF and sub-harmonic inputs (CPU side, shared by test_wn_blocks_reference.py
and test_gpu_wavenet_blocks.py).

The oracle (OracleModel.wavenet_blocks) is fed the engine's own WaveNet input, item by item at the item's own length: its
"pulse" stage folded into rows (or, for a pulse-PQMF model, its "pulse_ana" stage) plus sigma * noise.  "pulse_ana" itself is
compared with OracleModel.pulse_analysis of the engine's "pulse".  Held per tensor, over every checked item's valid rows:

    pulse_ana                     (rows of block 0, pulse_channels)
    cond, cond1 .. cond3          the conditioning rows of block b before the interpolation (frames * cond rows per frame, 2 C_b)
    wn_hidden, wn_skip            the LAST block's hidden state and skip sum (frames * its rows per frame, C_last)
    wn_out                        the WaveNet output behind the last up-sampling convolution (frames * steps_per_frame, n_out)

at tol = max(K * port_err, F * max(1, |ref|)) with port_err the float32 port's own error on that tensor (K = 8, F = 5e-7 as in
wn_reference.py).  A failure names the item, block, row, channel, the row's place in its 128- and 256-row tiles (at the
block's own rate) and the rows left before the item's end.
"""
import numpy as np

from oracle import mbexwn_oracle as orc
from wn_reference import F_FLOOR, K_PORT


def block_geometry(dims):
    """Per WaveNet block: channels C, up-sampling factor behind it, rows per frame, conditioning rows per frame."""
    out, spf = [], dims.wn_in_rows_per_frame
    for C, uu in zip(dims.wn_block_channels, dims.wn_block_ups):
        out.append({"C": int(C), "ups": int(uu), "spf": spf, "ccu": spf // dims.cond_lin_upsampling})
        spf *= uu
    return out


def cond_name(block):
    return "cond" if block == 0 else f"cond{block}"


def stage_layout(dims):
    """{stage: (block, rows per frame, channels)} of every stage this comparator knows for the model (wn_skip included)."""
    geo = block_geometry(dims)
    out = {}
    if dims.pulse_pqmf:
        out["pulse_ana"] = (0, dims.wn_in_rows_per_frame, dims.pulse_channels)
    for bb, g in enumerate(geo):
        out[cond_name(bb)] = (bb, g["ccu"], 2 * g["C"])
    last = len(geo) - 1
    out["wn_hidden"] = (last, geo[-1]["spf"], geo[-1]["C"])
    out["wn_skip"] = (last, geo[-1]["spf"], geo[-1]["C"])
    out["wn_out"] = (last, dims.steps_per_frame, dims.wn_out_channels)
    return out


def oracle_block_stages(om, x, mel, hook=None):
    """The WaveNet stages of one item (x (1, rows, cin), mel (1, frames, 80)) in the oracle's dtype."""
    out, blocks = om.wavenet_blocks(np.asarray(x).astype(om.dtype), np.asarray(mel).astype(om.dtype), hook=hook,
                                    return_blocks=True)
    st = {"wn_out": out[0], "wn_hidden": blocks[-1]["hidden"][0], "wn_skip": blocks[-1]["skip"][0]}
    for bb, blk in enumerate(blocks):
        st[cond_name(bb)] = blk["cond"][0]
    return st


class BlocksReference:
    """float64 oracle and float32 port of the WaveNet stages for the items ``items`` of a ragged batch.

    pulse: the engine's "pulse" stage (B, >= frames * pulse_per_frame * (1 + sub-harmonics)); noise (B, >= frames * rows
    per frame of block 0); mel (B, T, 80); lengths: frames per item.  pulse_ana: the engine's "pulse_ana" stage (B, >= rows,
    pulse_channels) of a pulse-PQMF model -- the WaveNet is fed it; None: the float32 port's analysis (a CPU stand-in)."""

    def __init__(self, om64, om32, dims, pulse, noise, mel, lengths, items=None, pulse_ana=None):
        self.om64, self.om32, self.dims = om64, om32, dims
        self.lengths = [int(ll) for ll in lengths]
        self.items = list(range(len(self.lengths))) if items is None else list(items)
        self.layout = stage_layout(dims)
        self.rpf = dims.wn_in_rows_per_frame
        self.pqmf = bool(dims.pulse_pqmf)
        B = len(self.lengths)
        self.pulse = np.asarray(pulse, dtype=np.float32).reshape(B, -1)
        self.noise = np.asarray(noise, dtype=np.float32).reshape(B, -1)
        self.mels = {ii: np.asarray(mel)[ii:ii + 1, :self.lengths[ii]] for ii in self.items}
        self.pulse_ana = None if pulse_ana is None else np.asarray(pulse_ana, dtype=np.float32).reshape(B, -1, dims.pulse_channels)
        self.ref = {ii: self._stages(om64, ii) for ii in self.items}
        self.port = {ii: self._stages(om32, ii) for ii in self.items}

    def item_pulse(self, ii):
        return self.pulse[ii:ii + 1, :self.lengths[ii] * self.dims.pulse_per_frame * (1 + self.dims.wt_subharm)]

    def wavenet_input(self, ii, rows=None):
        """The WaveNet input rows of item ii (1, rows, cin) in float64: the excitation rows (``rows``, or the engine's own)
        and sigma * noise."""
        n = self.lengths[ii] * self.rpf
        if rows is None:
            if self.pqmf:
                rows = (self.pulse_ana[ii:ii + 1, :n] if self.pulse_ana is not None else
                        self.om32.pulse_analysis(self.item_pulse(ii)).astype(np.float32))
            else:
                rows = self.item_pulse(ii).reshape(1, n, -1)
        x = np.asarray(rows, dtype=np.float64)
        if self.om64.sigma:
            x = np.concatenate((x, self.om64.sigma * self.noise[ii:ii + 1, :n, None].astype(np.float64)), axis=-1)
        return x

    def _stages(self, om, ii, hook=None, model_rows=False):
        rows = None
        st = {}
        if self.pqmf:
            st["pulse_ana"] = om.pulse_analysis(self.item_pulse(ii))[0]
            if model_rows:                   # a planted analysis defect reaches the WaveNet too
                rows = st["pulse_ana"][None].astype(np.float32)
        st.update(oracle_block_stages(om, self.wavenet_input(ii, rows), self.mels[ii], hook=hook))
        return st

    def rows(self, name, ii):
        return self.lengths[ii] * self.layout[name][1]

    def port_result(self, hook=None, hooks=None, model=None, models=None):
        """The float32 port's stages as a batch {name: (B, max rows, channels)} (rows behind an item's end are NaN), with an
        optional planted defect: ``hook`` for every item or ``hooks`` {item: hook} (hook(block, layer, hidden), see
        OracleModel.wavenet_blocks), or ``model`` / ``models`` {item: model}: a float32 OracleModel to run instead of the port."""
        hooks, models = dict(hooks or {}), dict(models or {})
        per = {}
        for ii in self.items:
            hk, md = hooks.get(ii, hook), models.get(ii, model)
            if hk is None and md is None:
                per[ii] = self.port[ii]
            else:
                per[ii] = self._stages(self.om32 if md is None else md, ii, hook=hk, model_rows=md is not None)
        B = len(self.lengths)
        out = {}
        for name in per[self.items[0]]:
            R = max(self.lengths) * self.layout[name][1]
            arr = np.full((B, R, self.layout[name][2]), np.nan, dtype=np.float64)
            for ii in self.items:
                arr[ii, :self.rows(name, ii)] = per[ii][name]
            out[name] = arr
        return out

    def compare(self, got, names, k=K_PORT, f=F_FLOOR):
        """Per tensor of ``names``: max |got - ref| over every checked item's valid rows against its bar.  got: {name: array
        (B, >= max rows, channels) or {item: (>= rows, channels)}}.  Returns {name: record}; record["ok"] is False where the
        bar is broken (a non-finite value breaks it too) and record["where"] locates the worst element."""
        report = {}
        for name in names:
            block = self.layout[name][0]
            worst, port_err, amp, where = -1.0, 0.0, 0.0, None
            for ii in self.items:
                n = self.rows(name, ii)
                ref = self.ref[ii][name]
                port_err = max(port_err, float(np.abs(self.port[ii][name] - ref).max()))
                amp = max(amp, float(np.abs(ref).max()))
                g = np.asarray(got[name][ii], dtype=np.float64)[:n]
                if g.shape != ref.shape:
                    raise AssertionError(f"{name} item {ii}: engine rows/channels {g.shape} against the oracle's {ref.shape}")
                diff = np.abs(g - ref)
                diff[~np.isfinite(diff)] = np.inf
                flat = int(np.argmax(diff))
                err = float(diff.flat[flat])
                if err > worst:
                    row, chan = divmod(flat, ref.shape[-1])
                    worst = err
                    where = {"item": ii, "block": block, "row": row, "channel": chan, "got": float(g[row, chan]),
                             "ref": float(ref[row, chan]), "row%256": row % 256, "row%128": row % 128, "rows_to_end": n - row,
                             "item_rows": n}
            tol = max(k * port_err, f * max(1.0, amp))
            report[name] = {"err": worst, "tol": tol, "port_err": port_err, "ref_max": amp, "ok": bool(worst <= tol),
                            "where": where}
        return report


def failures(report):
    """Readable lines for the tensors of a compare() report that break their bar ("" when none does)."""
    lines = []
    for name, rec in report.items():
        if rec["ok"]:
            continue
        w = rec["where"]
        lines.append(f"{name}: max err {rec['err']:.3e} > tol {rec['tol']:.3e} (float32 port {rec['port_err']:.2e}, |ref| "
                     f"{rec['ref_max']:.3g}) at item {w['item']} block {w['block']} row {w['row']} channel {w['channel']} (got "
                     f"{w['got']:.9g}, ref {w['ref']:.9g}); row % 256 = {w['row%256']}, row % 128 = {w['row%128']}, "
                     f"{w['rows_to_end']} rows before the item's end ({w['item_rows']} rows)")
    return "\n".join(lines)


def summary(report):
    return "  ".join(f"{name} {rec['err']:.2e}/{rec['tol']:.2e}" for name, rec in report.items())


def assert_matches(report):
    msg = failures(report)
    assert not msg, "WaveNet stage off the float64 oracle:\n" + msg


def engine_stages(eng, layout, names, batch, items):
    """The engine's stages of its last forward as {name: {item: (rows, channels)}} float64 arrays."""
    out = {}
    for name in names:
        arr = eng.stage(name).view(batch, -1, layout[name][2])
        out[name] = {ii: arr[ii].cpu().numpy().astype(np.float64) for ii in items}
    return out


def oracle_models(cfg, raw, wt):
    return orc.OracleModel(cfg, raw, wt), orc.OracleModel(cfg, raw, wt, dtype=np.float32)
