"""WaveNet stage reference and comparator (CPU side, shared by test_wn_reference.py and test_gpu_wavenet_stages.py).

The engine's WaveNet stages ("wn_out", "wn_hidden", "wn_skip") are compared with the float64 oracle run on the engine's own
excitation rows (its "pulse" stage plus sigma * noise, as test_gpu_forms.py does), item by item at the item's own length, so
that the F0 contour and the wavetable rounding stay out of the comparison.  The float32 port of the same graph
(OracleModel(dtype=np.float32)) on the same input sets the scale of float32 rounding: per tensor the bar is

    tol = max(K * port_err, F * max(1, |ref|))

with port_err the port's own max error on that tensor and |ref| the tensor's largest magnitude.  K = 8 and F = 5e-7 sit
about 4x below the smallest planted defect of test_wn_reference.py (one 32-channel tile of h in fp16 after one layer:
4.2e-6 in wn_out at |ref| 0.24), which the plain audio tolerance 1e-4 * max(1, |audio|) lets through; on an MI355X every
form, block shape and geometry of test_gpu_wavenet_stages.py stays at or below 0.55 of the bar
(profiles/wavenet_stages.json); the split-half-precision kernels at every channel edge, model variant and launch size at or below
0.37 (gfu-split "wn_out", deep12-split), where the numpy emulation of their arithmetic alone (test_split_reference.py) takes
0.09 - 0.16.
"""
import numpy as np

from oracle import mbexwn_oracle as orc

K_PORT = 8.0
F_FLOOR = 5e-7
STAGES = ("wn_out", "wn_hidden", "wn_skip")


def oracle_stages(om, x, mel, hook=None, taps=None):
    """The WaveNet stages of one item (x (1, rows, cin), mel (1, frames, 80)) in the oracle's dtype:
    {"wn_out": (rows, n_out), "wn_hidden": (rows, C), "wn_skip": (rows, C)}."""
    out, h, skip, _, _ = om.wavenet(np.asarray(x).astype(om.dtype), np.asarray(mel).astype(om.dtype), return_layers=True,
                                    hook=hook, taps=taps)
    return {"wn_out": out[0], "wn_hidden": h[0], "wn_skip": skip[0]}


def wavenet_inputs(om, pulse, noise, lengths, rows_per_frame):
    """Per item the WaveNet input rows (1, lengths[i] * rows_per_frame, cin) in float64: the excitation rows (pulse, (B, rows,
    channels) as the engine's "pulse" stage holds them) and, when the model has a noise channel, om.sigma * noise."""
    pulse = np.asarray(pulse, dtype=np.float64)
    xs = []
    for ii, ll in enumerate(lengths):
        rows = int(ll) * rows_per_frame
        x = pulse[ii:ii + 1, :rows]
        if om.sigma:
            x = np.concatenate((x, om.sigma * np.asarray(noise, dtype=np.float64)[ii:ii + 1, :rows, None]), axis=-1)
        xs.append(x)
    return xs


class WaveNetReference:
    """float64 oracle and float32 port of the WaveNet for the items ``items`` of a ragged batch.

    om64 / om32: OracleModel of the same weights in float64 / float32; xs: wavenet_inputs(...); mel (B, T, 80); lengths: frames
    per item; rows_per_frame: WaveNet rows per mel frame."""

    def __init__(self, om64, om32, xs, mel, lengths, rows_per_frame, items=None):
        self.om64, self.om32 = om64, om32
        self.lengths = [int(ll) for ll in lengths]
        self.rpf = rows_per_frame
        self.items = list(range(len(self.lengths))) if items is None else list(items)
        self.xs = {ii: xs[ii] for ii in self.items}
        self.mels = {ii: np.asarray(mel)[ii:ii + 1, :self.lengths[ii]] for ii in self.items}
        self.ref = {ii: oracle_stages(om64, self.xs[ii], self.mels[ii]) for ii in self.items}
        self.port = {ii: oracle_stages(om32, self.xs[ii], self.mels[ii]) for ii in self.items}

    def rows(self, ii):
        return self.lengths[ii] * self.rpf

    def port_result(self, hook=None, hooks=None, model=None, taps=None):
        """The float32 port's stages as a batch {name: (B, max rows, channels)} (rows behind an item's end are NaN), with an
        optional planted defect: ``hook`` for every item, or ``hooks`` {item: hook} (see OracleModel.wavenet), or ``model``: a
        float32 OracleModel to run instead of the port (one whose conditioning was altered, say), or ``taps`` {item: taps of
        OracleModel.wavenet} on a layer's gate output or res/skip output."""
        hooks, taps = dict(hooks or {}), dict(taps or {})
        per = {}
        for ii in self.items:
            hk = hooks.get(ii, hook)
            if hk is None and model is None and ii not in taps:
                per[ii] = self.port[ii]
            else:
                per[ii] = oracle_stages(self.om32 if model is None else model, self.xs[ii], self.mels[ii], hook=hk, taps=taps.get(ii))
        B, R = len(self.lengths), max(self.lengths) * self.rpf
        out = {}
        for name in STAGES:
            ch = per[self.items[0]][name].shape[-1]
            arr = np.full((B, R, ch), np.nan, dtype=np.float64)
            for ii in self.items:
                arr[ii, :self.rows(ii)] = per[ii][name]
            out[name] = arr
        return out

    def compare(self, got, names=("wn_out", "wn_hidden"), k=K_PORT, f=F_FLOOR):
        """Per tensor of ``names``: max |got - ref| over every checked item's valid rows against its bar.  got: {name: array
        (B, >= max rows, channels) or {item: (>= rows, channels)}}.  Returns {name: record}; record["ok"] is False where the bar is broken (a non-finite
        value breaks it too) and record["where"] locates the worst element."""
        report = {}
        for name in names:
            worst, port_err, amp = -1.0, 0.0, 0.0
            where = None
            for ii in self.items:
                n = self.rows(ii)
                ref = self.ref[ii][name]
                port_err = max(port_err, float(np.abs(self.port[ii][name] - ref).max()))
                amp = max(amp, float(np.abs(ref).max()))
                g = np.asarray(got[name][ii], dtype=np.float64)[:n, :ref.shape[-1]]
                if g.shape != ref.shape:
                    raise AssertionError(f"{name} item {ii}: engine rows/channels {g.shape} against the oracle's {ref.shape}")
                diff = np.abs(g - ref)
                diff[~np.isfinite(diff)] = np.inf
                flat = int(np.argmax(diff))
                err = float(diff.flat[flat])
                if err > worst:
                    row, chan = divmod(flat, ref.shape[-1])
                    worst = err
                    where = {"item": ii, "row": row, "channel": chan, "got": float(g[row, chan]), "ref": float(ref[row, chan]),
                             "row%256": row % 256, "row%128": row % 128, "rows_to_end": n - row, "item_rows": n}
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
                     f"{rec['ref_max']:.3g}) at item {w['item']} row {w['row']} channel {w['channel']} (got {w['got']:.9g}, "
                     f"ref {w['ref']:.9g}); row % 256 = {w['row%256']}, row % 128 = {w['row%128']}, {w['rows_to_end']} rows "
                     f"before the item's end ({w['item_rows']} rows)")
    return "\n".join(lines)


def summary(report):
    return "  ".join(f"{name} {rec['err']:.2e}/{rec['tol']:.2e}" for name, rec in report.items())


def assert_matches(report):
    msg = failures(report)
    assert not msg, "WaveNet stage off the float64 oracle:\n" + msg


def engine_stages(eng, names, batch, max_frames, items=None):
    """The engine's WaveNet stages of its last forward as {name: (batch, max rows, channels)} float64 arrays, or with
    ``items`` as {name: {item: (max rows, channels)}} for those items only."""
    rows = max_frames * eng.dims.wn_in_rows_per_frame
    out = {}
    for name in names:
        arr = eng.stage(name).view(batch, rows, -1)
        if items is None:
            out[name] = arr.cpu().numpy().astype(np.float64)
        else:
            out[name] = {ii: arr[ii].cpu().numpy().astype(np.float64) for ii in items}
    return out


def oracle_models(cfg, raw, wt):
    return orc.OracleModel(cfg, raw, wt), orc.OracleModel(cfg, raw, wt, dtype=np.float32)
