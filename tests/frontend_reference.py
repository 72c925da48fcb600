"""References and comparators of the stages in front of the WaveNet (CPU side, shared by test_frontend_reference.py and
test_gpu_frontend_stages.py): audio -> log-mel (csrc/mel_analysis.hip), the RMS normalisation (csrc/norm_mel.hip) and the
oscillator with its F0 contour (csrc/wavetable.hip).  Every comparison is per item at the item's own length.

Log-mel.  ``log_mel_reference`` is a plain float64 restatement that does not touch analysis.py: np.pad "reflect" by
(win // 2, win), the float32 window as float64, np.fft.rfft in float64, magnitude, product with the float32 basis as float64.
It takes the tables that compute_log_mel_device uploads (analysis.mel_analysis_tables), so table construction stays out of
the comparison (test_tables.py pins it).  ``log_mel_port`` does the same steps in float32 (the transform is torch's on the
CPU, see float32_rfft) and ends in the float32 log like the kernel; it also carries the planted defects of
test_frontend_reference.py.
The comparison is on AMPLITUDES, per item and per frame: exp(output) against the reference's mel amplitudes, both floored
at eps, so a quiet frame beside a loud one is judged on its own scale:

    tol(frame) = max(K * port_err(frame), F_MEL[geometry] * scale(frame)),    scale = the frame's largest reference mel amplitude

with K = 8 as in wn_reference.py and port_err the float32 port's own largest amplitude error in that frame.  A frame whose
reference amplitude is below eps in every channel must be log(eps) as float32, exactly.

F_MEL.  Measured here (test_frontend_reference.py::test_port_sets_the_mel_floor, every geometry and item of MEL_GEOMETRIES /
mel_items): the float32 port's worst error relative to its frame's scale is 1.70e-5, on the constant items of 1200 / 300 /
2048 / 1.  There the one triangle weighs bins 1 .. 1023 and leaves out DC, where the windowed constant has a bin of
magnitude 300: a float32 transform carries an error of about eps32 * ||frame||_2 = 6e-7 in every bin, and over the ~300
bins where the window's side lobes lie below that floor the magnitudes' errors add up instead of cancelling.  The 3- to
128-channel geometries show 4.7e-7 .. 6.5e-7, most of it the float32 rounding of the stored logarithm (|log| up to 16: half
an ulp is 4.8e-7 of the amplitude).  One floor for every launch, 4 x 1.70e-5 = 6.8e-5, would let that one geometry blunt
the other eight, so every geometry gets four times its OWN worst: 1.9e-6 .. 2.6e-6, and 6.8e-5 for 1200 / 300 / 2048 / 1
-- none above the single figure, each fixed from the reference and the port alone, never from the kernel.  The smallest
planted defect of test_frontend_reference.py (bin_hi one short on the narrow channel of 1200 / 300 / 2048 / 80 whose last
bin weighs least, or of 200 / 50 / 256 / 128) breaks its bar 880 times over.  On an MI355X the kernel stays at 0.42 .. 0.65 of the bar at the eight
geometries and at 0.15 at 1200 / 300 / 2048 / 1 (profiles/frontend_stages.json).  A first version of the port transformed
with numpy and measured 1.76e-6 at worst: that transform turned out to run in float64 (see float32_rfft), so the figure was
not float32's, and the kernel's constant items at 1200 / 300 / 2048 / 1 sat at 2.9 of a bar that no float32 transform meets.

RMS normalisation: thin wrappers around orc.normalize_inputs_by_rms (float64, and dtype=np.float32 as the port); mel_norm is
held to max(K * port_err, F_NORM * max(1, |ref|)), the per-sample gain to the same bar on the RELATIVE error
(|got - ref| / |ref|, floor F_NORM).  F_NORM = 5e-7: over the lengths and levels of NORM_LENGTHS / NORM_LEVELS the port is
within 7e-7 on mel_norm at |ref| about 10 and 4e-7 relative on the gain, so the bars sit near 5e-6.

Oscillator: OracleModel.wavetable / phase_from_f0 on the engine's own "f0" stage; the phase bit for bit, the pulse to the
project's 2e-6.  F0 contour: OracleModel.generate_f0 (float64) on the item's own frames, half a float32 ulp.
"""
import copy

import numpy as np

from oracle import mbexwn_oracle as orc

K_PORT = 8.0
F_NORM = 5e-7
PULSE_TOL = 2e-6
EPS32 = float(np.finfo(np.float32).eps)
FFT_THREADS = 256                      # csrc/fft_lds.h

# ------------------------------------------------------------------------------------------------------------------------
# audio -> log-mel: cases
# ------------------------------------------------------------------------------------------------------------------------
_BASE = {"sample_rate": 24000, "fmin": 0.0, "fmax": 12000.0}


def _geom(win, hop, fft, mels, **kw):
    return dict(_BASE, win_size=win, hop_size=hop, fft_size=fft, mel_channels=mels, **kw)


# window / hop / FFT / channels
MEL_GEOMETRIES = {
    "1200_300_2048_80": _geom(1200, 300, 2048, 80),
    "800_200_1024_80_16k": _geom(800, 200, 1024, 80, sample_rate=16000, fmax=8000.0),     # radix-2 pass
    "512_128_512_40": _geom(512, 128, 512, 40),                                           # window = FFT
    "1024_256_2048_80": _geom(1024, 256, 2048, 80),
    "1199_301_2048_80": _geom(1199, 301, 2048, 80),                                       # odd window and hop
    "6_2_8_3": _geom(6, 2, 8, 3),                         # the lower limit, fewer points than threads, radix-4 only
    "12_4_16_5": _geom(12, 4, 16, 5),                     # fewer points than threads, with the radix-2 pass
    "200_50_256_128": _geom(200, 50, 256, 128),           # triangles without a bin
    "1200_300_2048_1": _geom(1200, 300, 2048, 1),         # one triangle over 1023 bins
}


# the floor of each geometry's bar: four times the worst relative error the float32 port shows at that geometry (module
# docstring); none is above the 6.8e-5 that the worst geometry sets
F_MEL = {"1200_300_2048_80": 2.1e-6, "800_200_1024_80_16k": 2.0e-6, "512_128_512_40": 2.6e-6, "1024_256_2048_80": 1.9e-6,
         "1199_301_2048_80": 1.9e-6, "6_2_8_3": 2.5e-6, "12_4_16_5": 2.4e-6, "200_50_256_128": 2.3e-6, "1200_300_2048_1": 6.8e-5}
assert set(F_MEL) == set(MEL_GEOMETRIES)


def mel_lengths(cfg):
    """The item lengths of one launch: N (the longest, >= win/2 + 1), 0, 1, 2, hop - 1, hop, hop + 1, win/2 - 1, win/2,
    win/2 + 1, win - 1, win, a multiple of hop and a multiple minus one."""
    win, hop = int(cfg["win_size"]), int(cfg["hop_size"])
    n_max = max(9 * hop + hop // 2 + 1, 2 * win + 3)
    return [n_max, 0, 1, 2, hop - 1, hop, hop + 1, win // 2 - 1, win // 2, win // 2 + 1, win - 1, win, 7 * hop, 7 * hop - 1]


def mel_items(cfg, seed=29):
    """(sound (B, N) float32, lengths, labels) of one ragged launch: Gaussian noise at amplitudes 1e-4 .. 1 at every length
    of mel_lengths, then silence, a constant, unit impulses at sample 0, n - 1 and win / 2, a sinusoid on a bin centre and
    one between bins, and one item at amplitude 1e4."""
    win, hop, fft, sr = int(cfg["win_size"]), int(cfg["hop_size"]), int(cfg["fft_size"]), float(cfg["sample_rate"])
    rng = np.random.default_rng(seed)
    base = mel_lengths(cfg)
    n_max = base[0]
    items = []
    amps = np.geomspace(1e-4, 1.0, len(base))
    for nn, aa in zip(base, amps[rng.permutation(len(base))]):
        items.append((f"noise{aa:.0e}", (aa * rng.normal(size=nn)).astype(np.float32)))
    items.append(("silence", np.zeros(3 * hop + 1, np.float32)))
    items.append(("constant", np.full(n_max - 1, 0.25, np.float32)))
    items.append(("constant-short", np.full(max(win // 2 - 1, 1), -0.5, np.float32)))
    for name, nn, pos in (("impulse0", n_max - 2, 0), ("impulse-last", n_max - 3, n_max - 4), ("impulse-mid", n_max, win // 2),
                          ("impulse0-short", hop + 1, 0), ("impulse-last-short", hop + 1, hop),
                          ("impulse0-tiny", max(win // 4, 2), 0), ("impulse-last-tiny", max(win // 4, 2), max(win // 4, 2) - 1)):
        x = np.zeros(nn, np.float32)
        x[pos] = 1.0
        items.append((name, x))
    tt = np.arange(n_max)
    k_bin = max(fft // 16, 1)
    items.append(("sine-on-bin", (0.5 * np.sin(2 * np.pi * k_bin * tt / fft)).astype(np.float32)))
    items.append(("sine-between-bins", (0.5 * np.sin(2 * np.pi * (k_bin + 0.5) * tt / fft + 0.3)).astype(np.float32)))
    items.append(("noise1e4", (1e4 * rng.normal(size=5 * hop + 1)).astype(np.float32)))
    lengths = [int(x.size) for _, x in items]
    assert max(lengths) == n_max and n_max >= win // 2 + 1 and sr > 0
    sound = np.zeros((len(items), n_max), np.float32)
    for ii, (_, x) in enumerate(items):
        sound[ii, :x.size] = x
    return sound, lengths, [name for name, _ in items]


def reflections_needed(n, win, hop):
    """How often an item of n samples is folded by the reflect padding over its n // hop + 1 frames.  A centred first frame
    always leaves an item of two samples or more, so 0 is taken by n = 0 (nothing is read) and n = 1 (its one sample is
    repeated, not folded) alone."""
    if n < 2:
        return 0
    lo, hi = -(win // 2), (n // hop) * hop + win - win // 2 - 1
    front = (-lo + n - 2) // (n - 1) if lo < 0 else 0
    back = (hi - (n - 1) + n - 2) // (n - 1) if hi > n - 1 else 0
    return max(front, back)


def fft_passes(fft):
    """(radix-4 passes, radix-2 passes) of csrc/fft_lds.h for a real transform of fft points (fft / 2 complex points)."""
    lg = int(np.log2(fft // 2))
    return lg // 2, lg % 2


# ------------------------------------------------------------------------------------------------------------------------
# audio -> log-mel: reference, port, comparator
# ------------------------------------------------------------------------------------------------------------------------
def log_mel_reference(x, window, basis, hop, fft):
    """Mel AMPLITUDES (n // hop + 1, n_mels) float64 of one item x (n,): np.pad reflect by (win // 2, win), float32 window
    as float64, float64 rfft, magnitude, float32 basis as float64.  n = 0: one frame of zeros."""
    x = np.asarray(x, dtype=np.float64)
    win, n = int(window.size), int(x.size)
    if n == 0:
        return np.zeros((1, basis.shape[0]))
    xp = np.pad(x, (win // 2, win), mode="reflect")
    w64, b64 = np.asarray(window, dtype=np.float64), np.asarray(basis, dtype=np.float64)
    frames = np.stack([xp[t * hop: t * hop + win] * w64 for t in range(n // hop + 1)])
    return np.abs(np.fft.rfft(frames, fft, axis=-1)) @ b64.T


def reflect_index(s, n):
    """numpy "reflect" as an index map: period 2 (n - 1); n = 1 reads sample 0."""
    if n < 2:
        return np.zeros_like(s)
    m = np.mod(s, 2 * (n - 1))
    return np.where(m >= n, 2 * (n - 1) - m, m)


def reflect_twice_then_clamp_index(s, n):
    """(planted defect) the kernel's index rule before the closed form: one fold at the front, one at the end, a clamp."""
    s = np.where(s < 0, -s, s)
    s = np.where(s >= n, 2 * (n - 1) - s, s)
    return np.clip(s, 0, n - 1)


def symmetric_short_index(win):
    """(planted defect) "symmetric" (the edge sample repeated, period 2 n) on items below half a window."""
    def index(s, n):
        if n >= win // 2 + 1 or n < 2:
            return reflect_index(s, n)
        m = np.mod(s, 2 * n)
        return np.where(m >= n, 2 * n - 1 - m, m)
    return index


def swap_bins_1024(spec, fft, k=37):
    """(planted defect) bins k and fft / 2 - k exchanged in the real split of a 1024-point transform."""
    if fft != 1024:
        return spec
    spec = spec.copy()
    spec[..., [k, fft // 2 - k]] = spec[..., [fft // 2 - k, k]]
    return spec


def frames_short_at_hop_multiples(n, hop):
    """(planted defect) (n - 1) // hop + 1 frames: one short where n is a multiple of hop."""
    return (n - 1) // hop + 1 if n > 0 else 1


def float32_rfft(frames, fft):
    """rfft of float32 rows carried out in float32: torch's CPU transform.  numpy's is not used: where these tests were
    written, np.fft.rfft of a float32 array returns complex64 that is bit for bit the float64 transform rounded once
    (test_frontend_reference.py::test_port_transform_is_float32), so it does not show what float32 arithmetic costs."""
    import torch
    spec = torch.fft.rfft(torch.from_numpy(np.ascontiguousarray(frames, dtype=np.float32)), n=fft, dim=-1).numpy()
    assert spec.dtype == np.complex64
    return spec


def log_mel_port(x, window, basis, hop, fft, eps=EPS32, index=reflect_index, spec_hook=None, n_frames=None):
    """The float32 port: log-mel (frames, n_mels) float32 of one item, the steps of log_mel_reference in float32 with the
    padding as an index map.  index / spec_hook / n_frames / an altered basis plant defects."""
    x = np.asarray(x, dtype=np.float32)
    win, n = int(window.size), int(x.size)
    if n == 0:
        return np.full((1, basis.shape[0]), np.log(np.float64(np.float32(eps))), np.float32)
    nfr = n // hop + 1 if n_frames is None else n_frames(n, hop)
    xp = x[index(np.arange(-(win // 2), n + win), n)]
    frames = np.stack([xp[t * hop: t * hop + win] * np.asarray(window, np.float32) for t in range(nfr)])
    spec = float32_rfft(frames, fft)
    if spec_hook is not None:
        spec = spec_hook(spec, fft)
    mel = np.abs(spec) @ np.asarray(basis, np.float32).T
    assert mel.dtype == np.float32
    return np.log(np.maximum(mel, np.float32(eps)))


class MelReference:
    """float64 reference and float32 port of one ragged launch.  sound (B, N) float32, lengths, tables = (window, twiddle,
    basis, bin_lo, bin_hi) of analysis.mel_analysis_tables, cfg the preprocess configuration, floor the geometry's F_MEL."""

    def __init__(self, sound, lengths, tables, cfg, floor, eps=EPS32):
        self.floor = float(floor)                                   # F_MEL of the geometry
        self.sound, self.lengths = np.asarray(sound, np.float32), [int(nn) for nn in lengths]
        self.window, _, self.basis, self.lo, self.hi = tables
        self.hop, self.fft, self.eps = int(cfg["hop_size"]), int(cfg["fft_size"]), float(eps)
        self.ref = [log_mel_reference(self.sound[ii, :nn], self.window, self.basis, self.hop, self.fft)
                    for ii, nn in enumerate(self.lengths)]
        self.port = [log_mel_port(self.sound[ii, :nn], self.window, self.basis, self.hop, self.fft, self.eps)
                     for ii, nn in enumerate(self.lengths)]

    def frames(self, ii):
        return self.lengths[ii] // self.hop + 1

    def port_result(self, basis=None, **defect):
        """The port as compute_log_mel_device lays a launch out: (B, N // hop + 1, n_mels) float32, rows that are not
        written are 0.  ``defect``: keyword arguments of log_mel_port, ``basis``: an altered basis."""
        out = np.zeros((len(self.lengths), max(self.lengths) // self.hop + 1, self.basis.shape[0]), np.float32)
        for ii, nn in enumerate(self.lengths):
            if defect or basis is not None:
                lm = log_mel_port(self.sound[ii, :nn], self.window, self.basis if basis is None else basis, self.hop, self.fft,
                                  self.eps, **defect)
            else:
                lm = self.port[ii]
            out[ii, :lm.shape[0]] = lm
        return out

    def _amps(self, logs):
        with np.errstate(over="ignore", invalid="ignore"):
            return np.maximum(np.exp(np.asarray(logs, dtype=np.float64)), self.eps)

    def port_relative_error(self):
        """The float32 port's worst amplitude error relative to its frame's scale (what F_MEL is four times of)."""
        worst = 0.0
        for ii in range(len(self.lengths)):
            ref = np.maximum(self.ref[ii], self.eps)
            live = self.ref[ii].max(axis=1) >= self.eps
            if live.any():
                rel = np.abs(self._amps(self.port[ii]) - ref).max(axis=1) / ref.max(axis=1)
                worst = max(worst, float(rel[live].max()))
        return worst

    def compare(self, got, k=K_PORT, items=None):
        """got (B, >= frames, n_mels) float32 log-mel.  Returns the record of the frame with the worst error-to-bar ratio:
        {"ok", "ratio", "err", "tol", "port_err", "scale", "where": {item, frame, channel, length, n%hop, ...}}, and for the
        frames that are silent in the reference "silent_frames", "silent_wrong" (not log(eps) exactly), "silent_where"."""
        got = np.asarray(got)
        log_eps = np.float32(np.log(np.float64(np.float32(self.eps))))
        best = {"ok": True, "ratio": -1.0, "err": 0.0, "tol": 0.0, "port_err": 0.0, "scale": 0.0, "silent_frames": 0,
                "silent_wrong": 0, "silent_where": None, "where": None}
        for ii in (range(len(self.lengths)) if items is None else items):
            nn, nfr = self.lengths[ii], self.frames(ii)
            g = np.asarray(got[ii, :nfr], dtype=np.float32)
            ref = np.maximum(self.ref[ii], self.eps)
            scale = ref.max(axis=1)
            silent = self.ref[ii].max(axis=1) < self.eps
            port_err = np.abs(self._amps(self.port[ii]) - ref).max(axis=1)
            tol = np.maximum(k * port_err, self.floor * scale)
            diff = np.abs(self._amps(g) - ref)
            diff[~np.isfinite(diff) | ~np.isfinite(g)] = np.inf
            # a silent frame: the float32 nearest to log(eps), bit for bit; judged apart from the live frames
            wrong = silent[:, None] & (g.view(np.uint32) != log_eps.view(np.uint32))
            best["silent_frames"] += int(silent.sum())
            best["silent_wrong"] += int(wrong.any(axis=1).sum())
            if wrong.any() and best["silent_where"] is None:
                t, ch = (int(vv) for vv in np.argwhere(wrong)[0])
                best["silent_where"] = {"item": ii, "frame": t, "channel": ch, "length": nn, "n%hop": nn % self.hop,
                                        "frames": nfr, "got": float(g[t, ch]), "ref": float(log_eps)}
            ratio = np.where(silent, 0.0, diff.max(axis=1) / tol)
            t = int(np.argmax(ratio))
            if ratio[t] > best["ratio"]:
                ch = int(np.argmax(diff[t]))
                best.update(ratio=float(ratio[t]), err=float(diff[t, ch]), tol=float(tol[t]), port_err=float(port_err[t]),
                            scale=float(scale[t]),
                            where={"item": ii, "frame": t, "channel": ch, "length": nn, "n%hop": nn % self.hop,
                                   "frames": nfr, "got": float(g[t, ch]), "ref": float(np.log(ref[t, ch]))})
        best["ok"] = bool(best["ratio"] <= 1.0 and best["silent_wrong"] == 0)
        return best


def mel_failure(rec, labels=None):
    """Readable lines for a MelReference.compare record that breaks its bar ("" when it does not)."""
    lines = []

    def place(w):
        name = f" ({labels[w['item']]})" if labels else ""
        return (f"item {w['item']}{name} of {w['length']} samples (n % hop = {w['n%hop']}), frame {w['frame']} of {w['frames']}, "
                f"channel {w['channel']}: got log {w['got']:.9g}, ref {w['ref']:.9g}")
    if rec["ratio"] > 1.0:
        lines.append(f"log-mel: amplitude error {rec['err']:.3e} > tol {rec['tol']:.3e} ({rec['ratio']:.3g} bars; float32 port "
                     f"{rec['port_err']:.2e}, frame scale {rec['scale']:.3g}) at {place(rec['where'])}")
    if rec["silent_wrong"]:
        lines.append(f"log-mel: {rec['silent_wrong']} of {rec['silent_frames']} silent frames are not log(eps) exactly; first at "
                     f"{place(rec['silent_where'])}")
    return "\n".join(lines)


# ------------------------------------------------------------------------------------------------------------------------
# RMS normalisation
# ------------------------------------------------------------------------------------------------------------------------
NORM_LENGTHS = [1, 2, 3, 4, 5, 17, 64, 800]
NORM_LEVELS = {"mid": (-5.0, 2.0), "floor": (-20.0, 2.0), "loud": (3.0, 2.0)}


def norm_inputs(level, seed=41, lengths=NORM_LENGTHS, channels=80):
    """mel (B, max length, channels) float32 ~ N(mean, std) of NORM_LEVELS[level]."""
    mean, std = NORM_LEVELS[level]
    return np.random.default_rng(seed).normal(mean, std, size=(len(lengths), max(lengths), channels)).astype(np.float32)


def norm_reference(mel_item, cfg, dtype=np.float64):
    """(mel_norm (T, mel), gain (T hop,)) of one item's mel (T, mel): orc.normalize_inputs_by_rms at the item's own length."""
    mel_item = np.asarray(mel_item, dtype=np.float32)
    T = mel_item.shape[0]
    out, up = orc.normalize_inputs_by_rms(mel_item[None], cfg, T * int(cfg["preprocess_config"]["hop_size"]), dtype=dtype)
    return out[0], up[0]


def pinv_rms_kernel_order(mell, pinv, win_norm, rms_norm_fact):
    """normalize_use_pinv: the frame RMS (T,) summed in float32 in nm_rms_kernel's order: per bin a chain of fused
    multiply-adds over the channels, a lane's running sum over the bins lane, lane + 64, ... (fused), the xor butterfly over
    the 64 lanes.  mell (T, mel) float32, pinv (mel, bins) float32: the table the engine uploads (norm_mel.NormMel.pinv)."""
    f32, f64 = np.float32, np.float64
    lin = np.exp(np.asarray(mell, f32))
    T, K = lin.shape[0], pinv.shape[1]
    v = np.zeros((T, K), f32)
    for ch in range(pinv.shape[0]):
        v = (lin[:, ch:ch + 1].astype(f64) * pinv[ch].astype(f64) + v.astype(f64)).astype(f32)
    v = v * (f32(1.0) / f32(win_norm))
    vp = np.zeros((T, (K + 63) // 64 * 64), f32)
    vp[:, :K] = v
    vp = vp.reshape(T, -1, 64)
    s = np.zeros((T, 64), f32)
    for g in range(vp.shape[1]):
        s = (vp[:, g].astype(f64) * vp[:, g].astype(f64) + s.astype(f64)).astype(f32)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lane ^ o]
    return np.sqrt(s[:, 0] / f32(rms_norm_fact))


def norm_port_kernel_order(mel_item, cfg):
    """The float32 port of a normalize_use_pinv model with the frame RMS summed in the kernel's order."""
    from mbexwn_vocoder_amd.norm_mel import NormMel
    nm = NormMel(cfg)
    rms = pinv_rms_kernel_order(mel_item, nm.pinv, nm.win_norm, nm.rms_norm_fact)
    return norm_port_with_defect(mel_item, cfg, rms=rms)


def norm_port_with_defect(mel_item, cfg, defect=None, rms=None):
    """The float32 port restated with room for a planted defect (without one it reproduces
    orc.normalize_inputs_by_rms(dtype=np.float32)); band-width weighted RMS, or the frame values ``rms`` (T,).  defect: "edge_k_minus_1" (the edge
    extension reads k - 1 instead of k - 2), "gain_one_early" (the output gain read from win / 2 - 1), "sum_not_max"
    (log(m + off) where use_max_limit asks for log(max(m, off)))."""
    dt = np.float32
    pp, mb = cfg["preprocess_config"], cfg["mbexwn_config"]
    hop, win, n_mels = pp["hop_size"], pp.get("win_size", pp["fft_size"]), pp["mel_channels"]
    assert rms is not None or not mb.get("normalize_use_pinv", False)

    def hann(n):
        w = np.zeros(n)
        mid = (n - 1) // 2
        half = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(mid + 1) / (n - 1))
        w[:mid + 1] = half
        w[n - 1:n - 2 - mid:-1] = half
        return w

    def ola(frames):
        n_fr, flen = frames.shape[-2:]
        out = np.zeros(frames.shape[:-2] + ((n_fr - 1) * hop + flen,), dtype=dt)
        for tt in range(n_fr):
            out[..., tt * hop: tt * hop + flen] += frames[..., tt, :]
        return out

    mel_f = orc.slaney_mel_frequencies(n_mels + 2, pp["fmin"], pp["fmax"])
    inv_enorm = ((mel_f[2:] - mel_f[:n_mels]) / 2.0).astype(dt)
    gwin = hann(win).astype(dt)
    gwin = gwin / np.sum(gwin)
    sws = int(win * mb.get("normalize_smooth_win_scale", 1))
    ssw = hann(sws).astype(dt)
    if mb.get("normalize_smooth_with_squared_win", True):
        ssw = ssw ** 2
    mell = np.asarray(mel_item, dtype=dt)[None]
    T = mell.shape[1]
    mel = np.exp(mell)
    if rms is None:
        rms = np.sqrt(np.sum(np.square(mel * inv_enorm), axis=-1) / (pp["fft_size"] * win * 0.5))
    else:
        rms = np.asarray(rms, dt)[None]
    if mb.get("max_norm_fact", None):
        rms = np.maximum(rms, 1.0 / mb["max_norm_fact"])
    if mb.get("normalize_compressor_exp", None) is not None:
        rms = np.power(rms, mb["normalize_compressor_exp"])
    cut = sws // 2 + 2 * hop - win // 2
    norm_gain = ola(np.ones((1, T + 4, 1), dt) * ssw)[:, cut:]
    gain = None
    for _ in range(mb["normalize_rms_num_smooth_iters"]):
        if defect == "edge_k_minus_1":
            ext = np.concatenate((rms[:, :1], rms, rms[:, -1:], rms[:, -1:], rms[:, -1:]), axis=1)
        else:
            ext = np.concatenate((rms[:, :1], rms[:, :1], rms, rms[:, -1:], rms[:, -1:]), axis=1)
        gain = ola(ext[:, :, None] * ssw)[:, cut:] / np.maximum(1e-7, norm_gain)
        n_out = (gain.shape[1] - win) // hop + 1
        idx = np.arange(win)[None, :] + hop * np.arange(n_out)[:, None]
        rms = np.sum(gain[:, idx] * gwin, axis=-1)[:, :T]
    mel = mel / np.maximum(1e-7, rms[:, :, None]) * mb.get("lin_amp_scale", 1.0)
    off = mb.get("lin_amp_off", 1.0e-5)
    if mb.get("use_max_limit", False) and defect != "sum_not_max":
        out = mb.get("mel_amp_scale", 1.0) * np.log(np.maximum(mel, off))
    else:
        out = mb.get("mel_amp_scale", 1.0) * np.log(mel + off)
    first = win // 2 - (1 if defect == "gain_one_early" else 0)
    up = np.maximum(gain[:, first: first + T * hop], 1e-7)
    return out[0].astype(dt), up[0].astype(dt)


def _float_record(err, port_err, amp, floor, k, where):
    tol = max(k * port_err, floor * max(1.0, amp))
    return {"err": err, "tol": tol, "port_err": port_err, "ref_max": amp, "ok": bool(err <= tol), "where": where}


class NormReference:
    """float64 oracle and float32 port of the normalisation for a ragged batch: mel (B, T, mel) float32, lengths in frames."""

    def __init__(self, mel, lengths, cfg, items=None):
        self.mel, self.cfg = np.asarray(mel, np.float32), cfg
        self.lengths = [int(ll) for ll in lengths]
        self.hop = int(cfg["preprocess_config"]["hop_size"])
        self.items = list(range(len(self.lengths))) if items is None else list(items)
        self.ref = {ii: norm_reference(self.mel[ii, :self.lengths[ii]], cfg) for ii in self.items}
        self.port = {ii: norm_reference(self.mel[ii, :self.lengths[ii]], cfg, dtype=np.float32) for ii in self.items}

    def port_result(self, defect=None, only=None):
        """{"mel_norm": (B, T, mel), "gain": (B, T hop)} of the port (NaN behind an item's end); ``defect`` (see
        norm_port_with_defect) planted in the items ``only(length)`` selects (default: all)."""
        B, T = len(self.lengths), max(self.lengths)
        out = {"mel_norm": np.full((B, T, self.mel.shape[-1]), np.nan, np.float32), "gain": np.full((B, T * self.hop), np.nan, np.float32)}
        for ii in self.items:
            ll = self.lengths[ii]
            if defect is not None and (only is None or only(ll)):
                mn, gg = norm_port_with_defect(self.mel[ii, :ll], self.cfg, defect)
            else:
                mn, gg = self.port[ii]
            out["mel_norm"][ii, :ll], out["gain"][ii, :ll * self.hop] = mn, gg
        return out

    def compare(self, got, names=("mel_norm", "gain"), k=K_PORT, f=F_NORM, port=None):
        """got {"mel_norm": (B, >= T, mel), "gain": (B, >= T hop)}: mel_norm on the absolute error, the gain on the relative
        one.  ``port``: another float32 port {item: (mel_norm, gain)} to set the bar from (normalize_use_pinv)."""
        port = self.port if port is None else port
        report = {}
        for name in names:
            worst, port_err, amp, where = -1.0, 0.0, 0.0, None
            for ii in self.items:
                ll = self.lengths[ii]
                idx = 0 if name == "mel_norm" else 1
                ref = np.asarray(self.ref[ii][idx], dtype=np.float64)
                pt = np.asarray(port[ii][idx], dtype=np.float64)
                rows = ll if name == "mel_norm" else ll * self.hop
                g = np.asarray(got[name][ii], dtype=np.float64)[:rows]
                den = np.abs(ref) if name == "gain" else 1.0
                port_err = max(port_err, float((np.abs(pt - ref) / den).max()))
                amp = max(amp, float(np.abs(ref).max()))
                diff = np.abs(g - ref) / den
                diff[~np.isfinite(diff)] = np.inf
                flat = int(np.argmax(diff))
                if diff.flat[flat] > worst:
                    worst = float(diff.flat[flat])
                    row = flat // ref.shape[-1] if name == "mel_norm" else flat
                    where = {"item": ii, "frames": ll, "got": float(g.flat[flat]), "ref": float(ref.flat[flat]),
                             **({"frame": row, "channel": flat % ref.shape[-1]} if name == "mel_norm" else
                                {"sample": row, "frame": row // self.hop, "samples_to_end": rows - row})}
            report[name] = _float_record(worst, port_err, 1.0 if name == "gain" else amp, f, k, where)
            report[name]["ref_max"] = amp
        return report


# ------------------------------------------------------------------------------------------------------------------------
# oscillator and contour
# ------------------------------------------------------------------------------------------------------------------------
def unclamped_top_model(om):
    """(planted defect) the oracle with the grid position not clamped at the last table: above max_tf the weight of the
    last table falls off instead of staying 1."""
    bad = copy.copy(om)
    bad.wt = copy.copy(om.wt)
    bad.wt.max_transposition = np.float32(1e9)
    return bad


def phase_chunk_one_late(om, f0, n_batch_samples, chunk=1000):
    """(planted defect) an item SHORTER than its batch whose chunks end one sample late: the chunk's last running sum, which
    feeds the offset chain, includes the first sample of the next chunk.  Items that fill the batch are not touched."""
    f0 = np.asarray(f0, np.float32)
    if f0.shape[1] >= n_batch_samples:
        return om.phase_from_f0(f0)
    ft = np.float32
    vel = (f0 / ft(om.pulse_rate)).astype(ft)
    n = vel.shape[1]
    vel_p = np.pad(vel, ((0, 0), (0, (-n) % chunk + chunk)))
    n_chunks = (n + chunk - 1) // chunk
    phase = np.zeros((1, n_chunks * chunk), ft)
    off = ft(0)
    for c in range(n_chunks):
        cs = np.cumsum(vel_p[0, c * chunk:(c + 1) * chunk + 1], dtype=ft)
        phase[0, c * chunk:(c + 1) * chunk] = np.mod(cs[:chunk] + np.mod(off, ft(1)), ft(1))
        off = ft(off + np.mod(cs[chunk], ft(1)))
    return phase[:, :n]


PULSE_MODELS = {
    "canon": {},
    "subharm": {"mbexwn_config:wavetable_config:add_subharm_chans": 1},
    "sinfun": {"mbexwn_config:wavetable_config:use_sinusoid_as_fun": True, "mbexwn_config:wavetable_config:add_subharm_chans": 2},
    "white": {"mbexwn_config:wavetable_config:use_white_pulse": True},
}
PULSE_FRAMES = [20, 1, 1, 13, 7, 10, 12, 25, 3, 2]      # item 0: two whole 1000-sample chunks, item 5: exactly one


def pulse_model(name):
    """(cfg, raw weights, WaveTables) of an oscillator variant on the small WaveNet; the tables are built from the
    variant's own wavetable_config (use_white_pulse changes their content)."""
    from mbexwn_vocoder_amd.config import ModelDims, canonical_config
    from mbexwn_vocoder_amd.tables import WaveTables
    from mbexwn_vocoder_amd.weights import synthetic_weights
    cfg = canonical_config("SPEECH", **dict({"mbexwn_config:pp_mod_subnet:n_channels": 32, "mbexwn_config:pp_mod_subnet:n_layers": 3},
                                            **PULSE_MODELS[name]))
    raw = synthetic_weights(cfg, seed=1234, bias_std=0.05, alpha_jitter=0.05)
    return cfg, raw, WaveTables(sample_rate=ModelDims(cfg).pulse_rate, **cfg["mbexwn_config"]["wavetable_config"])


def pulse_values(wt, pulse_rate):
    """The constants of the contours, float32 Hz: every grid point nominalF0 * grid^r with one float32 ulp to either side,
    below min_tf and above max_tf (times nominalF0), 0 Hz, half the pulse rate and the pulse rate itself."""
    vals = []
    for ff in wt.F0_list:
        f = np.float32(ff)
        vals += [np.nextafter(f, np.float32(0)), f, np.nextafter(f, np.float32(np.inf))]
    nominal = float(wt.nominalF0)
    vals += [np.float32(0.5 * float(wt.min_transposition) * nominal), np.float32(1.3 * float(wt.max_transposition) * nominal),
             np.float32(0.0), np.float32(0.5 * pulse_rate), np.float32(pulse_rate)]
    return np.asarray(vals, np.float32)


def pulse_contours(wt, pulse_rate, ppf, frames=PULSE_FRAMES, fill=100.0):
    """(f0 (B, max frames * ppf) float32 Hz, frames): item 0 and item 7 step through every value of pulse_values inside
    their chunks (segments of 40 and of 50 samples), the others hold one value: a grid point, 0 Hz, above max_tf, below
    min_tf, half the pulse rate (phase velocity 0.5), the pulse rate (velocity 1), the top of the grid, and a step 0 Hz ->
    half the pulse rate.  Samples behind an item's end hold ``fill``."""
    vals = pulse_values(wt, pulse_rate)
    n_grid = 3 * len(wt.F0_list)
    below, above, zero, half, full = vals[n_grid:]
    f0 = np.full((len(frames), max(frames) * ppf), fill, np.float32)

    def steps(n, seg, order):
        return np.repeat(order, seg)[np.arange(n) % (seg * len(order))]
    const = {1: vals[3 * 3 + 1], 2: zero, 3: above, 4: below, 5: half, 6: full, 8: vals[n_grid - 2]}
    for ii, ff in enumerate(frames):
        n = ff * ppf
        if ii == 0:
            f0[ii, :n] = steps(n, 40, vals)
        elif ii == 7:
            f0[ii, :n] = steps(n, 50, vals[::-1])
        elif ii == 9:
            f0[ii, :n] = np.where(np.arange(n) < n // 2, zero, half)
        else:
            f0[ii, :n] = const[ii]
    return f0, list(frames)


class PulseReference:
    """OracleModel.wavetable / phase_from_f0 on a contour f0 (B, N) float32 (the engine's own "f0" stage), per item at its
    own number of samples ``samples[i]``."""

    def __init__(self, om64, om32, f0, samples, items=None):
        self.f0, self.samples = np.asarray(f0, np.float32), [int(nn) for nn in samples]
        self.items = list(range(len(self.samples))) if items is None else list(items)
        self.om64, self.om32 = om64, om32
        self.ref = {ii: (om64.wavetable(self.f0[ii:ii + 1, :nn])[0], om64.phase_from_f0(self.f0[ii:ii + 1, :nn])[0])
                    for ii, nn in ((ii, self.samples[ii]) for ii in self.items)}
        self.port = {ii: om32.wavetable(self.f0[ii:ii + 1, :self.samples[ii]])[0] for ii in self.items}

    def port_result(self, model=None, phase_fn=None):
        """{"pulse": (B, N[, channels]), "phase": (B, N)} of the float32 port (NaN behind an item's end); ``model``: another
        float32 OracleModel, ``phase_fn(om, f0_item, N)``: another phase (both plant defects)."""
        om = self.om32 if model is None else model
        B, N = self.f0.shape
        first = np.asarray(self.port[self.items[0]])
        out = {"pulse": np.full((B, N) + first.shape[1:], np.nan, np.float32), "phase": np.full((B, N), np.nan, np.float32)}
        for ii in self.items:
            nn = self.samples[ii]
            f = self.f0[ii:ii + 1, :nn]
            if phase_fn is not None:
                ph = phase_fn(om, f, N)
                bad = copy.copy(om)
                bad.phase_from_f0 = lambda _f, _ph=ph: _ph          # the instance attribute shadows the method
                pulse = bad.wavetable(f)[0]
            else:
                ph, pulse = om.phase_from_f0(f), om.wavetable(f)[0]
            out["pulse"][ii, :nn], out["phase"][ii, :nn] = pulse, ph[0]
        return out

    def compare(self, got, tol=PULSE_TOL):
        """got {"pulse": (B, >= N[, channels]), "phase": (B, >= N) or absent}: the phase bit for bit, the pulse to ``tol``."""
        worst, port_err, amp, where = -1.0, 0.0, 0.0, None
        mism, ph_where = 0, None
        for ii in self.items:
            nn = self.samples[ii]
            ref, ref_ph = self.ref[ii]
            ref = np.asarray(ref, np.float64)
            port_err = max(port_err, float(np.abs(np.asarray(self.port[ii], np.float64) - ref).max()))
            amp = max(amp, float(np.abs(ref).max()))
            g = np.asarray(got["pulse"][ii], np.float64)[:nn].reshape(ref.shape)
            diff = np.abs(g - ref)
            diff[~np.isfinite(diff)] = np.inf
            flat = int(np.argmax(diff))
            if diff.flat[flat] > worst:
                worst = float(diff.flat[flat])
                s = flat // (ref.shape[1] if ref.ndim > 1 else 1)
                where = {"item": ii, "samples": nn, "sample": s, "sample_in_chunk": s % 1000, "samples_to_end": nn - s,
                         "channel": flat % ref.shape[1] if ref.ndim > 1 else 0, "f0": float(self.f0[ii, s]),
                         "got": float(g.flat[flat]), "ref": float(ref.flat[flat])}
            if "phase" in got:
                gp = np.asarray(got["phase"][ii], np.float32)[:nn]
                bad = gp.view(np.uint32) != np.asarray(ref_ph, np.float32).view(np.uint32)
                mism += int(bad.sum())
                if bad.any() and ph_where is None:
                    s = int(np.argmax(bad))
                    ph_where = {"item": ii, "samples": nn, "sample": s, "sample_in_chunk": s % 1000, "chunk": s // 1000,
                                "got": float(gp[s]), "ref": float(ref_ph[s])}
        report = {"pulse": {"err": worst, "tol": tol, "port_err": port_err, "ref_max": amp, "ok": bool(worst <= tol), "where": where}}
        if "phase" in got:
            report["phase"] = {"bit_equal": mism == 0, "mismatch": mism, "ok": mism == 0, "where": ph_where}
        return report


def f0_reference(om64, mel, lengths, items=None):
    """{item: OracleModel.generate_f0 (float64) of the item's own frames (T ppf,)}."""
    items = range(len(lengths)) if items is None else items
    return {ii: om64.generate_f0(np.asarray(mel[ii:ii + 1, :lengths[ii]], np.float64))[0] for ii in items}


def compare_f0(got_f0, ref, lengths, ppf):
    """The engine's "f0" stage (B, T ppf) against f0_reference, in float32 ulps of the reference: {"ulps", "ok" (<= 0.5),
    "where"}; half an ulp plus the float64 rounding of the comparison itself (1e-6 of an ulp)."""
    worst, where = -1.0, None
    for ii, r in ref.items():
        n = lengths[ii] * ppf
        g = np.asarray(got_f0[ii, :n], np.float64)
        ulps = np.abs(g - r) / np.spacing(np.abs(r).astype(np.float32)).astype(np.float64)
        ulps[~np.isfinite(ulps)] = np.inf
        s = int(np.argmax(ulps))
        if ulps[s] > worst:
            worst = float(ulps[s])
            where = {"item": ii, "frames": lengths[ii], "sample": s, "frame": s // ppf, "got": float(g[s]), "ref": float(r[s])}
    return {"ulps": worst, "ok": bool(worst <= 0.5 + 1e-6), "where": where}


# ------------------------------------------------------------------------------------------------------------------------
# reports
# ------------------------------------------------------------------------------------------------------------------------
def failures(report):
    """Readable lines for the records of a NormReference / PulseReference report that break their bar."""
    lines = []
    for name, rec in report.items():
        if rec["ok"]:
            continue
        w = rec.get("where") or {}
        loc = ", ".join(f"{kk} {vv}" for kk, vv in w.items() if kk not in ("got", "ref"))
        if name == "phase":
            lines.append(f"phase: {rec['mismatch']} samples differ in their bits; first at {loc} (got {w.get('got')!r}, ref {w.get('ref')!r})")
        else:
            lines.append(f"{name}: max err {rec['err']:.3e} > tol {rec['tol']:.3e} (float32 port {rec['port_err']:.2e}, |ref| "
                         f"{rec['ref_max']:.3g}) at {loc} (got {w.get('got', float('nan')):.9g}, ref {w.get('ref', float('nan')):.9g})")
    return "\n".join(lines)


def assert_matches(report, what):
    msg = failures(report)
    assert not msg, f"{what} off the float64 oracle:\n" + msg


def record(report):
    """The JSON-able numbers of a report (profiles/frontend_stages.json)."""
    out = {}
    for name, rec in report.items():
        if name == "phase":
            out[name] = {"bit_equal": rec["bit_equal"]}
        else:
            out[name] = {kk: rec[kk] for kk in ("err", "tol", "port_err", "ref_max") if kk in rec}
            out[name]["ratio"] = rec["err"] / rec["tol"] if rec["tol"] > 0 else None
    return out


def oracle_models(cfg, raw, wt):
    return orc.OracleModel(cfg, raw, wt), orc.OracleModel(cfg, raw, wt, dtype=np.float32)
