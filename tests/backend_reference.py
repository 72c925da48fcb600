"""Synthesis back-end stage reference and comparator (CPU side, shared by test_backend_reference.py and
test_gpu_backend_stages.py).

The stages behind the WaveNet, and the VTF-net beside it, are compared with the float64 oracle item by item at the item's
own length.  Every stage's oracle input is the engine's own upstream stage, so errors do not compound across stages:

    cepstrum    VTF-net (OracleModel.run_subnet "PS") on the engine's mel (its "mel_norm" stage for RMS-normalising
                models); for sub-band-gain models the M log gains
    ceps_index  OracleModel.cepstral_window_index on the engine's "f0" stage (the contour after transposition or the
                external contour); an integer, held to EQUALITY
    subbands    post-net 1x1 on the engine's "wn_out"; sub-band-gain models: times the interpolated exp gains of the engine's
                "cepstrum" (OracleModel.generate_excitation)
    excitation  OracleModel.pqmf_synthesis of the engine's "subbands" (the reshape for models without PQMF)
    frames      irfft(rfft(hann * excitation frame) * envelope(cepstrum, ceps_index))[:win] * inv_win from the engine's
                "excitation", "cepstrum" and "ceps_index", the excitation zero-padded at the item's own T * hop
    audio       the float32 overlap-add of the engine's "frames" in frame order, as overlap_add_kernel adds them: the SAME
                BITS over the item, exact zeros behind its end; RMS-normalising models multiply the normalisation gain
                (oracle normalize_inputs_by_rms on the item's own mel), held to the float32-port bar; models without an
                envelope (ps_off, sub-band gains): the audio is the excitation, bit for bit

Float stages are held to

    tol = max(K * port_err, F * max(1, |ref|))

with port_err the max error of the float32 port (OracleModel(dtype=np.float32), numpy's float32 FFTs) on the same inputs
and |ref| the stage's largest magnitude.  K = 8 as in wn_reference.py.  The floors F were calibrated against the planted
defects of test_backend_reference.py (canonical SPEECH), each of which moves the audio by less than the end-to-end bar
1e-4 * max(1, |audio|) and the excitation by less than 2e-5 * max(1, |excitation|):

    cepstrum    F = 2e-7   coefficient 200 of one frame scaled by 1 + 1e-4 moves the cepstrum by 1.7e-5 (|ref| 0.29); the
                           float32 port's own error, 1.4e-7, sets the bar at 1.1e-6
    subbands    F = 5e-7   the post-net losing 30 % of the bias of one band: 1.1e-5; the floor sets the bar (port 4e-8)
    excitation  F = 5e-7   a short item's PQMF reading one step past its end at 2e-5 of a row's size: 7e-6 in its last
                           samples; the port (1.7e-7) sets the bar at 1.3e-6
    frames      F = 5e-7   an item's frames seeing the excitation up to the batch length (1/1000 of the PQMF ring-out there):
                           3.5e-5 in its last frame; the port (3.7e-7) sets the bar at 3e-6
    audio       F = 5e-7   RMS-normalising models only (an overlap-add is held bit for bit; the gain is the oracle's)

so every bar is at least 5x below its smallest defect.  On an MI355X the engine stays at or below 0.49 of the bar in every
case of test_gpu_backend_stages.py (subgain's excitation; profiles/backend_stages.json).

ceps_index: the kernel sums the 2 hop + 1 taps of the F0 smoother in float32 (strided partial sums, a shuffle reduction),
the oracle in float64.  Rounded to float32, pos = ratio * 29 carries ~10.7 * (relative error of the smoothed F0); a float32
sum of 601 positive terms is good to a few 1e-6 relative, so the positions agree to ~3e-5.  EPS_POS = 2^-13 (1.2e-4, 64
float32 ulps of 29) excuses a frame whose oracle position lies within EPS_POS of a half-integer: there either neighbour is
accepted.  The comparator counts the excused frames; more than MAX_EXCUSED_FRACTION (3 %) of a case's frames fails it (on
an MI355X no frame of any case needed the excuse).
"""
import types

import numpy as np

from oracle import mbexwn_oracle as orc

K_PORT = 8.0
F_FLOOR = {"cepstrum": 2e-7, "subbands": 5e-7, "excitation": 5e-7, "frames": 5e-7, "audio": 5e-7}
EPS_POS = 2.0 ** -13
MAX_EXCUSED_FRACTION = 0.03
N_LIFTER_ROWS = 30


# ------------------------------------------------------------------------------------------------------------------------
# model kind (what the engine runs behind the WaveNet)
# ------------------------------------------------------------------------------------------------------------------------
def backend_kind(dims, cfg):
    """The back-end branches a model takes, from ModelDims / config with the conditions of csrc/mbx_forward.hip (run_backend),
    csrc/stft_filter.hip::launch_stft_filter and csrc/pqmf.hip::launch_pqmf:
    {"envelope": STFT-domain filter, "lifter": lifter row selected in the kernel, "stft": "wave10_2" | "wave16_16" | "generic" |
     None, "pqmf": "mfma" | "generic" | "reshape", "gain": sub-band gains, "norm": RMS normalisation, "tail": "fused" |
     "unfused"}."""
    mb = cfg["mbexwn_config"]
    M = dims.subbands
    envelope = not dims.no_envelope
    lifter = bool(dims.ps_env_order_scale) and not mb.get("psns_use_cepstral_loss_constraint", False) and envelope
    stft = None
    if envelope:
        if dims.fft_size == 2048 and dims.stft_win <= dims.fft_size and dims.stft_win % 2 == 0:
            stft = "wave10_2" if dims.stft_win <= 1280 and dims.n_ceps <= 256 else "wave16_16"
        else:
            stft = "generic"
    if dims.no_pqmf:
        pqmf = "reshape"
    else:
        # polyphase taps per phase (csrc/mbx_create.hip, tables.pqmf_polyphase): n_dm = 2 ceil((taps / 2) / M) + 1
        half = int(mb["multi_band_config"]["taps"]) // 2
        n_dm = 2 * ((half + M - 1) // M) + 1
        pqmf = "generic" if M > 16 or n_dm * M > 4 * 48 else "mfma"
    # the end + post-net convolutions run fused when the tail fits launch_wn_tail (csrc/wn_tail.hip: at most 32 output
    # channels and 16 bands, C % 4 == 0), else as two plain convolutions.  "fused" does not tell apart the kernels behind it
    # (wn_tail2_kernel<NJ>, the per-row wn_tail_kernel for C < 16 or more than 352 channels, the folded skip path)
    tail = "fused" if dims.wn_out_channels <= 32 and M <= 16 and dims.wn_channels % 4 == 0 else "unfused"
    return {"envelope": envelope, "lifter": lifter, "stft": stft, "pqmf": pqmf, "gain": bool(dims.ps_subband_gain),
            "norm": bool(dims.normalize_rms_from_mell), "tail": tail}


# ------------------------------------------------------------------------------------------------------------------------
# the oracle's stages, one item at its own length
# ------------------------------------------------------------------------------------------------------------------------
def oracle_cepstrum(om, mel, dims):
    """VTF-net output (T, n_ceps) of one item's mel (T, mel_channels); sub-band-gain models: the M log gains."""
    n_out = dims.subbands if dims.ps_subband_gain else om.n_ceps
    x = om.run_subnet(np.asarray(mel)[None].astype(om.dtype), om.ps_specs, "PS", n_out, 1, None, pad_to_valid=om.ps_valid)
    return x[0]


def oracle_ceps_index(om, f0):
    """(index (T,), position (T,)) of one item's contour f0 (T * pulse_per_frame,)."""
    idx, pos = om.cepstral_window_index(np.asarray(f0)[None], return_position=True)
    return idx[0], pos[0].astype(np.float64)


def oracle_subbands(om, wn_out, ceps, dims, drop_bias=None):
    """Post-net (rows, M) of one item's WaveNet output (rows, n_out); sub-band gains from its cepstrum stage (T, M).
    drop_bias (test instrument): a band whose post-net bias is left out, or (band, fraction) for a part of it."""
    w, b = om.weight("post")
    if drop_bias is not None:
        band, frac = drop_bias if isinstance(drop_bias, tuple) else (drop_bias, 1.0)
        b = np.array(b)
        b[band] -= b.dtype.type(frac) * b[band]
    y = orc.conv1d_valid(np.asarray(wn_out)[None].astype(om.dtype), w, b)
    if dims.ps_subband_gain:
        lg = np.asarray(ceps)[None].astype(om.dtype)
        if om.preserve_energy:
            lg = lg - np.mean(lg, axis=-1, keepdims=True)
        gain = orc.lin_interp(np.exp(lg), om.hop, om.f32)
        y = y * gain[:, :y.shape[1]]
    return y[0]


def oracle_excitation(om, sub, dims):
    """PQMF synthesis (T * hop,) of one item's sub-band rows (rows, M); the reshape for models without PQMF."""
    x = np.asarray(sub)[None].astype(om.dtype)
    if dims.no_pqmf:
        return x.reshape(-1)
    return om.pqmf_synthesis(x)[0]


def oracle_frames(om, exc, ceps, idx, T, signal_len=None):
    """The T filtered STFT frames (T, win) of one item: frame t = irfft(rfft(hann * s[t hop - win/2 ...]) * H_t)[:win] *
    inv_win, with s the excitation zero-padded at the item's own T * hop (signal_len: test instrument, the samples of exc
    the frames may see) and H_t the envelope of cepstrum frame t (lifter row idx[t]; OracleModel.generate_specenv)."""
    dt = om.dtype
    win, hop, nfft = om.stft_win, om.hop, om.fft_size
    n_sig = T * hop if signal_len is None else signal_len
    sig = np.zeros(win // 2 + max(n_sig, T * hop) + win, dtype=dt)
    sig[win // 2: win // 2 + n_sig] = np.asarray(exc, dtype=dt)[:n_sig]
    pos = hop * np.arange(T)[:, None] + np.arange(win)[None, :]
    spec = np.fft.rfft(sig[pos] * om.hann, n=nfft, axis=-1)
    c = np.asarray(ceps, dtype=dt)[:T]
    if om.env_scale and not om.use_ceps_constraint:
        c = c * om.ceps_windows[np.asarray(idx)[:T]]
    full = np.zeros((T, nfft), dtype=dt)
    first = 0 if om.preserve_energy else 1
    full[:, first:om.n_ceps] = c[:, first:om.n_ceps]
    s = np.fft.rfft(full, axis=-1)
    if om.max_log_range:
        env = np.exp(dt(om.max_log_range) * np.tanh(s.real) + 1j * s.imag)
    else:
        env = np.exp(s)
    if om.preserve_energy:
        env = env / np.sqrt(np.mean(np.square(np.abs(env)), axis=-1, keepdims=True))
    return np.fft.irfft(spec * env.astype(spec.dtype), n=nfft, axis=-1)[:, :win] * om.inv_win


def overlap_add_f32(frames, T, hop):
    """float32 overlap-add of frames (T, win) in frame order from 0.f, sliced [win/2, win/2 + T hop): what
    overlap_add_kernel computes, so bit for bit."""
    frames = np.asarray(frames, dtype=np.float32)
    win = frames.shape[-1]
    sig = np.zeros((T - 1) * hop + win, dtype=np.float32)
    for t in range(T):
        sig[t * hop: t * hop + win] += frames[t]
    return sig[win // 2: win // 2 + T * hop]


# ------------------------------------------------------------------------------------------------------------------------
# the engine's stages
# ------------------------------------------------------------------------------------------------------------------------
def engine_backend_stages(eng, B, T):
    """The stages of the engine's last forward that the back-end comparison reads, as numpy arrays:
    mel_in (B, T, mel) only for RMS-normalising models, f0 (B, T ppf), wn_out (B, T spf, n_out), cepstrum (B, T, n_ceps),
    ceps_index (B, T) (only with a lifter), subbands (B, T spf, M), excitation (B, T hop), frames (B, T, win) (only with
    an envelope)."""
    d = eng.dims
    kind = backend_kind(d, eng.config)
    spf = d.steps_per_frame
    out = {"f0": eng.stage("f0").cpu().numpy().reshape(B, T * d.pulse_per_frame),
           "wn_out": eng.stage("wn_out").cpu().numpy().reshape(B, T * spf, d.wn_out_channels),
           "subbands": eng.stage("subbands").cpu().numpy().reshape(B, T * spf, d.subbands),
           "excitation": eng.stage("excitation").cpu().numpy().reshape(B, T * d.hop_size)}
    if not d.ps_off:
        out["cepstrum"] = eng.stage("cepstrum").cpu().numpy().reshape(B, T, d.n_ceps)
    if kind["norm"]:
        out["mel_in"] = eng.stage("mel_norm").cpu().numpy().reshape(B, T, d.mel_channels)
    if kind["lifter"]:
        out["ceps_index"] = eng.stage("ceps_index").cpu().numpy().reshape(B, T)
    if kind["envelope"]:
        out["frames"] = eng.stage("frames").cpu().numpy().reshape(B, T, d.stft_win)
    return out


def port_backend_stages(om, mel, noise, lengths, f0=None):
    """The same stages computed by the float32 port on the CPU (a stand-in for the engine in the CPU tests), per item at
    its own length and laid out as a ragged batch (rows behind an item's end hold NaN).  Single-block models with the
    plain pulse channels (no pulse PQMF).  f0: optional external contour (B, T ppf)."""
    d_hop, spf, M = om.hop, om.steps_per_frame, om.M
    B, T = len(lengths), max(lengths)
    win = om.stft_win
    n_ceps = M if _subband_gain(om) else om.n_ceps
    nan = np.float32(np.nan)
    # the ModelDims fields the oracle stage functions read
    kind = types.SimpleNamespace(ps_subband_gain=_subband_gain(om), no_pqmf=not om.mb.get("pp_mod_subnet_use_pqmf", True))
    out = {"f0": np.full((B, T * om.pulse_per_frame), nan, np.float32),
           "wn_out": np.full((B, T * spf, int(om.wn["n_out_channels"])), nan, np.float32),
           "cepstrum": np.full((B, T, n_ceps), nan, np.float32),
           "ceps_index": np.zeros((B, T), np.int32),
           "subbands": np.full((B, T * spf, M), nan, np.float32),
           "excitation": np.full((B, T * d_hop), nan, np.float32),
           "frames": np.full((B, T, win), nan, np.float32),
           "audio": np.zeros((B, T * d_hop), np.float32)}
    for ii, ll in enumerate(lengths):
        m = np.asarray(mel[ii:ii + 1, :ll], dtype=np.float32)
        f = om.generate_f0(m) if f0 is None else np.asarray(f0[ii:ii + 1, :ll * om.pulse_per_frame], np.float32)
        f = f.astype(np.float32)
        out["f0"][ii, :f.shape[1]] = f[0]
        pulse = om.wavetable(f)
        x = pulse.reshape(1, -1, om.pulse_channels).astype(np.float32)
        if om.sigma:
            x = np.concatenate((x, om.sigma * np.asarray(noise[ii:ii + 1, :ll * spf, None], np.float32)), axis=-1)
        wn = om.wavenet(x, m).astype(np.float32)
        out["wn_out"][ii, :ll * spf] = wn[0]
        ce = om.run_subnet(m, om.ps_specs, "PS", n_ceps, 1, None, pad_to_valid=om.ps_valid).astype(np.float32)[0]
        out["cepstrum"][ii, :ll] = ce
        idx = None
        if om.env_scale and not om.use_ceps_constraint:
            idx = om.cepstral_window_index(f)[0]
            out["ceps_index"][ii, :ll] = idx
        sub = oracle_subbands(om, wn[0], ce, kind).astype(np.float32)
        out["subbands"][ii, :ll * spf] = sub
        exc = oracle_excitation(om, sub, kind).astype(np.float32)
        out["excitation"][ii, :ll * d_hop] = exc
        fr = oracle_frames(om, exc, ce, idx, ll).astype(np.float32)
        out["frames"][ii, :ll] = fr
        out["audio"][ii, :ll * d_hop] = overlap_add_f32(fr, ll, d_hop)
    return out


def _subband_gain(om):
    return not om.mb.get("ps_use_stft", True) and not om.mb.get("ps_off", False)


# ------------------------------------------------------------------------------------------------------------------------
# the comparator
# ------------------------------------------------------------------------------------------------------------------------
def _where_float(stage, ii, flat, shape, g, ref, n_rows, dims):
    """Location of the worst element of a float stage, with the position in the tile that computes it."""
    row, ch = divmod(flat, shape[-1]) if len(shape) > 1 else (flat, 0)
    w = {"stage": stage, "item": ii, "got": float(g.flat[flat]), "ref": float(ref.flat[flat])}
    if stage == "cepstrum":
        # mel-rate convolution tiles: 128 output columns (conv_mel.hip); frames are the rows
        w.update(frame=row, coefficient=ch, column_tile=ch // 128, column_in_tile=ch % 128, frame_in_64=row % 64,
                 frames_to_end=n_rows - row)
    elif stage == "subbands":
        w.update(row=row, band=ch, row_in_256=row % 256, frame=row // dims.steps_per_frame, rows_to_end=n_rows - row)
    elif stage == "excitation":
        M = dims.subbands
        w.update(sample=row, step=row // M, phase=row % M, step_in_block=(row // M) % 64, samples_to_end=n_rows - row)
    elif stage == "frames":
        w.update(frame=row, sample_in_frame=ch, frame_in_block=row % 4, frames_to_end=n_rows - row)
    elif stage == "audio":
        w.update(sample=row, frame=row // dims.hop_size, samples_to_end=n_rows - row)
    return w


class BackendReference:
    """float64 oracle and float32 port of the back-end stages for the items ``items`` of a ragged batch, fed the engine's
    own upstream stages.

    om64 / om32: OracleModel of the same weights in float64 / float32; dims: ModelDims; got: the engine's stages
    (engine_backend_stages or port_backend_stages); mel: the batch's mel (B, T, mel_channels) (the VTF-net input unless
    got holds "mel_in"); lengths: frames per item."""

    def __init__(self, om64, om32, dims, cfg, got, mel, lengths, items=None):
        self.om64, self.om32, self.dims, self.cfg = om64, om32, dims, cfg
        self.kind = backend_kind(dims, cfg)
        self.lengths = [int(ll) for ll in lengths]
        self.items = list(range(len(self.lengths))) if items is None else list(items)
        self.mel = np.asarray(got["mel_in"] if "mel_in" in got else mel, dtype=np.float32)
        self.raw_mel = np.asarray(mel, dtype=np.float32)
        self.ref = {ii: self._stages(om64, got, ii) for ii in self.items}
        self.port = {ii: self._stages(om32, got, ii) for ii in self.items}

    def rows(self, stage, ii):
        d, T = self.dims, self.lengths[ii]
        return {"cepstrum": T, "ceps_index": T, "subbands": T * d.steps_per_frame, "excitation": T * d.hop_size,
                "frames": T, "audio": T * d.hop_size}[stage]

    def stages(self):
        k = self.kind
        names = ["subbands", "excitation"]
        if not self.dims.ps_off:
            names.insert(0, "cepstrum")
        if k["lifter"]:
            names.insert(1, "ceps_index")
        if k["envelope"]:
            names.append("frames")
        return names

    def _stages(self, om, got, ii):
        """The oracle's stages of item ii in om's dtype from the engine's upstream stages ``got``."""
        d, T = self.dims, self.lengths[ii]
        out = {}
        ce = None
        if not d.ps_off:
            out["cepstrum"] = oracle_cepstrum(om, self.mel[ii, :T], d)
            ce = np.asarray(got["cepstrum"][ii, :T])
        if self.kind["lifter"]:
            out["ceps_index"], out["ceps_pos"] = oracle_ceps_index(om, np.asarray(got["f0"][ii, :T * d.pulse_per_frame]))
        out["subbands"] = oracle_subbands(om, np.asarray(got["wn_out"][ii, :T * d.steps_per_frame]), ce, d)
        out["excitation"] = oracle_excitation(om, np.asarray(got["subbands"][ii, :T * d.steps_per_frame]), d)
        if self.kind["envelope"]:
            idx = np.asarray(got["ceps_index"][ii, :T]) if self.kind["lifter"] else None
            out["frames"] = oracle_frames(om, np.asarray(got["excitation"][ii]), ce, idx, T)
        if self.kind["norm"]:
            out["norm_gain"] = orc.normalize_inputs_by_rms(self.raw_mel[ii:ii + 1, :T], self.cfg, T * d.hop_size,
                                                           dtype=om.dtype)[1][0]
        return out

    def compare(self, got, names=None, k=K_PORT, f=None):
        """Per stage of ``names`` (default: every stage of this model plus the audio when ``got`` holds it): a record with
        "ok" False where the stage breaks its bar and "where" locating the worst element.  got: {stage: (B, ...) arrays}."""
        f = dict(F_FLOOR, **(f or {}))
        if names is None:
            names = self.stages() + (["audio"] if "audio" in got else [])
        report = {}
        for name in names:
            if name == "ceps_index":
                report[name] = self._compare_index(got)
            elif name == "audio":
                report[name] = self._compare_audio(got, k, f["audio"])
            else:
                report[name] = self._compare_float(got, name, k, f[name])
        return report

    def _compare_float(self, got, name, k, floor):
        worst, port_err, amp, where = -1.0, 0.0, 0.0, None
        for ii in self.items:
            n = self.rows(name, ii)
            ref = np.asarray(self.ref[ii][name], dtype=np.float64)
            port = np.asarray(self.port[ii][name], dtype=np.float64)
            port_err = max(port_err, float(np.abs(port - ref).max()))
            amp = max(amp, float(np.abs(ref).max()))
            g = np.asarray(got[name][ii], dtype=np.float64)[:n]
            if g.shape != ref.shape:
                raise AssertionError(f"{name} item {ii}: engine shape {g.shape} against the oracle's {ref.shape}")
            diff = np.abs(g - ref)
            diff[~np.isfinite(diff)] = np.inf
            flat = int(np.argmax(diff))
            err = float(diff.flat[flat])
            if err > worst:
                worst = err
                where = _where_float(name, ii, flat, ref.shape, g, ref, n, self.dims)
        tol = max(k * port_err, floor * max(1.0, amp))
        return {"err": worst, "tol": tol, "port_err": port_err, "ref_max": amp, "ok": bool(worst <= tol), "where": where}

    def _compare_index(self, got):
        """Lifter rows: equal to the oracle's, or either neighbour where the oracle's position is within EPS_POS of a
        half-integer.  Also reports which rows and clamp ends the checked items select."""
        frames = excused = 0
        where, bad = None, 0
        rows, lo_clamp, hi_clamp = set(), 0, 0
        for ii in self.items:
            T = self.lengths[ii]
            ref, pos = self.ref[ii]["ceps_index"], self.ref[ii]["ceps_pos"]
            g = np.asarray(got["ceps_index"][ii][:T]).astype(np.int64)
            frames += T
            rows.update(int(r) for r in ref)
            lo_clamp += int(np.sum(pos == 0.0))
            hi_clamp += int(np.sum(pos == float(N_LIFTER_ROWS - 1)))
            near = np.abs(pos - np.floor(pos) - 0.5) < EPS_POS
            ok = (g == ref) | (near & ((g == np.floor(pos)) | (g == np.floor(pos) + 1)))
            excused += int(np.sum(near & (g != ref) & ok))
            if not ok.all():
                t = int(np.argmax(~ok))
                bad += int(np.sum(~ok))
                if where is None:
                    where = {"stage": "ceps_index", "item": ii, "frame": t, "got": int(g[t]), "ref": int(ref[t]),
                             "pos": float(pos[t]), "frame_in_block": t % 4, "frames_to_end": T - t}
        ok = bad == 0 and excused <= MAX_EXCUSED_FRACTION * max(frames, 1)
        return {"mismatch": bad, "excused": excused, "frames": frames, "ok": bool(ok), "where": where,
                "rows": sorted(rows), "low_clamp_frames": lo_clamp, "high_clamp_frames": hi_clamp}

    def _compare_audio(self, got, k, floor):
        """The engine's audio against the overlap-add of its own frames: bit for bit (times the normalisation gain at the
        port bar for RMS-normalising models); models without an envelope: the excitation, bit for bit.  Exact zeros behind
        every item's end."""
        d = self.dims
        worst, where, port_err, amp, bits = 0.0, None, 0.0, 0.0, True
        for ii in self.items:
            T, n = self.lengths[ii], self.lengths[ii] * d.hop_size
            a = np.asarray(got["audio"][ii], dtype=np.float32)
            tail = a[n:]
            if tail.size and not np.all(tail == 0.0):
                s = int(np.argmax(tail != 0.0))
                return {"ok": False, "bit_equal": False, "err": float("inf"), "tol": 0.0,
                        "where": {"stage": "audio", "item": ii, "sample": n + s, "samples_to_end": -s,
                                  "got": float(tail[s]), "ref": 0.0, "behind_the_end": True}}
            base = (overlap_add_f32(got["frames"][ii, :T], T, d.hop_size) if self.kind["envelope"]
                    else np.asarray(got["excitation"][ii, :n], dtype=np.float32))
            if self.kind["norm"]:
                ref = base.astype(np.float64) * self.ref[ii]["norm_gain"]
                port = (base * self.port[ii]["norm_gain"].astype(np.float32)).astype(np.float64)
                port_err = max(port_err, float(np.abs(port - ref).max()))
                amp = max(amp, float(np.abs(ref).max()))
                diff = np.abs(a[:n].astype(np.float64) - ref)
                diff[~np.isfinite(diff)] = np.inf
                flat = int(np.argmax(diff))
                if diff[flat] > worst or where is None:
                    worst = float(diff[flat])
                    where = _where_float("audio", ii, flat, ref.shape, a[:n].astype(np.float64), ref, n, d)
            else:
                same = a[:n].view(np.uint32) == base.view(np.uint32)
                if not same.all():
                    s = int(np.argmax(~same))
                    diff = float(abs(float(a[s]) - float(base[s])))
                    if bits or diff > worst:
                        worst = diff if np.isfinite(diff) else float("inf")
                        where = _where_float("audio", ii, s, (n,), a[:n].astype(np.float64), base.astype(np.float64), n, d)
                    bits = False
        if self.kind["norm"]:
            tol = max(k * port_err, floor * max(1.0, amp))
            return {"ok": bool(worst <= tol), "bit_equal": None, "err": worst, "tol": tol, "port_err": port_err,
                    "ref_max": amp, "where": where}
        return {"ok": bits, "bit_equal": bits, "err": worst, "tol": 0.0, "where": where}


def failures(report):
    """Readable lines for the stages of a compare() report that break their bar ("" when none does)."""
    lines = []
    for name, rec in report.items():
        if rec["ok"]:
            continue
        w = rec.get("where") or {}
        loc = ", ".join(f"{kk} {vv}" for kk, vv in w.items() if kk not in ("stage", "got", "ref"))
        if name == "ceps_index":
            lines.append(f"ceps_index: {rec['mismatch']} frames select another lifter row than the oracle, {rec['excused']} of "
                         f"{rec['frames']} excused at a half-integer position (at most {MAX_EXCUSED_FRACTION:.0%}); first at "
                         f"{loc} (got row {w.get('got')}, oracle row {w.get('ref')})")
        elif name == "audio" and rec.get("bit_equal") is not None:
            lines.append(f"audio: not the bit-exact overlap-add of the engine's own frames: |diff| {rec['err']:.3e} at {loc} "
                         f"(got {w.get('got')!r}, expected {w.get('ref')!r})")
        else:
            lines.append(f"{name}: max err {rec['err']:.3e} > tol {rec['tol']:.3e} (float32 port {rec.get('port_err', 0):.2e}, "
                         f"|ref| {rec.get('ref_max', 0):.3g}) at {loc} (got {w.get('got', float('nan')):.9g}, ref "
                         f"{w.get('ref', float('nan')):.9g})")
    return "\n".join(lines)


def summary(report):
    parts = []
    for name, rec in report.items():
        if name == "ceps_index":
            parts.append(f"ceps_index {rec['mismatch']} off / {rec['excused']} excused / {rec['frames']}")
        elif name == "audio" and rec.get("bit_equal") is not None:
            parts.append(f"audio {'bit-equal' if rec['bit_equal'] else 'DIFFERS'}")
        else:
            parts.append(f"{name} {rec['err']:.2e}/{rec['tol']:.2e}")
    return "  ".join(parts)


def record(report):
    """The JSON-able numbers of a report (profiles/backend_stages.json)."""
    out = {}
    for name, rec in report.items():
        if name == "ceps_index":
            out[name] = {kk: rec[kk] for kk in ("mismatch", "excused", "frames", "low_clamp_frames", "high_clamp_frames")}
            out[name]["rows"] = len(rec["rows"])
        elif name == "audio" and rec.get("bit_equal") is not None:
            out[name] = {"bit_equal": rec["bit_equal"]}
        else:
            out[name] = {kk: rec[kk] for kk in ("err", "tol", "port_err", "ref_max")}
            out[name]["ratio"] = rec["err"] / rec["tol"] if rec["tol"] > 0 else None
    return out


def assert_matches(report):
    msg = failures(report)
    assert not msg, "back-end stage off the float64 oracle:\n" + msg


def oracle_models(cfg, raw, wt):
    return orc.OracleModel(cfg, raw, wt), orc.OracleModel(cfg, raw, wt, dtype=np.float32)
