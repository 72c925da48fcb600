"""References for the per-frame controls where they meet (pitch: mbx_forward_options.f0_frames / f0_scale / f0_item_mask;
formant: env_factor of mbxe_forward, include/mbexwn_envelope.h), shared by tests/test_control_reference.py (CPU),
tests/test_gpu_controls.py and tests/test_gpu_memory_contract.py:

* ``warp_envelope_f64``: THE DEFINITION of include/mbexwn_envelope.h in float64 -- not the float32 restatement
  envelope.warp_envelope_host, which the kernel is bit-equal to and which therefore cannot see an error both share;
* ``controlled_oracle_audio``: the float64 oracle's audio of one item whose excitation and spectral envelope come from other
  rows (the warped ones) than its pitch contour, and ``oracle_contour``, the contour the oracle itself gives an item that keeps
  the F0-net under a transposition;
* ``serve``: one streaming driver for every combination of control rows.
"""
import numpy as np

from oracle import mbexwn_oracle as orc


def warp_envelope_f64(mel, factors, centres, n_frames=None):
    """``mel`` (..., frames, n) rows, ``factors`` (..., frames), ``centres`` (n,) strictly increasing -> the warped rows in
    float64, the inputs taken as the exact numbers they are.  Per frame with factor phi:  phi == 1: the row;  otherwise, per
    channel m, f = c[m] / phi, k = the number of centres <= f; k == 0: x[0]; k == n: x[n - 1]; else i = k - 1,
    w = (f - c[i]) / (c[i + 1] - c[i]), x[i] + w (x[i + 1] - x[i]).  ``n_frames`` (one count per item of a (batch, frames, n)
    input): the rows at or behind an item's count are copies."""
    x = np.asarray(mel, dtype=np.float64)
    c = np.asarray(centres, dtype=np.float64)
    n = c.shape[0]
    assert x.ndim >= 2 and x.shape[-1] == n and n >= 2
    phi = np.broadcast_to(np.asarray(factors, dtype=np.float64), x.shape[:-1])
    keep = phi == 1.0
    if n_frames is not None:
        assert x.ndim == 3
        keep = keep | (np.arange(x.shape[1])[None, :] >= np.asarray(n_frames).reshape(-1, 1))
    out = x.copy()
    for at in zip(*np.nonzero(~keep)):
        row = x[at]
        f = c / phi[at]
        k = np.searchsorted(c, f, side="right")                      # centres <= f
        i = np.clip(k - 1, 0, n - 2)
        w = (f - c[i]) / (c[i + 1] - c[i])
        val = row[i] + w * (row[i + 1] - row[i])
        out[at] = np.where(k == 0, row[0], np.where(k == n, row[n - 1], val))
    return out


class ForceCausalOracle(orc.OracleModel):
    """OracleModel for ``force_causal: true`` (reference custom_pulsed_generator.py:213-217), which the oracle itself does not
    read: the WaveNet pads CAUSAL whatever pp_mod_subnet.padding says (:474-475), every explicit pad of the two sub-nets puts
    its ks - 1 rows in front (same type; :76-79, 93-95, 111-113, 128-130), and the convolutions that pad themselves -- sub-pixel
    layers and the final layer without valid padding -- take Keras "CAUSAL": ks - 1 zeros in front (:53).
    tests/test_control_reference.py holds it to the reference's own float64 run of three force_causal models."""

    def __init__(self, config, raw_weights, wavetables, **kw):
        super().__init__(config, raw_weights, wavetables, **kw)
        assert config["mbexwn_config"].get("force_causal", False)
        self.wn["padding"] = "CAUSAL"

    def run_subnet(self, x, specs, base_name, final_n_channels, final_nks, final_activation, target_ups=None,
                   pad_to_valid=False):
        """OracleModel.run_subnet (custom_pulsed_generator.py:38-148) with force_causal = True."""
        total_ups = 1
        explicit = "EDGE" if pad_to_valid else "SYMMETRIC"
        for ii, spec in enumerate(specs):
            if spec[0] == "L":
                x = orc.lin_interp(x, int(spec[1]), self.f32)
                continue
            ks, up, linear_up = int(spec[0]), 1, False
            if len(spec) > 2:
                if isinstance(spec[2], str):
                    linear_up = spec[2][0] == "L"
                    up = int(spec[2][1:])
                else:
                    up = int(spec[2])
            w, b = self.weight(f"{base_name}_Layer_{ii}")
            front = (ks - 1) // 2 + ((ks - 1) % 2) + (ks - 1) // 2
            if linear_up:
                x = orc.lin_interp(orc.conv1d_valid(orc.pad_time(x, front, 0, explicit), w, b), up, self.f32)
            elif up > 1:
                x = orc.conv1d_valid(orc.pad_time(x, front, 0, "EDGE"), w, b) if pad_to_valid else orc.conv1d_causal(x, w, b)
                x = orc.depth_to_time(x, up)
            else:
                x = orc.conv1d_valid(orc.pad_time(x, front, 0, explicit), w, b)
            if self.use_prelu:
                x = orc.prelu(x, np.asarray(self.raw[f"{base_name}_ActLayer_{ii}.alpha"]).astype(self.dtype))
            else:
                x = np.where(x > 0, x, self.alpha * x)
            total_ups *= up
        if final_nks is not None:
            w, b = self.weight(f"{base_name}_Layer_final")
            if pad_to_valid:
                fk = final_nks
                x = orc.conv1d_valid(orc.pad_time(x, (fk - 1) // 2 + ((fk - 1) % 2) + (fk - 1) // 2, 0, "EDGE"), w, b)
            else:
                x = orc.conv1d_causal(x, w, b)
            if target_ups is not None and total_ups != target_ups:
                up = target_ups // total_ups
                if total_ups * up != target_ups:
                    raise RuntimeError("Upsampling to target upsampling factor is not possible")
                x = orc.lin_interp(x, up, self.f32)
            if final_activation is not None:
                x = orc._FINAL_ACTS[final_activation](x)
        return x


def oracle_model(cfg, raw, wt, **kw):
    """The oracle of a model: OracleModel, or ForceCausalOracle for a force_causal one."""
    causal = bool(cfg["mbexwn_config"].get("force_causal", False))
    return (ForceCausalOracle if causal else orc.OracleModel)(cfg, raw, wt, **kw)


def formant_rows(rng, batch, frames):
    """Formant factors of the control tests: float32 in [0.7, 1.4], another value on every frame, about one frame in five
    exactly 1.0 (the copy without arithmetic)."""
    rows = rng.uniform(0.7, 1.4, size=(batch, frames)).astype(np.float32)
    rows[rng.random(size=(batch, frames)) < 0.2] = np.float32(1.0)
    return rows


def _normalises(cfg):
    return bool(cfg["mbexwn_config"].get("normalize_rms_from_mell", False))


def chain_rows(cfg, mel):
    """The rows the mel-rate chains of the model read, as the oracle computes them, and the gain behind the model: the mel
    itself and None, or -- RMS-normalising model -- the float64 normalisation rounded to float32 and its gain (1, T hop)."""
    mel = np.asarray(mel, dtype=np.float32)
    if not _normalises(cfg):
        return mel, None
    hop = int(cfg["preprocess_config"]["hop_size"])
    rows, gain = orc.normalize_inputs_by_rms(mel, cfg, mel.shape[1] * hop)
    return rows.astype(np.float32), gain


def oracle_contour(cfg, raw, wt, mel, scale=None):
    """The pulse-rate contour (1, T ppf) the float64 oracle gives an item that keeps the F0-net (f0_item_mask 0):
    generate_f0 of the UNWARPED rows (the normalised ones of a normalising model), times the transposition rows ``scale``
    (1, T) brought to the pulse rate by the model's linear interpolator."""
    om = oracle_model(cfg, raw, wt)
    rows, _ = chain_rows(cfg, mel)
    f0 = om.generate_f0(rows.astype(om.dtype))
    if scale is not None:
        li = orc.lin_interp(np.asarray(scale, dtype=np.float32).astype(np.float64)[:, :, None], om.pulse_per_frame)[:, :, 0]
        f0 = f0 * li
    return f0


def controlled_oracle_audio(cfg, raw, wt, mel, noise, contour, env_rows=None):
    """The float64 oracle's audio of one item (1, T hop), composed from OracleModel parts: the excitation (the conditioning of
    every WaveNet block, the sub-band gains) and the spectral envelope read ``env_rows`` -- the rows the chains read after the
    formant shift, (1, T, mel), default: unwarped --, the oscillator and the lifter selection read ``contour`` (1, T ppf; None:
    oracle_contour of ``mel`` without a transposition).  For an RMS-normalising model ``env_rows`` are warped rows of
    chain_rows(cfg, mel)[0], and the gain of that normalisation multiplies the audio."""
    om = oracle_model(cfg, raw, wt)
    T = mel.shape[1]
    rows, gain = chain_rows(cfg, mel)
    env = np.asarray(rows if env_rows is None else env_rows, dtype=np.float32).astype(om.dtype)
    assert env.shape == rows.shape
    if contour is None:
        contour = om.generate_f0(rows.astype(om.dtype))
    contour = np.asarray(contour, dtype=np.float32).astype(np.float64)
    exc = om.generate_excitation(env, contour, noise)
    if om.mb.get("ps_off", False) or not om.mb.get("ps_use_stft", True):
        audio = exc[:, :T * om.hop]
    else:
        out_len = contour.shape[1] * int(om.sample_rate // om.pulse_rate)
        audio = om.istft(om.stft(exc, T) * om.generate_specenv(env, contour), out_len)[:, :T * om.hop]
    return audio if gain is None else audio * gain


def serve(syn, streams, packets, max_ticks=400, join_late=None):
    """Push every stream's frames in packets and tick until all are finished.  streams: {sid: (mel (T, mel), noise, f0 rows or
    None, transposition rows or None, formant rows or None)}; packets(sid) -> frames of the next packet; join_late: {sid: first
    tick}.  Returns ({sid: audio}, the kinds of tick that emitted -- last_tick_layer_rows > 0 --, per tick whether it was a
    replayed graph, None for a tick that emitted nothing)."""
    got = {sid: [] for sid in streams}
    pos = {sid: 0 for sid in streams}
    opened, kinds, replayed = set(), set(), []
    spf = syn.dims.steps_per_frame
    for tick in range(max_ticks):
        for sid, (mel, noise, f0, scale, formant) in streams.items():
            if join_late and tick < join_late.get(sid, 0):
                continue
            if sid not in opened:
                syn.open(sid, f0="net" if f0 is None else "frames")
                opened.add(sid)
            lo = pos[sid]
            if lo < mel.shape[0]:
                hi = min(lo + packets(sid), mel.shape[0])
                syn.push(sid, mel[lo:hi], noise[lo * spf:hi * spf], last=hi == mel.shape[0],
                         f0=None if f0 is None else f0[lo:hi], transposition=None if scale is None else scale[lo:hi],
                         formant=None if formant is None else formant[lo:hi])
                pos[sid] = hi
        out = syn.tick()
        if out:
            kinds.add(syn.last_tick_layer_rows > 0)
        replayed.append(syn.last_tick_replayed if out else None)
        for sid, audio in out.items():
            got[sid].append(np.array(audio))
        if len(opened) == len(streams) and all(syn.finished(sid) for sid in streams):
            break
    return {sid: np.concatenate(vv) for sid, vv in got.items()}, kinds, replayed
