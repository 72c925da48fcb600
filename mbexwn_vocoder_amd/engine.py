"""Host-side driver of the HIP engine (include/mbexwn.h) on top of its ctypes binding, abi.py.

``MBExWNEngine`` plays the role of the reference's Keras model object: it is what
``MELInverter.model`` holds and what ``model.infer(mell, synth_length=...)`` is called on
(reference MBExWN_NVoc/mel_inverter.py:151-154, MBExWN_NVoc/vocoder/model/wavegen_1d.py:483-526).
PyTorch is used for device memory and streams only.

There is NO CPU fallback: the engine refuses to load without the compiled HIP library, and refuses
to run without a GPU.
"""
import ctypes
import os

import numpy as np

from . import tables as tb
# the binding itself (structures, constants, the function table, load_library) is abi.py; its names stay importable from here
from .abi import (CONV_FORMS, GATE_KERNEL_NAMES, MBX_ABI_VERSION, MBX_MAX_PRECOND, MBX_MAX_SUBNET_OPS,  # noqa: F401
                  MBX_MAX_WN_BLOCKS, MBX_MAX_WN_LAYERS, MBX_NAME_LEN, RESSKIP_KERNEL_NAMES, TAIL_KERNEL_NAMES, _check,
                  load_library, mbx_config, mbx_conv_form_info, mbx_forward_options, mbx_kernel_report_info, mbx_plan_info,
                  mbx_subnet_op, mbx_tensor, symbols)
from .build import LIB_PATH  # noqa: F401
from .config import ModelDims
from .flac import EncodedFlac  # noqa: F401  (what encode_flac16 returns; the name stays importable from here)
# the weight images are packing.py; its public names stay importable from here (tensor_table is what the engine itself calls)
from .packing import (fold_skip_weights, fold_start_weights, pack_end_weights, pack_gate_f16_weights,  # noqa: F401
                      pack_resskip_f16_weights, pack_resskip_wave_weights, pack_resskip_weights, pack_resskip_wide_weights,
                      pack_winograd2w_weights, pack_winograd4w_weights, tensor_table)
from .subnet import build_subnet

# what the build hook checks in the library: the functions of include/mbexwn.h and include/mbexwn_audio.h (abi.TABLE)
EXPORTED_SYMBOLS = symbols("mbexwn.h")
AUDIO_SYMBOLS = symbols("mbexwn_audio.h")

_CONV_FORM_NAMES = {vv: kk for kk, vv in CONV_FORMS.items()}

_OP_KIND = {"conv": 0, "lin": 1, "prelu": 2, "leaky": 3, "act": 4}
_ACT = {"linear": 0, "soft_sigmoid": 1, "tanh": 2, "sigmoid": 3, "soft_sign": 4, "soft_sqrt": 5, "exp": 6, "relu": 7}


# ------------------------------------------------------------------------------------------------
# host-side model description
# ------------------------------------------------------------------------------------------------
def subnet_ops(config):
    """(f0 ops, vtf ops): the reference's sub-net grammar flattened (see subnet.build_subnet)."""
    dims = ModelDims(config)
    mb = config["mbexwn_config"]
    use_prelu = mb.get("use_prelu", True)
    f0_ops, _, _ = build_subnet(mb["pp_subnet"], "PulsPar", dims.mel_channels, 1, 1,
                                mb.get("pp_activation", "soft_sigmoid"), target_ups=dims.pulse_per_frame,
                                pad_to_valid=mb.get("pp_subnet_use_valid_padding", False),
                                remove_inactive_pad_layers=mb.get("remove_inactive_pad_layers", False),
                                use_prelu=use_prelu, alpha=dims.alpha, force_causal=mb.get("force_causal", False))
    vtf_ops = []
    if not dims.ps_off:
        vtf_ops, _, _ = build_subnet(mb["ps_subnet"], "PS", dims.mel_channels, dims.n_ceps, 1, None,
                                     pad_to_valid=mb.get("ps_subnet_use_valid_padding", False),
                                     remove_inactive_pad_layers=mb.get("remove_inactive_pad_layers", False),
                                     use_prelu=use_prelu, alpha=dims.alpha, force_causal=mb.get("force_causal", False))
    return f0_ops, vtf_ops


def _fill_ops(dst, ops):
    if len(ops) > MBX_MAX_SUBNET_OPS:
        raise ValueError("sub-net too deep for the engine")
    for ii, op in enumerate(ops):
        cop = dst[ii]
        cop.kind = _OP_KIND[op["kind"]]
        cop.ks = op.get("ks", 0)
        cop.cin = op.get("cin", 0)
        cop.cout = op.get("cout", 0)
        cop.pad_l = op.get("pad_l", 0)
        cop.pad_r = op.get("pad_r", 0)
        cop.pad_mode = op.get("pad_mode", 0)
        cop.up = op.get("up", 1)
        if op["kind"] == "act":
            if op["fn"] not in _ACT:
                raise RuntimeError(f"ActivationLayer::error::unkown activation selected {op['fn']}")
            cop.act = _ACT[op["fn"]]
        cop.alpha = op.get("alpha", 0.0)
        cop.name = op.get("name", "").encode()
    return len(ops)


def experiment_overrides():
    """The MBX_* environment variables of the experiment scripts and fuzzers, mapped onto the mbx_config policy fields
    (the library itself reads no environment variable): MBX_WINOGRAD=0|2|4|44 -> conv_form direct / f23 / f43 / f43 +
    batch_invariant, MBX_FOLD_SKIP=0 / MBX_FOLD_START=0 -> keep_skip / keep_start, MBX_WG_SMALL=0|1 -> tune_gate_shape 1|2,
    MBX_RV_TILES=n -> tune_resskip_wave_tiles (0 = never), MBX_RV_SPLIT=1|2|3 -> tune_resskip_split.  Only consulted for
    policy arguments the caller left unset, and only when the process opts in with MBX_EXPERIMENT=1 (the experiment scripts
    do): a stray MBX_WINOGRAD in a user's shell must not change the numerics of a default engine.  Every variable in effect
    -- or ignored for want of the opt-in -- is named on stderr."""
    env, out = os.environ, {}
    knobs = ("MBX_WINOGRAD", "MBX_FOLD_SKIP", "MBX_FOLD_START", "MBX_WG_SMALL", "MBX_RV_TILES", "MBX_RV_SPLIT")
    if env.get("MBX_EXPERIMENT", "0") != "1":
        stray = [kk for kk in knobs if kk in env]
        if stray:
            import sys
            print(f"mbexwn_vocoder_amd: ignoring {' '.join(f'{kk}={env[kk]}' for kk in stray)} (experiment variables need "
                  f"MBX_EXPERIMENT=1)", file=sys.stderr)
        return out
    if "MBX_WINOGRAD" in env:
        mode = int(env["MBX_WINOGRAD"])
        out["conv_form"] = {0: "direct", 2: "f23", 4: "f43", 44: "f43"}[mode]
        if mode == 44:
            out["batch_invariant"] = True
    if env.get("MBX_FOLD_SKIP", "1") == "0":
        out["keep_skip"] = True
    if env.get("MBX_FOLD_START", "1") == "0":
        out["keep_start"] = True
    tune = {}
    if "MBX_WG_SMALL" in env:
        tune["gate_shape"] = 1 if int(env["MBX_WG_SMALL"]) == 0 else 2
    if "MBX_RV_TILES" in env:
        tune["resskip_wave_tiles"] = int(env["MBX_RV_TILES"]) or -1
    if "MBX_RV_SPLIT" in env:
        tune["resskip_split"] = int(env["MBX_RV_SPLIT"])
    if tune:
        out["tune"] = tune
    if out:
        import sys
        names = [kk for kk in knobs if kk in env]
        print(f"mbexwn_vocoder_amd: experiment variables in effect: {' '.join(f'{kk}={env[kk]}' for kk in names)}",
              file=sys.stderr)
    return out


PRECISIONS = {"f32": 0, "split_f16": 1}
F0_ACCUMULATE = {"f64": 0, "f32": 1}       # mbx_config.f0_accumulate: MBX_F0_ACC_F64 (default) / MBX_F0_ACC_F32


def make_config(config, wavetables, conv_form=None, batch_invariant=None, keep_skip=None, keep_start=None,
                calib_fraction=None, tune=None, precision="f32", f0_accumulate="f64"):
    """mbx_config of a model.  Policy arguments (None = default, or the experiment variable if one is set):
    conv_form "auto" | "direct" | "f23" | "f43" (mbx_config.wn_conv_form), batch_invariant, keep_skip, keep_start,
    calib_fraction, tune = {"gate_shape": 0|1|2|3|4, "resskip_wave_tiles": n, "resskip_split": 0..3}.  gate_shape 0 keeps the
    launch-size rule; 1 | 4 pin the F(4,3) block shape of large launches (256-row blocks of one column tile | 256-row
    blocks of two) at every launch size, 2 | 3 that of small ones (product-split | product-split of half a column tile) for
    launches of fewer than 4 * 768 256-row blocks (csrc/wn_plan.h, gate_shape_policy).  resskip_wave_tiles -1: never the wave-tiled res/skip
    kernel."""
    dims = ModelDims(config)
    mb = config["mbexwn_config"]
    cc = mbx_config()
    cc.struct_size = ctypes.sizeof(mbx_config)
    cc.abi_version = MBX_ABI_VERSION
    cc.sample_rate, cc.hop_size, cc.mel_channels = dims.sample_rate, dims.hop_size, dims.mel_channels
    cc.subbands = dims.subbands
    cc.pqmf_taps = int(mb["multi_band_config"]["taps"])
    cc.pulse_channels, cc.pulse_per_frame, cc.steps_per_frame = dims.pulse_channels, dims.pulse_per_frame, dims.steps_per_frame
    cc.pulse_rate = dims.pulse_rate
    cc.noise_sigma = dims.noise_sigma
    cc.f0_min, cc.f0_max = dims.f0_min, dims.f0_max
    cc.wn_channels, cc.wn_layers, cc.wn_kernel_size = dims.wn_channels, dims.wn_layers, dims.wn_kernel_size
    cc.wn_out_channels, cc.wn_in_channels = dims.wn_out_channels, dims.wn_in_channels
    if dims.wn_layers > MBX_MAX_WN_LAYERS:
        raise ValueError("too many WaveNet layers for the engine")
    for ll in range(dims.wn_layers):
        cc.wn_dilations[ll] = dims.wn_dilation(ll)
    cc.cond_kernel_size = dims.cond_kernel_size
    cc.cond_conv_upsampling = dims.cond_conv_upsampling
    cc.cond_lin_upsampling = dims.cond_lin_upsampling
    cc.stft_win, cc.fft_size, cc.n_ceps = dims.stft_win, dims.fft_size, dims.n_ceps
    use_windows = (bool(dims.ps_env_order_scale) and not mb.get("psns_use_cepstral_loss_constraint", False) and
                   not dims.no_envelope)
    cc.n_ceps_windows = 30 if use_windows else 0
    cc.filter_max_log_range = dims.filter_max_log_range
    cc.wt_n_period, cc.wt_n_tables = wavetables.n_period, wavetables.n_tables
    cc.wt_nominal_f0 = wavetables.nominalF0
    cc.wt_min_transposition = float(wavetables.min_transposition)
    cc.wt_max_transposition = float(wavetables.max_transposition)
    cc.wt_grid_norm = float(wavetables.grid_norm)
    cc.phase_chunk = 1000
    cc.wn_gate_activation = {"gtu": 0, "gfu": 1, "gsu": 2, "glu": 3}[dims.wn_activation]
    cc.wn_disable_conditioning = int(dims.wn_disable_conditioning)
    if len(dims.wn_pre_cond_channels) > MBX_MAX_PRECOND:
        raise ValueError("too many pre-conditioning layers for the engine")
    cc.n_precond = len(dims.wn_pre_cond_channels)
    for ii, chans in enumerate(dims.wn_pre_cond_channels):
        cc.precond_channels[ii] = chans
    cc.spect_preserve_energy = int(dims.preserve_energy)
    cc.wt_subharm_channels = dims.wt_subharm
    cc.wt_sinusoid_as_fun = int(dims.wt_sinusoid_as_fun)
    cc.ps_off, cc.no_pqmf = int(dims.ps_off), int(dims.no_pqmf)
    cc.pulse_pqmf_taps = int(dims.pulse_pqmf["taps"]) if dims.pulse_pqmf else 0
    cc.ps_subband_gain = int(dims.ps_subband_gain)
    cc.wn_causal = int(dims.wn_padding == "CAUSAL")
    if dims.wn_multi:                 # several WaveNet blocks / in-block upsampling: the generic path of the library
        if dims.n_wn_blocks > MBX_MAX_WN_BLOCKS:
            raise ValueError("too many WaveNet blocks for the engine")
        cc.n_wn_blocks = dims.n_wn_blocks
        for bb in range(dims.n_wn_blocks):
            cc.wn_block_channels[bb], cc.wn_block_ups[bb] = dims.wn_block_channels[bb], dims.wn_block_ups[bb]
    f0_ops, vtf_ops = subnet_ops(config)
    cc.n_f0_ops = _fill_ops(cc.f0_ops, f0_ops)
    cc.n_vtf_ops = _fill_ops(cc.vtf_ops, vtf_ops)
    if mb.get("normalize_rms_from_mell", False):                     # row A14 (reference wavegen_1d.py:93-104)
        from .norm_mel import NormMel
        nm = NormMel(config)
        if nm.win != dims.stft_win:
            raise RuntimeError("normalize_rms_from_mell: preprocess win_size must equal the generator's STFT window")
        cc.nm_iters, cc.nm_smooth_win = nm.iters, nm.smooth_win_size
        cc.nm_use_compressor = int(nm.compressor_exp is not None)
        cc.nm_use_max_limit = int(nm.use_max_limit)
        cc.nm_rms_norm_fact = float(nm.rms_norm_fact)
        cc.nm_rms_floor = float(1.0 / nm.max_norm_fact) if nm.max_norm_fact else 0.0
        cc.nm_compressor_exp = float(nm.compressor_exp) if nm.compressor_exp is not None else 1.0
        cc.nm_lin_amp_scale, cc.nm_lin_amp_off = float(nm.lin_amp_scale), float(nm.lin_amp_off)
        cc.nm_mel_amp_scale = float(nm.mel_amp_scale)
        cc.nm_use_pinv, cc.nm_win_norm = int(nm.use_pinv), float(nm.win_norm)
    over = experiment_overrides() if None in (conv_form, batch_invariant, keep_skip, keep_start, tune) else {}
    conv_form = over.get("conv_form", "auto") if conv_form is None else conv_form
    if conv_form not in CONV_FORMS:
        raise ValueError(f"conv_form must be one of {sorted(CONV_FORMS)}")
    cc.wn_conv_form = CONV_FORMS[conv_form]
    cc.batch_invariant = int(over.get("batch_invariant", False) if batch_invariant is None else batch_invariant)
    cc.wn_keep_skip = int(over.get("keep_skip", False) if keep_skip is None else keep_skip)
    cc.wn_keep_start = int(over.get("keep_start", False) if keep_start is None else keep_start)
    cc.calib_fraction = float(calib_fraction or 0.0)
    tune = over.get("tune", {}) if tune is None else tune
    cc.tune_gate_shape = int(tune.get("gate_shape", 0))
    cc.tune_resskip_wave_tiles = int(tune.get("resskip_wave_tiles", 0))
    cc.tune_resskip_split = int(tune.get("resskip_split", 0))
    if precision not in PRECISIONS:
        raise ValueError(f"precision must be one of {sorted(PRECISIONS)}")
    cc.wn_precision = PRECISIONS[precision]
    if f0_accumulate not in F0_ACCUMULATE:
        raise ValueError(f"f0_accumulate must be one of {sorted(F0_ACCUMULATE)}")
    cc.f0_accumulate = F0_ACCUMULATE[f0_accumulate]
    return cc, dims


# ------------------------------------------------------------------------------------------------
# the engine
# ------------------------------------------------------------------------------------------------
def forward_entry_point(state, active, control, f0, transposed):
    """The library entry point of a forward, from which of its arguments are present: stream_state, active, any of the
    per-frame pitch control (f0_frames / f0_scale / f0_item_mask), an f0 contour, a transposition other than 1.  The plain
    entry points serve the calls that need no mbx_forward_options.  (A formant shift takes mbxe_forward of mbexwn_envelope.h
    instead, with the options the call would have without it, or none.)"""
    if state:
        return "mbx_forward_ex" if active or control else "mbx_forward_stream"
    return "mbx_forward_ex" if f0 or transposed or control else "mbx_forward"


def _kernel_report(gate_kernel, n_gate, rep, n_resskip):
    """The five-key kernel report (MBExWNEngine.kernel_report) from the gate kernel codes of n_gate layers and a structure
    with resskip_kernel[n_resskip], gate_block_channels, tail_kernel and tail_folded: mbx_kernel_report_info or mbx_plan_info."""
    resskip = [RESSKIP_KERNEL_NAMES[rep.resskip_kernel[ll]] for ll in range(n_resskip)]
    return {"gate_kernels": [GATE_KERNEL_NAMES[gate_kernel[ll]] for ll in range(n_gate)],
            "gate_block_channels": [int(rep.gate_block_channels[ll]) for ll in range(n_gate)],
            "resskip_kernels": [kk for kk in resskip if kk != "none"],
            "tail_kernel": TAIL_KERNEL_NAMES[rep.tail_kernel], "tail_folded": bool(rep.tail_folded)}


class MBExWNEngine:
    """Device-resident MBExWN generator. One instance per GPU (one process per GPU)."""

    def __init__(self, config, raw_weights, wavetables=None, device=None, weight_images=True, conv_form=None,
                 batch_invariant=None, keep_skip=None, keep_start=None, calib_fraction=None, tune=None, precision="f32",
                 f0_accumulate="f64"):
        """``weight_images=False`` hands mbx_create only the folded weights and the tables (what a minimal binding of the
        C ABI would do): the engine then runs its generic kernels instead of the specialised ones.

        ``conv_form`` = "auto" (default: Winograd F(4,3) when a calibration forward on this model's own weights stays
        within a quarter of the parity budget of the direct form, else F(2,3), else the direct form -- see
        :meth:`conv_form_info`, :meth:`calibrate`), "direct", "f23" or "f43"; ``batch_invariant=True`` pins the kernels so
        that an utterance's bits do not depend on the batch it ran in; ``keep_skip`` / ``keep_start`` keep the un-folded
        graph; ``tune`` holds measurement knobs (make_config).  ``precision="split_f16"`` is an opt-in experiment (never
        the default): the res/skip layers (and the gate layers behind the first one) contract on the 16-bit matrix pipe with fp16-split operands
        (three products, float32 accumulation; csrc/wn_resskip_f16.hip).  ``f0_accumulate`` = "f64" (default: the F0-net's
        contractions accumulate in float64 and round once -- its contour feeds the phase integrator) or "f32" (the float32
        kernels of the other mel-rate sub-nets: the behaviour up to ABI 8, kept for A/B measurements)."""
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("MBExWNEngine needs an AMD GPU (no CPU fallback for the mel-inversion path)")
        self._torch = torch
        self._lib = load_library()
        self.config = config
        if wavetables is None:
            dims = ModelDims(config)
            wavetables = tb.WaveTables(sample_rate=dims.pulse_rate, **config["mbexwn_config"]["wavetable_config"])
        self.wavetables = wavetables
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        cconf, self.dims = make_config(config, wavetables, conv_form=conv_form, batch_invariant=batch_invariant,
                                       keep_skip=keep_skip, keep_start=keep_start, calib_fraction=calib_fraction, tune=tune,
                                       precision=precision, f0_accumulate=f0_accumulate)
        self.normalizes_rms = cconf.nm_iters > 0            # row A14: done on the device inside mbx_forward
        self._tensors = tensor_table(config, raw_weights, wavetables, split_f16=precision == "split_f16")   # keep the host arrays alive
        if not weight_images:
            self._tensors = {kk: vv for kk, vv in self._tensors.items()
                             if kk.startswith("table.") or kk.rsplit(".", 1)[-1] in ("w", "b", "alpha", "w64")}
        arr = (mbx_tensor * len(self._tensors))()
        for ii, (name, val) in enumerate(self._tensors.items()):
            arr[ii].name = name.encode()
            arr[ii].data = val.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
            arr[ii].ndim = val.ndim
            for dd in range(val.ndim):
                arr[ii].shape[dd] = val.shape[dd]
        handle = ctypes.c_void_p()
        _check(self._lib.mbx_create(ctypes.byref(cconf), arr, len(self._tensors), self.device.index,
                                    ctypes.byref(handle)))
        self._handle = handle
        self._workspace = None
        self._last_shape = None
        self._env_mel = None                                # formant shift: the scratch of the warped rows (forward)

    def close(self):
        if getattr(self, "_handle", None):
            self._lib.mbx_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- properties the reference's model object exposes to MELInverter / scripts
    @property
    def sample_rate(self):
        return self.dims.sample_rate

    @property
    def spect_hop_size(self):
        return self.dims.hop_size

    @property
    def mel_channels(self):
        return self.dims.mel_channels

    def _stream(self):
        return ctypes.c_void_p(self._torch.cuda.current_stream(self.device).cuda_stream)

    def _is(self, t, dtype, shape=None, contiguous=False):
        """True when t is a tensor of that dtype on the engine's device -- of that shape if one is given (None in it: any
        size), contiguous if that is asked for.  The one predicate of the argument checks below."""
        return (self._torch.is_tensor(t) and t.dtype == dtype and t.device == self.device and
                (shape is None or (t.dim() == len(shape) and all(ss is None or ss == dd for ss, dd in zip(shape, t.shape)))) and
                (not contiguous or t.is_contiguous()))

    def workspace_bytes(self, batch, max_frames):
        return int(self._lib.mbx_workspace_size(self._handle, batch, max_frames))

    def _get_workspace(self, batch, max_frames):
        need = self.workspace_bytes(batch, max_frames)
        if self._workspace is None or self._workspace.numel() < need:
            self._workspace = self._torch.empty(need, dtype=self._torch.uint8, device=self.device)
        return self._workspace, need

    def layer_state_info(self):
        """(floats per slot of the per-layer state store, rows between the end of a WaveNet region and its last exact
        sub-band row, smallest number of new rows of a steady tick); floats == 0: this handle cannot carry layer state."""
        ff, rr, mm = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        _check(self._lib.mbx_layer_state_info(self._handle, ctypes.byref(ff), ctypes.byref(rr), ctypes.byref(mm)))
        return ff.value, rr.value, mm.value

    def forward(self, mel, n_frames=None, noise=None, out=None, stream_state=None, active=None, wavenet=None, carry=None,
                layers=None, state_out=None, frontend=None, f0=None, transposition=1.0, f0_frames=None, f0_scale=None,
                f0_item_mask=None, formant=None):
        """mel (B,T,80) float32 cuda tensor; n_frames int32 cuda tensor (B,) or None;
        noise (B, T*steps_per_frame) float32 cuda tensor (N(0,1) draw) -> audio (B, T*hop) cuda tensor.

        f0: optional external F0 contour, float32 cuda tensor (B, T*pulse_per_frame) in Hz at the pulse rate, used instead
        of the F0-net's (``mbx_forward_options.f0``, reference wavegen_1d.py:546-550); transposition scales the contour, the
        F0-net's or the given one (``mbx_forward_options.transposition``).  Both apply to whole items (no stream_state).

        f0_frames / f0_scale: optional per-frame pitch control, float32 cuda tensors (B, T): Hz and transposition factor, one
        value per mel frame, brought to the pulse rate by the model's linear interpolator (``mbx_forward_options.f0_frames /
        f0_scale``); f0_item_mask: optional int32 cuda tensor (B,), 1 = the item takes f0_frames, 0 = it keeps the F0-net
        (None: every item takes them).  Legal with and without stream_state and the window arguments; not together with f0 /
        a transposition other than 1.

        formant: optional formant shift, float32 cuda tensor (B, T): one factor per mel frame, > 1 moves the formants up
        (``mbxe_forward`` of include/mbexwn_envelope.h: ``env_factor``).  The VTF-net and the conditioning chains read the mel rows
        warped along the frequency axis (envelope.warp_envelope_host gives their bits, ``stage("mel_env")`` returns them), the
        F0-net reads the rows as they are: the pitch contour keeps its bits.  Legal with every other argument.

        stream_state: optional int32 cuda tensor (B, 6) holding one ``mbx_stream_state`` per item (see
        streaming.pack_state); the call then returns (audio, state_out) with the carried phase state.
        active: optional (begin_frame, int32 cuda tensor (B,) of frames[, max of them]) with stream_state: the stages from the WaveNet
        on run on that region of the window only (``mbx_forward_options.active_begin / active_frames``); the audio
        outside the region is undefined.  wavenet: optional (begin_frame, int32 tensor (B,)) inner region of the WaveNet;
        carry: optional (store float32 tensor (slots, rows, subbands), int32 tensor (B, 5)) sub-band rows carried between
        ticks (``wn_begin / wn_frames / sub_store / sub_carry``); layers: optional (store float32 tensor (slots, floats),
        int32 tensor (B, 3), new rows) per-layer WaveNet state carried between ticks (``layer_store / layer_carry /
        layer_rows``)."""
        torch = self._torch
        if mel.dim() != 3 or mel.shape[2] != self.dims.mel_channels:
            raise ValueError(f"mel must be (batch, frames, {self.dims.mel_channels})")
        if not self._is(mel, torch.float32):
            raise ValueError("mel must be a float32 tensor on the engine's device")
        mel = mel.contiguous()
        B, T = int(mel.shape[0]), int(mel.shape[1])
        if B == 0 or T == 0:
            return torch.zeros((B, T * self.dims.hop_size), dtype=torch.float32, device=self.device)
        if T * self.dims.steps_per_frame >= 1 << 24:
            # mbx_forward's own limit (32-bit row / sample indices inside the kernels), checked before any allocation
            raise NotImplementedError(f"an item may have at most 2^24 - 1 sub-band rows ({(1 << 24) // self.dims.steps_per_frame} "
                                      f"frames); split longer recordings")
        steps = T * self.dims.wn_in_rows_per_frame            # one noise value per row of the (first) WaveNet block
        if self.dims.noise_sigma:
            if noise is None:
                raise ValueError("noise is required (the noise channel is an explicit input, see SURVEY.md F7)")
            if not self._is(noise, torch.float32, (B, steps)):
                raise ValueError(f"noise must be float32 ({B}, {steps}) on the engine's device")
            noise = noise.contiguous()
        if n_frames is not None:
            if not self._is(n_frames, torch.int32, (B,)):
                raise ValueError("n_frames must be an int32 tensor of shape (batch,) on the engine's device")
            n_frames = n_frames.contiguous()
        if formant is not None and not self._is(formant, torch.float32, (B, T)):
            raise ValueError(f"formant must be a float32 tensor of shape ({B}, {T}) on the engine's device")
        if out is None:
            out = torch.empty((B, T * self.dims.hop_size), dtype=torch.float32, device=self.device)
        ws, need = self._get_workspace(B, T)
        # (alive: the tensors opt points at, up to the call)
        entry, opt, alive, stream_state, state_out = self._forward_options(
            B, T, stream_state, state_out, active, wavenet, carry, layers, frontend, f0, transposition, f0_frames, f0_scale,
            f0_item_mask)
        common = (self._handle, mel.data_ptr(), n_frames.data_ptr() if n_frames is not None else None, B, T,
                  noise.data_ptr() if noise is not None else None, out.data_ptr(), ws.data_ptr(), need)
        if formant is not None:
            # (mbxe_forward takes the options of the call without the shift: none where that is mbx_forward)
            if entry == "mbx_forward_stream":
                opt = mbx_forward_options()
                opt.struct_size, opt.transposition = ctypes.sizeof(mbx_forward_options), 1.0
                opt.state_in, opt.state_out = stream_state.data_ptr(), state_out.data_ptr()
            formant = formant.contiguous()
            scratch = self._envelope_scratch(B * T * self.dims.mel_channels)
            _check(self._lib.mbxe_forward(*common, ctypes.byref(opt) if opt is not None else None, formant.data_ptr(),
                                          self._envelope_centres().data_ptr(), scratch.data_ptr(), self._stream()))
        elif entry == "mbx_forward":
            _check(self._lib.mbx_forward(*common, self._stream()))
        elif entry == "mbx_forward_stream":
            _check(self._lib.mbx_forward_stream(*common, stream_state.data_ptr(), state_out.data_ptr(), self._stream()))
        else:
            _check(self._lib.mbx_forward_ex(*common, ctypes.byref(opt), self._stream()))
        self._last_shape = (B, T)
        return out if stream_state is None else (out, state_out)

    def _forward_options(self, B, T, stream_state, state_out, active, wavenet, carry, layers, frontend, f0, transposition,
                         f0_frames, f0_scale, f0_item_mask):
        """The arguments of a forward behind mel / n_frames / noise, checked: (library entry point (forward_entry_point), its
        mbx_forward_options or None, the tensors the options point at -- to be kept alive up to the call --, stream_state
        made contiguous, state_out allocated if none was given)."""
        torch = self._torch
        if stream_state is None and (active is not None or wavenet is not None or carry is not None or layers is not None):
            raise ValueError("active / wavenet / carry / layers describe a streaming window: pass stream_state as well")
        if stream_state is not None and (f0 is not None or transposition != 1.0):
            raise ValueError("f0 / transposition apply to whole items: not with stream_state")
        control = self._pitch_control(B, T, f0, transposition, f0_frames, f0_scale, f0_item_mask)
        entry = forward_entry_point(stream_state is not None, active is not None, any(cc is not None for cc in control),
                                    f0 is not None, transposition != 1.0)
        opt, keep = None, list(control)
        if entry == "mbx_forward_ex":
            opt = mbx_forward_options()
            opt.struct_size = ctypes.sizeof(mbx_forward_options)
            opt.transposition = 1.0
            opt.f0_frames, opt.f0_scale, opt.f0_item_mask = (None if cc is None else cc.data_ptr() for cc in control)
        if stream_state is not None:
            if not self._is(stream_state, torch.int32, (B, 6)):
                raise ValueError("stream_state must be an int32 tensor of shape (batch, 6) on the engine's device")
            stream_state = stream_state.contiguous()
            if state_out is None:
                state_out = torch.empty_like(stream_state)
            elif not self._is(state_out, torch.int32, (B, 6), contiguous=True):
                raise ValueError("state_out must be a contiguous int32 tensor of shape (batch, 6) on the engine's device")
            if active is None and (wavenet is not None or carry is not None or layers is not None or frontend is not None):
                raise ValueError("wavenet / carry / layers describe regions inside the active one: pass active as well")
            if opt is not None:
                opt.state_in, opt.state_out = stream_state.data_ptr(), state_out.data_ptr()
            if active is not None:
                self._window_options(opt, keep, B, T, active, wavenet, carry, layers, frontend)
        elif opt is not None:
            if not transposition > 0.0:
                raise ValueError("transposition must be positive")
            opt.transposition = float(transposition)
            if f0 is not None:
                if not self._is(f0, torch.float32, (B, T * self.dims.pulse_per_frame)):
                    raise ValueError(f"f0 must be a float32 tensor of shape ({B}, {T * self.dims.pulse_per_frame}) on the "
                                     "engine's device")
                f0 = f0.contiguous()
                keep.append(f0)
                opt.f0 = f0.data_ptr()
        return entry, opt, keep, stream_state, state_out

    def _window_options(self, opt, keep, B, T, active, wavenet, carry, layers, frontend):
        """The streaming-window arguments of a forward, checked and written into opt (the tensors they point at: keep)."""
        torch = self._torch
        a0, act = int(active[0]), active[1]
        if not self._is(act, torch.int32, (B,)) or not 0 <= a0 < T:
            raise ValueError("active = (begin frame inside the window, int32 tensor of shape (batch,) on the device)")
        act = act.contiguous()
        keep.append(act)
        opt.active_begin, opt.active_frames = a0, act.data_ptr()
        if len(active) > 2:
            opt.active_max_frames = int(active[2])
        if wavenet is not None:
            w0, wfr = int(wavenet[0]), wavenet[1]
            if not self._is(wfr, torch.int32, (B,)) or not a0 <= w0 < T:
                raise ValueError("wavenet = (begin frame inside the active region, int32 tensor (batch,) on the device)")
            wfr = wfr.contiguous()
            keep.append(wfr)
            opt.wn_begin, opt.wn_frames = w0, wfr.data_ptr()
            if len(wavenet) > 2:
                opt.wn_max_frames = int(wavenet[2])
        if carry is not None:
            store, desc = carry
            if not self._is(store, torch.float32, (None, None, self.dims.subbands), contiguous=True):
                raise ValueError("carry store must be a contiguous float32 tensor (slots, rows, subbands) on the device")
            if not self._is(desc, torch.int32, (B, 5)):
                raise ValueError("carry descriptors must be an int32 tensor of shape (batch, 5) on the device")
            desc = desc.contiguous()
            keep.append(desc)
            opt.sub_store, opt.sub_store_rows, opt.sub_carry = store.data_ptr(), int(store.shape[1]), desc.data_ptr()
        if layers is not None:
            lstore, ldesc, lrows = layers
            if not self._is(lstore, torch.float32, (None, None), contiguous=True):
                raise ValueError("layer store must be a contiguous float32 tensor (slots, floats) on the device")
            if not self._is(ldesc, torch.int32, (B, 3)):
                raise ValueError("layer descriptors must be an int32 tensor of shape (batch, 3) on the device")
            ldesc = ldesc.contiguous()
            keep.append(ldesc)
            opt.layer_store, opt.layer_store_floats = lstore.data_ptr(), int(lstore.shape[1])
            opt.layer_carry, opt.layer_rows = ldesc.data_ptr(), int(lrows)
        if frontend is not None:
            ring, fpos, fnew, fmargin = frontend[:4]
            opt.fe_end_frames = int(frontend[4]) if len(frontend) > 4 else 0
            if not self._is(ring, torch.float32, (None, None, self.frontend_frame_floats), contiguous=True):
                raise ValueError("front-end ring must be a contiguous float32 tensor (slots, ring frames, "
                                 f"{self.frontend_frame_floats}) on the device")
            if not self._is(fpos, torch.int32, (B,)) or carry is None:
                raise ValueError("front-end positions must be an int32 tensor (batch,) on the device; carry is required")
            fpos = fpos.contiguous()
            keep.append(fpos)
            opt.fe_store, opt.fe_ring_frames, opt.fe_pos = ring.data_ptr(), int(ring.shape[1]), fpos.data_ptr()
            opt.fe_new_frames, opt.fe_margin_frames = int(fnew), int(fmargin)

    def _pitch_control(self, B, T, f0, transposition, f0_frames, f0_scale, f0_item_mask):
        """The per-frame pitch control of a forward, checked: (f0_frames, f0_scale, f0_item_mask) as contiguous tensors or
        None.  The combinations mbx_forward_ex refuses raise ValueError here, before the call."""
        torch = self._torch
        if f0_frames is not None and f0 is not None:
            raise ValueError("f0_frames (per mel frame) and f0 (per pulse sample) exclude each other")
        if (f0_frames is not None or f0_scale is not None) and transposition != 1.0:
            raise ValueError("f0_frames / f0_scale need transposition == 1: put the factor into f0_scale")
        if f0_item_mask is not None and f0_frames is None:
            raise ValueError("f0_item_mask needs f0_frames")
        for name, rows in (("f0_frames", f0_frames), ("f0_scale", f0_scale)):
            if rows is not None and not self._is(rows, torch.float32, (B, T)):
                raise ValueError(f"{name} must be a float32 tensor of shape ({B}, {T}) on the engine's device")
        if f0_item_mask is not None and not self._is(f0_item_mask, torch.int32, (B,)):
            raise ValueError(f"f0_item_mask must be an int32 tensor of shape ({B},) on the engine's device")
        return tuple(None if cc is None else cc.contiguous() for cc in (f0_frames, f0_scale, f0_item_mask))

    def _envelope_centres(self):
        """The device table of the mel channels' centre frequencies (envelope.channel_centres of the model's analysis)."""
        from .envelope import device_centres
        return device_centres(self.config["preprocess_config"], self.device)

    def _envelope_scratch(self, floats):
        """The warped mel rows of a forward with ``formant`` (env_mel of mbxe_forward; the stage "mel_env"): the engine's,
        grown as needed -- like the workspace, one forward at a time uses it."""
        if self._env_mel is None or self._env_mel.numel() < floats:
            self._env_mel = self._torch.empty(floats, dtype=self._torch.float32, device=self.device)
        return self._env_mel

    def warp_envelope(self, mel, factors, n_frames=None):
        """The formant shift on its own (``mbxe_warp_envelope``, include/mbexwn_envelope.h): mel float32 cuda (B, T,
        mel_channels) -- a view with a batch stride of its own is passed as it is, the result then has that stride --, factors float32 cuda (B, T), n_frames
        optional int32 cuda (B,) -> the warped rows (B, T, mel_channels), bit-equal to envelope.warp_envelope_host."""
        from .envelope import warp_envelope_device
        torch, n = self._torch, self.dims.mel_channels
        if not self._is(mel, torch.float32, (None, None, n)):
            raise ValueError(f"mel must be a float32 tensor (batch, frames, {n}) on the engine's device")
        B, T = int(mel.shape[0]), int(mel.shape[1])
        if not self._is(factors, torch.float32, (B, T)):
            raise ValueError(f"factors must be a float32 tensor of shape ({B}, {T}) on the engine's device")
        if n_frames is not None and not self._is(n_frames, torch.int32, (B,)):
            raise ValueError("n_frames must be an int32 tensor of shape (batch,) on the engine's device")
        return warp_envelope_device(mel, factors, self._envelope_centres(), n_frames)

    def track_f0(self, audio, n_samples, centres, n_frames, **params):
        """F0 and periodicity of every frame from the audio itself (``mbxp_track_f0``, include/mbexwn_pitch.h) on the
        engine's stream: ``f0track.track_f0_device`` at the model's sample rate; ``params`` are ``f0track.params``'
        keywords (f0_min, f0_max, window, threshold, rms_floor).  Returns (f0, periodicity), cuda (batch, max_frames)."""
        from . import f0track
        if not self._torch.is_tensor(audio) or audio.device != self.device:
            raise ValueError("audio must be a float32 tensor (batch, stride) on the engine's device")
        with self._torch.cuda.device(self.device):
            return f0track.track_f0_device(audio, n_samples, centres, n_frames, f0track.params(self.dims.sample_rate, **params))

    def encode_flac16(self, audio, n_samples, sample_rate=None, wait=True, compression="verbatim"):
        """The FLAC frames (``flac.encode`` of the item without its 42-byte header) and max |x| of every item
        audio[b, :n_samples[b]] of a device batch (B, stride) float32, encoded on the engine's stream and copied into pinned
        host memory asynchronously.  ``n_samples``: host integers; ``sample_rate`` defaults to the model's.
        ``compression="verbatim"`` is mbx_encode_flac16; ``"fixed"`` is mbxf_encode_flac16_fixed (fixed predictors and Rice
        codes, the bytes of ``flac.encode(..., compression="fixed")``): the frame lengths come back first (the call waits
        for them), then only the bytes the frames take, and the int16 samples for the MD5.  Returns an
        :class:`EncodedFlac`; with ``wait=False`` the copies may still be in flight (``EncodedFlac.wait()`` before reading)."""
        from . import flac
        if compression not in flac.COMPRESSIONS:
            raise ValueError(f"compression must be one of {flac.COMPRESSIONS}, got {compression!r}")
        if not self._is(audio, self._torch.float32, (None, None)):
            raise ValueError("audio must be a float32 tensor (batch, stride) on the engine's device")
        return flac.encode_device(audio, n_samples, self.dims.sample_rate if sample_rate is None else sample_rate,
                                  compression=compression, wait=wait)

    def keyed_noise(self, seeds, item_keys, counts, first_step=None, out=None):
        """Keyed N(0,1) noise (include/mbexwn_noise.h, ``mbxn_fill_normal``): row b holds the values ``first_step[b] ..
        first_step[b] + counts[b]`` of the item ``(seeds[b], item_keys[b])``, zeros behind them.  ``seeds`` / ``item_keys``:
        integers (taken mod 2^64), one per item, or one seed for all; ``counts`` / ``first_step``: host integers.  Returns a
        float32 device tensor (B, max(counts)); ``out``: a zeroed float32 device tensor (B, stride >= max(counts)) to fill
        instead.  A value depends on its seed, key and step alone: not on the batch, the row or the window it is asked
        in."""
        from .noise import fill_normal_device
        return fill_normal_device(seeds, item_keys, counts, first_step=first_step, out=out, device=self.device)

    def window_advance(self, mel_window, mel_new, noise_window=None, noise_new=None):
        """mbx_window_advance: shift the device-resident windows (B, T, mel_channels) / (B, T*steps_per_frame) left by the
        frames of mel_new (B, step, mel_channels) / noise_new (B, step*steps_per_frame) and append those, in place."""
        torch = self._torch
        B, T, step = int(mel_window.shape[0]), int(mel_window.shape[1]), int(mel_new.shape[1])
        for tt in (mel_window, mel_new, noise_window, noise_new):
            if tt is not None and not self._is(tt, torch.float32, contiguous=True):
                raise ValueError("windows and new frames must be contiguous float32 tensors on the engine's device")
        if tuple(mel_new.shape) != (B, step, self.dims.mel_channels) or mel_window.shape[2] != self.dims.mel_channels:
            raise ValueError("mel_new must be (batch, step, mel_channels)")
        if noise_window is not None and (tuple(noise_window.shape) != (B, T * self.dims.steps_per_frame) or
                                         noise_new is None or tuple(noise_new.shape) != (B, step * self.dims.steps_per_frame)):
            raise ValueError("noise_window / noise_new must be (batch, frames * steps_per_frame) / (batch, step * steps_per_frame)")
        _check(self._lib.mbx_window_advance(self._handle, mel_window.data_ptr(), mel_new.data_ptr(),
                                            noise_window.data_ptr() if noise_window is not None else None,
                                            noise_new.data_ptr() if noise_window is not None else None, B, T, step,
                                            self._stream()))

    def shader_clock_under(self, work, seconds=0.02):
        """Shader clock (GHz) the part delivers while ``work()`` -- a callable that enqueues kernels on the engine's stream --
        runs: a one-wave probe (mbx_clock_probe) spins on a second stream for ``seconds`` and counts shader cycles against the
        constant 100 MHz clock.  ``work`` should enqueue at least that much device time.  Synchronises."""
        torch = self._torch
        out = torch.zeros(4, dtype=torch.int64, device=self.device)
        side = torch.cuda.Stream(device=self.device)
        work()                                                    # the chip is busy before the probe starts
        _check(self._lib.mbx_clock_probe(self._handle, out.data_ptr(), int(seconds * 1e8), ctypes.c_void_p(side.cuda_stream)))
        work()
        torch.cuda.synchronize(self.device)
        c0, c1, r0, r1 = (int(vv) for vv in out.cpu().numpy())
        return (c1 - c0) / max(r1 - r0, 1) * 0.1                    # cycles per 10 ns tick -> GHz

    def window_update(self, mel_window, mel_new, noise_window, noise_new, shift, keep):
        """mbx_window_update: frames [shift, shift + keep) of the device-resident windows move to the front, the frames of
        mel_new / noise_new land behind them; one launch."""
        B, T, step = int(mel_window.shape[0]), int(mel_window.shape[1]), int(mel_new.shape[1])
        _check(self._lib.mbx_window_update(self._handle, mel_window.data_ptr(), mel_new.data_ptr(),
                                           noise_window.data_ptr() if noise_window is not None else None,
                                           noise_new.data_ptr() if noise_window is not None else None, B, T, int(shift), int(keep),
                                           step, self._stream()))

    def emit_rows(self, audio, first, count, host_out):
        """mbx_emit_rows: samples [first, first + count) of every row of the device tensor `audio` (B, n) into the pinned
        host tensor host_out (B, count) as one strided copy on the engine's stream."""
        B, n = int(audio.shape[0]), int(audio.shape[1])
        if (tuple(host_out.shape) != (B, count) or not host_out.is_contiguous() or
                not self._is(audio, self._torch.float32, contiguous=True)):
            raise ValueError("emit_rows: host_out must be a contiguous (batch, count) tensor, audio contiguous")
        _check(self._lib.mbx_emit_rows(self._handle, audio.data_ptr(), n, B, int(first), int(count), host_out.data_ptr(),
                                       self._stream()))

    @property
    def frontend_carry_supported(self):
        """True when mbx_forward_ex can carry the mel-rate front end between streaming ticks (fe_store): no RMS
        normalisation, an F0-net that ends at the pulse rate, per-frame sizes that are multiples of 4 floats."""
        dd = self.dims
        f0_ops, _ = subnet_ops(self.config)
        factor = 1
        for op in f0_ops:
            factor *= op.get("up", 1) if op["kind"] in ("conv", "lin") else 1
        sizes = (2 * dd.wn_channels * dd.cond_conv_upsampling, dd.n_ceps, dd.pulse_per_frame)
        return not self.normalizes_rms and factor == dd.pulse_per_frame and all(vv % 4 == 0 for vv in sizes)

    @property
    def frontend_frame_floats(self):
        """Floats per mel frame of the carried front end: conditioning rows, cepstrum, F0 contour."""
        dd = self.dims
        return 2 * dd.wn_channels * dd.cond_conv_upsampling + dd.n_ceps + dd.pulse_per_frame

    def profile_enable(self, enabled=True):
        _check(self._lib.mbx_profile_enable(self._handle, 1 if enabled else 0))

    def profile_read(self, kernel):
        """(summed device ms, launches) of the WaveNet GEMM kernel 'gate' or 'res_skip' since the last read."""
        ms, cnt = ctypes.c_double(), ctypes.c_int64()
        _check(self._lib.mbx_profile_read(self._handle, kernel.encode(), ctypes.byref(ms), ctypes.byref(cnt)))
        return ms.value, cnt.value

    def profile_read_launches(self, kernel, capacity=4096):
        """Device ms of every bracketed launch group of a stage since the last read, in launch order (mbx_profile_read_launches);
        "gate": the layers of each forward in order (behind the folded first layer)."""
        buf = (ctypes.c_float * capacity)()
        cnt = ctypes.c_int64()
        _check(self._lib.mbx_profile_read_launches(self._handle, kernel.encode(), buf, capacity, ctypes.byref(cnt)))
        return [float(buf[ii]) for ii in range(min(capacity, cnt.value))]

    def conv_form_info(self):
        """What the handle decided about the dilated convolution (mbx_conv_form): dict with ``requested`` / ``form`` /
        ``stream_form`` ("auto" | "direct" | "f23" | "f43"), ``calibrated`` (0 no, 1 on the built-in synthetic mel at
        creation, 2 on caller data), ``batch_invariant``, ``fold_skip``, ``fold_start``, and the calibration's numbers
        ``err_f43`` / ``err_f23`` (max |audio(form) - audio(direct)|, None: form not available), ``ref_max``,
        ``threshold``; with ``precision="split_f16"`` also ``err_split`` (max |audio(this handle in split precision) -
        audio(float32 direct form)| of the calibration run at creation) and ``split_rejected`` (True: that error was above the
        threshold or not finite, the handle runs float32 after all: ``split_f16_layers`` is 0 then).  ``gate_kernels``: the
        gate kernel of every layer of the last forward, block-major (block b, layer l at b * n_layers + l) on a model with
        several WaveNet blocks.  From mbx_kernel_report: ``resskip_kernels``, one entry (RESSKIP_KERNEL_NAMES) per layer whose
        res/skip launch ran, in the same order (the last layer of a handle with ``fold_skip`` has none: the tail takes its
        share), ``tail_kernel`` (TAIL_KERNEL_NAMES), ``tail_folded`` and ``gate_block_channels``: per entry of ``gate_kernels``
        the gate channels of one F(4,3) block (64: blocks of two column tiles, 32: of one, 16: of half a tile; 0: no F(4,3)
        block ran the layer)."""
        info = mbx_conv_form_info()
        info.struct_size = ctypes.sizeof(mbx_conv_form_info)
        _check(self._lib.mbx_conv_form(self._handle, ctypes.byref(info)))
        rep = mbx_kernel_report_info()
        rep.struct_size = ctypes.sizeof(mbx_kernel_report_info)
        _check(self._lib.mbx_kernel_report(self._handle, ctypes.byref(rep)))
        return {"requested": _CONV_FORM_NAMES[info.requested], "form": _CONV_FORM_NAMES[info.form],
                "stream_form": _CONV_FORM_NAMES[info.stream_form], "calibrated": info.calibrated,
                "batch_invariant": bool(info.batch_invariant), "fold_skip": bool(info.fold_skip),
                "fold_start": bool(info.fold_start), "split_f16_layers": int(info.split_f16_layers),
                "split_f16_gate_layers": int(info.split_f16_gate_layers),
                "err_f43": None if info.err_f43 < 0 else float(info.err_f43),
                "err_f23": None if info.err_f23 < 0 else float(info.err_f23),
                "ref_max": float(info.ref_max), "threshold": float(info.threshold),
                "err_split": None if info.err_split < 0 else float(info.err_split),
                "split_rejected": bool(info.split_rejected), "f0_float64_chain": bool(info.f0_float64_chain),
                **_kernel_report(info.gate_kernel, info.n_gate_layers, rep, rep.n_resskip_layers)}

    def kernel_report(self):
        """What the most recent forward ran, per layer: ``gate_kernels``, ``gate_block_channels``, ``resskip_kernels``,
        ``tail_kernel`` and ``tail_folded`` of :meth:`conv_form_info`."""
        info = self.conv_form_info()
        return {kk: info[kk] for kk in ("gate_kernels", "gate_block_channels", "resskip_kernels", "tail_kernel", "tail_folded")}

    def calibrate(self, mel, n_frames=None, noise=None):
        """mbx_calibrate: repeat the form calibration on the caller's own mel batch (device tensors as for
        :meth:`forward`) and adopt its decision; returns :meth:`conv_form_info`.  Synchronises."""
        torch = self._torch
        mel = mel.to(self.device, torch.float32).contiguous()
        B, T = int(mel.shape[0]), int(mel.shape[1])
        if self.dims.noise_sigma and noise is None:
            noise = torch.randn((B, T * self.dims.wn_in_rows_per_frame), device=self.device, dtype=torch.float32)
        if noise is not None:
            noise = noise.to(self.device, torch.float32).contiguous()
        ws, need = self._get_workspace(B, T)
        _check(self._lib.mbx_calibrate(self._handle, mel.data_ptr(), n_frames.data_ptr() if n_frames is not None else None,
                                       B, T, noise.data_ptr() if noise is not None else None, ws.data_ptr(), need,
                                       self._stream()))
        return self.conv_form_info()

    def _plan_info(self, batch, max_frames):
        info = mbx_plan_info()
        info.struct_size = ctypes.sizeof(mbx_plan_info)
        _check(self._lib.mbx_plan(self._handle, int(batch), int(max_frames), ctypes.byref(info)))
        return info

    def plan(self, batch, max_frames):
        """What a whole-item :meth:`forward` of this size would run, without launching (mbx_plan): the dict of
        :meth:`kernel_report`, which equals it after such a forward."""
        info = self._plan_info(batch, max_frames)
        return _kernel_report(info.gate_kernel, info.n_layers, info, info.n_layers)

    def gate_form(self, batch, max_frames):
        """Which float32 implementation of the dilated convolution a forward of this size runs, as the library plans it
        (mbx_plan; csrc/wn_plan.h): the kernel of the first layer behind a folded first layer -- the handle's form and, for
        F(4,3), the block shape of the launch-size rule (256-row blocks, or 128-row blocks whose waves split the six products
        where those spread the work clearly more evenly over the SIMDs, or product-split blocks of half a column tile where even
        those load the CUs unevenly; all give the same bits): "direct", "winograd_f23", "winograd_f43", "winograd_f43_psplit" or
        "winograd_f43_hsplit"."""
        info = self._plan_info(batch, max_frames)
        first = 1 if info.n_layers > 1 and info.gate_kernel[0] == 8 else 0        # MBX_GATE_K_FOLDED_START
        kernel = GATE_KERNEL_NAMES[info.gate_kernel_f32[first]]
        if kernel == "folded_start":              # a one-layer model: no layer runs a gate kernel of the form
            kernel = self.conv_form_info()["form"]
        return {"direct": "direct", "f23": "winograd_f23", "f43": "winograd_f43", "f43_strided": "winograd_f43",
                "f43_psplit": "winograd_f43_psplit", "f43_strided_psplit": "winograd_f43_psplit", "f43_hsplit": "winograd_f43_hsplit"}[kernel]

    @property
    def folds_start(self):
        """True when layer 0 runs with the start convolution folded in (csrc/wn_gate0.hip): what mbx_create decided."""
        return self.conv_form_info()["fold_start"]

    def stage(self, name):
        """Intermediate tensor of the last forward (copy), shaped (B, count); see mbx_stage.  On a model with several WaveNet
        blocks "wn_hidden" / "wn_skip" are the last block's (its rows and channels), "cond1" .. "cond3" the conditioning rows
        of blocks 1 .. 3; a pulse-PQMF model also has "pulse_ana", the rows its WaveNet reads."""
        torch = self._torch
        ptr, cnt, stride = ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_int64()
        status = self._lib.mbx_stage(self._handle, name.encode(), ctypes.byref(ptr), ctypes.byref(cnt), ctypes.byref(stride))
        if status != 0 and name == "wn_hidden":
            # split precision with the fp16 planes as the hidden state (csrc/mbx_forward.hip: ForwardCtx::planes_only): the float32 tensor was
            # not written; rebuild hi + 2^-11 lo' from the planes -- per row [C8 hi halves | C8 lo' halves]
            planes = self.stage("wn_hidden_planes")
            C, c8 = self.dims.wn_channels, (self.dims.wn_channels + 7) // 8 * 8
            halves = planes.view(torch.float16).view(planes.shape[0], -1, 2, c8).float()
            return (halves[:, :, 0, :C] + halves[:, :, 1, :C] / 2048.0).reshape(planes.shape[0], -1)
        _check(status)
        B = self._last_shape[0]
        dtype = torch.int32 if name == "ceps_index" else torch.float32
        ws = self._env_mel.view(torch.uint8) if name == "mel_env" else self._workspace      # (the caller's scratch: ours)
        offset = ptr.value - ws.data_ptr()
        flat = ws[offset: offset + B * stride.value * 4].view(dtype)
        return flat.view(B, stride.value)[:, :cnt.value].clone()

    def _prepare(self, spect, synth_length, noise):
        """Common front of infer / infer_components: device mel (last frame repeated when the mel is shorter than
        synth_length, reference wavegen_1d.py:490-491, 537-538) and the noise draw."""
        torch = self._torch
        mel = torch.as_tensor(np.asarray(spect, dtype=np.float32) if not torch.is_tensor(spect) else spect)
        mel = mel.to(self.device, torch.float32)
        if mel.shape[1] * self.dims.hop_size < synth_length:
            mel = torch.cat((mel, mel[:, -1:]), dim=1)
        mel = mel.contiguous()
        if noise is None and self.dims.noise_sigma:
            # the reference draws tf.random.normal here (custom_pulsed_generator.py:905-906)
            noise = torch.randn((mel.shape[0], mel.shape[1] * self.dims.wn_in_rows_per_frame), device=self.device,
                                dtype=torch.float32)
        elif noise is not None:
            noise = torch.as_tensor(noise).to(self.device, torch.float32).contiguous()
        return mel, noise

    def _envelope(self, B, T):
        """Spectral envelope (B, T, fft/2+1) complex64 of the last forward, rebuilt on the host from its cepstrum stage
        (reference custom_pulsed_generator.py:801-855): lifter row, one-sided cepstrum -> rfft -> exp(R tanh(Re) + j Im)."""
        ceps = self.stage("cepstrum").cpu().numpy().reshape(B, T, self.dims.n_ceps)
        if "table.ceps_windows" in self._tensors:
            idx = self.stage("ceps_index").cpu().numpy()
            ceps = ceps * self._tensors["table.ceps_windows"][idx]
        full = np.zeros((B, T, self.dims.fft_size), dtype=np.float32)
        full[:, :, 1:self.dims.n_ceps] = ceps[:, :, 1:]
        spec = np.fft.rfft(full, axis=-1)
        rng = self.dims.filter_max_log_range
        env = np.exp(rng * np.tanh(spec.real) + 1j * spec.imag) if rng else np.exp(spec)
        return env.astype(np.complex64)

    def infer(self, spect, sigma=None, z_in=None, synth_length=0, F0=None, return_F0=False, return_components=False,
              training=False, test_grad=None, noise=None, **_):
        """Keras-model look-alike of PaNWaveNet.infer (reference wavegen_1d.py:483-526):
        spect numpy/torch (B,T,80) -> tensor with .numpy() of shape (B, synth_length).

        As in the reference: ``sigma`` and ``z_in`` are unused; ``F0`` is only used by the training branch of
        ``MBExWN.call`` (custom_pulsed_generator.py:640-663: at inference ``pulse_frequency_ = pulse_frequency``), so it is
        ignored here -- :meth:`infer_components` is the F0-injection path; ``synth_length = 0`` means the model's
        ``segment_length`` (wavegen_1d.py:489).  ``return_F0`` adds the parameter list
        ``[["F0", .], ["PSig", excitation], ["PS", |envelope|]]`` (custom_pulsed_generator.py:756-767, every entry cut to
        ``[:, :synth_length]`` as wavegen_1d.py:512-515 does), ``return_components`` returns the list of signals.
        ``noise`` (B, T*steps_per_frame) is this build's explicit N(0,1) draw of the noise channel."""
        if training or test_grad is not None:
            raise NotImplementedError("infer(): training / test_grad belong to the training graph, not to the "
                                      "mel-inversion path")
        synth_length = int(synth_length) if synth_length else int(self.dims.segment_length)
        if synth_length <= 0:
            raise ValueError("infer(): synth_length is 0 and the model configuration has no segment_length to fall back "
                             "to (reference wavegen_1d.py:489)")
        mel, noise = self._prepare(spect, synth_length, noise)
        # the optional RMS normalisation of the mel input and the matching output gain (reference
        # wavegen_1d.py:493-495, 506-507, row A14) run inside mbx_forward
        audio = self.forward(mel, noise=noise)
        signals = [_HostTensor(audio[:, :synth_length])]
        if not return_F0:
            return signals if return_components else signals[0]
        B, T = int(mel.shape[0]), int(mel.shape[1])
        rate = int(self.dims.sample_rate // self.dims.pulse_rate)
        f0 = self.stage("f0")[:, :audio.shape[1]:rate]               # the reference's own slice (:757)
        params = [["F0", _HostTensor(f0[:, :synth_length])]]
        if not self.dims.no_envelope:     # ps_off / sub-band gains: neither excitation_signal nor source_filter_stft exist (reference :756-767)
            params += [["PSig", _HostTensor(self.stage("excitation")[:, :audio.shape[1]][:, :synth_length])],
                       ["PS", _HostTensor(np.abs(self._envelope(B, T))[:, :synth_length])]]
        return (signals, params) if return_components else (signals[0], params)

    def infer_components(self, spect, synth_length=0, F0=None, transposition_factor=None, noise=None):
        """PaNWaveNet.infer_components (reference wavegen_1d.py:528-557): returns
        (F0 (B, T*pulse_per_frame), excitation (B, T*hop), spectral envelope complex (B, T, fft/2+1), upsampled_rms or
        None) as numpy arrays; ``F0`` may be given (Hz at the pulse rate), ``transposition_factor`` scales it.  As in the
        reference, ``synth_length`` is replaced by ``F0.shape[1]`` when a contour is given and only decides whether the
        last mel frame is repeated and how long ``upsampled_rms`` is.
        Additionally the (transposed) synthesis itself is available as ``self.last_audio`` (device tensor)."""
        torch = self._torch
        if self.dims.no_envelope:
            raise NotImplementedError("infer_components(): a ps_off / ps_use_stft: false model has no spectral envelope "
                                      "(the reference's generate_specenv has no cepstral VTF-net to run)")
        synth_length = int(synth_length) if F0 is None else int(np.asarray(F0).shape[1])
        mel, noise = self._prepare(spect, synth_length, noise)
        ppf = self.dims.pulse_per_frame
        B, T = int(mel.shape[0]), int(mel.shape[1])
        gain = None
        if self.normalizes_rms:                                      # 4th output: upsampled_rms (reference :539-542)
            gain = self.norm_mel_stage(mel)[1][:, :synth_length].cpu().numpy()
        f0_dev = None
        if F0 is not None:
            f0_np = np.zeros((B, T * ppf), dtype=np.float32)
            src = np.asarray(F0, dtype=np.float32).reshape(B, -1)
            nn = min(src.shape[1], f0_np.shape[1])
            f0_np[:, :nn] = src[:, :nn]
            f0_np[:, nn:] = src[:, -1:]
            f0_dev = torch.as_tensor(f0_np, device=self.device)
        self.last_audio = self.forward(mel, noise=noise, f0=f0_dev,
                                       transposition=float(transposition_factor) if transposition_factor else 1.0)
        f0 = self.stage("f0").cpu().numpy()
        exc = self.stage("excitation").cpu().numpy()
        return f0, exc, self._envelope(B, T), gain

    # -- stage entry points (unit parity tests)
    def pqmf_synthesis(self, x):
        torch = self._torch
        x = x.contiguous()
        B, S, M = x.shape
        y = torch.empty((B, S * M), dtype=torch.float32, device=self.device)
        _check(self._lib.mbx_pqmf_synthesis(self._handle, x.data_ptr(), B, S, y.data_ptr(), self._stream()))
        return y

    def conv1d(self, x, w, b=None, alpha=None, dilation=1, pad_l=0, pad_mode=0, f64_accumulate=False):
        """mbx_conv1d, or mbx_conv1d_f64acc with ``f64_accumulate`` (float64 sums, one rounding per output)."""
        torch = self._torch
        x, w = x.contiguous(), w.contiguous()
        B, R, cin = x.shape
        ks, _, cout = w.shape
        y = torch.empty((B, R, cout), dtype=torch.float32, device=self.device)
        fn = self._lib.mbx_conv1d_f64acc if f64_accumulate else self._lib.mbx_conv1d
        _check(fn(self._handle, x.data_ptr(), B, R, cin, w.data_ptr(),
                  b.data_ptr() if b is not None else None,
                  alpha.data_ptr() if alpha is not None else None, ks, cout, dilation, pad_l,
                  pad_mode, y.data_ptr(), self._stream()))
        return y

    def lin_interp(self, x, up):
        torch = self._torch
        x = x.contiguous()
        B, R, C = x.shape
        y = torch.empty((B, R * up, C), dtype=torch.float32, device=self.device)
        _check(self._lib.mbx_lin_interp(self._handle, x.data_ptr(), B, R, C, up, y.data_ptr(), self._stream()))
        return y

    def wavetable(self, f0):
        torch = self._torch
        f0 = f0.contiguous()
        B, N = f0.shape
        nch = 1 + self.dims.wt_subharm                       # pulse + sub-harmonic sinusoid channels per sample
        pulse = torch.empty((B, N, nch) if nch > 1 else (B, N), dtype=torch.float32, device=self.device)
        phase = torch.empty_like(f0)
        scratch = torch.empty(B * (N + N // 1000 + 3), dtype=torch.float32, device=self.device)
        _check(self._lib.mbx_wavetable(self._handle, f0.data_ptr(), B, N, pulse.data_ptr(), phase.data_ptr(),
                                       scratch.data_ptr(), self._stream()))
        return pulse, phase

    def norm_mel_stage(self, mel, n_frames=None):
        """NormMelComponents.normalize_inputs_by_rms on the device: mel (B,T,80) -> (mel' (B,T,80), gain (B,T*hop))."""
        torch = self._torch
        mel = mel.contiguous()
        B, T = int(mel.shape[0]), int(mel.shape[1])
        out = torch.empty_like(mel)
        gain = torch.zeros((B, T * self.dims.hop_size), dtype=torch.float32, device=self.device)
        scratch = torch.empty(2 * B * T, dtype=torch.float32, device=self.device)
        _check(self._lib.mbx_norm_mel(self._handle, mel.data_ptr(), n_frames.data_ptr() if n_frames is not None else None,
                                      B, T, out.data_ptr(), gain.data_ptr(), scratch.data_ptr(), self._stream()))
        return out, gain

    def stft_filter(self, excitation, cepstrum, ceps_index=None):
        torch = self._torch
        excitation, cepstrum = excitation.contiguous(), cepstrum.contiguous()
        B, T = cepstrum.shape[:2]
        audio = torch.empty((B, T * self.dims.hop_size), dtype=torch.float32, device=self.device)
        scratch = torch.empty(B * T * self.dims.stft_win, dtype=torch.float32, device=self.device)
        _check(self._lib.mbx_stft_filter(self._handle, excitation.data_ptr(), cepstrum.data_ptr(),
                                         ceps_index.contiguous().data_ptr() if ceps_index is not None else None,
                                         B, T, audio.data_ptr(), scratch.data_ptr(), self._stream()))
        return audio


class EncodedFlac:
    """What :meth:`MBExWNEngine.encode_flac16` returns: the frames of every item in one pinned host buffer (item b at
    ``offsets[b]:offsets[b + 1]``) and max |x| per item, behind the event of their device-to-host copies.  Compressed frames
    (``compression="fixed"``) come with their lengths (``frame_lengths(b)``) and the int16 samples they hold (``pcm(b)``)."""

    def __init__(self, host, offsets, max_abs, n_samples, rate, event, frame_lengths=None, frame_bounds=None, pcm=None):
        self._host, self._host_max, self._event = host, max_abs, event
        self.offsets, self.n_samples, self.rate = offsets, list(n_samples), rate
        self._lengths, self._bounds, self._pcm = frame_lengths, frame_bounds, pcm
        self.compression = "verbatim" if frame_lengths is None else "fixed"
        self.max_abs = None

    def wait(self):
        if self._event is not None:
            self._event.synchronize()
            self._event = None
            self.max_abs = self._host_max.numpy()[:len(self.n_samples)]
        return self

    def frames(self, b):
        """The frames of item b (a numpy view of the pinned buffer)."""
        self.wait()
        return self._host.numpy()[self.offsets[b]:self.offsets[b + 1]]

    def frame_lengths(self, b):
        """The lengths of the compressed frames of item b; None for uncompressed frames (``flac.frame_layout`` has those)."""
        if self._lengths is None:
            return None
        return self._lengths[self._bounds[b]:self._bounds[b + 1]]

    def pcm(self, b):
        """The int16 samples the compressed frames of item b hold; None for uncompressed frames (they hold them as they are)."""
        if self._pcm is None:
            return None
        self.wait()
        return self._pcm.numpy()[b, :self.n_samples[b]]

    def stream(self, b):
        """The whole FLAC stream of item b (``flac.assemble``); only for an item whose max |x| is finite -- any other goes
        through the host writer, ``flac.encode``."""
        from . import flac
        return flac.assemble(self.frames(b), self.n_samples[b], self.rate, frame_lengths=self.frame_lengths(b), pcm=self.pcm(b))

    def write(self, path, b):
        """``stream(b)`` into a file (``flac.write_frames``: the frames are written as they are)."""
        from . import flac
        return flac.write_frames(path, self.frames(b), self.n_samples[b], self.rate, frame_lengths=self.frame_lengths(b),
                                 pcm=self.pcm(b))


class _HostTensor:
    """What ``model.infer(...)`` returns: something with ``.numpy()`` (reference mel_inverter.py:152)."""

    def __init__(self, tensor):
        self.tensor = tensor

    def numpy(self):
        if isinstance(self.tensor, np.ndarray):
            return self.tensor
        return self.tensor.detach().cpu().numpy()

    @property
    def shape(self):
        return tuple(self.tensor.shape)
