"""ctypes binding of libmbexwn_hip.so: the structures and constants of include/mbexwn.h, and ONE table of every function the
sixteen headers under include/ declare, from which ``load_library`` sets each ``restype`` / ``argtypes``.

Nothing else lives here: a tool that only resamples imports this module, not the engine's driver.  The table is declared in
Python (the package loads without include/ beside it); tests/test_abi_headers.py holds it to the headers name by name and
parameter by parameter, and every field of every structure to the C compiler's layout."""
import ctypes
import os
import sys

from .build import LIB_PATH

MBX_ABI_VERSION = 11
MBX_MAX_SUBNET_OPS = 32
MBX_MAX_WN_LAYERS = 64
MBX_MAX_PRECOND = 8
MBX_MAX_WN_BLOCKS = 4
MBX_NAME_LEN = 64

i32, i64, f32, vp, size_t = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t
P = ctypes.POINTER


class mbx_subnet_op(ctypes.Structure):
    _fields_ = [("kind", i32), ("ks", i32), ("cin", i32), ("cout", i32), ("pad_l", i32), ("pad_r", i32), ("pad_mode", i32),
                ("up", i32), ("act", i32), ("alpha", f32), ("name", ctypes.c_char * MBX_NAME_LEN)]


class mbx_config(ctypes.Structure):
    _fields_ = [("struct_size", i32), ("abi_version", i32), ("sample_rate", i32), ("hop_size", i32), ("mel_channels", i32),
                ("subbands", i32), ("pqmf_taps", i32), ("pulse_channels", i32), ("pulse_per_frame", i32),
                ("steps_per_frame", i32), ("pulse_rate", f32), ("noise_sigma", f32), ("f0_min", f32), ("f0_max", f32),
                ("wn_channels", i32), ("wn_layers", i32), ("wn_kernel_size", i32), ("wn_out_channels", i32),
                ("wn_in_channels", i32), ("wn_dilations", i32 * MBX_MAX_WN_LAYERS),
                ("cond_kernel_size", i32), ("cond_conv_upsampling", i32), ("cond_lin_upsampling", i32),
                ("stft_win", i32), ("fft_size", i32), ("n_ceps", i32), ("n_ceps_windows", i32), ("filter_max_log_range", f32),
                ("wt_n_period", i32), ("wt_n_tables", i32), ("wt_nominal_f0", f32), ("wt_min_transposition", f32),
                ("wt_max_transposition", f32), ("wt_grid_norm", f32), ("phase_chunk", i32),
                ("n_f0_ops", i32), ("f0_ops", mbx_subnet_op * MBX_MAX_SUBNET_OPS),
                ("n_vtf_ops", i32), ("vtf_ops", mbx_subnet_op * MBX_MAX_SUBNET_OPS),
                ("nm_iters", i32), ("nm_smooth_win", i32), ("nm_use_compressor", i32), ("nm_use_max_limit", i32),
                ("nm_rms_norm_fact", f32), ("nm_rms_floor", f32), ("nm_compressor_exp", f32), ("nm_lin_amp_scale", f32),
                ("nm_lin_amp_off", f32), ("nm_mel_amp_scale", f32), ("wn_gate_activation", i32),
                ("wn_disable_conditioning", i32), ("n_precond", i32), ("precond_channels", i32 * MBX_MAX_PRECOND),
                ("spect_preserve_energy", i32), ("wt_subharm_channels", i32), ("wt_sinusoid_as_fun", i32), ("ps_off", i32),
                ("no_pqmf", i32), ("n_wn_blocks", i32), ("wn_block_channels", i32 * MBX_MAX_WN_BLOCKS),
                ("wn_block_ups", i32 * MBX_MAX_WN_BLOCKS), ("pulse_pqmf_taps", i32), ("ps_subband_gain", i32),
                ("wn_causal", i32), ("wn_conv_form", i32), ("batch_invariant", i32), ("wn_keep_skip", i32),
                ("wn_keep_start", i32), ("calib_fraction", f32), ("tune_gate_shape", i32), ("tune_resskip_wave_tiles", i32),
                ("tune_resskip_split", i32), ("nm_use_pinv", i32), ("nm_win_norm", f32), ("wn_precision", i32),
                ("f0_accumulate", i32)]


class mbx_conv_form_info(ctypes.Structure):
    _fields_ = [("struct_size", i32), ("requested", i32), ("form", i32), ("stream_form", i32), ("calibrated", i32),
                ("batch_invariant", i32), ("fold_skip", i32), ("fold_start", i32), ("split_f16_layers", i32),
                ("split_f16_gate_layers", i32), ("err_f43", f32), ("err_f23", f32), ("ref_max", f32), ("threshold", f32),
                ("err_split", f32), ("split_rejected", i32), ("f0_float64_chain", i32), ("n_gate_layers", i32),
                ("gate_kernel", i32 * MBX_MAX_WN_LAYERS)]


GATE_KERNEL_NAMES = {0: "none", 1: "direct", 2: "f23", 3: "f43", 4: "f43_psplit", 5: "f43_hsplit", 6: "f43_strided",
                     7: "f43_strided_psplit", 8: "folded_start", 9: "split_f16", 10: "split_f16_wide",
                     11: "split_f16_f32h"}


class mbx_kernel_report_info(ctypes.Structure):
    _fields_ = [("struct_size", i32), ("n_resskip_layers", i32), ("resskip_kernel", i32 * MBX_MAX_WN_LAYERS),
                ("tail_kernel", i32), ("tail_folded", i32), ("gate_block_channels", i32 * MBX_MAX_WN_LAYERS)]


class mbx_plan_info(ctypes.Structure):
    _fields_ = [("struct_size", i32), ("n_layers", i32), ("gate_kernel", i32 * MBX_MAX_WN_LAYERS),
                ("gate_kernel_f32", i32 * MBX_MAX_WN_LAYERS), ("gate_block_channels", i32 * MBX_MAX_WN_LAYERS),
                ("resskip_kernel", i32 * MBX_MAX_WN_LAYERS), ("tail_kernel", i32), ("tail_folded", i32), ("planes_only", i32)]


# MBX_RESSKIP_K_* / MBX_TAIL_K_* of include/mbexwn.h (mbx_kernel_report)
RESSKIP_KERNEL_NAMES = {0: "none", 1: "conv1d", 2: "packed64", 3: "packed128", 4: "wide11_res10", 5: "wide11", 6: "wide6x2",
                        7: "wave11", 8: "wave12", 9: "wave6x2", 10: "wave4x3", 11: "split_f16"}
TAIL_KERNEL_NAMES = {0: "none", 1: "unfused", 2: "tail2_nj4", 3: "tail2_nj8", 4: "tail2_nj12", 5: "tail2_nj20", 6: "tail2_nj22",
                     7: "tail"}

CONV_FORMS = {"auto": 0, "direct": 1, "f23": 2, "f43": 3}


class mbx_forward_options(ctypes.Structure):
    _fields_ = [("struct_size", i32), ("transposition", f32), ("f0", vp), ("state_in", vp), ("state_out", vp),
                ("active_begin", i32), ("active_frames", vp), ("wn_begin", i32), ("wn_frames", vp),
                ("active_max_frames", i32), ("wn_max_frames", i32), ("sub_store", vp), ("sub_store_rows", i32),
                ("sub_carry", vp), ("layer_store", vp), ("layer_store_floats", i32), ("layer_carry", vp), ("layer_rows", i32),
                ("fe_store", vp), ("fe_ring_frames", i32), ("fe_pos", vp), ("fe_new_frames", i32), ("fe_margin_frames", i32),
                ("fe_end_frames", i32),
                # per-frame pitch control; struct_size may also be the offset of f0_frames (all three NULL)
                ("f0_frames", vp), ("f0_scale", vp), ("f0_item_mask", vp)]


class mbx_tensor(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char_p), ("data", P(f32)), ("ndim", i32), ("shape", i64 * 4)]


STRUCTS = [mbx_subnet_op, mbx_config, mbx_tensor, mbx_conv_form_info, mbx_kernel_report_info, mbx_plan_info, mbx_forward_options]

# ------------------------------------------------------------------------------------------------
# THE table: header -> [(function, restype, argtypes)] in the header's order.  i32 as a restype is mbx_status.  A device
# buffer is bound as vp (callers pass tensor.data_ptr()); a typed pointer is a host pointer that ctypes checks.
# ------------------------------------------------------------------------------------------------
i64p, cstr = P(i64), ctypes.c_char_p
_forward = [vp, vp, vp, i32, i32, vp, vp, vp, size_t]   # handle, mel, n_frames, batch, max_frames, noise, audio, workspace, bytes
_conv1d = [vp, vp, i32, i32, i32, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp]
_mel_tables = [vp, vp, vp, vp, vp, f32, vp]             # window, twiddle, basis, bin_lo, bin_hi, eps, out
_f0_frames = [vp, i64, i32, vp, vp, vp, i32, i32, i32, i32, i32]   # audio, stride, batch, n_samples, centres, n_frames, ... tau_max
TABLE = {
    "mbexwn.h": [
        ("mbx_last_error", cstr, []),
        ("mbx_create", i32, [P(mbx_config), P(mbx_tensor), i32, i32, P(vp)]),
        ("mbx_destroy", i32, [vp]),
        ("mbx_conv_form", i32, [vp, P(mbx_conv_form_info)]),
        ("mbx_kernel_report", i32, [vp, P(mbx_kernel_report_info)]),
        ("mbx_plan", i32, [vp, i32, i32, P(mbx_plan_info)]),
        ("mbx_calibrate", i32, [vp, vp, vp, i32, i32, vp, vp, size_t, vp]),
        ("mbx_workspace_size", size_t, [vp, i32, i32]),
        ("mbx_forward", i32, _forward + [vp]),
        ("mbx_forward_stream", i32, _forward + [vp, vp, vp]),
        ("mbx_layer_state_info", i32, [vp, P(i32), P(i32), P(i32)]),
        ("mbx_forward_ex", i32, _forward + [P(mbx_forward_options), vp]),
        ("mbx_window_advance", i32, [vp, vp, vp, vp, vp, i32, i32, i32, vp]),
        ("mbx_window_update", i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
        ("mbx_emit_rows", i32, [vp, vp, i64, i32, i64, i64, vp, vp]),
        ("mbx_stage", i32, [vp, cstr, P(vp), i64p, i64p]),
        ("mbx_profile_enable", i32, [vp, i32]),
        ("mbx_profile_read", i32, [vp, cstr, P(ctypes.c_double), i64p]),
        ("mbx_profile_read_launches", i32, [vp, cstr, P(f32), i64, i64p]),
        ("mbx_clock_probe", i32, [vp, vp, i64, vp]),
        ("mbx_pqmf_synthesis", i32, [vp, vp, i32, i32, vp, vp]),
        ("mbx_conv1d", i32, _conv1d),
        ("mbx_conv1d_f64acc", i32, _conv1d),
        ("mbx_lin_interp", i32, [vp, vp, i32, i32, i32, i32, vp, vp]),
        ("mbx_wavetable", i32, [vp, vp, i32, i32, vp, vp, vp, vp]),
        ("mbx_stft_filter", i32, [vp, vp, vp, vp, i32, i32, vp, vp, vp]),
        ("mbx_mel_analysis", i32, [vp, vp, i32, i32, i32, i32, i32, i32] + _mel_tables + [i32, vp]),
        ("mbx_encode_flac16", i32, [vp, i64, i32, i64p, i32, vp, vp, i64, vp, vp]),
        ("mbx_norm_mel", i32, [vp, vp, vp, i32, i32, vp, vp, vp, vp])],
    "mbexwn_audio.h": [("mbxa_resample_poly", i32, [vp, vp, i32, i32, i32, i32, vp, i32, vp, i32, vp])],
    "mbexwn_live.h": [
        ("mbxl_ring_append", i32, [vp, i64, vp, i32, i32, vp, i32, i32, vp]),
        ("mbxl_mel_frames", i32, [vp, i32, i32, vp, i32, i32, i32, i32, i32, i32] + _mel_tables + [vp])],
    "mbexwn_live_resample.h": [
        ("mbxr_resample_rings", i32, [vp, i32, i32, vp, i32, i32, i32, i32, vp, i32, vp, i32, i32, vp])],
    "mbexwn_live_out.h": [("mbxo_resample_emit", i32, [vp, i32, i32, vp, i32, i32, i32, i32, vp, i32, vp, i64, vp])],
    "mbexwn_flac.h": [("mbxf_encode_flac16_fixed", i32, [vp, i64, i32, i64p, i32, vp, vp, i64, vp, vp, vp, vp, vp])],
    "mbexwn_noise.h": [("mbxn_fill_normal", i32, [vp, i64, i32, vp, vp, vp, i32, vp])],
    "mbexwn_warp.h": [("mbxw_mel_frames_at", i32, [vp, i64, i32, vp, vp, vp, i32, i32, i32, i32] + _mel_tables + [vp])],
    "mbexwn_envelope.h": [
        ("mbxe_warp_envelope", i32, [vp, i64, i32, vp, i32, i32, vp, vp, vp, vp]),
        ("mbxe_forward", i32, _forward + [P(mbx_forward_options), vp, vp, vp, vp])],
    "mbexwn_pitch.h": [("mbxp_track_f0", i32, _f0_frames + [f32, f32, vp, vp, vp])],
    # thresholds and weights are HOST pointers
    "mbexwn_contour.h": [
        ("mbxc_f0_candidates", i32, _f0_frames + [f32, P(f32), P(f32), i32, i32, vp, vp, vp, vp]),
        ("mbxc_decode_f0", i32, [vp, vp, vp, vp, i32, i32, i32, f32, f32, vp, vp, vp])],
    # rings, n_slots, ring_samples, desc, n_streams, max_new_frames, hop, sample_rate, window, tau_min, tau_max, ...
    "mbexwn_live_pitch.h": [("mbxt_f0_frames", i32, [vp, i32, i32, vp, i32, i32, i32, i32, i32, i32, i32, f32, f32, vp, vp, vp])],
    # the streaming tracker's ring arguments, then mbxc_f0_candidates' rule (thresholds and weights are HOST pointers) and
    # tables; tables, desc, n_streams, max_new_frames, hop, state, n_slots, lag, sample_rate, w_jump, w_switch, f0, periodicity, max_out
    "mbexwn_live_contour.h": [
        ("mbxv_f0_candidate_frames", i32, [vp, i32, i32, vp, i32, i32, i32, i32, i32, i32, i32, f32, P(f32), P(f32), i32, i32,
                                           vp, vp, vp, vp]),
        ("mbxv_lag_state_words", size_t, []),
        ("mbxv_decode_f0_frames", i32, [vp, vp, vp, vp, i32, i32, i32, vp, i32, i32, i32, f32, f32, vp, vp, i32, vp])],
    # mel_a, mel_b, n_frames_a, n_frames_b, batch, max_frames_a, max_frames_b, n_mels, band, cost, stream
    "mbexwn_align.h": [
        ("mbxg_local_cost", i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp]),
        ("mbxg_align_workspace_size", size_t, [i32, i32, i32]),
        ("mbxg_align_path", i32, [vp, vp, vp, i32, i32, i32, vp, size_t, vp, vp, vp, vp, vp])],
    # n_samples, hops, coefs and targets are HOST arrays, abs_gate and ceiling HOST pointers to one double
    "mbexwn_level.h": [
        ("mbxl_measure", i32, [vp, i64, i32, i64p, P(i32), P(ctypes.c_double), P(ctypes.c_double), vp, i32, vp, i32, vp, vp]),
        ("mbxl_gains", i32, [vp, i32, P(ctypes.c_double), vp, P(ctypes.c_double), i32, vp, vp]),
        ("mbxl_apply", i32, [vp, i64, i32, i64p, vp, vp, i64, vp])],
    # n_samples is a HOST array; audio, stride, batch, n_samples, gains, ceiling, h, hold, weights, taps, n_taps, out, ...
    "mbexwn_limiter.h": [
        ("mbxd_limit", i32, [vp, i64, i32, i64p, vp, f32, i32, i32, vp, vp, i32, vp, i64, vp, vp, i64, vp]),
        ("mbxd_limit_workspace_floats", size_t, [i64, i32, i32, i32, i32]),
        ("mbxd_limit_emit", i32, [vp, i32, i32, vp, i32, i32, f32, i32, i32, vp, vp, i64, vp, vp])],
}


def symbols(header):
    """The functions include/<header> declares, in its order."""
    return [name for name, _, _ in TABLE[header]]


def all_symbols():
    return [name for header in TABLE for name in symbols(header)]


_STATUS_EXC = {1: ValueError, 2: RuntimeError, 3: RuntimeError, 4: NotImplementedError}

_lib = None


def load_library():
    """Load libmbexwn_hip.so (built in-tree by mbexwn_vocoder_amd.build). Fails loudly when absent."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch must be loaded first: the engine works on torch's device pointers and streams, so both have to
    # live in ONE HIP runtime instance (torch bundles libamdhip64.so.7; loading ours first would give the
    # process a second, separate runtime).
    import torch  # noqa: F401
    # MBX_LIB_PATH: another build of the same library (kernel experiments, scripts/experiments/, whose ablated kernels
    # produce wrong audio on purpose) -- never a fallback; said on stderr so that a stale variable cannot go unnoticed
    path = os.environ.get("MBX_LIB_PATH") or LIB_PATH
    if path != LIB_PATH:
        print(f"mbexwn_vocoder_amd: MBX_LIB_PATH overrides the product library: loading {path}", file=sys.stderr)
    if not os.path.exists(path):
        raise RuntimeError(f"HIP extension {path} is missing: run `python -m mbexwn_vocoder_amd.build` "
                           "(there is no CPU fallback for the mel-inversion path)")
    lib = ctypes.CDLL(path)
    for functions in TABLE.values():
        for name, restype, argtypes in functions:
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


def _check(status):
    if status != 0:
        msg = load_library().mbx_last_error().decode("utf-8", "replace")
        raise _STATUS_EXC.get(status, RuntimeError)(f"mbexwn_hip: {msg}")
