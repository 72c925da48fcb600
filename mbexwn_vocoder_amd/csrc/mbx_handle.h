// The engine's handle and what mbx_create.hip, mbx_forward.hip and mbx_api.hip share: the last-error string, the uploaded
// tensors and the records that resolve them once (mbx_create), workspace carving, the argument builders of the launch
// sequence.  mbx_stages.hip, whose entry points take no handle, includes it for fail, launch_status and HIP_TRY alone.
// Internal: the C ABI is include/mbexwn.h and the eleven headers beside it.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/mbexwn.h"
#include "mbx_kernels.h"

namespace mbx_host {

inline thread_local std::string g_last_error;

inline mbx_status fail(mbx_status st, const std::string &msg) {
    g_last_error = msg;
    return st;
}

// the end of an entry point that only enqueued kernels: the launch error, if there is one, behind `prefix`
inline mbx_status launch_status(const char *prefix = "") {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? MBX_OK : fail(MBX_ERR_HIP, std::string(prefix) + hipGetErrorString(e));
}

#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t err__ = (expr);                                                                     \
        if (err__ != hipSuccess)                                                                       \
            return fail(MBX_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(err__));            \
    } while (0)

struct DevTensor {
    float *ptr = nullptr;
    int ndim = 0;
    long long shape[4] = {0, 0, 0, 0};
    long long count = 0;
};

struct StageRef {
    const void *ptr = nullptr;
    long long count = 0, stride = 0;
};

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Makes the handle's device current for the duration of a call and puts the caller's device back afterwards, so
// that an engine can be created for / used from a thread whose current device is another one.
struct DeviceGuard {
    int prev = -1;
    bool switched = false, ok = true;
    explicit DeviceGuard(int device) {
        ok = hipGetDevice(&prev) == hipSuccess;
        if (ok && prev != device) {
            ok = hipSetDevice(device) == hipSuccess;
            switched = ok;
        }
    }
    DeviceGuard(const DeviceGuard &) = delete;
    ~DeviceGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
};

// ---- the tensors of the launch sequence, resolved once at mbx_create (mbx_handle::tensors never changes afterwards).
// A required tensor is non-null on every handle mbx_create returned; an optional weight image is non-null only where
// the host supplied it with the shape its kernel reads (resolve_tensors in mbx_create.hip holds every such predicate).

// one op of a sub-net (F0-net, VTF-net, conditioning chain): convolution weights, PReLU slopes
struct SubnetOpTensors {
    const DevTensor *w = nullptr, *b = nullptr, *alpha = nullptr;
    const double *w64 = nullptr;      // "<layer>.w64": float64 weights of the right size, 8-byte aligned
};

// the images of one folded res/skip layer; for layer 0 also those with the start convolution folded in (rows [a0 | x'])
struct FoldImages {
    const DevTensor *fold = nullptr, *wide = nullptr, *wave = nullptr, *f16 = nullptr;
};

struct WnLayerTensors {
    const DevTensor *w = nullptr, *b = nullptr;                          // conv1D_<l>.w / .b
    const DevTensor *wino4w = nullptr, *wino2w = nullptr, *gate_f16 = nullptr, *start_fold = nullptr;
    const DevTensor *res_w = nullptr, *res_b = nullptr, *packed = nullptr, *fold_b = nullptr;    // res_skip_<l>.*
    FoldImages plain, start;          // .fold* and .fold_start*
    FoldImages run;                   // the set the layer runs with: start for layer 0 under mbx_handle::fold_start, else plain
};

// the WN_IMG_* bits of a layer (wn_plan.h): which of its weight images are there, the fold set being the one it runs with
inline unsigned layer_images(const WnLayerTensors &t) {
    return (t.wino4w ? mbx::WN_IMG_WINO4W : 0) | (t.wino2w ? mbx::WN_IMG_WINO2W : 0) | (t.run.fold ? mbx::WN_IMG_FOLD : 0) |
           (t.run.wide ? mbx::WN_IMG_WIDE : 0) | (t.run.wave ? mbx::WN_IMG_WAVE : 0) | (t.run.f16 ? mbx::WN_IMG_F16 : 0) |
           (t.packed ? mbx::WN_IMG_PACKED : 0);
}

struct WnBlockTensors {
    const DevTensor *start_w = nullptr, *start_b = nullptr, *end_w = nullptr, *end_b = nullptr, *end_packed = nullptr;
    const DevTensor *tail_fold = nullptr, *tail_fold_b = nullptr;
    const DevTensor *up_w = nullptr, *up_b = nullptr;                    // "up<b>": the sub-pixel convolution behind the block
    std::vector<WnLayerTensors> layer;
    std::vector<SubnetOpTensors> cond;                                   // its conditioning chain (block 0: mbx_handle::cond_ops)
};

struct HandleTensors {
    const DevTensor *post_w = nullptr, *post_b = nullptr;
    const DevTensor *wavetables = nullptr, *pulse_ana = nullptr, *hann = nullptr, *inv_win = nullptr;
    const DevTensor *ceps_windows = nullptr, *ceps_log10f0 = nullptr, *f0_smooth = nullptr;
    const DevTensor *nm_inv_enorm = nullptr, *nm_pinv = nullptr, *nm_gwin = nullptr, *nm_smooth_win = nullptr;
    std::vector<SubnetOpTensors> f0, vtf;                                // parallel to mbx_config.f0_ops / vtf_ops
};

}  // namespace mbx_host

// stages of the launch sequence that mbx_profile_read can report (names: kProfNames in mbx_api.hip)
enum { PROF_GATE = 0, PROF_RES_SKIP, PROF_FRONTEND, PROF_WAVETABLE, PROF_START, PROF_TAIL, PROF_PQMF, PROF_STFT_FILTER,
       PROF_OVERLAP_ADD, PROF_NORM_MEL, PROF_GATE0, PROF_RES_SKIP_F16, PROF_KINDS };

struct mbx_handle {
    mbx_config cfg;
    int device = 0;
    char *arena = nullptr;
    size_t arena_bytes = 0;
    std::map<std::string, mbx_host::DevTensor> tensors;
    mbx_host::HandleTensors tab;                  // post-net, tables, sub-net ops
    std::vector<mbx_host::WnBlockTensors> wn;     // per WaveNet block ([0]: "wn.", the only one of a single-block model)
    std::map<int, std::pair<float *, float *>> lerp;   // interpolation factor -> (w0, w1)
    float *twiddle = nullptr;
    float *zeros = nullptr;   // 256 bytes of zeros (padding source of the LDS-DMA GEMMs)
    float *poly = nullptr;
    float *poly_t = nullptr;          // the same table as the MFMA B operand: (4 * ceil(K / 4), 16), K = poly_ndm * subbands, zero padded
    int poly_ndm = 0, poly_dm_min = 0;
    std::map<std::string, mbx_host::StageRef> stages;
    // derived
    int f0_time_factor = 1, vtf_time_factor = 1;
    long long subnet_buf_per_frame = 0;   // floats per frame of one ping-pong buffer
    mbx::WnPolicy pol;                    // what kernel selection depends on (wn_plan.h): the form, the tuning pins, split precision, folds, images
    mbx::WnPlan last_plan;                // the plan of the most recent forward (mbx_conv_form, mbx_kernel_report); n_layers == 0: none yet
    bool f0_full64 = false;               // mbx_config.f0_accumulate == MBX_F0_ACC_F64 and the F0-net has the shape (conv [prelu | leaky])* head
                                          // with its "<layer>.w64" tensors: float64 weights and hidden layers (f0_chain_is_full64)
    std::vector<mbx_subnet_op> cond_ops;  // pre-conditioning convolutions + the conditioning layer (empty: conditioning disabled)
    long long cond_buf_per_frame = 0;     // floats per frame of a ping-pong buffer of that chain (0: no pre-conditioning layers)
    // several WaveNet blocks (mbx_config.n_wn_blocks > 1; empty: the single-block path)
    struct WnBlock {
        int C = 0, ups = 1, spf = 0, ccu = 0;      // channels, upsampling factor behind the block, rows per frame, conditioning rows per frame
        std::string prefix;                        // "wn." | "wn1." ...
        std::vector<mbx_subnet_op> cond_ops;       // its pre-conditioning + conditioning chain (empty: conditioning disabled)
    };
    std::vector<WnBlock> blocks;
    long long mb_hc_per_frame = 0;                 // max over the blocks of rows per frame x channels
    float calib_err_split = -1.f;    // max |audio(split precision) - audio(float32 direct form)| of the calibration run
    int split_rejected = 0;          // the calibration switched the split precision off (error above the threshold, or not finite)
    // what mbx_conv_form reports
    int calibrated = 0;
    float calib_err43 = -1.f, calib_err23 = -1.f, calib_ref = 0.f, calib_threshold = 0.f;
    // bench-only kernel timing (mbx_profile_*): one event pool per stage of the launch sequence
    bool profiling = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool[PROF_KINDS];
    size_t ev_used[PROF_KINDS] = {};
};

namespace mbx_host {

struct Workspace {
    float *mel_norm, *nm_a, *nm_b;
    double *f0h0, *f0h1;   // float64 hidden layers of the F0-net (mbx_handle::f0_full64)
    float *sub0, *sub1, *sub2, *sub3, *sub4, *sub5, *f0_wide, *f0, *cum, *chunk_last, *pulse, *cond, *h, *a, *skip, *wn_out, *sub, *exc, *ceps, *frames;
    float *mb_h, *mb_a, *mb_skip, *mb_y0, *mb_y1, *mb_cond[MBX_MAX_WN_BLOCKS];   // several WaveNet blocks only
    float *pulse_ana;   // PQMF analysis of the pulse signal (pulse_pqmf_taps > 0): the WaveNet's excitation rows
    float *h16;         // split half precision: the hidden state as fp16 planes (ConvArgs::h_split), round_up(C, 8) words per row
    int *ceps_index;
    size_t total;
};

inline Workspace carve(const mbx_handle *hd, char *base, int B, int T) {
    const mbx_config &c = hd->cfg;
    Workspace w;
    size_t off = 0;
    auto take = [&](size_t n_floats) {
        char *p = base ? base + off : nullptr;
        off += align_up(n_floats * sizeof(float), 256);
        return reinterpret_cast<float *>(p);
    };
    const size_t BT = (size_t)B * T;
    const size_t npulse = (size_t)T * c.pulse_per_frame, nsteps = (size_t)T * c.steps_per_frame;
    const int chunks = (int)((npulse + c.phase_chunk - 1) / c.phase_chunk) + 1;
    const bool nm = c.nm_iters > 0;
    w.mel_norm = take((nm || hd->f0_full64) ? BT * c.mel_channels : 0);    // (also: aligned copy of a misaligned mel for the float64 F0 chain)
    w.nm_a = take(nm ? BT : 0);
    w.nm_b = take(nm ? BT : 0);
    w.sub0 = take(BT * hd->subnet_buf_per_frame);
    w.sub1 = take(BT * hd->subnet_buf_per_frame);
    w.sub2 = take(BT * hd->subnet_buf_per_frame);   // VTF-net ping-pong (its convolutions share launches with the F0-net's)
    w.sub3 = take(BT * hd->subnet_buf_per_frame);
    w.f0h0 = reinterpret_cast<double *>(take(hd->f0_full64 ? 2 * BT * hd->subnet_buf_per_frame : 0));
    w.f0h1 = reinterpret_cast<double *>(take(hd->f0_full64 ? 2 * BT * hd->subnet_buf_per_frame : 0));
    w.sub4 = take(BT * hd->cond_buf_per_frame);     // pre-conditioning layers (usually none: zero floats)
    w.sub5 = take(BT * hd->cond_buf_per_frame);
    // an F0-net with a bare ["L", up] entry runs at a multiple of the pulse rate and is cut to it (reference
    // custom_pulsed_generator.py:57-60, 787): the uncut contour lives here
    w.f0_wide = take(hd->f0_time_factor > c.pulse_per_frame ? BT * hd->f0_time_factor : 0);
    w.f0 = take(B * npulse);
    w.cum = take(B * npulse);
    w.chunk_last = take((size_t)B * chunks);
    w.pulse = take(B * npulse * (1 + c.wt_subharm_channels));
    w.pulse_ana = take(c.pulse_pqmf_taps > 0 ? B * npulse : 0);
    w.cond = take(BT * 2 * c.wn_channels * c.cond_conv_upsampling);
    w.h = take(B * nsteps * c.wn_channels);
    w.a = take(B * nsteps * (c.wn_channels + 16));   // layer 0 appends the excitation channels to its rows (wn_gate0.hip)
    w.skip = take(B * nsteps * c.wn_channels);
    w.h16 = take(hd->pol.split_f16_gate ? B * nsteps * (size_t)((c.wn_channels + 7) / 8 * 8) : 0);
    w.wn_out = take(B * nsteps * c.wn_out_channels);
    w.sub = take(B * nsteps * c.subbands);
    w.exc = take(BT * c.hop_size);
    w.ceps = take(BT * c.n_ceps);
    w.ceps_index = reinterpret_cast<int *>(take(BT));
    w.frames = take(BT * c.stft_win);
    const bool mb = !hd->blocks.empty();
    w.mb_h = take(mb ? BT * hd->mb_hc_per_frame : 0);
    w.mb_a = take(mb ? BT * hd->mb_hc_per_frame : 0);
    w.mb_skip = take(mb ? BT * hd->mb_hc_per_frame : 0);
    w.mb_y0 = take(mb ? B * nsteps * c.wn_out_channels : 0);
    w.mb_y1 = take(mb ? B * nsteps * c.wn_out_channels : 0);
    for (int b = 0; b < MBX_MAX_WN_BLOCKS; ++b)
        w.mb_cond[b] = take(mb && b >= 1 && b < (int)hd->blocks.size() ? BT * hd->blocks[b].ccu * 2 * hd->blocks[b].C : 0);
    w.total = off;
    return w;
}

inline mbx::ConvArgs conv_args(const float *x, long long x_bstride, int ldx, const int *n_frames, int rpf, int max_rows,
                               int batch, const DevTensor *w, const DevTensor *bias, int ks, int cin, int cout, int dil,
                               int pad_l, int pad_mode, float *out, long long out_bstride, int ldo) {
    mbx::ConvArgs a;
    std::memset(&a, 0, sizeof(a));
    a.x = x;
    a.x_bstride = x_bstride;
    a.ldx = ldx;
    a.n_frames = n_frames;
    a.rows_per_frame = rpf;
    a.max_rows = max_rows;
    a.batch = batch;
    a.w = w->ptr;
    a.bias = bias ? bias->ptr : nullptr;
    a.cin = cin;
    a.cout = cout;
    a.ks = ks;
    a.dil = dil;
    a.pad_l = pad_l;
    a.pad_mode = pad_mode;
    a.out = out;
    a.out_bstride = out_bstride;
    a.ldo = ldo;
    return a;
}

// Head of the F0-net: [conv 1x1 -> 1 channel] [lin] ([act]) at the end of the op list (reference
// custom_pulsed_generator.py:126-146): one float64 kernel (launch_f0_head) under mbx_config.f0_accumulate == MBX_F0_ACC_F64
inline bool is_f0_head(const mbx_subnet_op *ops, int n_ops, int i) {
    const int n_tail = n_ops - i;
    return ops[i].kind == MBX_OP_CONV && ops[i].ks == 1 && ops[i].cout == 1 && ops[i].up == 1 && (n_tail == 2 || n_tail == 3) &&
           ops[i + 1].kind == MBX_OP_LIN && (n_tail == 2 || ops[i + 2].kind == MBX_OP_ACT);
}

// brackets one launch with events when profiling is on
struct ScopedEvents {
    mbx_handle *hd;
    int kind;
    hipStream_t stream;
    hipEvent_t stop = nullptr;
    ScopedEvents(mbx_handle *h, int k, hipStream_t s) : hd(h), kind(k), stream(s) {
        if (!hd->profiling) return;
        auto &pool = hd->ev_pool[kind];
        if (hd->ev_used[kind] == pool.size()) {
            hipEvent_t a, b;
            if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
            pool.push_back({a, b});
        }
        auto &pr = pool[hd->ev_used[kind]++];
        (void)hipEventRecord(pr.first, stream);
        stop = pr.second;
    }
    ~ScopedEvents() {
        if (stop) (void)hipEventRecord(stop, stream);
    }
};

inline mbx::WaveTableConsts wavetable_consts(const mbx_handle *hd) {
    const mbx_config &c = hd->cfg;
    mbx::WaveTableConsts k;
    k.tables = hd->tab.wavetables->ptr;
    k.n_period = c.wt_n_period;
    k.n_tables = c.wt_n_tables;
    k.pulse_rate = c.pulse_rate;
    k.nominal_f0 = c.wt_nominal_f0;
    k.min_tf = c.wt_min_transposition;
    k.max_tf = c.wt_max_transposition;
    k.grid_norm = c.wt_grid_norm;
    k.chunk = c.phase_chunk;
    k.n_sub = c.wt_subharm_channels;
    k.sin_fun = c.wt_sinusoid_as_fun;
    return k;
}

inline mbx::NormMelConsts norm_mel_consts(const mbx_handle *hd) {
    const mbx_config &c = hd->cfg;
    mbx::NormMelConsts k;
    k.iters = c.nm_iters;
    k.mel_channels = c.mel_channels;
    k.hop = c.hop_size;
    k.win = c.stft_win;
    k.smooth_win = c.nm_smooth_win;
    k.cut = c.nm_smooth_win / 2 + 2 * c.hop_size - c.stft_win / 2;
    k.rms_norm_fact = c.nm_rms_norm_fact;
    k.rms_floor = c.nm_rms_floor;
    k.compressor_exp = c.nm_compressor_exp;
    k.lin_amp_scale = c.nm_lin_amp_scale;
    k.lin_amp_off = c.nm_lin_amp_off;
    k.mel_amp_scale = c.nm_mel_amp_scale;
    k.use_compressor = c.nm_use_compressor;
    k.use_max_limit = c.nm_use_max_limit;
    k.inv_enorm = hd->tab.nm_inv_enorm->ptr;
    k.pinv = c.nm_use_pinv ? hd->tab.nm_pinv->ptr : nullptr;
    k.n_bins = c.fft_size / 2 + 1;
    k.win_norm = c.nm_win_norm;
    k.gwin = hd->tab.nm_gwin->ptr;
    k.smooth_win_table = hd->tab.nm_smooth_win->ptr;
    return k;
}

inline mbx::StftConsts stft_consts(const mbx_handle *hd) {
    const mbx_config &c = hd->cfg;
    mbx::StftConsts k;
    k.hop = c.hop_size;
    k.win = c.stft_win;
    k.fft_size = c.fft_size;
    k.n_ceps = c.n_ceps;
    k.n_ceps_windows = c.n_ceps_windows;
    k.max_log_range = c.filter_max_log_range;
    k.preserve_energy = c.spect_preserve_energy;
    k.hann = hd->tab.hann->ptr;
    k.inv_win = hd->tab.inv_win->ptr;
    k.twiddle = hd->twiddle;
    k.ceps_windows = c.n_ceps_windows ? hd->tab.ceps_windows->ptr : nullptr;
    k.ceps_log10f0 = c.n_ceps_windows ? hd->tab.ceps_log10f0->ptr : nullptr;
    k.f0_smooth = c.n_ceps_windows ? hd->tab.f0_smooth->ptr : nullptr;
    k.pulse_per_frame = c.pulse_per_frame;
    return k;
}

// Geometry of the per-layer state a stream carries between ticks (mbx_forward_options.layer_store): layer l reaches
// r[l] rows to either side; it is exact up to row e_l = E - reach_rows + c[l] when the region ends at row E, with
// e_l = e_{l-1} - step[l] (step = the reach rounded up to even rows: the rows of the n_out-wide accumulator stay 8-byte
// aligned).  A slot keeps per layer l >= 1 the rows [e_l - r[l], e_l + step[l]) of h_l and [e_l, e_l + step[l]) of the
// accumulator.
// CAUSAL padding: layer l reads r[l] = 2 d rows in front of an output and none behind (ahead[l] = 0), so no layer's
// error at a region end spreads backwards: every layer is exact up to the same row e = E - reach_rows (the clamped
// conditioning tail only), c[l] = step[l] = 0, and a slot keeps per layer l >= 1 the rows [e - 2 d, e) of h_l (no
// accumulator rows: every layer adds to the same new rows).
struct LayerGeom {
    int floats, reach_rows, min_rows;
    int r[MBX_MAX_WN_LAYERS], ahead[MBX_MAX_WN_LAYERS], step[MBX_MAX_WN_LAYERS], c[MBX_MAX_WN_LAYERS];
    long long off[MBX_MAX_WN_LAYERS];
};

struct LayerOpts {
    float *store;
    int floats;
    const int32_t *carry;
    int rows;
};

// everything mbx_forward_stream / mbx_forward_ex add to mbx_forward (see mbx_forward_options in mbexwn.h)
struct ForwardExtras {
    const mbx::StreamState *st_in = nullptr;
    mbx::StreamState *st_out = nullptr;
    const float *f0_in = nullptr;
    float transposition = 1.f;
    // per-frame pitch control (mbx_forward_options.f0_frames / f0_scale / f0_item_mask): device (batch, max_frames) rows
    const float *f0_frames = nullptr, *f0_scale = nullptr;
    const int32_t *f0_item_mask = nullptr;
    // formant shift (mbxe_forward of include/mbexwn_envelope.h: env_factor / env_centres / env_mel): all three or none
    const float *env_factor = nullptr, *env_centres = nullptr;
    float *env_mel = nullptr;
    int active_begin = 0;
    const int32_t *active_frames = nullptr;
    int wn_begin = 0;
    const int32_t *wn_frames = nullptr;
    float *sub_store = nullptr;
    int sub_store_rows = 0;
    const int32_t *sub_carry = nullptr;
    int active_max_frames = 0, wn_max_frames = 0;
    const LayerOpts *lay = nullptr;
    float *fe_store = nullptr;
    int fe_ring_frames = 0, fe_new_frames = 0, fe_margin_frames = 0, fe_end_frames = 0;
    const int32_t *fe_pos = nullptr;
};

// mbx_create.hip: the form of the dilated convolution (mbx_config.wn_conv_form)
bool form_available(const mbx_handle *hd, int form);
void set_form(mbx_handle *hd, int form);
int current_form(const mbx_handle *hd);
// mbx_api.hip: the calibration mbx_create runs on the handle's own weights
mbx_status calibrate_on_synthetic_mel(mbx_handle *hd, bool forms);
// mbx_forward.hip
LayerGeom layer_geom(const mbx_handle *hd);
mbx::WnPlan plan_whole_items(const mbx_handle *hd, int batch, int max_frames);
mbx_status forward_impl(mbx_handle *hd, const float *mel, const int32_t *n_frames, int32_t batch, int32_t max_frames,
                        const float *noise, float *audio, void *workspace, size_t workspace_bytes, void *hip_stream,
                        const ForwardExtras &ex = ForwardExtras());

}  // namespace mbx_host
