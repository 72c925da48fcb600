// Internal launch interface between the C ABI (mbx_create.hip, mbx_forward.hip, mbx_api.hip, mbx_stages.hip) and the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mbexwn.h"   // MBX_RESSKIP_K_* / MBX_TAIL_K_*: what the res/skip and tail launchers return
#include "ring_rows.h"   // RingStore: the ring stores of the live stages, and their descriptor rows
#include "wn_plan.h"   // ConvArgs / Gate0Args (mbx_args.h), the WaveNet kernels' selectors and shape constants

namespace mbx {

// Gate of a WaveNet layer (reference custom_AE_layers.py:312-321): act(zt) * sigmoid(zs) with act = tanh (kind 0, gtu),
// z / (1 + |z|) (1, gfu), z / (1 + sqrt|z|) (2, gsu) or z itself (3, glu: accepted at :156, no branch at :312-318).  One
// reciprocal for the whole product:
//   tanh(zt) sigmoid(zs) = (t - 1) / ((t + 1)(1 + s)),  t = e^(2 zt), s = e^(-zs)   (zt is clamped where tanh is 1 in
//   float32, so t stays finite; s = inf gives 0, as it should);   zt / ((1 + |zt|)(1 + s)) etc. for the others.
// `kind` is a kernel argument: the branch is wave-uniform.
#if defined(__HIPCC__)
// Rows (frames, samples) of batch item b: its own count from the device array -- clamped into [0, bound], so that an item
// that claims more frames than the window holds is cut to the window instead of addressing past its buffers -- or the
// bound itself when the batch has no per-item lengths.
__device__ __forceinline__ int item_rows(const int *n_frames, int b, int per_frame, int bound) {
    if (!n_frames) return bound;
    const long long n = (long long)max(n_frames[b], 0) * per_frame;
    return n < bound ? (int)n : bound;
}

__device__ __forceinline__ float wn_gate_act(int kind, float zt, float zs) {
    const float sg = __builtin_amdgcn_exp2f(zs * -1.4426950408889634f);
    if (kind == 0) {
        const float t = __builtin_amdgcn_exp2f(fminf(zt, 15.f) * 2.885390081777927f);
        const float tp = t + 1.0f;
        return (t - 1.0f) * __builtin_amdgcn_rcpf(fmaf(sg, tp, tp));
    }
    if (kind == 3) return zt * __builtin_amdgcn_rcpf(1.0f + sg);
    const float az = fabsf(zt);
    const float den = 1.0f + (kind == 1 ? az : __builtin_amdgcn_sqrtf(az));
    return zt * __builtin_amdgcn_rcpf(fmaf(sg, den, den));
}
#endif

// ---------------------------------------------------------------------------------------------
// conv1d as an implicit GEMM on the fp32 matrix cores (conv_mfma.hip; the mel-rate sub-nets: conv_mel.hip)
// ---------------------------------------------------------------------------------------------

void launch_conv1d(const ConvArgs &a, int epilogue, hipStream_t stream);
// n <= 3 independent EPI_LINEAR convolutions; the mel-rate ones share one launch (conv_mel.hip)
void launch_conv1d_group(const ConvArgs *convs, int n, hipStream_t stream);
// one EPI_LINEAR convolution in a launch of its own with the mel-rate tiles (conv_mel.hip); false: the shape is not theirs,
// nothing was launched
bool launch_conv1d_mel_single(const ConvArgs &a, hipStream_t stream);
// ---- WaveNet layers.  Which kernel runs a layer, and whether the layer fits it, is decided on the host by the selectors of
// wn_plan.h; a launcher is told the instantiation, checks what the caller guarantees (non-null, aligned pointers), computes the
// grid and launches.  Return value: nullptr, or what is wrong with the pointers (nothing was launched).
// Winograd F(4,3) form on v_mfma_f32_16x16x4_f32, wave tile 16 groups x 64 columns (wn_winograd4w.hip); a.w = image of
// packing.pack_winograd4w_weights (ceil(C/32), ceil(C/8), 3072); k.shape: 0 = 256-row blocks, 1 = 128-row blocks whose waves
// split the six products, 2 = product-split blocks of half a column tile, 3 = 256-row blocks of TWO column tiles (d <= 16,
// cond_up >= 10; an odd last tile runs in 256-row blocks): same bits, all four
const char *launch_wn_gate_winograd4w(const ConvArgs &a, const GateChoice &k, hipStream_t stream);
// Winograd F(2,3) form on v_mfma_f32_16x16x4_f32 with wave-granular tiles (wn_winograd2w.hip: streams, per-layer regions,
// MBX_CONV_F23); a.w = image of packing.pack_winograd2w_weights (ceil(C/32), ceil(C/8), 2048)
const char *launch_wn_gate_winograd2w(const ConvArgs &a, hipStream_t stream);
// the dilated convolution + gate in split half precision, direct form (wn_gate_f16.hip; opt-in, mbx_config.wn_precision);
// a.w = image of packing.pack_gate_f16_weights (ceil(C/32), ceil(C/32), 6144); kernel: MBX_GATE_K_SPLIT_F16*
const char *launch_wn_gate_f16(const ConvArgs &a, int kernel, hipStream_t stream);
// First WaveNet layer with the start convolution folded into it (wn_gate0.hip)
const char *launch_wn_gate0(const Gate0Args &a, hipStream_t stream);
// the dynamic-LDS opt-ins of the kernels above, once per handle with its device current (mbx_create): WN_LDS_* bits granted
unsigned wn_gate_f16_lds_opt_in();
unsigned wn_gate_winograd4q_lds_opt_in();
// WaveNet residual/skip layer for large row counts (wn_resskip.hip); a.w = host-packed weights (ceil(cout/128), ceil(C/16), 2048);
// kernel: MBX_RESSKIP_K_PACKED64 | _PACKED128
const char *launch_wn_resskip(const ConvArgs &a, int kernel, hipStream_t stream);
// the same layer for large launches, one block owning all columns of its rows (wn_resskip_wide.hip); a.w = image of
// packing.pack_resskip_wide_weights (ceil(cin/8), ceil(cout/32), 256); kernel: MBX_RESSKIP_K_WIDE*
const char *launch_wn_resskip_wide(const ConvArgs &a, int kernel, hipStream_t stream);
// the same layer for small launches (one utterance, streaming ticks), tiled at wave granularity (wn_resskip_wave.hip);
// a.w = image of packing.pack_resskip_wave_weights (ceil(cin/16), 12, 512); kernel: MBX_RESSKIP_K_WAVE*
const char *launch_wn_resskip_wave(const ConvArgs &a, int kernel, hipStream_t stream);
// the same layer in split half precision (wn_resskip_f16.hip; opt-in, mbx_config.wn_precision); a.w = image of
// packing.pack_resskip_f16_weights (ceil(cin/32), 12, 1024); a.gate_act must be set (glu is refused)
const char *launch_wn_resskip_f16(const ConvArgs &a, hipStream_t stream);
// the pointers of a folded res/skip launch (wide, wave-tiled, split half precision): the workspace is carved in 256-byte
// pieces and tensors come from the device allocator, so a failure here is a bug of the caller
inline const char *wn_resskip_folded_pointers(const ConvArgs &a) {
    const bool ok = (uintptr_t)a.x % 16 == 0 && (uintptr_t)a.w % 16 == 0 && (uintptr_t)a.h % 8 == 0 && (uintptr_t)a.skip % 8 == 0 &&
                    (!a.bias || (uintptr_t)a.bias % 8 == 0) && a.zeros && a.h && a.skip;
    return ok ? nullptr : "folded res/skip layer: a pointer is null or not aligned";
}
// WaveNet end convolution + post-net in one pass over the skip tensor (wn_tail.hip); w_end_packed = host-packed
// weights (ceil(C/8), 2, 32, 4); kind: MBX_TAIL_K_TAIL2_* | MBX_TAIL_K_TAIL
const char *launch_wn_tail(int kind, const float *skip, long long skip_bstride, const int *n_frames, int rows_per_frame, int max_rows,
                           int batch, int C, const float *w_end_packed, const float *b_end, int n_out, const float *w_post,
                           const float *b_post, int M, const float *y_acc, float *y, long long y_bstride, float *sub,
                           long long sub_bstride, hipStream_t stream);

// ---------------------------------------------------------------------------------------------
// element-wise / bandwidth-type stages (elementwise.hip)
// ---------------------------------------------------------------------------------------------
// linear interpolation (B,rows,C) -> (B,rows*up,C), optional final activation and affine (y*scale+offset)
void launch_lin_interp(const float *x, long long x_bstride, const int *n_frames, int rows_per_frame, int max_rows,
                       int batch, int channels, int up, const float *w0, const float *w1, int act, float scale,
                       float offset, float *y, long long y_bstride, hipStream_t stream);
// Head of the F0-net in float64 (elementwise.hip::f0_head_kernel): 1x1 convolution cin -> 1 (+ bias), linear interpolation by
// `up`, final activation, y * scale + offset -- float32 in, one rounding to float32 at the end
// (reference custom_pulsed_generator.py:126-146, 773-791; custom_AE_layers.py:91-99)
// x32 or x64: the hidden layer as float32 or float64; w32 or w64 likewise
void launch_f0_head(const float *x32, const double *x64, long long x_bstride, int cin, const int *n_frames, int rows_per_frame,
                    int max_rows, int batch, const float *w32, const double *w64, const float *bias, int up, const float *w0,
                    const float *w1, int act, float scale, float offset, float *y, long long y_bstride, hipStream_t stream);
// y = act(x)*scale + offset on (B, rows, C)
// sub-band rows carried between the ticks of a stream (elementwise.hip); desc (batch, 5) int32 on the device
void launch_sub_carry(float *sub, long long sub_bstride, float *store, long long slot_stride, const int *desc, int batch,
                      int max_rows, int row_floats, int dir, hipStream_t stream);
// per-layer WaveNet state carried between the ticks of a stream (elementwise.hip); desc (batch, 3) int32 on the device
struct LayerCarryArgs {
    float *h;                 // (batch, rows, C) hidden state of the window
    long long h_bstride;
    int C;
    float *acc;               // (batch, rows, n_out) output accumulator of the window (folded skip path)
    long long acc_bstride;
    int n_out;
    float *store;             // (slots, slot_stride) caller's persistent buffer
    long long slot_stride, layer_off;   // floats: between slots, of this layer inside a slot
    const int *desc;          // (batch, 3): slot, end row of the stored state, end row of the state to store (-1: none)
    int inject;               // 0: desc[b][1] is ignored (nothing is taken from the store)
    int base_off;             // e_l - end: last exact row (+1) of this layer relative to the end row
    int h_before, h_rows;     // stored rows of h: [e_l - h_before, + h_rows)
    int acc_rows;             // stored rows of acc: [e_l, + acc_rows)
};
void launch_layer_carry(const LayerCarryArgs &a, int batch, hipStream_t stream);
// mel-rate front end (conditioning rows, cepstrum, F0 contour) carried between the ticks of a stream (elementwise.hip):
// per slot a ring of ring_frames frames of [cond | ceps | f0]; window frame f of item b lives at ring frame
// (pos[b] + f) % ring_frames.  Frames [0, first_new) of the window are read from the ring, frames [first_new, frames) --
// [first_new, n_frames[b]) with n_frames -- are written to it.
struct FrontendCarryArgs {
    float *cond, *ceps, *f0;          // (batch, frames * floats) window buffers
    int cond_floats, ceps_floats, f0_floats;
    int frames;
    const int *n_frames;              // (batch) or null
    float *store;                     // (slots, ring_frames, cond_floats + ceps_floats + f0_floats)
    int ring_frames;
    const int *pos;                   // (batch) ring frame of window frame 0
    const int *slot_desc;             // (batch, 5): [0] = slot of the item (the sub-band carry descriptors)
    int first_new;
    int skip_f0;                      // 1: the F0 lane is neither read nor written (no F0-net ran: the window's contour is
                                      // not this call's to copy, and every item takes its contour from f0_frames)
};
void launch_frontend_carry(const FrontendCarryArgs &a, int batch, hipStream_t stream);
// per-frame pitch control (mbx_forward_options.f0_frames / f0_scale / f0_item_mask) in place on the pulse-rate contour
// f0 (batch, max_frames * up): for the pulse samples of item b's own frames, base = LI(frames[b]) where the item takes
// the frames (frames given and mask null or mask[b] != 0), the contour as it stands otherwise; f0 = base * LI(scale[b])
// with scale given.  LI = lin_interp_kernel's arithmetic with the weight vectors w0 / w1 of `up`.  frames, scale:
// (batch, max_frames) or null; mask: (batch) or null
void launch_f0_control(const float *frames, const float *scale, const int *mask, const int *n_frames, int max_frames, int batch,
                       int up, const float *w0, const float *w1, float *f0, hipStream_t stream);
// device-resident streaming windows: shift every item's window left by step_frames and append the new frames
void launch_clock_probe(unsigned long long *out, unsigned long long real_ticks, hipStream_t stream);
bool launch_window_update(float *mel, const float *mel_new, float *noise, const float *noise_new, int batch, int win_frames,
                          int shift_frames, int keep_frames, int new_frames, int mel_channels, int steps_per_frame,
                          hipStream_t stream);
bool launch_window_advance(float *mel, const float *mel_new, float *noise, const float *noise_new, int batch, int frames,
                           int step_frames, int mel_channels, int steps_per_frame, hipStream_t stream);
void launch_activation(const float *x, long long x_bstride, const int *n_frames, int rows_per_frame, int max_rows,
                       int batch, int channels, int act, float scale, float offset, float *y, long long y_bstride,
                       hipStream_t stream);
// PReLU / leaky in place (used when a conv is not directly followed by its activation)
void launch_prelu(float *x, long long x_bstride, const int *n_frames, int rows_per_frame, int max_rows, int batch,
                  int channels, const float *alpha, float leaky, hipStream_t stream);
// sub-band gains of the ps_use_stft: false variant (reference custom_pulsed_generator.py:857-884, 670, 916-917):
// sub[b, r, m] *= lerp_{hop}(exp(log_gain[b, :, m] (- mean over m)))[r], log_gain (B, max_frames, M)
void launch_subband_gain(float *sub, long long sub_bstride, const float *log_gain, long long gain_bstride, const int *n_frames,
                         int max_frames, int rows_per_frame, int batch, int M, int hop, const float *w0, const float *w1,
                         int remove_mean, hipStream_t stream);
// PQMF analysis of the pulse signal (reference tf_preprocess.py:188-200): pulse (B, n_max) -> out (B, n_max) viewed as
// (rows, K): out[r, k] = sum_n ana[n, k] * pulse[r K + n - taps / 2], zero outside the item
void launch_pulse_analysis(const float *pulse, long long bstride, const int *n_frames, int samples_per_frame, int n_max,
                           int batch, const float *ana, int taps, int K, float *out, hipStream_t stream);
// WaveNet input: fold pulse (B, steps*pc) + noise (B, steps) and apply the start 1x1 conv -> h (B, steps, C)
void launch_wn_start(const float *pulse, long long pulse_bstride, const float *noise, long long noise_bstride,
                     float sigma, const int *n_frames, int steps_per_frame, int max_steps, int batch,
                     int pulse_channels, const float *w, const float *bias, int channels, float *h,
                     long long h_bstride, hipStream_t stream);

// ---------------------------------------------------------------------------------------------
// wavetable oscillator (wavetable.hip)
// ---------------------------------------------------------------------------------------------
struct WaveTableConsts {
    const float *tables;   // (n_period+1, n_tables)
    int n_period, n_tables;
    float pulse_rate, nominal_f0, min_tf, max_tf, grid_norm;
    int chunk;
    int n_sub;             // add_subharm_chans: extra channels sin(2 pi phase / ii), ii = 2 .. n_sub + 1, behind the pulse
    int sin_fun;           // use_sinusoid_as_fun: pulse = sin(2 pi phase) * 0.5 * (1 - cos(2 pi phase)), no table lookup
};
// carried phase-accumulator state of a stream (== mbx_stream_state of include/mbexwn.h)
struct StreamState {
    float cum;            // running sum of the chunk in progress, just in front of start_sample
    float offset_sum;     // un-wrapped sum of (chunk totals mod 1) of all finished chunks
    int pos_in_chunk;     // position of start_sample inside its 1000-sample chunk
    int start_sample;     // window-relative pulse sample the state applies to
    int save_sample;      // window-relative pulse sample whose state is written to the output (< start: none)
    int reserved;
};
// f0 (B, n_max) -> pulse (B, n_max, 1 + n_sub); cum / chunk_last are scratch: cum (B, n_max), chunk_last (B, n_chunks_max + 1)
void launch_wavetable(const WaveTableConsts &c, const float *f0, long long bstride, const int *n_frames,
                      int samples_per_frame, int n_max, int batch, float *pulse, float *phase_out, float *cum,
                      float *chunk_last, const StreamState *st_in, StreamState *st_out, hipStream_t stream);

// ---------------------------------------------------------------------------------------------
// PQMF synthesis (pqmf.hip)
// ---------------------------------------------------------------------------------------------
// x (B, steps, M) -> y (B, steps*M); poly = polyphase table (M, n_dm, M) with dm_min; poly_t = the same table as the MFMA
// B operand (4 * ceil(n_dm * M / 4), 16), zero padded, or null (M > 16)
void launch_pqmf(const float *x, long long x_bstride, const int *n_frames, int steps_per_frame, int max_steps,
                 int batch, int subbands, const float *poly, const float *poly_t, int n_dm, int dm_min, float *y,
                 long long y_bstride, hipStream_t stream);

// ---------------------------------------------------------------------------------------------
// STFT-domain envelope filter (stft_filter.hip)
// ---------------------------------------------------------------------------------------------
struct StftConsts {
    int hop, win, fft_size, n_ceps, n_ceps_windows;
    int preserve_energy;              // spect_filters_preserve_energy: cepstral coefficient 0 kept, H / rms_k |H|
    float max_log_range;
    const float *hann, *inv_win;      // (win)
    const float *twiddle;             // (fft_size/2, 2)
    const float *ceps_windows;        // (n_ceps_windows, n_ceps) or null
    const float *ceps_log10f0;        // (n_ceps_windows)
    const float *f0_smooth;           // (2*hop+1)
    int pulse_per_frame;
};
void launch_stft_filter(const StftConsts &c, const float *exc, long long exc_bstride, const float *ceps,
                        long long ceps_bstride, const int *index, const float *f0, long long f0_bstride,
                        int *index_out, const int *n_frames, int max_frames, int batch, float *frames,
                        hipStream_t stream);
// overlap-add of the windowed frames + slice -> audio (B, out_frames*hop), tail zeroed; max_frames = item stride of `frames`
void launch_overlap_add(const StftConsts &c, const float *frames, const int *n_frames, int max_frames, int out_frames, int batch,
                        float *audio, long long audio_bstride, hipStream_t stream);

// audio -> log-mel analysis (mel_analysis.hip); tables from the host module analysis.py
struct MelAnalysisArgs {
    const float *audio;       // (batch, max_samples)
    long long audio_bstride;
    const int *n_samples;     // (batch) or null
    int max_samples, batch;
    int win, hop, fft_size, n_mels;
    const float *window;      // (win)
    const float *twiddle;     // (fft_size/2, 2): exp(-2 pi i m / fft_size)
    const float *basis;       // (n_mels, fft_size/2 + 1) dense rows
    const int *bin_lo, *bin_hi;   // (n_mels) first / last non-zero bin of a row
    float eps;
    float log_eps;            // float32 nearest to log(eps); launch_mel_analysis fills it in
    float *out;               // (batch, max_frames, n_mels), frames of item b: n_samples[b] / hop + 1
    int max_frames;
};
bool launch_mel_analysis(const MelAnalysisArgs &a, hipStream_t stream);

// streaming mel analysis (mel_stream.hip; include/mbexwn_live.h: mbxl_ring_append, mbxl_mel_frames): a ring of the last
// ring_samples samples per stream slot, frames computed from it by absolute sample index with mel_frame.h's body
struct RingAppendArgs {
    const float *packed;          // (packed_samples) the new samples of every stream of the tick, back to back
    long long packed_samples;
    const long long *desc;        // (n_streams, 4): slot, abs_start, count, offset into packed
    int n_streams, max_count;     // max_count sizes the grid only: a larger count is still appended whole
    RingStoreOut rings;
};
struct MelStreamArgs {
    RingStore rings;
    const long long *desc;        // (n_streams, 4): slot, first_frame, n_frames, n_total (< 0: the stream is still open)
    int n_streams, max_new_frames;
    int win, hop, fft_size, n_mels;
    const float *window, *twiddle, *basis;
    const int *bin_lo, *bin_hi;
    float eps;
    float *out;                   // (n_streams, max_new_frames, n_mels); rows beyond a stream's n_frames are not written
};
// nullptr when the arguments describe a valid launch, else what is wrong with them
const char *check_ring_append(const RingAppendArgs &a);
void launch_ring_append(const RingAppendArgs &a, hipStream_t stream);
const char *check_mel_stream(const MelStreamArgs &a);
void launch_mel_stream(const MelStreamArgs &a, hipStream_t stream);

// polyphase FIR resampler of a ragged batch (resample_poly.hip; include/mbexwn_audio.h: mbxa_resample_poly)
constexpr int RS_TILE = 1024;                   // outputs per block; MBXA_RESAMPLE_TILE of the header
struct ResampleArgs {
    const float *audio;       // (batch, max_samples)
    const int *n_samples;     // (batch) or null
    int batch, max_samples;
    int up, down;
    const float *taps;        // (n_taps), natural order, gain included
    int n_taps;
    float *out;               // (batch, max_out); item b writes ceil(n_b * up / down) samples
    int max_out;
    int tiles, span_cap;      // launch_resample_poly fills these in: tiles per item, floats of the staged input span
};
// nullptr when the arguments describe a valid launch, else what is wrong with them
const char *check_resample_poly(const ResampleArgs &a);
void launch_resample_poly(const ResampleArgs &a, hipStream_t stream);

// streaming resampler (resample_stream.hip; include/mbexwn_live_resample.h: mbxr_resample_rings): from a ring store at the
// input rate into the model-rate ring store of the streaming analysis, with resample_chain.h's chain
struct ResampleStreamArgs {
    RingStore in_rings;
    const long long *desc;        // (n_rows, 6): in_slot, out_slot, first_out, n_out_new, n_total_in (< 0: still open), 0
    int n_rows, max_new_out;      // max_new_out sizes the grid only: a larger n_out_new is still produced whole
    int up, down;
    const float *taps;            // (n_taps), natural order, gain included
    int n_taps;
    RingStoreOut out_rings;
};
// nullptr when the arguments describe a valid launch, else what is wrong with them
const char *check_resample_stream(const ResampleStreamArgs &a);
void launch_resample_stream(const ResampleStreamArgs &a, hipStream_t stream);

// the same resampler on the way out (resample_stream.hip; include/mbexwn_live_out.h: mbxo_resample_emit): from a model-rate
// ring store into packed rows at the output rate
struct ResampleEmitArgs {
    RingStore in_rings;
    const long long *desc;        // (n_rows, 6): in_slot, first_out, n_out_new, n_total_in (< 0: still open), out_offset, 0
    int n_rows, max_new_out;      // max_new_out sizes the grid only: a larger n_out_new is still produced whole
    int up, down;
    const float *taps;            // (n_taps), natural order, gain included
    int n_taps;
    float *out;                   // output first_out + i of a row at out[out_offset + i]
    long long out_floats;         // a row that does not fit is skipped
};
const char *check_resample_emit(const ResampleEmitArgs &a);
void launch_resample_emit(const ResampleEmitArgs &a, hipStream_t stream);

// FLAC frames of 16-bit mono audio (flac_frames.hip): flac.py::encode's stream behind its 42-byte header
constexpr int FLAC_BLOCK = 4096;                // samples per frame (the last one may be shorter)
constexpr int FLAC_THREADS = 256;
constexpr int FLAC_ITEMS_PER_LAUNCH = 32;       // the items' lengths and offsets travel in the kernel arguments
constexpr int FLAC_CRC_SHIFTS = 16;             // operators M_{2^k}, k < 16, of the CRC-16 combine (frames are < 2^14 bytes)
constexpr long long FLAC_MAX_SAMPLES = 65536LL * FLAC_BLOCK;   // frame numbers of at most 3 bytes
struct FlacFramesArgs {
    const float *audio;          // item i of the launch at audio + i * stride
    long long stride;
    const uint16_t *crc_tables;  // CRC-16 byte table (256), then FLAC_CRC_SHIFTS x 16 operator columns
    uint8_t *out;                // item i's frames at out + offset[i]
    float *max_abs;              // (items) max |x| of every item, as the maximum of the bit patterns; zeroed before the launch
    int items, rate_code;
    long long n_samples[FLAC_ITEMS_PER_LAUNCH];
    long long offset[FLAC_ITEMS_PER_LAUNCH];
};
long long flac_frames_bytes(long long n);       // bytes of the frames of an n-sample item
// nullptr when the arguments describe a valid launch, else what is wrong with them
const char *check_flac_frames(const float *audio, long long stride, int batch, const int64_t *n_samples, int sample_rate,
                              const uint16_t *crc_tables, const uint8_t *out, long long out_bytes, const float *max_abs);
// items packed back to back in `out` (item b behind the frames of the items in front of it); max_abs must be zeroed
void launch_flac_frames(const float *audio, long long stride, int batch, const int64_t *n_samples, int sample_rate,
                        const uint16_t *crc_tables, uint8_t *out, float *max_abs, hipStream_t stream);

// compressed FLAC frames (flac_fixed.hip; include/mbexwn_flac.h: mbxf_encode_flac16_fixed): flac.py::encode(...,
// compression="fixed") behind its header -- fixed predictors of orders 0-4 and partitioned Rice codes
long long flac_fixed_frames(int batch, const int64_t *n_samples);      // frames of the batch
int flac_rate_code(int rate);                   // the frame header's 4-bit code of a sample rate (flac_frames.hip)
// nullptr when the arguments describe a valid launch, else what is wrong with them
const char *check_flac_fixed(const float *audio, long long stride, int batch, const int64_t *n_samples, int sample_rate,
                             const uint16_t *crc_tables, const uint8_t *out, long long out_bytes, const int32_t *frame_bytes,
                             const int64_t *workspace, const float *max_abs);
// plan, scan and encode passes; frames packed densely from out[0]; max_abs must be zeroed
void launch_flac_fixed(const float *audio, long long stride, int batch, const int64_t *n_samples, int sample_rate,
                       const uint16_t *crc_tables, uint8_t *out, int32_t *frame_bytes, int64_t *workspace, int16_t *pcm_out,
                       float *max_abs, hipStream_t stream);

// keyed N(0,1) noise (noise_keyed.hip; include/mbexwn_noise.h: mbxn_fill_normal): Philox4x32-10 quads keyed by (seed, item
// key), counted by the absolute step, Box-Muller in float32
constexpr int NOISE_TILE = 4096;                // values per block
struct NoiseArgs {
    float *out;                  // (batch, stride)
    long long stride;
    int batch;
    const uint64_t *keys;        // (batch, 2): seed, item key
    const int64_t *first_step;   // (batch) or null = 0
    const int32_t *counts;       // (batch)
    int max_count;
    int tiles;                   // set by the launcher
};
// nullptr when the arguments describe a valid launch, else what is wrong with them
const char *check_fill_normal(const NoiseArgs &a);
void launch_fill_normal(const NoiseArgs &a, hipStream_t stream);

// log-mel frames at arbitrary centre samples (mel_warp.hip; include/mbexwn_warp.h: mbxw_mel_frames_at): mel_analysis.hip's
// frame with its position read from a table; tables from the host module analysis.py
struct MelWarpArgs {
    const float *audio;          // (batch, stride)
    long long stride;
    int batch;
    const int32_t *n_samples;    // (batch), clamped in the kernel to [0, stride]
    const int64_t *centres;      // (batch, max_frames), clamped in the kernel to [0, n_samples[b]]
    const int32_t *n_frames;     // (batch): rows k >= n_frames[b] are not written
    int max_frames;
    int win, fft_size, n_mels;
    const float *window, *twiddle, *basis;
    const int *bin_lo, *bin_hi;
    float eps;
    float log_eps;               // float32 nearest to log(eps); launch_mel_warp fills it in
    float *out;                  // (batch, max_frames, n_mels)
};
// nullptr when the arguments describe a valid launch, else what is wrong with them
const char *check_mel_warp(const MelWarpArgs &a);
void launch_mel_warp(const MelWarpArgs &a, hipStream_t stream);

// formant shift: every mel row read at f / phi (mel_envelope.hip; include/mbexwn_envelope.h: mbxe_warp_envelope, and the
// forward with it, mbxe_forward); the centre table from the host module envelope.py
struct EnvelopeArgs {
    const float *mel;            // (batch, max_frames, n_mels), items bstride floats apart
    long long bstride;           // of mel and of out
    int batch;
    const int32_t *n_frames;     // (batch), clamped in the kernel to [0, max_frames]; rows behind are copied; null: max_frames
    int max_frames, n_mels;
    const float *centres;        // (n_mels) Hz, strictly increasing
    const float *factors;        // (batch, max_frames)
    float *out;                  // laid out like mel
    int frames_per_block;        // set by the launcher
};
// nullptr when the arguments describe a valid launch, else what is wrong with them
const char *check_envelope(const EnvelopeArgs &a);
void launch_envelope(const EnvelopeArgs &a, hipStream_t stream);

// F0 of every analysis frame from the audio itself (f0_track.hip; include/mbexwn_pitch.h: mbxp_track_f0): a YIN-type
// tracker on the frame grid of the mel analysis; the host definition is f0track.py::track_f0_host
struct PitchArgs {
    const float *audio;          // (batch, stride)
    long long stride;
    int batch;
    const int32_t *n_samples;    // (batch), clamped in the kernel to [0, stride]
    const int64_t *centres;      // (batch, max_frames), clamped in the kernel to [0, n_samples[b]]
    const int32_t *n_frames;     // (batch): rows k >= n_frames[b] are not written
    int max_frames;
    int sample_rate, window, tau_min, tau_max;
    float threshold, e_min;
    float *f0, *periodicity;     // (batch, max_frames) each
};
// nullptr when the arguments describe a valid launch, else what is wrong with them
const char *check_track_f0(const PitchArgs &a);
void launch_track_f0(const PitchArgs &a, hipStream_t stream);

// the same tracker for sounds that are still arriving (f0_stream.hip; include/mbexwn_live_pitch.h: mbxt_f0_frames): frames
// at t * hop from the ring store of the streaming mel analysis, on its descriptor table
struct PitchStreamArgs {
    RingStore rings;             // ring_samples at least window + tau_max
    const long long *desc;       // (n_streams, 4): slot, first_frame, n_frames, n_total (< 0: the stream is still open)
    int n_streams, max_new_frames;
    int hop, sample_rate, window, tau_min, tau_max;
    float threshold, e_min;
    float *f0, *periodicity;     // (n_streams, max_new_frames) each; rows at or behind a stream's n_frames are not written
};
// nullptr when the arguments describe a valid launch, else what is wrong with them
const char *check_f0_stream(const PitchStreamArgs &a);
void launch_f0_stream(const PitchStreamArgs &a, hipStream_t stream);

// A decoded contour (f0_decode.hip; include/mbexwn_contour.h: mbxc_f0_candidates, mbxc_decode_f0): per frame up to seven
// candidate lags and an "unvoiced" state from the tracker's d', then a Viterbi path per item; the host definition is
// f0decode.py (candidates_host, viterbi_host)
constexpr int F0_SLOTS = 8;
constexpr int F0_MAX_THRESHOLDS = 16;
constexpr int F0_DECODE_MAX_FRAMES = 16000;      // 4 bytes of back pointers per frame in 64 000 bytes of LDS
struct CandidateArgs {
    PitchArgs frame;             // audio .. e_min as for the tracker; threshold, f0 and periodicity are not used
    float thresholds[F0_MAX_THRESHOLDS];         // ascending; entries from n_thresholds on are not read
    float weights[F0_MAX_THRESHOLDS];
    int n_thresholds, n_cand;
    float *period, *cost, *dprime;               // (batch, max_frames, 8) each
};
// thresholds and weights are HOST pointers: checked and copied into the arguments here.  nullptr when valid.
const char *fill_f0_candidates(CandidateArgs &a, const float *thresholds, const float *weights);
void launch_f0_candidates(const CandidateArgs &a, hipStream_t stream);

struct DecodeArgs {
    const float *period, *cost, *dprime;         // (batch, max_frames, 8) each
    const int32_t *n_frames;     // (batch), clamped in the kernel to [0, max_frames]; rows behind are not written
    int max_frames, batch, sample_rate;
    float w_jump, w_switch;
    float *f0, *periodicity;     // (batch, max_frames) each
};
const char *check_decode_f0(const DecodeArgs &a);
void launch_decode_f0(const DecodeArgs &a, hipStream_t stream);

// The decoded contour of sounds that are still arriving (f0_lag.hip; include/mbexwn_live_contour.h: mbxv_f0_candidate_frames,
// mbxv_decode_f0_frames): the candidates of the new frames from the ring store, then the Viterbi
// recursion continued from a state row per stream, frame t decided once frame t + lag is there; the host definition is
// f0decode.py (viterbi_lag_host, LagDecoder)
// the rule part of fill_f0_candidates: checks n_thresholds, n_cand and the HOST arrays, and fills th and ww (16 each)
const char *fill_f0_rule(float *th, float *ww, int n_thresholds, int n_cand, const float *thresholds, const float *weights);
struct CandidateStreamArgs {
    PitchStreamArgs ring;        // rings .. e_min as for the streaming tracker; threshold, f0 and periodicity are not used
    float thresholds[F0_MAX_THRESHOLDS];
    float weights[F0_MAX_THRESHOLDS];
    int n_thresholds, n_cand;
    float *period, *cost, *dprime;               // (n_streams, max_new_frames, 8) each
};
const char *fill_f0_stream_candidates(CandidateStreamArgs &a, const float *thresholds, const float *weights);
void launch_f0_stream_candidates(const CandidateStreamArgs &a, hipStream_t stream);

constexpr int F0_MAX_LAG = 128;                  // f0decode.MAX_LAG
constexpr int F0_LAG_CHUNK = 64;                 // frames of a sub-chunk: forward steps, then one decided frame per lane
constexpr int F0_LAG_RING = 256;                 // frames of the ring, a power of two >= F0_MAX_LAG + 1 + F0_LAG_CHUNK
// one stream's state, in 32-bit words: [0] done, [1] decided, [2 .. 9] delta, [10 .. 17] and [18 .. 25] periods and costs of
// the last frame, [26 .. 31] zero; then per ring frame (index t & 255) the pointer word, 8 periods, 8 dprimes
constexpr int F0_LAG_HEAD = 32;
constexpr int F0_LAG_STATE_WORDS = F0_LAG_HEAD + F0_LAG_RING * (1 + 2 * F0_SLOTS);
struct LagDecodeArgs {
    const float *period, *cost, *dprime;         // (n_streams, max_new_frames, 8) each
    const long long *desc;       // (n_streams, 4): slot, first_frame, n_frames, n_total (< 0: the stream is still open)
    int n_streams, max_new_frames, hop;
    unsigned *state;             // (n_slots, F0_LAG_STATE_WORDS)
    int n_slots, lag, sample_rate;
    float w_jump, w_switch;
    float *f0, *periodicity;     // (n_streams, max_out) each; entries behind a stream's decided count are not written
    int max_out;
};
const char *check_lag_decode(const LagDecodeArgs &a);
void launch_lag_decode(const LagDecodeArgs &a, hipStream_t stream);

// Timing alignment (mel_align.hip; include/mbexwn_align.h: mbxg_local_cost, mbxg_align_path): the quantised band costs of a
// guide's and a source's log-mel, then a DTW path per item; the host definition is align.py (local_cost_host, path_host)
constexpr int ALIGN_MAX_FRAMES = 65535;          // nodes * 16384 < 2^31
constexpr int ALIGN_MAX_BAND = 511;              // one thread per band cell: 2 band + 1 <= 1024
constexpr int ALIGN_MAX_MELS = 240;              // 64 source rows of n_mels | 1 floats and the guide row in 64 KiB of LDS
struct AlignCostArgs {
    const float *mel_a, *mel_b;  // (batch, max_frames_a, n_mels), (batch, max_frames_b, n_mels)
    const int32_t *n_frames_a, *n_frames_b;      // (batch) each, clamped in the kernel to [0, max_frames_*]
    int batch, max_frames_a, max_frames_b, n_mels, band;
    uint16_t *cost;              // (batch, max_frames_a, 2 band + 1); rows behind n_frames_a[b] are not written
};
const char *check_align_cost(const AlignCostArgs &a);
void launch_align_cost(const AlignCostArgs &a, hipStream_t stream);

struct AlignPathArgs {
    const uint16_t *cost;        // (batch, max_frames_a, 2 band + 1)
    const int32_t *n_frames_a, *n_frames_b;      // (batch) each
    int batch, max_frames_a, band;
    uint8_t *workspace;          // align_workspace_bytes: back pointers, then the nodes in walking order
    size_t workspace_bytes;
    int32_t *nodes_i, *nodes_j;  // (batch, max_frames_a) each; entries behind count[b] are not written
    int32_t *count, *total;      // (batch) each
};
size_t align_workspace_bytes(long long batch, long long max_frames_a, long long band);
const char *check_align_path(const AlignPathArgs &a);
void launch_align_path(const AlignPathArgs &a, hipStream_t stream);

// ---------------------------------------------------------------------------------------------
// optional RMS normalisation of the mel input / de-normalisation of the audio (norm_mel.hip)
// ---------------------------------------------------------------------------------------------
struct NormMelConsts {
    int iters, mel_channels, hop, win, smooth_win, cut;    // cut = smooth_win/2 + 2 hop - win/2
    float rms_norm_fact, rms_floor, compressor_exp, lin_amp_scale, lin_amp_off, mel_amp_scale;
    int use_compressor, use_max_limit;
    const float *inv_enorm;          // (mel_channels)
    const float *pinv;               // normalize_use_pinv: (mel_channels, n_bins) pseudo inverse of the mel filters, else null
    int n_bins;                      // fft_size / 2 + 1
    float win_norm;                  // L2 norm of the analysis window
    const float *gwin;               // (win) unit-sum analysis window
    const float *smooth_win_table;   // (smooth_win)
};
// returns the (B, Tmax) buffer the output gain is built from (pass it to launch_norm_mel_gain)
const float *launch_norm_mel(const NormMelConsts &c, const float *mell, long long mel_bstride, const int *n_frames,
                             int max_frames, int batch, float *rms_a, float *rms_b, float *mell_out,
                             hipStream_t stream);
// audio *= gain (overwrite: audio = gain), gain = max(gain[win/2 + n], eps) of the last smoothing pass
void launch_norm_mel_gain(const NormMelConsts &c, const float *r_last, const int *n_frames, int max_frames, int batch,
                          float *audio, long long audio_bstride, bool overwrite, hipStream_t stream);

}  // namespace mbx
