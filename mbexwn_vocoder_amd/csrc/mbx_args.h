// Argument records of the convolution and WaveNet launchers: plain data, no HIP types, so that the host-only kernel
// selection (wn_plan.h) can be compiled without the HIP headers.
#pragma once

namespace mbx {

enum ConvEpilogue {
    EPI_LINEAR = 0,   // y = acc + bias, optional PReLU / leaky slope
    EPI_GATE = 1,     // a = tanh(acc_t + bias_t + cond_t) * sigmoid(acc_s + bias_s + cond_s)
    EPI_RESSKIP = 2   // h += r[:, :C] ; skip (+)= r[:, C:]   (last layer: skip += r)
};

struct ConvArgs {
    // input (batch, rows, cin) channels-last
    const float *x;
    long long x_bstride;      // floats between batch items
    int ldx;                  // floats between rows
    // rows per item: n_frames ? n_frames[b] * rows_per_frame : max_rows
    const int *n_frames;
    int rows_per_frame;
    int max_rows;
    int batch;
    // weights (ks*cin, cout) row-major, bias (cout) or null
    const float *w;
    const float *bias;
    int cin, cout, ks, dil, pad_l, pad_mode;
    // output
    float *out;
    long long out_bstride;
    int ldo;
    // EPI_LINEAR extras
    const float *alpha;       // PReLU slopes (cout) or null
    float leaky;              // slope when use_leaky
    int use_leaky;
    // EPI_GATE extras: conditioning (batch, rows/cond_up, 2*C), interpolated on the fly
    const float *cond;
    long long cond_bstride;
    int cond_up;
    int cond_phase;           // item row r sits at conditioning-rate position r + cond_phase (0 <= cond_phase < cond_up; F(2,3) gate kernel only)
    const float *lerp_w0, *lerp_w1;   // (cond_up) float32 interpolation weights
    int channels;             // C (gate: cout == 2C, out has C columns; res/skip: split point)
    int gate_act;             // EPI_GATE and the gate kernels: 0 gtu, 1 gfu, 2 gsu, 3 glu (wn_gate_act)
    // EPI_RESSKIP extras
    float *h;                 // (batch, rows, C) updated in place
    float *skip;              // (batch, rows, skip_ld)
    int skip_ld;              // floats between rows of skip (0: C)
    long long skip_bstride;   // floats between batch items of skip (0: max_rows * skip_ld, or hs_bstride when skip_ld == 0)
    long long hs_bstride;
    int skip_init;            // 1: skip = s (first layer)  0: skip += s
    int h_init;               // 1: h = r (first layer with the start convolution folded in: x carries [a | x'], cin > C)
    int last_layer;           // 1: cout == C, everything goes to skip
    int acc_preloaded;        // set by the launcher: accumulators start from bias + old value, epilogue only stores
    int remap, n_tiles, m_tiles_per_item, m_tiles_total;   // XCD-aware 1-D grid (set by the launcher)
    int out_row0, out_rows;   // wave-tiled F(2,3) gate kernel: only the rows [out_row0, out_row0 + out_rows) of every item are
                              // computed (out_rows == 0: all rows; out_row0 a multiple of 2 * dil)
    const float *zeros;       // >= 16 bytes of zeros in global memory (LDS-DMA source of padding lanes)
    int fast_dma;             // set by the launcher: 32-bit source offsets are safe (LDS-DMA with a uniform base)
    int tile0;                // set by launch_wn_gate_winograd4w: first column tile of the launch (the 256-row blocks that finish an odd
                              // tile count behind the blocks of two column tiles), 0 otherwise
    int vstride;              // set by launch_wn_gate_winograd4w for dilations above 16: every item is treated as vstride interleaved
                              // virtual items (rows s, s + vstride, s + 2 vstride ...) convolved with dilation dil / vstride
    // split half precision (mbx_config.wn_precision): the hidden state as fp16 planes, written by wn_resskip_f16_kernel and read
    // by wn_gate_f16_kernel -- row r: [hi: h_split_ld halves][lo': h_split_ld halves] (h_split_ld = channels rounded up to 8,
    // the padding zero), i.e. h_split_ld float32 words per row
    float *h_split;
    long long h_split_bstride;   // float32 words between batch items
    int h_split_ld;
    int h_planes_only;        // wn_resskip_f16_kernel: the planes ARE the hidden state -- old values are read from them (hi + 2^-11 lo'),
                              // the float32 tensor h is neither read nor written (every consumer of h takes the planes)
    int tune_split;           // wave-tiled res/skip kernel: 1..3 pins its column split (mbx_config.tune_resskip_split; same bits), 0: by launch size
    // EPI_LINEAR, the F0-net (conv_mel.hip: conv1d_f64_tile / conv1d_f64_tile32): contraction on v_mfma_f64_16x16x4_f64
    int precise;              // 1: float64 accumulation; with only this set x, w and out are the float32 ones above (one rounding per output)
    const double *x64;        // input as float64 (same strides, counted in elements) instead of x; needs w64
    const double *w64;        // weights (ks*cin, cout) as float64 instead of w
    double *out64;            // output as float64 (same strides) instead of out
};

// First WaveNet layer with the start convolution folded into it (wn_gate0.hip)
struct Gate0Args {
    const float *pulse;       // (batch, rows * pulse_channels): the excitation, folded to pulse_channels per row
    long long pulse_bstride;
    const float *noise;       // (batch, rows) or null
    long long noise_bstride;
    float sigma;
    int pulse_channels;
    const int *n_frames;
    int rows_per_frame, max_rows, batch;
    const float *w;           // image of packing.fold_start_weights (ceil(C/32), 3, 2, 64, 4)
    const float *bias;        // (2C) gate bias or null
    int channels, dil;
    int causal;               // 0: SAME (taps t - d, t, t + d), 1: CAUSAL (taps t - 2d, t - d, t)
    const float *cond;        // (batch, rows/cond_up, 2C)
    long long cond_bstride;
    int cond_up;
    const float *lerp_w0, *lerp_w1;
    int gate_act;             // 0 gtu, 1 gfu, 2 gsu, 3 glu (wn_gate_act)
    float *out;               // (batch, rows, ldo): C gate channels, then x' padded to 16 channels if write_inputs
    long long out_bstride;
    int ldo, write_inputs;
    int n_tiles, m_tiles_per_item;   // set by the launcher
};

}  // namespace mbx
