// Which kernel runs every WaveNet layer of a forward pass, decided on the host in front of the first launch.
//
// Host arithmetic only -- no HIP type, no HIP call -- so a plain host compiler builds it (tests/test_wn_plan_host.py prints
// its decisions for a table of cases).  Three layers:
//   selectors   one per launcher (wn_*_select / wn_*_fits): does the layer's geometry fit the kernel, and which of its
//               instantiations runs.  They look at dimensions, strides and the policy; pointer alignment and non-null
//               pointers are guarantees of the caller that the launchers check themselves (wn_*.hip).
//   policies    gate_shape_policy, resskip_shape_policy: which of the kernels that fit a launch of this size prefers.
//   the plan    wn_plan_gate / wn_plan_resskip per layer, wn_plan for the single block: the order in which the kernels are
//               considered, the error of a layer that fits none, and whether the fp16 planes can be the hidden state.
// mbx_forward.hip fills a WnPlan in check_forward_args and launches by `switch` on its codes; mbx_plan reports it
// without launching; mbx_conv_form / mbx_kernel_report copy the plan of the most recent forward.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "../../include/mbexwn.h"
#include "mbx_args.h"

namespace mbx {

// ---- shape constants of the kernels that the selectors need (the kernels' own files hold the rest) ---------------------
constexpr int GH_ROWS = 256;                               // wn_gate_f16.hip
constexpr int GH_HALO = 16;
constexpr int GH_BK = 32;
constexpr int GH_COND_ROWS = 28;                           // conditioning rows of 64 floats (cond_up >= 10)
constexpr int WW_HALO = 16;                                // wn_winograd4w.hip
constexpr int WW_BK = 8;
constexpr int WQ_COND_ROWS = 28;                           // WqShape::COND_ROWS (blocks of two column tiles)
constexpr int W2_HALO = 16;                                // wn_winograd2w.hip: largest dilation
constexpr int W2_BK = 8;
constexpr int W2_TROWS = 32;                               // output rows of a wave tile
constexpr int W2_COND_ROWS = 8;                            // conditioning rows of a wave tile (64 floats each)
constexpr int G0_ROWS = 256;                               // wn_gate0.hip
constexpr int G0_MAX_DIL = 16;
constexpr int G0_COND_ROWS = 32;
constexpr int RW_BK = 8;                                   // wn_resskip_wide.hip
constexpr int RV_BK = 16;                                  // wn_resskip_wave.hip

// Kernels that need more dynamic LDS than a launch gets by default: mbx_create opts in once per handle, on the handle's
// device (wn_lds_opt_in, wn_gate_f16.hip / wn_winograd4w.hip), and keeps one bit per group that the device granted.
enum { WN_LDS_GATE_F16 = 1,     // wn_gate_f16_kernel<true | false>
       WN_LDS_GATE_F16W = 2,    // wn_gate_f16w_kernel
       WN_LDS_F43Q = 4 };       // wn_gate_winograd4q_kernel<0 | -1>

// What runs a gate layer.  shape: the F(4,3) block shape (0 256-row | 1 product-split | 2 product-split, half column tiles |
// 3 256-row, two column tiles), block_channels: gate channels per F(4,3) block (0: no F(4,3) kernel).
struct GateChoice {
    int kernel = MBX_GATE_K_NONE;   // MBX_GATE_K_*
    int shape = 0, block_channels = 0;
    int cr = 28;                    // F(4,3), 256-row blocks at d <= 16: conditioning rows of the instantiation (28 | 56)
    int vs_arg = 0;                 // F(4,3) at d > 16: 1, or 2 where a 256-row block takes two sub-sequences
};

inline int wn_log2_ceil(int d) {
    int log2d = 0;
    while ((1 << log2d) < d) ++log2d;
    return log2d;
}

// ---- selectors ------------------------------------------------------------------------------------------------------

// split half precision, direct form (wn_gate_f16.hip).  planes: the res/skip layer in front leaves the hidden state as fp16
// planes (a.h_split_ld, a.h_split_bstride describe them).  MBX_GATE_K_SPLIT_F16_WIDE: wn_gate_f16w_kernel,
// MBX_GATE_K_SPLIT_F16: wn_gate_f16_kernel<true>, MBX_GATE_K_SPLIT_F16_F32H: wn_gate_f16_kernel<false>, which reads the float32
// hidden state: it runs where the res/skip layer in front left no planes, which a legal tensor table reaches -- one without
// wn.res_skip_0.fold_start_f16 runs layer 0's res/skip in float32 and layer 1's gate here (tests/test_gpu_wavenet_stages.py:
// speech-split-f32h).
inline int wn_gate_f16_select(const ConvArgs &a, bool planes, unsigned lds_ok) {
    const int log2d = wn_log2_ceil(a.dil);
    const bool ok = a.ks == 3 && (1 << log2d) == a.dil && a.dil <= GH_HALO && a.pad_l == a.dil && a.pad_mode == 0 &&
                    a.cin % 4 == 0 && a.ldx % 4 == 0 && a.x_bstride % 4 == 0 && a.channels % 4 == 0 && a.cin == a.channels &&
                    a.cout == 2 * a.channels && a.cond_bstride % 4 == 0 && a.cond_up >= 1 && a.cond_up <= 64 &&
                    (GH_ROWS + a.cond_up - 2) / a.cond_up + 2 <= GH_COND_ROWS &&
                    a.cond_phase == 0 && a.out_rows == 0 && a.max_rows < (1 << 24) &&
                    (!planes || (a.h_split_ld % 8 == 0 && a.h_split_ld >= a.channels && a.h_split_bstride % 4 == 0));
    if (!ok || !(lds_ok & WN_LDS_GATE_F16)) return MBX_GATE_K_NONE;
    const int n_tiles = (a.channels + 31) / 32;
    const int m_tiles_total = (a.max_rows + GH_ROWS - 1) / GH_ROWS * a.batch;
    // 256 x 128 tiles (pairs of column tiles) for launches of several rounds of blocks: 0.83 against 0.93 ms at 16 x 10 s; one
    // utterance of 10 s is 315 such blocks on 256 CUs and keeps the 256 x 64 tiles (72.5 against 78.7 us).  Same bits.
    const long long blocks2 = 8LL * ((m_tiles_total + 7) / 8) * ((n_tiles + 1) / 2);
    if (planes && (lds_ok & WN_LDS_GATE_F16W) && (a.cin + GH_BK - 1) / GH_BK >= 2 && blocks2 >= 4 * 256) return MBX_GATE_K_SPLIT_F16_WIDE;
    return planes ? MBX_GATE_K_SPLIT_F16 : MBX_GATE_K_SPLIT_F16_F32H;
}

// Winograd F(4,3) in the block shape `shape` (wn_winograd4w.hip); kernel == MBX_GATE_K_NONE: the layer does not fit that shape.
// Shape 3 does not apply at d > 16, with cond_up < 10 (its CR = 28 geometry), to one column tile, or where the device
// refused its LDS size.
inline GateChoice wn_gate_winograd4w_select(const ConvArgs &a, int shape, unsigned lds_ok) {
    const bool split = shape == 1 || shape == 2;
    // dilations above the halo: d = 16 s runs as s interleaved virtual items per item at dilation 16 (kernels' VS variants)
    const int vs = a.dil > WW_HALO ? a.dil / WW_HALO : 1;
    const int dil_v = vs > 1 ? WW_HALO : a.dil;
    const int log2d = wn_log2_ceil(dil_v);
    const int rows_blk = split ? 128 : 256;
    const int nk8 = (a.cin + WW_BK - 1) / WW_BK;
    const int cond_rows = vs > 1 ? 1 : a.cond_up >= 1 ? (rows_blk + a.cond_up - 2) / a.cond_up + 2 : 1 << 30;   // conditioning rows a block's tile holds
    const bool ok = a.ks == 3 && (1 << log2d) == dil_v && dil_v * vs == a.dil && nk8 >= 4 && a.pad_mode == 0 &&
                    (a.pad_l == a.dil || (vs == 1 && a.pad_l == 2 * a.dil)) &&
                    a.cin % 4 == 0 && a.ldx % 4 == 0 && a.x_bstride % 4 == 0 && a.channels % 4 == 0 &&
                    a.cout == 2 * a.channels && a.cond_bstride % 4 == 0 && a.cond_up >= 1 &&
                    a.cond_up <= 64 && cond_rows <= (split ? 16 : 56) && a.max_rows < (1 << 24) &&
                    (vs == 1 || (shape != 2 && a.max_rows >= a.cond_up &&
                                 (long long)(rows_blk + 2 * WW_HALO) * vs * a.ldx * 4 < (1LL << 32)));
    GateChoice k;
    if (!ok) return k;
    // the CR = 28 geometry only (cond_up >= 10), here and in the one-tile blocks of an odd last tile
    if (shape == 3 && (vs > 1 || cond_rows > WQ_COND_ROWS || (a.channels + 31) / 32 < 2 || !(lds_ok & WN_LDS_F43Q))) return k;
    // (the blocks of two column tiles are a block shape of MBX_GATE_K_F43: the size rule of large launches picks either)
    k.kernel = a.dil > 16 ? (shape ? MBX_GATE_K_F43_STRIDED_PSPLIT : MBX_GATE_K_F43_STRIDED)
                          : (shape == 2 ? MBX_GATE_K_F43_HSPLIT : shape == 1 ? MBX_GATE_K_F43_PSPLIT : MBX_GATE_K_F43);
    k.shape = shape;
    k.block_channels = shape == 3 ? 64 : shape == 2 ? 16 : 32;
    k.cr = cond_rows <= 28 ? 28 : 56;
    const int vrows = (a.max_rows + vs - 1) / vs;         // rows of the longest virtual item
    // sub-sequences of at most 128 rows: a 256-row block takes two of them (VS == 2)
    const bool two = vs > 1 && !split && vrows <= 128 && vs % 2 == 0 && log2d == 4;
    k.vs_arg = vs > 1 ? (two ? 2 : 1) : 0;
    return k;
}

// Winograd F(2,3), wave-granular tiles (wn_winograd2w.hip).  a.out_row0 / a.out_rows: the rows of every item that are
// computed (out_rows == 0: all of them; out_row0 a multiple of 2 * dilation, so that the output pairs are those of a
// whole-item run).
inline bool wn_gate_winograd2w_fits(const ConvArgs &a) {
    const int log2d = wn_log2_ceil(a.dil);
    const int nk8 = (a.cin + W2_BK - 1) / W2_BK;
    return a.ks == 3 && (1 << log2d) == a.dil && a.dil <= W2_HALO && nk8 >= 3 && a.pad_mode == 0 &&
           (a.pad_l == a.dil || a.pad_l == 2 * a.dil) &&
           a.cin % 4 == 0 && a.ldx % 4 == 0 && a.x_bstride % 4 == 0 && a.channels % 4 == 0 &&
           a.cout == 2 * a.channels && a.cond_bstride % 4 == 0 && a.cond_up >= 1 &&
           (W2_TROWS + a.cond_up - 2) / a.cond_up + 2 <= W2_COND_ROWS &&
           a.max_rows < (1 << 24) && a.cond_phase >= 0 && a.cond_phase < a.cond_up && a.out_row0 >= 0 &&
           a.out_rows >= 0 && a.out_row0 % (2 * a.dil) == 0 && a.ldo % 2 == 0 && a.out_bstride % 2 == 0;
}

// geometry the folded first layer's kernel is built for (wn_gate0.hip; mbx_create keeps the un-folded first layer otherwise)
inline bool wn_gate0_fits(int channels, int pulse_channels, int dil, int cond_up) {
    return pulse_channels >= 1 && pulse_channels + 2 <= 8 && channels % 4 == 0 && cond_up >= 1 && dil >= 1 &&
           dil <= G0_MAX_DIL && (G0_ROWS + cond_up - 2) / cond_up + 2 <= G0_COND_ROWS;
}
// ... and the launch's strides
inline bool wn_gate0_select(const Gate0Args &a) {
    return wn_gate0_fits(a.channels, a.pulse_channels, a.dil, a.cond_up) && a.ldo % 4 == 0 && a.out_bstride % 4 == 0 &&
           a.cond_bstride % 4 == 0 && (!a.write_inputs || a.ldo >= a.channels + 16);
}

// What the three kernels of a folded res/skip layer (wide, wave-tiled, split half precision) ask of it alike
inline bool wn_resskip_folded_fits(const ConvArgs &a) {
    return a.ks == 1 && (a.h_init ? a.cin >= a.channels : a.cin == a.channels) && !a.last_layer && a.skip_ld > 0 &&
           a.cin % 4 == 0 && a.ldx % 4 == 0 && a.x_bstride % 4 == 0 &&
           a.channels % 2 == 0 && a.skip_ld % 2 == 0 && a.cout % 2 == 0 && a.cout <= a.channels + a.skip_ld &&
           a.hs_bstride % 2 == 0;
}

// large launches, one block owning all columns of its rows (wn_resskip_wide.hip): np = ceil(cout/32) in {11, 12}
inline int wn_resskip_wide_select(const ConvArgs &a) {
    const int np = (a.cout + 31) / 32;
    if (!(wn_resskip_folded_fits(a) && (np == 11 || np == 12) && a.cin >= 3 * RW_BK)) return MBX_RESSKIP_K_NONE;
    // 11 pairs (C = 320): one block owns all columns of its rows.  12 pairs (C = 340) would need 96 accumulator registers
    // per wave, which leaves one 8-wave block per CU (162 VGPRs; measured 0.53 of the peak): two blocks per row tile own
    // six pairs each instead and read the rows of `a` twice (the second read is an L2 hit)
    return np == 12 ? MBX_RESSKIP_K_WIDE6X2 : a.channels >= 320 ? MBX_RESSKIP_K_WIDE11_RES10 : MBX_RESSKIP_K_WIDE11;
}

// small launches, tiled at wave granularity (wn_resskip_wave.hip).  The cut (pairs per wave) follows the number of wave
// tiles: all columns per wave while the tiles alone give every SIMD about one wave, column splits below that.
// a.tune_split: 1..3 pins the cut (mbx_config.tune_resskip_split).
inline int wn_resskip_wave_select(const ConvArgs &a) {
    const int np = (a.cout + 31) / 32;
    const int nk = (a.cin + RV_BK - 1) / RV_BK;
    if (!(wn_resskip_folded_fits(a) && (np == 11 || np == 12) && nk >= 4)) return MBX_RESSKIP_K_NONE;
    const int m_tiles_total = (a.max_rows + 15) / 16 * a.batch;
    // waves per SIMD with s column splits = tiles * s / 1024: take the cut whose last round is fullest
    int split = a.tune_split;
    if (split != 1 && split != 2 && split != 3) {
        double best = -1.0;
        for (int s = 1; s <= 3; ++s) {
            const double per_simd = (double)m_tiles_total * s / 1024.0;
            const double fill = per_simd / std::ceil(per_simd);
            const double score = fill - 0.02 * (s - 1);            // prefer fewer splits (less re-reading of the rows)
            if (score > best) {
                best = score;
                split = s;
            }
        }
    }
    return split == 1 ? (np == 11 ? MBX_RESSKIP_K_WAVE11 : MBX_RESSKIP_K_WAVE12) : split == 2 ? MBX_RESSKIP_K_WAVE6X2 : MBX_RESSKIP_K_WAVE4X3;
}

// split half precision (wn_resskip_f16.hip).  planes: the kernel also writes the new hidden state as fp16 planes
// (a.h_split_ld, a.h_split_bstride); a.gate_act must be set
inline int wn_resskip_f16_select(const ConvArgs &a, bool planes) {
    const bool ok = wn_resskip_folded_fits(a) && a.cout <= 384 &&
                    (!planes || (a.h_split_ld % 8 == 0 && a.h_split_ld >= a.channels && a.h_split_ld <= a.cout + 32 && a.h_split_bstride % 4 == 0)) &&
                    a.gate_act != 3;            // glu: the layer's input is not bounded by 1
    return ok ? MBX_RESSKIP_K_SPLIT_F16 : MBX_RESSKIP_K_NONE;
}

// LDS-DMA kernel with host-packed weights (wn_resskip.hip), folded layers and layers with a skip tensor
inline int wn_resskip_select(const ConvArgs &a) {
    const bool ok = a.ks == 1 && (a.h_init ? a.cin >= a.channels && !a.last_layer : a.cin == a.channels) && a.cin % 4 == 0 && a.ldx % 4 == 0 && a.x_bstride % 4 == 0 &&
                    a.cout > 0 && (long long)a.max_rows * a.channels < (1LL << 31) &&
                    (a.skip_ld ? a.cout <= a.channels + a.skip_ld : a.cout == (a.last_layer ? a.channels : 2 * a.channels));
    if (!ok) return MBX_RESSKIP_K_NONE;
    // 64-row blocks while the 128-row grid is less than three rounds of the 768 resident blocks (3 per CU x 256 CUs)
    const long long big_blocks = (long long)((a.max_rows + 127) / 128) * a.batch * ((a.cout + 127) / 128);
    return big_blocks < 3 * 768 ? MBX_RESSKIP_K_PACKED64 : MBX_RESSKIP_K_PACKED128;
}

// end convolution + post-net in one pass over the skip tensor (wn_tail.hip); MBX_TAIL_K_NONE: the shapes do not fit
inline int wn_tail_select(int C, int n_out, int M, long long skip_bstride) {
    if (n_out > 32 || M > 16 || C % 4 != 0 || skip_bstride % 4 != 0) return MBX_TAIL_K_NONE;
    // rows owned by waves (wn_tail2_kernel): up to 352 channels (22 blocks of 16 in a lane's registers)
    const int nc8 = (C + 7) / 8, nj = (8 * nc8 + 15) / 16;
    // the smallest instantiation that holds the row: a lane issues NJ loads and keeps 4 NJ registers whatever C is
    // (same arithmetic in the same order for every NJ >= nj; ADVICE round 5: C = 64 used to issue 20 loads for 4)
    return !(nj <= 22 && C >= 16) ? MBX_TAIL_K_TAIL : nj <= 4 ? MBX_TAIL_K_TAIL2_NJ4 : nj <= 8 ? MBX_TAIL_K_TAIL2_NJ8 :
           nj <= 12 ? MBX_TAIL_K_TAIL2_NJ12 : nj <= 20 ? MBX_TAIL_K_TAIL2_NJ20 : MBX_TAIL_K_TAIL2_NJ22;
}

// ---- what selection depends on from the handle (mbx_handle::pol: filled at mbx_create; the form and the split precision
// change where a calibration decides them) --------------------------------------------------------------------------------

// weight images of a layer that the host supplied with the shape their kernel reads (mbx_create.hip: resolve_tensors)
enum { WN_IMG_WINO4W = 1, WN_IMG_WINO2W = 2, WN_IMG_FOLD = 4, WN_IMG_WIDE = 8, WN_IMG_WAVE = 16, WN_IMG_F16 = 32,   // (the fold set the layer runs with)
       WN_IMG_PACKED = 64 };

struct WnPolicy {
    int winograd = 0;                // gate layer form in effect: 0 direct, 2 Winograd F(2,3), 4 Winograd F(4,3) (needs the packed weights)
    bool winograd4_always = false;   // mbx_config.batch_invariant with F(4,3): the large-launch kernel shapes at every size
    int gate_small_shape = -1;       // mbx_config.tune_gate_shape: pins the F(4,3) block shape (0: 256-row and 3: 256-row blocks of two column tiles, at every launch size | 1: product-split | 2: product-split, half column tiles, small launches only; same bits)
    long long resskip_wave_tiles = 2048;   // default policy: res/skip launches of at most this many 16-row tiles run the wave-tiled kernel
    int resskip_split = 0;           // mbx_config.tune_resskip_split
    bool split_f16 = false;          // mbx_config.wn_precision == MBX_PRECISION_SPLIT_F16 and the images are there
    bool split_f16_gate = false;     // ... for the gate layers too (wn_gate_f16.hip)
    bool fold_skip = false;          // skip path folded into the end convolution (needs the *.fold tensors)
    bool fold_start = false;         // start convolution folded into layer 0 (needs fold_skip and the *.start_fold / *.fold_start tensors)
    unsigned lds_ok = 0;             // WN_LDS_*: the dynamic-LDS sizes the handle's device granted
    // the single block's shape (mbx_config)
    int C = 0, n_out = 0, M = 0, L = 0, cond_up = 1, ks = 3, causal = 0, gate_act = 0;
    int pulse_channels = 0;          // excitation floats per WaveNet row's fold: pulse_channels * (1 + wt_subharm_channels)
    int dil[MBX_MAX_WN_LAYERS] = {};
    unsigned char img[MBX_MAX_WN_LAYERS] = {};   // WN_IMG_* per layer of the single block
    bool end_packed = false;         // wn.end.packed is there (un-folded tail kernel)
};

// ---- launch-shape policy: pure functions of the policy fields and the launch's size ------------------------------------

struct GateShape {
    int shape;      // F(4,3) block shape: 0 256-row | 1 product-split | 2 product-split, half column tiles | 3 256-row, two column tiles
    bool f43;       // false: the direct form costs less than F(4,3) for this launch (dilations above 16 only)
};

// 256-row one-tile blocks from which a launch takes the blocks of two column tiles (gate_shape_policy).  Measured in one
// process, pins 1 and 4 alternating (scripts/experiments/gate_shapes.py --ab 1 4, profiles/r07_gate_shapes_ab.txt; C = 320,
// B x 800 frames, us per launch, one tile | two tiles): B = 1: 106.6 | 137.5, 2: 172.7 | 208.7, 4: 331.8 | 334.0 (no
// difference: its spread is larger), 8: 661.9 | 639.7 (-3.4 %), 16: 1 329.0 | 1 280.1 (-3.7 %).  8 x 800 frames = 5 040 blocks.
constexpr long long WIDE_FROM_BLOCKS = 5040;

inline GateShape gate_shape_policy(const WnPolicy &hd, int C, int B, long long nsteps, int span_rows, int d) {
    // F(4,3) block shape: what a launch of a few blocks per CU costs is the largest number of wave tiles a SIMD gets.
    // 256-row blocks put one whole tile (16 groups x 64 columns x 6 products) on every SIMD of their CU, the 128-row
    // product-split blocks half a tile: the finer shape runs when its worst SIMD gets clearly less work (a 10 s
    // utterance: 630 blocks = 2.46 per CU -> 3 tiles, against 1250 = 4.88 -> 5 halves).  Both give the same bits.
    // Streams run F(2,3): a window is bit-identical to an offline result only if both use one form with one group
    // alignment (streaming.py), and F(2,3) needs the shorter alignment; MBX_CONV_F23 makes offline runs use it too.
    const long long full_blocks = ((nsteps + 255) / 256) * B * ((C + 31) / 32);
    const long long half_blocks = ((nsteps + 127) / 128) * B * ((C + 31) / 32);
    const double load_full = (double)((full_blocks + 255) / 256), load_half = 0.5 * (double)((half_blocks + 255) / 256);
    // measured (scripts/experiments/gate_shapes.py, one item of 3 / 5 / 10 / 15 s: 51 / 65 / 102 / 155 us against 53 / 80 /
    // 110 / 167 us; two items of 10 s: 194 against 176 us): the finer shape wins up to about one resident round of
    // 256-row blocks and loses behind it, where both shapes divide evenly and the 128-row block's extra LDS-DMA traffic
    // per MFMA (the weight slice serves half the rows) and shorter slices tell
    bool split4 = !hd.winograd4_always && full_blocks <= 1024 && load_half <= load_full;
    // round 5: product-split blocks of HALF a column tile (one channel parity: twice the blocks of half the work; same bits
    // as the other shapes).  The idea: a 3 s utterance is 380 product-split blocks on 256 CUs, the worst CU works two
    // while the average is 1.5; 760 half blocks give every CU three.
    // Measured (scripts/experiments/gate_shapes.py, profiles/r05_gate_shapes.txt; one item of 1 / 2 / 3 / 4 / 5 / 10 s):
    // 32.4 / 43.8 / 54.0 / 65.9 / 70.4 / 131.8 us against 32.1 / 48.5 / 48.8 / 64.3 / 63.5 / 100.7 us for the product-split
    // blocks -- the estimate above was wrong: a block of half the matrix work lasts almost as long (40 barrier-separated
    // slices whose round trips, not whose MFMAs, set its time), so the finer shape only pays where the product-split
    // blocks leave CUs empty (<= 256 of them) and the half blocks do not (> 256): utterances around 2 s.
    int shape4 = split4 ? ((half_blocks <= 256 && 2 * half_blocks > 256) ? 2 : 1) : 0;
    // round 7: 256-row blocks of TWO column tiles (wn_gate_winograd4q_kernel; same bits, so batch_invariant handles follow
    // the same size rule): the input combinations and the activation staging are spent once per 96 MFMAs instead of once
    // per 48.  WIDE_FROM_BLOCKS: see the measurements at its definition.
    if (shape4 == 0 && full_blocks >= WIDE_FROM_BLOCKS) shape4 = 3;
    // mbx_config.tune_gate_shape: 1 and 4 pin the two shapes of large launches at every size, 2 and 3 the shape of small ones
    const int pin = hd.gate_small_shape;
    if (pin == 0 || pin == 3) shape4 = pin;
    else if (pin > 0 && !hd.winograd4_always && full_blocks < 4 * 768) shape4 = pin;
    split4 = shape4 == 1 || shape4 == 2;
    bool f43 = true;
    if (d > 16) {
        // Dilations above 16 (the reference's default depth reaches 2048, custom_AE_layers.py:229-233): F(4,3) over the
        // d / 16 interleaved sub-sequences of every item (wn_winograd4w.hip, VS kernels).  A block covers 256 (128) rows
        // of ONE sub-sequence, so short items pad: cost in 256-row block units, the product-split block 0.56 of one
        // (half the products, ~12 % slower per product), the direct form twice the multiplies of the unpadded rows.
        // Both block shapes give the same bits; whether F(4,3) or the direct form runs depends on the launch only
        // under the default policy (batch_invariant: always F(4,3)).
        const int vs = d / 16;
        const long long vrows = ((long long)span_rows + vs - 1) / vs, tiles = (C + 31) / 32;
        // (sub-sequences of at most 128 rows: a 256-row block takes two of them)
        const double cost_full = (vrows <= 128 ? 0.5 : (double)((vrows + 255) / 256)) * B * vs * tiles;
        const double cost_half = 0.56 * (double)((vrows + 127) / 128) * B * vs * tiles;
        const double cost_direct = 2.0 * ((double)span_rows / 256.0) * B * tiles;
        if (hd.gate_small_shape >= 0 && !hd.winograd4_always) {
            shape4 = hd.gate_small_shape == 3 ? 0 : hd.gate_small_shape;      // mbx_config.tune_gate_shape pins the shape (and F(4,3) itself); no two-tile blocks above d = 16
        } else {
            split4 = split4 || cost_half < 0.95 * cost_full;
            shape4 = split4 ? 1 : 0;
            if (!hd.winograd4_always && std::min(cost_full, cost_half) > 0.9 * cost_direct) f43 = false;
        }
    }
    return GateShape{shape4, f43};
}

struct ResSkipShape { bool wide, wave; };     // the folded res/skip kernels a launch may take, in the order they are considered

inline ResSkipShape resskip_shape_policy(const WnPolicy &hd, int B, long long nsteps, int span_rows, bool streamed) {
    // large launches (>= two rounds of the 512 resident 128-row blocks): one block owns all columns of its rows.
    // Like the gate kernels' block shape this follows the launch size only under the default policy: a pinned
    // form (MBX_CONV_DIRECT, MBX_CONV_F23, batch_invariant, streams) pins the kernel, so results do not depend on the batch they ran in.
    const long long wide_blocks = ((nsteps + 127) / 128) * B;
    const bool wide = hd.winograd4_always || (hd.winograd == 4 && !streamed && wide_blocks >= 2 * 512);
    // small launches: wave-granular tiles (wn_resskip_wave.hip).  The form pinned by the streams and by
    // MBX_CONV_F23 (F(2,3) gate) runs this kernel at every size: an output's arithmetic does not depend on
    // its cut, so windows, per-layer regions and whole utterances agree bit for bit.
    const long long wave_tiles = ((long long)span_rows + 15) / 16 * B;
    const bool pinned23 = hd.winograd == 2 || (hd.winograd != 0 && streamed);
    const bool wave = pinned23 || (hd.winograd == 4 && !hd.winograd4_always && wave_tiles <= hd.resskip_wave_tiles);
    return ResSkipShape{wide, wave};
}

// ---- geometry of the launches: the dimension and stride fields of the launchers' arguments that selection looks at (no
// pointers, no per-item row counts: mbx_forward.hip adds those) --------------------------------------------------------------

// the rows of the window one launch treats as the item (mbx_forward.hip: Span), as far as selection looks at them
struct WnSpan { int max_rows, cphase, out0, out_rows; };

inline int wn_gate_pad(int causal, int ks, int d) { return causal ? d * (ks - 1) : d * (ks - 1) / 2; }

// Gate layer of a block with C channels at dilation d: h, a are (B, rows, C) with the batch stride bstride, the
// conditioning rows (B, rows / cond_up, 2 C) with cond_bstride
inline ConvArgs wn_gate_dims(const WnPolicy &p, int C, int d, long long bstride, const WnSpan &sp, int B, long long cond_bstride) {
    ConvArgs g = ConvArgs();
    g.x_bstride = bstride;
    g.ldx = C;
    g.max_rows = sp.max_rows;
    g.batch = B;
    g.cin = C;
    g.cout = 2 * C;
    g.ks = p.ks;
    g.dil = d;
    g.pad_l = wn_gate_pad(p.causal, p.ks, d);
    g.pad_mode = MBX_PAD_ZERO;
    g.out_bstride = bstride;
    g.ldo = C;
    g.cond_bstride = cond_bstride;
    g.cond_up = p.cond_up;
    g.cond_phase = sp.cphase;
    g.out_row0 = sp.out0;
    g.out_rows = sp.out_rows;
    g.channels = C;
    g.gate_act = p.gate_act;
    return g;
}

// the hidden state as fp16 planes between a split res/skip layer and the split gate behind it
inline void wn_planes_dims(ConvArgs &a, int C, long long nsteps) {
    a.h_split_ld = (C + 7) / 8 * 8;
    a.h_split_bstride = nsteps * (long long)a.h_split_ld;
}

// res/skip layer with a skip tensor (un-folded single block, block runner): a, h, skip are (B, rows, C)
inline ConvArgs wn_resskip_dims(int C, bool first, bool last, long long bstride, int max_rows, int B) {
    ConvArgs r = ConvArgs();
    r.x_bstride = bstride;
    r.ldx = C;
    r.max_rows = max_rows;
    r.batch = B;
    r.cin = C;
    r.cout = last ? C : 2 * C;
    r.ks = 1;
    r.dil = 1;
    r.pad_mode = MBX_PAD_ZERO;
    r.channels = C;
    r.hs_bstride = bstride;
    r.skip_init = first;
    r.last_layer = last;
    return r;
}

// res/skip layer with the skip path folded into the end convolution: layers 0..L-2 update h and add a W_skip W_end to the
// n_out-wide output accumulator; the last layer's contribution is added by the tail kernel.
// ext: layer 0 with the start convolution folded in: rows [a0 | x'] (C + 16 channels) x [Wr ; Ws'], h starts from the bias
inline ConvArgs wn_resskip_fold_dims(const WnPolicy &p, bool first, bool ext, long long nsteps, int max_rows, int B) {
    const int cin_l = ext ? p.C + 16 : p.C;
    ConvArgs r = ConvArgs();
    r.x_bstride = nsteps * cin_l;
    r.ldx = cin_l;
    r.max_rows = max_rows;
    r.batch = B;
    r.cin = cin_l;
    r.cout = p.C + p.n_out;
    r.ks = 1;
    r.dil = 1;
    r.pad_mode = MBX_PAD_ZERO;
    r.h_init = ext;
    r.channels = p.C;
    r.skip_ld = p.n_out;
    r.skip_bstride = nsteps * p.n_out;
    r.hs_bstride = nsteps * p.C;
    r.skip_init = first;
    return r;
}

// Layer 0 with the start convolution folded in (wn_gate0.hip): rows of ldo floats out
inline Gate0Args wn_gate0_dims(const WnPolicy &p, const ConvArgs &g, long long nsteps) {
    Gate0Args g0 = Gate0Args();
    g0.pulse_channels = p.pulse_channels;
    g0.max_rows = g.max_rows;
    g0.batch = g.batch;
    g0.channels = g.channels;
    g0.gate_act = g.gate_act;
    g0.dil = g.dil;
    g0.causal = p.causal;
    g0.cond_bstride = g.cond_bstride;
    g0.cond_up = g.cond_up;
    g0.ldo = (p.fold_start && p.L > 1) ? p.C + 16 : p.C;      // row stride of layer 0's output
    g0.out_bstride = nsteps * g0.ldo;
    g0.write_inputs = p.L > 1;
    return g0;
}

// ---- the plan ---------------------------------------------------------------------------------------------------------

struct WnGeometry {
    int B = 0;
    long long nsteps = 0;            // sub-band rows of the window (batch strides)
    long long cond_bstride = 0;      // conditioning floats between batch items
    bool streamed = false;           // the call carries oscillator state (mbx_forward_stream)
    bool active = false;             // the call names an active region (mbx_forward_options.active_frames)
    bool layer_state = false;        // ... or carries per-layer state (layer_store)
    WnSpan gate[MBX_MAX_WN_LAYERS] = {};
    int res_rows[MBX_MAX_WN_LAYERS] = {};
};

struct WnPlan {
    int n_layers = 0;                                    // entries in use (several blocks: block-major, capped at MBX_MAX_WN_LAYERS)
    GateChoice gate[MBX_MAX_WN_LAYERS];
    int gate_f32[MBX_MAX_WN_LAYERS] = {};                // MBX_GATE_K_* of the float32 kernel the layer takes with the split precision off
    int resskip[MBX_MAX_WN_LAYERS] = {};                 // MBX_RESSKIP_K_*; MBX_RESSKIP_K_NONE: no launch of its own (the folded tail's share)
    bool planes_out[MBX_MAX_WN_LAYERS] = {};             // the res/skip layer also writes the hidden state as fp16 planes
    int tail = MBX_TAIL_K_NONE, tail_folded = 0;
    bool planes_only = false;                            // the fp16 planes ARE the hidden state: the float32 h is not written
    mbx_status status = MBX_OK;                          // != MBX_OK: a layer fits no kernel; nothing may be launched
    const char *error = nullptr;
};

// Gate of one layer (dilated convolution + conditioning + gate): split half precision, then F(4,3) in the shape the policy
// prefers, then its 256-row shape, then F(2,3), then the direct form.  generic: the block runner -- F(4,3) in the 256-row
// shape at every size, or the direct form.  planes: the res/skip layer in front leaves the hidden state as fp16 planes.
// f32: where the float32 choice is reported (null: not).  kernel == MBX_GATE_K_NONE: nothing fits (per-layer regions need F(2,3)).
inline GateChoice wn_plan_gate(const WnPolicy &p, unsigned img, const ConvArgs &g, long long nsteps, bool streamed, bool generic,
                               bool planes, int *f32) {
    const int d = g.dil, C = g.channels;
    const bool whole = g.cond_phase == 0 && g.out_rows == 0;
    GateChoice k;
    const GateShape pol = generic ? GateShape{0, true} : gate_shape_policy(p, C, g.batch, nsteps, g.max_rows, d);
    if (p.winograd == 4 && !streamed && pol.f43 && (img & WN_IMG_WINO4W) && g.cond_phase == 0) {
        // (the product-split shape holds 16 conditioning rows: cond_up >= 10; the 256-row shape takes cond_up >= 5)
        k = wn_gate_winograd4w_select(g, pol.shape, p.lds_ok);
        if (!k.kernel && pol.shape != 0) k = wn_gate_winograd4w_select(g, 0, p.lds_ok);
    }
    // F(2,3): wave-tiled kernel on v_mfma_f32_16x16x4_f32 (wn_winograd2w.hip): streams, per-layer regions, MBX_CONV_F23
    if (!k.kernel && !generic && p.winograd && (img & WN_IMG_WINO2W) && wn_gate_winograd2w_fits(g)) k.kernel = MBX_GATE_K_F23;
    if (!k.kernel && whole) k.kernel = MBX_GATE_K_DIRECT;
    if (f32) *f32 = k.kernel;
    // opt-in split half precision: whole-item forwards of the layers behind the folded first one
    if (p.split_f16_gate && !streamed && whole) {
        ConvArgs gh = g;
        if (planes) wn_planes_dims(gh, C, nsteps);
        const int kh = wn_gate_f16_select(gh, planes, p.lds_ok);
        if (kh) {
            k = GateChoice();
            k.kernel = kh;
        }
    }
    return k;
}

// res/skip of one layer: split half precision, then the wide, then the wave-tiled kernel (folded layers: img holds the
// layer's image set), then the packed LDS-DMA kernel, then the generic one (layers with a skip tensor only).
// want_planes: a split launch also writes the planes.  MBX_RESSKIP_K_NONE: a folded layer that fits no kernel.
inline int wn_plan_resskip(const WnPolicy &p, unsigned img, const ConvArgs &r, long long nsteps, bool streamed, bool folded,
                           bool want_planes, bool *planes_out) {
    int k = MBX_RESSKIP_K_NONE;
    *planes_out = false;
    if (folded) {
        // opt-in split half precision (mbx_config.wn_precision): every launch size, every layer whose split image the
        // host supplied (layer 0 with the folded start convolution too: its rows [a0 | x'] have the image *.fold_start_f16)
        if (p.split_f16 && (img & WN_IMG_F16)) {
            ConvArgs rh = r;
            rh.gate_act = p.gate_act;
            if (want_planes) wn_planes_dims(rh, r.channels, nsteps);
            k = wn_resskip_f16_select(rh, want_planes);
            *planes_out = k && want_planes;
        }
        const ResSkipShape pol = resskip_shape_policy(p, r.batch, nsteps, r.max_rows, streamed);
        if (!k && (img & WN_IMG_WIDE) && pol.wide) k = wn_resskip_wide_select(r);
        if (!k && (img & WN_IMG_WAVE) && pol.wave) {
            ConvArgs rw = r;
            rw.tune_split = p.resskip_split;
            k = wn_resskip_wave_select(rw);
        }
    }
    // LDS-DMA kernel with host-packed weights (folded layers: the image the layer was built with)
    if (!k && (img & (folded ? WN_IMG_FOLD : WN_IMG_PACKED))) k = wn_resskip_select(r);
    if (!k && !folded) k = MBX_RESSKIP_K_CONV1D;
    return k;
}

inline WnPlan wn_plan_fail(WnPlan plan, mbx_status st, const char *msg) {
    plan.status = st;
    plan.error = msg;
    return plan;
}

// The single block (the measured path): every layer's kernels, the tail, and whether the planes are the hidden state.
inline WnPlan wn_plan(const WnPolicy &p, const WnGeometry &geo) {
    WnPlan plan;
    const int L = p.L, C = p.C;
    plan.n_layers = L;
    // the res/skip layers write the planes for the gates behind them on whole-item calls of a handle whose gates take them
    const bool want_planes = p.split_f16_gate && !geo.active;
    bool planes = false;            // the hidden state in front of the layer is there as planes
    for (int l = 0; l < L; ++l) {
        const ConvArgs g = wn_gate_dims(p, C, p.dil[l], geo.nsteps * C, geo.gate[l], geo.B, geo.cond_bstride);
        if (l == 0 && p.fold_start) {
            // start convolution folded into the layer: a K = 24 contraction of the excitation (wn_gate0.hip)
            if (geo.gate[0].cphase != 0 || !wn_gate0_select(wn_gate0_dims(p, g, geo.nsteps)))
                return wn_plan_fail(plan, MBX_ERR_INVALID_ARGUMENT, "folded first layer does not fit its kernel");
            plan.gate[l].kernel = plan.gate_f32[l] = MBX_GATE_K_FOLDED_START;
        } else {
            plan.gate[l] = wn_plan_gate(p, p.img[l], g, geo.nsteps, geo.streamed, false, planes, &plan.gate_f32[l]);
            if (!plan.gate[l].kernel) return wn_plan_fail(plan, MBX_ERR_UNSUPPORTED, "per-layer regions need the Winograd F(2,3) gate kernel");
        }
        if (!p.fold_skip) {
            const ConvArgs r = wn_resskip_dims(C, l == 0, l == L - 1, geo.nsteps * C, geo.res_rows[l], geo.B);
            plan.resskip[l] = wn_plan_resskip(p, p.img[l], r, geo.nsteps, geo.streamed, false, false, &plan.planes_out[l]);
        } else if (l < L - 1) {
            const ConvArgs r = wn_resskip_fold_dims(p, l == 0, l == 0 && p.fold_start, geo.nsteps, geo.res_rows[l], geo.B);
            plan.resskip[l] = wn_plan_resskip(p, p.img[l], r, geo.nsteps, geo.streamed, true, want_planes, &plan.planes_out[l]);
            if (!plan.resskip[l]) return wn_plan_fail(plan, MBX_ERR_INVALID_ARGUMENT, "folded res/skip layer does not fit its kernel");
        }                           // (else: the tail kernel adds the last layer's share)
        planes = plan.planes_out[l];
    }
    // end of the block: the last layer's share of the folded skip path, or the end convolution on the skip tensor; then
    // the post-net 1x1 into the sub-band rows (one kernel where the images are there)
    plan.tail_folded = p.fold_skip ? 1 : 0;
    plan.tail = (p.fold_skip || p.end_packed) ? wn_tail_select(C, p.n_out, p.M, geo.nsteps * C) : MBX_TAIL_K_NONE;
    if (p.fold_skip && !plan.tail) return wn_plan_fail(plan, MBX_ERR_INVALID_ARGUMENT, "folded WaveNet tail does not fit its kernel");
    if (!plan.tail) plan.tail = MBX_TAIL_K_UNFUSED;
    // split half precision, round 6: where every consumer of the hidden state takes the planes -- the split gate of every layer
    // behind the first one (dilation <= 16: wn_gate_f16.hip) and the split res/skip layer of every layer in front of the last
    // one, layer 0's with the folded start convolution included -- the planes ARE the hidden state: hi + 2^-11 lo' keeps 22-23 of
    // float32's 24 bits, and the float32 tensor h (328 MB written and read again per layer at 16 x 10 s) is not touched.
    // Read off the plan itself: a layer that took a float32 kernel keeps the float32 h for everyone.
    bool planes_only = p.split_f16 && p.split_f16_gate && p.fold_skip && p.fold_start && !geo.streamed && !geo.active && !geo.layer_state && L >= 2;
    for (int l = 1; l < L && planes_only; ++l)
        planes_only = plan.gate[l].kernel == MBX_GATE_K_SPLIT_F16 || plan.gate[l].kernel == MBX_GATE_K_SPLIT_F16_WIDE;
    for (int l = 0; l + 1 < L && planes_only; ++l) planes_only = plan.resskip[l] == MBX_RESSKIP_K_SPLIT_F16 && plan.planes_out[l];
    plan.planes_only = planes_only;
    return plan;
}

}  // namespace mbx
