// The mel-rate sub-net convolutions: F0-net, VTF-net and the conditioning convolutions (EPI_LINEAR: bias, optional PReLU /
// leaky slope; same formula and padding rules as conv_mfma.hip, which keeps the shapes this family does not take).
//
// Contract: a row's bits do not depend on the launch it ran in.  Whatever the tile, the launch size or the neighbours in a
// shared launch, every output element is summed in ONE order:
//   - K = ks * cin is cut into groups of 8 input channels of a tap (float64 tiles: 16; the last group of a tap may be short),
//     the groups into four quarters: quarter w holds the groups [n_groups * w / 4, n_groups * (w + 1) / 4);
//   - a quarter is one sequential MFMA chain that starts from +0: v_mfma_f32_32x32x2_f32 steps in channel order (lane half h
//     of a step holds channel 8 g + 4 h + s, s = 0..3), v_mfma_f64_16x16x4_f64 steps for the float64 tiles;
//   - the quarters are folded from the left and the bias comes last:  ((q0 + q1) + q2) + q3 + bias,  then the activation.
// Rows outside the item are formed by the padding rule from the item's own length (map_row), so a padded batch stays
// bit-identical to one-at-a-time runs, and a large launch to the same rows in small launches (tests/test_gpu_parity.py).  The
// reason is the F0 contour: it feeds the phase accumulator, and rounding there is audible in the last bits everywhere
// downstream.
//
// Three tile sizes (launch_conv1d_group / launch_conv1d_mel_single choose; all are blocks of 4 waves):
//   32 x 32, split K     conv1d_small_tile32   small launches (below 12 288 rows in all) and every single float32 launch: wave w
//                                              runs quarter w, operands straight from L2, the quarters meet through LDS
//   64 x 128, LDS-DMA    conv1d_mel_tile_dma   large shared launches: wave w owns 32 columns of both 32-row tiles and runs the
//                                              four quarters one after the other, folding as it goes
//   float64              conv1d_f64_tile       16 x 16, split K like the 32 x 32 tile: small launches and every single launch
//                        conv1d_f64_tile32     32 x 32 = four 16 x 16 sub-tiles, wave w contracts quarter w of all four: large launches
//
// Float64 members (ConvArgs::precise; the F0-net under mbx_config.f0_accumulate, the default) have three operand modes:
//   x float32, W float32           float64 accumulation only (sub-net shapes outside the full-float64 pattern, handles
//                                  without the *.w64 tensors): one rounding to float32 per output
//   x float32, W float64 (w64)     first layer of the full-float64 chain: reads the mel input, writes float64 (out64)
//   x float64 (x64), W float64     hidden layers of the chain
// The float64 weights are the exact weight-norm fold g v / |v| (host, packing.tensor_table "<layer>.w64").
#include <type_traits>

#include "conv_tile.h"
#include "mbx_kernels.h"

namespace mbx {

// scalar 0 / 1 flags and selects that stay on the scalar unit
__device__ __forceinline__ int s_flag_ge(int a, int b) {
    int r;
    asm("s_cmp_ge_i32 %1, %2\n\ts_cselect_b32 %0, 1, 0" : "=s"(r) : "s"(a), "s"(b) : "scc");
    return r;
}
__device__ __forceinline__ int s_select(int flag, int a, int b) {          // flag ? a : b
    int r;
    asm("s_cmp_lg_u32 %1, 0\n\ts_cselect_b32 %0, %2, %3" : "=s"(r) : "s"(flag), "s"(a), "s"(b) : "scc");
    return r;
}
__device__ __forceinline__ const float *s_ptr_add(const float *base, int byte_off) {
    const unsigned long long u = (unsigned long long)(uintptr_t)base;
    unsigned lo, hi;
    asm("s_add_u32 %0, %2, %4\n\ts_addc_u32 %1, %3, 0" : "=&s"(lo), "=&s"(hi) : "s"((unsigned)u), "s"((unsigned)(u >> 32)), "s"(byte_off) : "scc");
    return reinterpret_cast<const float *>((uintptr_t)(((unsigned long long)hi << 32) | lo));
}

// a load from global memory at (wave-uniform base + per-lane byte offset): said with a global address-space pointer, so that the
// compiler emits global_load (scalar base + vector offset) and counts it with vmcnt only -- a pointer rebuilt from integers is
// a generic one: flat_load, 64-bit vector address arithmetic per load and waits on lgkmcnt as well
typedef float g_f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float g_load_f32(const float *sbase, unsigned voff_bytes) {
    typedef __attribute__((address_space(1))) const char g_char;
    typedef __attribute__((address_space(1))) const float g_float;
    return *reinterpret_cast<g_float *>((g_char *)sbase + voff_bytes);
}
__device__ __forceinline__ float4 g_load_f32x4(const float *sbase, unsigned voff_bytes) {
    typedef __attribute__((address_space(1))) const char g_char;
    typedef __attribute__((address_space(1))) const g_f32x4 g_quad;
    const g_f32x4 v = *reinterpret_cast<g_quad *>((g_char *)sbase + voff_bytes);
    return make_float4(v.x, v.y, v.z, v.w);
}

// rows outside the item / channels behind cin: the lane's four operand values become zeros
template <typename Q>
__device__ __forceinline__ void mask_quad(Q &v, bool ok) {
    typedef decltype(v.x) T;
    v.x = ok ? v.x : (T)0;
    v.y = ok ? v.y : (T)0;
    v.z = ok ? v.z : (T)0;
    v.w = ok ? v.w : (T)0;
}

// The 32 x 32 split-K tile (needs cin % 8 == 0 and 16-byte aligned rows: small_conv_eligible).  A 32 x 32 output tile per block
// keeps >= 200 blocks in flight for 800 rows; what then bounds a block is the serial chain of K/2 dependent-rate MFMAs, so wave
// w runs quarter w of it.  Operands go straight from global memory (L2) to the MFMA registers: the tile is too small to amortise
// an LDS stage.  Lane (row r, half h) loads A[r][8g+4h..+3] as one float4 and feeds it to four MFMA steps; the B lane (col c,
// half h) loads W[8g+4h+s][c] for the same steps.  (Larger register tiles per block were measured slower than the LDS-staged
// conv1d_mel_tile_dma below, which takes the large launches.)
// Round 5: the loop rewritten for its issue budget (the sums and their order are those of the head comment, hence the same bits).
// A streaming tick is 64 items of a dozen rows, a 3 s utterance 240 rows: the launch is a few thousand short blocks, eight of
// them resident per CU, and what a wave does between its MFMAs competes with the other waves' MFMAs for the SIMD (DESIGN.md
// section 4).  The round-4 loop spent ~45 vector instructions per group of 4 MFMAs: the tap by division and map_row per
// group, 64-bit address arithmetic for five loads, the row masks, and the copy of the prefetched batch into the current one.
// Now: tap / channel group advance in scalar registers, a load is a scalar base + a per-lane 32-bit offset computed once (per
// tap at the item's edges), the two operand sets ping-pong, the row mask is formed once per tap and skipped in the interior.
template <bool INTERIOR>
__device__ __forceinline__ void conv1d_small_tile32_body(const ConvArgs &p, int bx, int by, int b, float *red, int rows) {
    const int m0 = bx * 32, n0 = by * 32;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lrow = lane & 31, lk = lane >> 5;
    const float *xb = p.x + (long long)b * p.x_bstride;
    const int cin = p.cin, cout = p.cout, ldx = p.ldx, dil = p.dil, pad_l = p.pad_l;
    const int gpt = cin >> 3;                               // groups of 8 input channels per tap
    const int n_groups = p.ks * gpt;
    const int g_begin = (n_groups * wave) / 4, g_end = (n_groups * (wave + 1)) / 4;
    const int col = n0 + lrow;
    const bool col_ok = col < cout;
    // weights: W[8 g + 4 lk + st][col] = scalar base of the group + the lane's offset of step st
    unsigned w_voff[4];
#pragma unroll
    for (int st = 0; st < 4; ++st) w_voff[st] = (unsigned)((4 * lk + st) * cout + min(col, cout - 1)) * 4u;
    // activations: x[source row of the lane at the tap][8 cg + 4 lk ..] = scalar base (item + channel group; in the interior +
    // tap) + the lane's offset; at the item's edges the offset holds the mapped row of the tap and `a_ok` says whether it exists
    unsigned a_voff = (unsigned)((m0 + lrow - pad_l) * ldx + 4 * lk) * 4u;       // interior: relative to tap 0 (never negative there)
    bool a_ok = true;
    int c_tap = __builtin_amdgcn_readfirstlane(g_begin / gpt);
    int c_cg = __builtin_amdgcn_readfirstlane(g_begin - (g_begin / gpt) * gpt);
    auto edge_tap = [&]() {                                  // (!INTERIOR) the lane's source row at tap c_tap
        const int src = map_row(m0 + lrow - pad_l + c_tap * dil, rows, p.pad_mode);
        a_ok = src >= 0;
        a_voff = (unsigned)(max(src, 0) * ldx + 4 * lk) * 4u;
    };
    if (!INTERIOR) edge_tap();
    constexpr int DEPTH = 4;                                 // groups in flight beside the batch being multiplied (round 4, with the loads really batched: 2: 47.8, 3: 45.9, 4: 45.7, 6: 47.1, 9: 48.8, 12: 54 us front end of 3 s)
    struct Set {
        float4 a[DEPTH];
        float b[DEPTH][4];
        bool ok[DEPTH];
    };
    auto request = [&](Set &s, int g0) {                     // groups g0 .. g0 + DEPTH - 1 (those below g_end) at the cursor
#pragma unroll
        for (int d = 0; d < DEPTH; ++d) {
            if (g0 + d < g_end) {
                const float *xs = s_ptr_add(xb, ((INTERIOR ? c_tap * dil * ldx : 0) + c_cg * 8) * 4);
                s.a[d] = g_load_f32x4(xs, a_voff);
                s.ok[d] = a_ok;
                const float *ws = s_ptr_add(p.w, (c_tap * cin + c_cg * 8) * cout * 4);
#pragma unroll
                for (int st = 0; st < 4; ++st) s.b[d][st] = g_load_f32(ws, w_voff[st]);
                const int wrap = s_flag_ge(c_cg + 1, gpt);
                c_cg = s_select(wrap, 0, c_cg + 1);
                c_tap += wrap;
                if (!INTERIOR && wrap) edge_tap();
            }
        }
    };
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    auto consume = [&](Set &s, int g0) {
#pragma unroll
        for (int d = 0; d < DEPTH; ++d) {
            if (g0 + d < g_end) {
                float4 av = s.a[d];
                if (!INTERIOR) mask_quad(av, s.ok[d]);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, s.b[d][0], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, s.b[d][1], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, s.b[d][2], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, s.b[d][3], acc, 0, 0, 0);
            }
        }
    };
    Set s0, s1;
    request(s0, g_begin);
    for (int g = g_begin; g < g_end; g += 2 * DEPTH) {
        request(s1, g + DEPTH);
        consume(s0, g);
        if (g + DEPTH >= g_end) break;
        request(s0, g + 2 * DEPTH);
        consume(s1, g + DEPTH);
    }
    // reduce the four K quarters: the waves 1..3 park their partial tile in LDS, wave 0 adds the quarters in wave order.
    // (This fold is written out in each of the three split-K tiles: through a common helper the compiler allocates this kernel's
    // registers anew -- 80 VGPRs and occupancy 5 where the loop was measured at 82 and 4 -- and changes the float64 tiles'
    // instruction streams, measurably at 1 x 240 frames; NOTEBOOK.md.)
    auto slot = [&](int w, int r) { return red + ((w * 16 + r) * 64 + lane); };
    if (wave != 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) *slot(wave, r) = acc[r];
    }
    __syncthreads();
    if (wave != 0 || !col_ok) return;
    const float bias = p.bias ? p.bias[col] : 0.f;
    const float slope = p.alpha ? p.alpha[col] : p.leaky;
    const bool act = p.alpha != nullptr || p.use_leaky;
    float *ob = p.out + (long long)b * p.out_bstride;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = m0 + (r & 3) + 8 * (r >> 2) + 4 * lk;
        if (row < rows) {
            float v = ((acc[r] + *slot(1, r)) + *slot(2, r)) + *slot(3, r) + bias;
            if (act) v = v > 0.f ? v : slope * v;
            ob[(long long)row * p.ldo + col] = v;
        }
    }
}

__device__ __forceinline__ void conv1d_small_tile32(const ConvArgs &p, int bx, int by, int b, float *red) {
    const int rows = __builtin_amdgcn_readfirstlane(item_rows(p.n_frames, b, p.rows_per_frame, p.max_rows));
    const int m0 = bx * 32;
    if (m0 >= rows) return;
    if (m0 - p.pad_l >= 0 && m0 + 31 - p.pad_l + (p.ks - 1) * p.dil < rows) conv1d_small_tile32_body<true>(p, bx, by, b, red, rows);
    else conv1d_small_tile32_body<false>(p, bx, by, b, red, rows);
}

// ---------------------------------------------------------------------------------------------------------
// The F0-net's convolutions in float64 (ConvArgs::precise; the operand modes: head comment).
// The F0 contour is the one quantity of the graph that is INTEGRATED (phase = running float32 sum of f0 / pulse_rate,
// reference tf_wavetable.py:429-492): a contour that differs from the exact one in the last bit of a few samples sends the
// float32 phase chain down another rounding path, the difference stays for the rest of the utterance and moves every pulse
// behind it -- measured end to end it, not the WaveNet, spent the float32 error budget, and the error grew with the length
// of the utterance (scripts/experiments/f0_error_probe.py).  The net is mel-rate and < 1 % of the
// work, so it runs on v_mfma_f64_16x16x4_f64.
// The 16 x 16 tile has the skeleton of the 32 x 32 float32 tile: operands straight from L2, K in groups of 16 channels of a tap
// split over the block's four waves, the quarters summed through LDS in wave order (head comment).  Lane (r = lane & 15, kq =
// lane >> 4) loads A[r][16g + 4kq .. + 3] for four MFMA steps (step s contracts the channels 16g + 4kq' + s, kq' = 0..3) and
// W[16g + 4kq + s][col r].
// C/D layout of the f64 MFMA (MI355X_MICROARCH.md): col = lane & 15, row = (lane >> 4) + 4 * reg.
// Needs cin % 4 == 0 and 16-byte aligned rows (f64_conv_eligible; other shapes keep the float32 kernels).
typedef double f64x4 __attribute__((ext_vector_type(4)));

template <bool F64> struct F64Operand;
template <> struct F64Operand<false> {
    typedef float scalar;
    typedef float4 quad;
    static __device__ __forceinline__ const float *pick(const float *f32, const double *) { return f32; }
};
template <> struct F64Operand<true> {
    typedef double scalar;
    typedef double4 quad;
    static __device__ __forceinline__ const double *pick(const float *, const double *f64) { return f64; }
};

template <bool XF64, bool WF64>
__device__ __forceinline__ void conv1d_f64_tile(const ConvArgs &p, int bx, int by, int b, double *red) {
    typedef typename F64Operand<XF64>::scalar xs_t;
    typedef typename F64Operand<XF64>::quad xq_t;
    typedef typename F64Operand<WF64>::scalar ws_t;
    const int rows = item_rows(p.n_frames, b, p.rows_per_frame, p.max_rows);
    const int m0 = bx * 16;
    if (m0 >= rows) return;
    const int n0 = by * 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const xs_t *xb = F64Operand<XF64>::pick(p.x, p.x64) + (long long)b * p.x_bstride;
    const ws_t *wbase = F64Operand<WF64>::pick(p.w, p.w64);
    const int groups_per_tap = (p.cin + 15) >> 4;          // groups of 16 input channels (the last one of a tap may be short)
    const int n_groups = p.ks * groups_per_tap;
    const int g_begin = (n_groups * wave) / 4, g_end = (n_groups * (wave + 1)) / 4;
    const bool col_ok = n0 + r16 < p.cout;
    const ws_t *wcol = wbase + min(n0 + r16, p.cout - 1);
    f64x4 acc;
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = 0.0;

    // Requests only (clamped addresses); the masks follow when the batch is consumed.  (Round 4, read off the ISA: with
    // `ok ? t : 0` right behind each load the compiler waited for every group's five loads before it issued the next group's
    // -- serial round trips for a batch of groups "in flight".)
    auto load_group = [&](int g, xq_t &av, ws_t (&bv)[4]) {
        const int tap = g / groups_per_tap;
        const int ci = min((g - tap * groups_per_tap) * 16 + 4 * kq, p.cin - 4);
        const long long ci_x = ci;      // (widened here, in front of map_row: the compiler then orders the load's address code as it always did)
        const int src = map_row(m0 + r16 - p.pad_l + tap * p.dil, rows, p.pad_mode);
        av = *reinterpret_cast<const xq_t *>(xb + (long long)max(src, 0) * p.ldx + ci_x);
        const ws_t *wk = wcol + (long long)(tap * p.cin + ci) * p.cout;
#pragma unroll
        for (int st = 0; st < 4; ++st) bv[st] = wk[(long long)st * p.cout];
    };
    auto mask_group = [&](int g, xq_t &av) {
        const int tap = g / groups_per_tap;
        const bool ci_ok = (g - tap * groups_per_tap) * 16 + 4 * kq < p.cin;      // short last group of a tap
        const bool ok = ci_ok && map_row(m0 + r16 - p.pad_l + tap * p.dil, rows, p.pad_mode) >= 0;
        mask_quad(av, ok);
    };
    // groups in flight beside the one being multiplied: the tile spends 4 MFMAs (256 cycles) on a group, an L2 round trip is
    // several times that
    constexpr int DEPTH = XF64 ? 3 : 4;
    xq_t a_cur[DEPTH], a_nxt[DEPTH];
    ws_t b_cur[DEPTH][4], b_nxt[DEPTH][4];
#pragma unroll
    for (int d = 0; d < DEPTH; ++d)
        if (g_begin + d < g_end) load_group(g_begin + d, a_cur[d], b_cur[d]);
#pragma unroll
    for (int d = 0; d < DEPTH; ++d)
        if (g_begin + d < g_end) mask_group(g_begin + d, a_cur[d]);
    for (int g = g_begin; g < g_end; g += DEPTH) {
#pragma unroll
        for (int d = 0; d < DEPTH; ++d)
            if (g + DEPTH + d < g_end) load_group(g + DEPTH + d, a_nxt[d], b_nxt[d]);
#pragma unroll
        for (int d = 0; d < DEPTH; ++d) {
            if (g + d < g_end) {
#pragma unroll
                for (int st = 0; st < 4; ++st) {
                    const xs_t af = st == 0 ? a_cur[d].x : st == 1 ? a_cur[d].y : st == 2 ? a_cur[d].z : a_cur[d].w;
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64((double)af, (double)b_cur[d][st], acc, 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int d = 0; d < DEPTH; ++d)
            if (g + DEPTH + d < g_end) mask_group(g + DEPTH + d, a_nxt[d]);
#pragma unroll
        for (int d = 0; d < DEPTH; ++d) {
            a_cur[d] = a_nxt[d];
#pragma unroll
            for (int st = 0; st < 4; ++st) b_cur[d][st] = b_nxt[d][st];
        }
    }
    // the four K quarters: the waves 1..3 park their partial tile in LDS, wave 0 adds the quarters in wave order (and, writing
    // float32, rounds ONCE)
    auto slot = [&](int w, int r) { return red + ((w * 4 + r) * 64 + lane); };
    if (wave != 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) *slot(wave, r) = acc[r];
    }
    __syncthreads();
    // (a loop of one tile with `continue`, the shape the fold has in the 32 x 32 tile: as a plain `if` or an early return the
    // compiler lays out the epilogue's branches differently -- NOTEBOOK.md)
#pragma unroll
    for (int tile = 0; tile < 1; ++tile) {
        if (wave != tile || !col_ok) continue;
        const int col = n0 + r16;
        const double bias = p.bias ? (double)p.bias[col] : 0.0;
        const double slope = (double)(p.alpha ? p.alpha[col] : p.leaky);
        const bool act = p.alpha != nullptr || p.use_leaky;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = m0 + kq + 4 * r;
            if (row < rows) {
                double q[4];
#pragma unroll
                for (int w = 0; w < 4; ++w) q[w] = w == 0 ? acc[r] : *slot(w, r);
                double v = ((q[0] + q[1]) + q[2]) + q[3] + bias;
                if (act) v = v > 0.0 ? v : slope * v;
                const long long at = (long long)b * p.out_bstride + (long long)row * p.ldo + col;
                if (p.out64) p.out64[at] = v;
                else p.out[at] = (float)v;
            }
        }
    }
}

// The 32 x 32 float64 tile of the large launches (round 5).  Same sums in the same order as conv1d_f64_tile -- wave w contracts
// K quarter w of all four 16 x 16 sub-tiles, the quarters meet through LDS in wave order --, but the loop is written for the
// issue budget of a CU it shares with fp32 MFMA blocks (every vector instruction of a wave waits for a gap in the co-resident
// waves' MFMA bursts): tap / channel group of a quarter advance in scalar registers (no division per group), the operand
// addresses are a per-lane base + one scalar offset per group, two loop bodies ping-pong the operand registers (no copies),
// row masks only in the first / last tile of an item.
template <bool XF64, bool WF64, bool INTERIOR>
__device__ __forceinline__ void conv1d_f64_tile32_body(const ConvArgs &p, int bx, int by, int b, double *red, int rows) {
    typedef typename F64Operand<XF64>::scalar xs_t;
    typedef typename F64Operand<XF64>::quad xq_t;
    typedef typename F64Operand<WF64>::scalar ws_t;
    const int m0 = bx * 32, n0 = by * 32;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, kq = lane >> 4;
    const xs_t *xb = F64Operand<XF64>::pick(p.x, p.x64) + (long long)b * p.x_bstride;
    const ws_t *wbase = F64Operand<WF64>::pick(p.w, p.w64);
    const int cin = p.cin, cout = p.cout, ldx = p.ldx;
    const int gpt = (cin + 15) >> 4;                        // groups of 16 input channels per tap (the last one may be short)
    const int n_groups = p.ks * gpt;
    const int g_begin = (n_groups * wave) / 4, g_end = (n_groups * (wave + 1)) / 4;
    const bool short_tail = (cin & 15) != 0;
    bool col_ok[2];
    const ws_t *wlane[2];                                   // W[4 kq][column] of the lane
    const xs_t *xlane[2];                                   // x[tile row of the lane at tap 0][4 kq]
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
        const int col = n0 + 16 * ct + r16;
        col_ok[ct] = col < cout;
        wlane[ct] = wbase + min(col, cout - 1) + (long long)(4 * kq) * cout;
    }
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) xlane[rt] = xb + (long long)(m0 + 16 * rt + r16 - p.pad_l) * ldx + 4 * kq;
    f64x4 acc[2][2];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[rt][ct][r] = 0.0;

    // scalar cursor of the quarter: tap and channel group of the next group to request
    int c_tap = g_begin / gpt, c_cg = g_begin - c_tap * gpt;
    c_tap = __builtin_amdgcn_readfirstlane(c_tap);
    c_cg = __builtin_amdgcn_readfirstlane(c_cg);
    auto request = [&](xq_t (&av)[2], ws_t (&bv)[2][4]) {   // the group at the cursor; the cursor moves on
        // channels 16 cg + 4 kq .. + 3 of the lane; behind cin (short last group of a tap) the lane reads the tap's last four
        // channels and is masked when the group is consumed
        const int ci_lane = short_tail ? min(16 * c_cg + 4 * kq, cin - 4) - 4 * kq : 16 * c_cg;
        if (INTERIOR) {
            const long long xoff = (long long)c_tap * p.dil * ldx + ci_lane;
#pragma unroll
            for (int rt = 0; rt < 2; ++rt) av[rt] = *reinterpret_cast<const xq_t *>(xlane[rt] + xoff);
        } else {
#pragma unroll
            for (int rt = 0; rt < 2; ++rt) {
                const int src = map_row(m0 + 16 * rt + r16 - p.pad_l + c_tap * p.dil, rows, p.pad_mode);
                av[rt] = *reinterpret_cast<const xq_t *>(xb + (long long)max(src, 0) * ldx + 4 * kq + ci_lane);
            }
        }
        const long long woff = ((long long)c_tap * cin + ci_lane) * cout;
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int st = 0; st < 4; ++st) bv[ct][st] = wlane[ct][woff + (long long)st * cout];
        const int wrap = s_flag_ge(c_cg + 1, gpt);
        c_cg = s_select(wrap, 0, c_cg + 1);
        c_tap += wrap;
    };
    auto consume = [&](int tap, int cg, xq_t (&av)[2], ws_t (&bv)[2][4]) {
        if (!INTERIOR || short_tail) {
            const bool ci_ok = 16 * cg + 4 * kq < cin;
#pragma unroll
            for (int rt = 0; rt < 2; ++rt) {
                const bool ok = ci_ok && (INTERIOR || map_row(m0 + 16 * rt + r16 - p.pad_l + tap * p.dil, rows, p.pad_mode) >= 0);
                mask_quad(av[rt], ok);
            }
        }
#pragma unroll
        for (int st = 0; st < 4; ++st)
#pragma unroll
            for (int rt = 0; rt < 2; ++rt) {
                const xs_t af = st == 0 ? av[rt].x : st == 1 ? av[rt].y : st == 2 ? av[rt].z : av[rt].w;
                const double a64 = (double)af;
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) acc[rt][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a64, (double)bv[ct][st], acc[rt][ct], 0, 0, 0);
            }
    };
    xq_t a0[2], a1[2];
    ws_t b0[2][4], b1[2][4];
    int t0 = c_tap, g0 = c_cg, t1 = 0, g1 = 0;               // tap / channel group of the groups held in set 0 / 1
    if (g_begin < g_end) request(a0, b0);
    for (int g = g_begin; g < g_end; g += 2) {
        if (g + 1 < g_end) {
            t1 = c_tap;
            g1 = c_cg;
            request(a1, b1);
        }
        consume(t0, g0, a0, b0);
        if (g + 1 >= g_end) break;
        if (g + 2 < g_end) {
            t0 = c_tap;
            g0 = c_cg;
            request(a0, b0);
        }
        consume(t1, g1, a1, b1);
    }
    // the four K quarters: every wave parks its partial tiles in LDS, tile t is finished by wave t, which adds the quarters in
    // wave order (and, writing float32, rounds ONCE)
    auto slot = [&](int w, int tile, int r) { return red + (((w * 4 + tile) * 4 + r) * 64 + lane); };
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
            const int tile = rt * 2 + ct;
            if (wave != tile) {
#pragma unroll
                for (int r = 0; r < 4; ++r) *slot(wave, tile, r) = acc[rt][ct][r];
            }
        }
    __syncthreads();
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
            const int tile = rt * 2 + ct;
            if (wave != tile || !col_ok[ct]) continue;
            const int col = n0 + 16 * ct + r16;
            const double bias = p.bias ? (double)p.bias[col] : 0.0;
            const double slope = (double)(p.alpha ? p.alpha[col] : p.leaky);
            const bool act = p.alpha != nullptr || p.use_leaky;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m0 + 16 * rt + kq + 4 * r;
                if (row < rows) {
                    double q[4];
#pragma unroll
                    for (int w = 0; w < 4; ++w) q[w] = w == tile ? acc[rt][ct][r] : *slot(w, tile, r);
                    double v = ((q[0] + q[1]) + q[2]) + q[3] + bias;
                    if (act) v = v > 0.0 ? v : slope * v;
                    const long long at = (long long)b * p.out_bstride + (long long)row * p.ldo + col;
                    if (p.out64) p.out64[at] = v;
                    else p.out[at] = (float)v;
                }
            }
        }
}

template <bool XF64, bool WF64>
__device__ __forceinline__ void conv1d_f64_tile32(const ConvArgs &p, int bx, int by, int b, double *red) {
    const int rows = __builtin_amdgcn_readfirstlane(item_rows(p.n_frames, b, p.rows_per_frame, p.max_rows));
    const int m0 = bx * 32;
    if (m0 >= rows) return;
    if (m0 - p.pad_l >= 0 && m0 + 31 - p.pad_l + (p.ks - 1) * p.dil < rows) conv1d_f64_tile32_body<XF64, WF64, true>(p, bx, by, b, red, rows);
    else conv1d_f64_tile32_body<XF64, WF64, false>(p, bx, by, b, red, rows);
}

__device__ __forceinline__ void conv1d_f64_dispatch32(const ConvArgs &p, int bx, int by, int b, double *red) {
    if (p.x64) conv1d_f64_tile32<true, true>(p, bx, by, b, red);
    else if (p.w64) conv1d_f64_tile32<false, true>(p, bx, by, b, red);
    else conv1d_f64_tile32<false, false>(p, bx, by, b, red);
}

// operand mode of a float64 member: wave-uniform (kernel arguments)
__device__ __forceinline__ void conv1d_f64_dispatch(const ConvArgs &p, int bx, int by, int b, double *red) {
    if (p.x64) conv1d_f64_tile<true, true>(p, bx, by, b, red);
    else if (p.w64) conv1d_f64_tile<false, true>(p, bx, by, b, red);
    else conv1d_f64_tile<false, false>(p, bx, by, b, red);
}

__global__ __launch_bounds__(256) void conv1d_f64_kernel(ConvArgs p) {
    __shared__ double red[4 * 4 * 64];
    conv1d_f64_dispatch(p, blockIdx.x, blockIdx.y, blockIdx.z, red);
}

__global__ __launch_bounds__(256) void conv1d_small_kernel(ConvArgs p) {
    __shared__ float red[4 * 16 * 64];
    conv1d_small_tile32(p, blockIdx.x, blockIdx.y, blockIdx.z, red);
}

// Up to three independent small convolutions in one launch (the n-th layers of the F0-net, the VTF-net and the
// conditioning convolution all read the mel input): at a few hundred rows a launch is latency-bound, so sharing it
// costs nothing and removes launches from the critical path.  Blocks [start[k], start[k+1]) belong to convolution k.
struct SmallConvGroup {
    ConvArgs c[3];
    int start[4];
    int gx[3], gy[3];
};

__global__ __launch_bounds__(256) void conv1d_small_group_kernel(SmallConvGroup g) {
    __shared__ __attribute__((aligned(16))) float red[4 * 16 * 64];      // 16 384 bytes: four quarters of a 32 x 32 float32 tile (the f64 tile uses 8 192 bytes of it: 4 * 4 * 64 doubles)
    const int id = blockIdx.x;
    const int k = (id >= g.start[1]) + (id >= g.start[2]);
    const int local = id - g.start[k];
    const int bx = local % g.gx[k];
    const int t = local / g.gx[k];
    if (g.c[k].precise) conv1d_f64_dispatch(g.c[k], bx, t % g.gy[k], t / g.gy[k], reinterpret_cast<double *>(red));   // 16 x 16 tiles
    else conv1d_small_tile32(g.c[k], bx, t % g.gy[k], t / g.gy[k], red);
}

// The same convolutions at large launches (batch 16 x 10 s: 12 800 rows): an LDS-staged tile kernel with the summation
// order of the head comment.  Block = 4 waves, 64 rows x 128 columns; wave w owns the columns 32 w .. 32 w + 31 of both
// 32-row tiles.  K runs in slices of groups of 8 channels that never cross a quarter boundary.  A wave keeps two accumulator
// sets per tile: the chain of the quarter in progress and the running sum q0, q0 + q1, ... -- the same left fold
// ((q0 + q1) + q2) + q3 + bias, the same MFMA steps in the same order, hence bit-identical results.
// (Rounds 3-4 staged the slices through registers -- conv1d_mel_tile, removed in round 5: see below.)
constexpr int MT_COLS = 128;

// Round 5: the slices are brought in by LDS-DMA and the K loop has no vector bookkeeping.
// What the round-4 kernel (conv1d_mel_tile, register-staged) lost, read off in-kernel stamps and ablations (NOTEBOOK.md, round 5): at 16 x
// 10 s its members ran at 0.39 / 0.29 / 0.41 of the matrix peak although neither the loads (ablated: -6 %) nor the LDS traffic
// bound them.  Two or three blocks share a CU; while one wave is inside its burst of 64-cycle MFMAs, every VECTOR instruction of
// a co-resident wave waits for a gap between them (~one MFMA each).  A wave's non-MFMA phase of ~25 vector instructions per
// slice (address arithmetic for 18 loads and 6 ds_writes, cursor selects the compiler put on the vector ALU, LDS addresses)
// thereby took longer than the other wave's MFMA burst -- the SIMD idled 40 % of the time --, the four quarter folds (96 vector
// instructions each) and the epilogue (300) likewise.  Here, per slice of two groups of 8 channels, a wave issues
//   3 LDS-DMA requests (activations: 32 rows x 8 channels of its group and row tile; weights: four k rows x 128 columns),
//   8 LDS reads, 16 MFMAs, one counted wait + one barrier,
// and NO vector ALU instruction: the slice cursor lives in scalar registers (s_cmp / s_cselect through inline asm: the
// compiler lowers a uniform bool -> int through v_cndmask + v_readfirstlane), the request addresses are scalar bases + per-lane
// offsets computed once, the four stages of the ring are four unrolled loop bodies whose LDS offsets are immediates.  Folds are
// packed adds (16 + 8 moves per fold), the epilogue 3.5 vector instructions per output.
// Same MFMA steps in the same order, the same quarter fold: bit-identical to conv1d_small_tile32 (tests: the large launch against
// the same rows in small launches).
//   activations of a stage: [group j][row tile t][32 rows][2 halves of 4 channels], half h of row r at slot h ^ ((r >> 3) & 1)
//                           (the 16 rows of a ds_read_b128 phase then hit all 16 bank quads)
//   weights of a stage:     [16 k rows][128 columns], the row's 16-byte chunks rotated by 8 positions when (k >> 2) & 1 (the two
//                           k rows of a ds_read_b32 -- lanes 0-31 and 32-63 -- then sit in different banks)
constexpr int M2_NG = 2, M2_STAGES = 4;
constexpr int M2_A_FLOATS = M2_NG * 64 * 8, M2_W_FLOATS = M2_NG * 8 * MT_COLS, M2_STAGE_FLOATS = M2_A_FLOATS + M2_W_FLOATS;

__device__ __forceinline__ void lds_dma16_s(const float *sbase, unsigned voff_bytes, unsigned lds_byte_addr) {
    asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(lds_byte_addr), "v"(voff_bytes), "s"(sbase) : "memory", "m0");
}
// INTERIOR: every source row of the tile (all taps) lies inside the item -- the activation request is then a scalar base + the
// lanes' constant offsets, and a slice is one basic block (the compiler interleaves its scalar code with the MFMAs)
template <bool INTERIOR>
__device__ __forceinline__ void conv1d_mel_tile_dma_body(const ConvArgs &p, int bx, int by, int b, float *lds, int rows) {
    typedef __attribute__((address_space(3))) float lds_float;
    const int m0 = bx * 64;
    const int n0 = by * MT_COLS;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lrow = lane & 31, lk = lane >> 5;
    const int gpt = p.cin >> 3;                              // groups of 8 input channels per tap
    const int n_groups = p.ks * gpt;
    const int cout = p.cout, ldx = p.ldx;
    const unsigned lds_base = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(lds_float *)lds);

    // ---- DMA roles.  The wave fetches group jw = wave >> 1 of a slice: the activations of row tile tw = wave & 1 and the k
    // rows 4 (wave & 1) .. + 3 of the group's eight.  (A slice of one group: the waves of group 1 fetch group 0 again -- the
    // same three requests per wave and slice whatever the slice, which is what the counted waits count.)
    const int jw = wave >> 1, tw = wave & 1;
    const int d_row = lane >> 1, d_half = (lane & 1) ^ ((lane >> 4) & 1);            // slot lane & 1 of row lane >> 1 holds half d_half
    const unsigned a_voff = (unsigned)(d_row * ldx + 4 * d_half) * 4u;               // interior of an item: row pitch x row + half
    const unsigned a_dst = lds_base + (unsigned)((jw * 2 + tw) * 256) * 4u;          // + stage
    // weights: instruction i covers k rows kin = 4 tw + 2 i + (lane >> 5) of the group; position lane & 31 of the row holds the
    // chunk (position - 8 ((kin >> 2) & 1)) & 31 = columns n0 + 4 chunk .. + 3 (clamped: columns behind cout are not stored)
    unsigned w_voff[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int kin = 4 * tw + 2 * i + (lane >> 5);
        const int chunk = ((lane & 31) - 8 * ((kin >> 2) & 1)) & 31;
        w_voff[i] = (unsigned)(kin * cout + min(n0 + 4 * chunk, cout - 4)) * 4u;
    }
    const unsigned w_dst = lds_base + (unsigned)(M2_A_FLOATS + (jw * 8 + 4 * tw) * MT_COLS) * 4u;      // + 1024 i + stage
    // scalar bases: the tile's first source row at tap 0 (may lie outside the item: only used when the whole 32-row piece is
    // inside) and the weight matrix; per slice a 32-bit byte offset is added (the launcher bounds both tensors by 2^31 bytes)
    const int r_tile = m0 + 32 * tw - p.pad_l;
    const float *xb = p.x + (long long)b * p.x_bstride;
    const float *x_tile = xb + (long long)r_tile * ldx;
    const float *wgt = p.w;
    const int tap_rows = p.dil, tap_bytes = p.dil * ldx * 4, group_bytes = 8 * cout * 4;

    // ---- the slice cursor (scalar registers only): quarter end qe, first group gs, its tap and channel group, and the byte
    // offsets that go with them.  A cursor that has reached the last slice stays there: the requests behind the end fetch the
    // last slice again into a free stage, so every iteration issues the same three requests and waits with the same count.
    int c_q = 0, c_gs = 0, c_qe = n_groups >> 2, c_tap = 0, c_cg = 0;
    auto cursor_groups = [&]() { return min(M2_NG, c_qe - c_gs); };
    auto cursor_info = [&]() {                               // groups | quarter complete << 2: what the MFMA side needs of a slice
        const int n = cursor_groups();
        return n | (s_flag_ge(c_gs + n, c_qe) << 2);
    };
    auto advance = [&]() {
        const int n = cursor_groups();
        const int gs2 = c_gs + n;
        int cg2 = c_cg + n, tap2 = c_tap;
#pragma unroll
        for (int i = 0; i < M2_NG; ++i) {                    // n <= M2_NG wraps at most (gpt >= 1)
            const int wrap = s_flag_ge(cg2, gpt);
            cg2 -= wrap * gpt;
            tap2 += wrap;
        }
        const int next_q = s_flag_ge(gs2, c_qe);             // (quarters are never empty: n_groups >= 4)
        const int q2 = c_q + next_q;
        const int qe2 = s_select(next_q, (n_groups * (q2 + 1)) >> 2, c_qe);
        const int last = s_flag_ge(gs2, n_groups);
        c_gs = s_select(last, c_gs, gs2);
        c_cg = s_select(last, c_cg, cg2);
        c_tap = s_select(last, c_tap, tap2);
        c_q = s_select(last, c_q, q2);
        c_qe = s_select(last, c_qe, qe2);
    };
    auto issue = [&](int stage) {
        const int ng = cursor_groups();
        const int second = jw & s_flag_ge(ng, M2_NG);        // this wave fetches the slice's second group
        const int wrap = second & s_flag_ge(c_cg + 1, gpt);
        const int cg = s_select(wrap, 0, c_cg + second);
        const int tap = c_tap + wrap;
        const int g = c_gs + second;
        const unsigned st_off = (unsigned)(stage * M2_STAGE_FLOATS) * 4u;
        if (INTERIOR) {
            lds_dma16_s(s_ptr_add(x_tile, tap * tap_bytes + cg * 32), a_voff, a_dst + st_off);
        } else {                                             // first / last tile of an item: padding per row
            const int src = map_row(r_tile + tap * tap_rows + d_row, rows, p.pad_mode);
            lds_dma16(src >= 0 ? xb + (long long)src * ldx + cg * 8 + 4 * d_half : p.zeros, a_dst + st_off);
        }
        const float *wk = s_ptr_add(wgt, g * group_bytes);
        lds_dma16_s(wk, w_voff[0], w_dst + st_off);
        lds_dma16_s(wk, w_voff[1], w_dst + st_off + 1024u);
    };

    f32x16 cur[2], sum[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) cur[t][r] = sum[t][r] = 0.f;

    int n_slices = 0;
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) n_slices += ((((n_groups * (qq + 1)) >> 2) - ((n_groups * qq) >> 2)) + M2_NG - 1) / M2_NG;
    // ring of the slices in flight: what the MFMA side needs of them
    int info0, info1, info2;
    info0 = cursor_info();
    issue(0);
    advance();
    info1 = cursor_info();
    issue(1);
    advance();
    info2 = cursor_info();
    issue(2);
    advance();
    // operand addresses of the MFMA lanes (floats, + stage): activations of (group j, tile t): + (2 j + t) 256; weights of
    // (group j, step st): + j 1024 + st 128
    const int bcol = 32 * wave + lrow;
    const float *al = lds + lrow * 8 + 4 * (lk ^ ((lrow >> 3) & 1));
    const float *bl = lds + M2_A_FLOATS + 4 * lk * MT_COLS + 4 * (((bcol >> 2) + 8 * lk) & 31) + (bcol & 3);

    auto body = [&](auto stage_c) {
        constexpr int ST = decltype(stage_c)::value;         // the stage of this slice; the request goes to the one before it
        // the slice has landed: this wave's requests (all but those of the two slices behind it), then everybody's
        asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        __syncthreads();                                     // ... and the stage read last in the slice before is free
        // the operands of both groups are requested first (a slice of one group reads a stale second group and drops it): their
        // LDS latency passes under the request code
        float4 av[M2_NG][2];
        float bv[M2_NG][4];
#pragma unroll
        for (int j = 0; j < M2_NG; ++j) {
#pragma unroll
            for (int t = 0; t < 2; ++t) av[j][t] = *reinterpret_cast<const float4 *>(al + ST * M2_STAGE_FLOATS + (2 * j + t) * 256);
#pragma unroll
            for (int st = 0; st < 4; ++st) bv[j][st] = bl[ST * M2_STAGE_FLOATS + j * 8 * MT_COLS + st * MT_COLS];
        }
        const int info = info0;
        info0 = info1;
        info1 = info2;
        info2 = cursor_info();
        issue((ST + M2_STAGES - 1) % M2_STAGES);
        advance();
        auto group = [&](int j) {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                f32x16 c = cur[t];
                c = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j][t].x, bv[j][0], c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j][t].y, bv[j][1], c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j][t].z, bv[j][2], c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j][t].w, bv[j][3], c, 0, 0, 0);
                cur[t] = c;
            }
        };
        group(0);
        if ((info & 3) == M2_NG) group(1);
        if (info >> 2) {                                     // the quarter is complete: ((q0 + q1) + q2) + q3, q0 as 0 + q0 (the
#pragma unroll                                               // chains start from +0, so q0 is never -0 and 0 + q0 has q0's bits)
            for (int t = 0; t < 2; ++t) {
                sum[t] = sum[t] + cur[t];
#pragma unroll
                for (int r = 0; r < 16; ++r) cur[t][r] = 0.f;
            }
        }
    };
    for (int sl = 0; sl < n_slices; sl += M2_STAGES) {
        body(std::integral_constant<int, 0>{});
        if (sl + 1 >= n_slices) break;
        body(std::integral_constant<int, 1>{});
        if (sl + 2 >= n_slices) break;
        body(std::integral_constant<int, 2>{});
        if (sl + 3 >= n_slices) break;
        body(std::integral_constant<int, 3>{});
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // the requests behind the end have landed before the block leaves

    const int col = n0 + bcol;
    if (col >= cout) return;
    const float bias = p.bias ? p.bias[col] : 0.f;
    const float slope = p.alpha ? p.alpha[col] : p.leaky;
    const bool act = p.alpha != nullptr || p.use_leaky;
    float *ob = p.out + (long long)b * p.out_bstride;
    if (m0 + 64 <= rows) {
        // a full tile: one address per lane (row 4 lk of the tile, its column), the 32 rows of the lane at scalar multiples of
        // the row pitch
        float *o0 = ob + (long long)(m0 + 4 * lk) * p.ldo + col;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float v = sum[t][r] + bias;
                if (act) v = v > 0.f ? v : slope * v;
                o0[(long long)(32 * t + (r & 3) + 8 * (r >> 2)) * p.ldo] = v;
            }
        return;
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = m0 + 32 * t + (r & 3) + 8 * (r >> 2) + 4 * lk;
            if (row < rows) {
                float v = sum[t][r] + bias;
                if (act) v = v > 0.f ? v : slope * v;
                ob[(long long)row * p.ldo + col] = v;
            }
        }
}

__device__ __forceinline__ void conv1d_mel_tile_dma(const ConvArgs &p, int bx, int by, int b, float *lds) {
    const int rows = __builtin_amdgcn_readfirstlane(item_rows(p.n_frames, b, p.rows_per_frame, p.max_rows));
    const int m0 = bx * 64;
    if (m0 >= rows) return;
    if (m0 - p.pad_l >= 0 && m0 + 63 - p.pad_l + (p.ks - 1) * p.dil < rows) conv1d_mel_tile_dma_body<true>(p, bx, by, b, lds, rows);
    else conv1d_mel_tile_dma_body<false>(p, bx, by, b, lds, rows);
}

__global__ __launch_bounds__(256, 3) void conv1d_mel_group_kernel(SmallConvGroup g) {
    __shared__ __attribute__((aligned(16))) float lds[M2_STAGES * M2_STAGE_FLOATS];
    const int id = blockIdx.x;
    const int k = (id >= g.start[1]) + (id >= g.start[2]);
    const int local = id - g.start[k];
    const int bx = local % g.gx[k];
    const int t = local / g.gx[k];
    if (g.c[k].precise) conv1d_f64_dispatch32(g.c[k], bx, t % g.gy[k], t / g.gy[k], reinterpret_cast<double *>(lds));     // 32 x 32 tiles
    else conv1d_mel_tile_dma(g.c[k], bx, t % g.gy[k], t / g.gy[k], lds);
}

static bool f64_conv_eligible(const ConvArgs &a) {
    // (the launch sequence only sets x64 / w64 / out64 when the shape is regular: rows of 4 k channels, 32-byte aligned)
    if (a.x64) return a.precise && a.w64 && a.cin % 4 == 0 && a.ldx % 4 == 0 && a.x_bstride % 4 == 0 && (uintptr_t)a.x64 % 32 == 0;
    return a.precise && a.cin % 4 == 0 && a.cin >= 4 && a.ldx % 4 == 0 && a.x_bstride % 4 == 0 && (uintptr_t)a.x % 16 == 0;
}

static bool small_conv_eligible(const ConvArgs &a) {
    if (f64_conv_eligible(a)) return true;              // a member of the shared mel-rate launches as well
    // no row limit: the mel-rate convolutions then sum K in the same order at every launch size, which keeps a padded
    // batch bit-identical to one-at-a-time runs (the F0 contour feeds the phase accumulator: rounding there is audible
    // in the last bits everywhere downstream)
    // (32-bit byte offsets inside an item and inside the weight tensor: conv1d_small_tile32)
    return a.cin % 8 == 0 && a.ldx % 4 == 0 && a.x_bstride % 4 == 0 && (uintptr_t)a.x % 16 == 0 &&
           (long long)a.ks * a.cin * a.cout * 4 < (1LL << 31) && ((long long)a.max_rows + a.ks * a.dil) * a.ldx * 4 < (1LL << 31);
}

bool launch_conv1d_mel_single(const ConvArgs &a, hipStream_t stream) {
    if (f64_conv_eligible(a)) {
        // F0-net convolution on its own (float64 accumulation): split-K 16x16 tiles at every size
        dim3 grid((a.max_rows + 15) / 16, (a.cout + 15) / 16, a.batch);
        hipLaunchKernelGGL(conv1d_f64_kernel, grid, dim3(256), 0, stream, a);
    } else if (small_conv_eligible(a)) {
        // mel-rate sub-nets at small batch: latency bound, split-K 32x32 tiles
        dim3 grid((a.max_rows + 31) / 32, (a.cout + 31) / 32, a.batch);
        hipLaunchKernelGGL(conv1d_small_kernel, grid, dim3(256), 0, stream, a);
    } else {
        return false;
    }
    return true;
}

void launch_conv1d_group(const ConvArgs *convs, int n, hipStream_t stream) {
    int small[3], n_small = 0;
    for (int i = 0; i < n && i < 3; ++i)
        if (convs[i].max_rows > 0 && convs[i].batch > 0 && small_conv_eligible(convs[i])) small[n_small++] = i;
    // large launches: LDS-staged 64 x 128 tiles (conv1d_mel_tile_dma: same sums in the same order), also for a single convolution
    // (the conditioning chains of the WaveNet blocks behind the first one come one by one).  The tile's LDS-DMA needs 16-byte
    // weight chunks, the zero page and tensors below 2^31 bytes (32-bit offsets); other shapes keep the small-launch kernel.
    long long work = 0;
    bool dma_ok = true;
    for (int k = 0; k < n_small; ++k) {
        const ConvArgs &c = convs[small[k]];
        work += (long long)c.max_rows * c.batch;
        if (f64_conv_eligible(c)) continue;
        // (at least four groups of 8 channels: the tile's slice cursor takes every K quarter to be non-empty)
        dma_ok = dma_ok && c.zeros && c.cout % 4 == 0 && c.cout >= 4 && (uintptr_t)c.w % 16 == 0 && c.ks * (c.cin >> 3) >= 4 &&
                 (long long)c.ks * c.cin * c.cout * 4 < (1LL << 31) && ((long long)c.max_rows + c.ks * c.dil) * c.ldx * 4 < (1LL << 31);
    }
    const bool big = work >= 3 * 4096 && dma_ok;
    if (n > 3 || n_small < 1 || (n_small < 2 && !big)) {
        for (int i = 0; i < n; ++i) launch_conv1d(convs[i], EPI_LINEAR, stream);
        return;
    }
    // Block order inside the launch: the float32 members first, the longest chain (largest K) in front, so that the MFMA-bound
    // blocks are resident from the start; the float64 members (short, latency-bound blocks) behind them fill the slots the others
    // leave.  Round 5, 16 x 10 s, same box: float64 last 241 us front end, by K alone 257, float64 first 294.
    auto before = [&](int a, int b) {                        // member a goes in front of member b
        const bool fa = f64_conv_eligible(convs[a]), fb = f64_conv_eligible(convs[b]);
        if (fa != fb) return fb;
        return convs[a].ks * convs[a].cin > convs[b].ks * convs[b].cin;
    };
    for (int i = 0; i < n_small; ++i)
        for (int j = i + 1; j < n_small; ++j)
            if (before(small[j], small[i])) {
                const int t = small[i];
                small[i] = small[j];
                small[j] = t;
            }
    const int tile_m = big ? 64 : 32, tile_n = big ? MT_COLS : 32;
    SmallConvGroup g;
    int total = 0;
    for (int k = 0; k < 3; ++k) {
        g.start[k] = total;
        if (k < n_small) {
            g.c[k] = convs[small[k]];
            g.c[k].precise = f64_conv_eligible(g.c[k]) ? 1 : 0;
            // float64-accumulating members (the F0-net): 16 x 16 tiles in the small launches, 32 x 32 in the large ones
            const int tm = g.c[k].precise ? (big ? 32 : 16) : tile_m, tn = g.c[k].precise ? (big ? 32 : 16) : tile_n;
            g.gx[k] = (g.c[k].max_rows + tm - 1) / tm;
            g.gy[k] = (g.c[k].cout + tn - 1) / tn;
            total += g.gx[k] * g.gy[k] * g.c[k].batch;
        } else {
            g.c[k] = convs[small[0]];
            g.gx[k] = g.gy[k] = 1;
        }
    }
    g.start[3] = total;
    for (int k = n_small; k < 3; ++k) g.start[k] = 0x7fffffff;
    if (big) hipLaunchKernelGGL(conv1d_mel_group_kernel, dim3((unsigned)total), dim3(256), 0, stream, g);
    else hipLaunchKernelGGL(conv1d_small_group_kernel, dim3((unsigned)total), dim3(256), 0, stream, g);
    for (int i = 0; i < n; ++i) {
        bool in_group = false;
        for (int k = 0; k < n_small; ++k) in_group |= small[k] == i;
        if (!in_group) launch_conv1d(convs[i], EPI_LINEAR, stream);
    }
}

}  // namespace mbx
