// A decoded F0 contour: Viterbi over YIN candidates (include/mbexwn_contour.h: mbxc_f0_candidates, mbxc_decode_f0; DESIGN.md
// section 6i; the host definition is mbexwn_vocoder_amd/f0decode.py::candidates_host and ::viterbi_host).
//
// f0_candidates_kernel: one 256-thread block per (frame, item).  Up to d' it is the tracker's frame (f0_frame.h).  Then wave
// 0 alone: every lane scans its lags once and keeps, for each of the up to 16 ascending thresholds, the first lag below it;
// 16 first-index reductions over the wave; lane n < N walks pick_n on to its local minimum; the weight sums P (per distinct
// lag, in ascending n) and U (no pick), the ranks by counting, and lanes 0 .. 7 write the eight slots.
//
// f0_decode_kernel: one 64-lane wave per item.  Lane 8 j + i owns the transition i -> j.  The chain of a step is: v =
// delta[i] + tr(i, j); the minimum over i inside the groups of 8 lanes by DPP (quad_perm twice, row_half_mirror); new[j] =
// best + loc[j]; one ds_bpermute (the crossbar, no LDS memory) hands lane 8 j + i the new[i] of group i; the minimum over
// that group is the frame's m, and delta[i] = new[i] - m.  Selects only: the wave never splits.  Off the chain: the
// arg-minimum is the first set bit of the group's byte in the wave's mask of v == best (the smallest i wins a tie), and
// the back pointers of a frame are 8 x 3 bits gathered by lane swaps into one word in LDS (16000 frames: 64 000 bytes).
// Costs, availabilities and transition costs do not depend on the chain either: the loads of the next sixteen frames are in
// flight while sixteen steps run.  Lane 0 then walks back through LDS, leaving the state of every frame in place of its
// pointers, and the wave writes the outputs (a walk on the scalar unit, the words fetched 64 at a time and read lane by
// lane, was measured and was slower).  Every loop runs to the clamped n_frames[b].
//
// Host and device must give the same bits: plain operators, contraction off, no fused multiply-add, the correctly rounded
// division.
#include <algorithm>
#include <climits>
#include <cmath>

#include "f0_frame.h"
#include "mbx_kernels.h"

#pragma clang fp contract(off)

namespace mbx {

constexpr float F0_COST_LIMIT = 1e6f;                       // f0decode.LIMIT

__global__ __launch_bounds__(F0_THREADS) void f0_candidates_kernel(CandidateArgs p) {
    extern __shared__ __attribute__((aligned(16))) float f0_smem[];
    __shared__ float s_energy;
    const PitchArgs &f = p.frame;
    const int k = blockIdx.x, b = blockIdx.y;
    if (k >= f.n_frames[b]) return;
    const int W = f.window, TM = f.tau_max, L = W + TM;
    float *d = f0_smem + L;                                 // (TM + 1) d'; f0_frame.h has the layout
    // length and centre from the device arrays, clamped to the item's row: a wrong entry must not address outside the buffer
    const long long n = min(max((long long)f.n_samples[b], 0LL), f.stride);
    const long long c = min(max(f.centres[(long long)b * f.max_frames + k], 0LL), n);
    const int bad = f0_frame_load(F0RowFetch(f.audio + (long long)b * f.stride, n, c, L), L, f0_smem);
    f0_frame_dprime(W, TM, f0_smem, &s_energy);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (wave != 0) return;

    // per threshold the first lag below it, and the first lag of the minimum, over [lo, hi]: per lane, then over the wave
    // (thresholds from n_thresholds on are -inf: nothing is below them)
    const int lo = max(f.tau_min, 2), hi = TM - 1, N = p.n_thresholds;
    int first[F0_MAX_THRESHOLDS];
#pragma unroll
    for (int nn = 0; nn < F0_MAX_THRESHOLDS; ++nn) first[nn] = INT_MAX;
    int best = INT_MAX;
    float best_v = INFINITY;
    for (int tau = lo + lane; tau <= hi; tau += 64) {
        const float v = d[tau];
#pragma unroll
        for (int nn = 0; nn < F0_MAX_THRESHOLDS; ++nn)
            if (v < p.thresholds[nn] && first[nn] == INT_MAX) first[nn] = tau;
        if (v < best_v) {
            best_v = v;
            best = tau;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
        for (int nn = 0; nn < F0_MAX_THRESHOLDS; ++nn) first[nn] = min(first[nn], __shfl_xor(first[nn], m, 64));
        const float ov = __shfl_xor(best_v, m, 64);
        const int oi = __shfl_xor(best, m, 64);
        if (ov < best_v || (ov == best_v && oi < best)) {
            best_v = ov;
            best = oi;
        }
    }
    // lane n < N: pick_n, walked on to its local minimum; INT_MAX is "no pick"
    const bool usable = !bad && s_energy >= f.e_min;
    int tau_n = INT_MAX;
#pragma unroll
    for (int nn = 0; nn < F0_MAX_THRESHOLDS; ++nn)
        if (lane == nn) tau_n = first[nn];
    if (!usable || lane >= N) tau_n = INT_MAX;
    if (tau_n != INT_MAX)
        while (tau_n + 1 <= hi && d[tau_n + 1] < d[tau_n]) ++tau_n;
    // P of this lane's lag and U, both added in ascending n; the first lane with a lag leads it
    float P = 0.f, U = 0.f;
    int leader = tau_n != INT_MAX;
#pragma unroll
    for (int m = 0; m < F0_MAX_THRESHOLDS; ++m) {
        const int tm = __shfl(tau_n, m, 64);
        const float wm = p.weights[m];
        if (m < N) {
            if (tm == INT_MAX) {
                U = U + wm;
            } else if (tm == tau_n) {
                P = P + wm;
                if (m < lane) leader = 0;
            }
        }
    }
    // keep the n_cand leaders with the largest P (the smaller lag wins a tie), listed by ascending lag
    int rank = 0;
#pragma unroll
    for (int m = 0; m < F0_MAX_THRESHOLDS; ++m) {
        const int tm = __shfl(tau_n, m, 64), lm = __shfl(leader, m, 64);
        const float pm = __shfl(P, m, 64);
        if (lm && m != lane && (pm > P || (pm == P && tm < tau_n))) ++rank;
    }
    const int keep = leader && rank < p.n_cand;
    int slot = 0;
#pragma unroll
    for (int m = 0; m < F0_MAX_THRESHOLDS; ++m) {
        const int tm = __shfl(tau_n, m, 64), km = __shfl(keep, m, 64);
        if (km && tm < tau_n) ++slot;
    }
    const int mine = keep ? slot : -1;
    int w_tau = INT_MAX;
    float w_P = 0.f;
#pragma unroll
    for (int m = 0; m < F0_MAX_THRESHOLDS; ++m) {
        const int tm = __shfl(tau_n, m, 64), sm = __shfl(mine, m, 64);
        const float pm = __shfl(P, m, 64);
        if (sm == lane) {
            w_tau = tm;
            w_P = pm;
        }
    }
    if (lane >= F0_SLOTS) return;
    float period = 0.f, cost = INFINITY, dprime = 1.f;
    if (lane == F0_SLOTS - 1) {
        cost = fmaxf(1.f - U, 0.f);
        if (!bad) dprime = best == INT_MAX ? d[lo] : best_v;
    } else if (w_tau != INT_MAX) {
        period = f0_refined_lag(d, w_tau);
        cost = fmaxf(1.f - w_P, 0.f);
        dprime = d[w_tau];
    }
    const long long o = ((long long)b * f.max_frames + k) * F0_SLOTS + lane;
    p.period[o] = period;
    p.cost[o] = cost;
    p.dprime[o] = dprime;
}

const char *fill_f0_candidates(CandidateArgs &a, const float *thresholds, const float *weights) {
    if (!a.period || !a.cost || !a.dprime || !thresholds || !weights) return "null pointer";
    PitchArgs f = a.frame;                                  // the tracker's checks of the arguments the two share
    f.threshold = 0.f;
    f.f0 = a.period;
    f.periodicity = a.cost;
    if (const char *why = check_track_f0(f)) return why;
    if (a.n_thresholds < 1 || a.n_thresholds > F0_MAX_THRESHOLDS) return "n_thresholds must be in 1 .. 16";
    if (a.n_cand < 1 || a.n_cand > F0_SLOTS - 1) return "n_cand must be in 1 .. 7";
    for (int nn = 0; nn < F0_MAX_THRESHOLDS; ++nn) {
        a.thresholds[nn] = -INFINITY;
        a.weights[nn] = 0.f;
    }
    for (int nn = 0; nn < a.n_thresholds; ++nn) {
        if (!std::isfinite(thresholds[nn])) return "the thresholds must be finite";
        if (nn > 0 && !(thresholds[nn] > thresholds[nn - 1])) return "the thresholds must be strictly ascending";
        if (!std::isfinite(weights[nn]) || weights[nn] < 0.f) return "the weights must be finite and not negative";
        a.thresholds[nn] = thresholds[nn];
        a.weights[nn] = weights[nn];
    }
    return nullptr;
}

void launch_f0_candidates(const CandidateArgs &a, hipStream_t stream) {
    if (a.frame.batch == 0) return;
    const size_t smem = (size_t)(a.frame.window + 2 * a.frame.tau_max + 1) * sizeof(float);
    hipLaunchKernelGGL(f0_candidates_kernel, dim3(a.frame.max_frames, a.frame.batch), dim3(F0_THREADS), smem, stream, a);
}

// ------------------------------------------------------------------------------------------------------------------------

constexpr int F0_DECODE_AHEAD = 16;                         // frames whose loads are in flight while as many steps run

// what lane 8 j + i holds of a frame: period and cost of its slots i and j
struct DecodeFrame {
    float pi, ci, pj, cj;
};

__device__ inline unsigned f0_dpp_quad_1032(unsigned v) { return __builtin_amdgcn_update_dpp(0u, v, 0xB1, 0xf, 0xf, true); }
__device__ inline unsigned f0_dpp_quad_2301(unsigned v) { return __builtin_amdgcn_update_dpp(0u, v, 0x4E, 0xf, 0xf, true); }
__device__ inline unsigned f0_dpp_half_mirror(unsigned v) { return __builtin_amdgcn_update_dpp(0u, v, 0x141, 0xf, 0xf, true); }

// the smaller of (v, arg) and a partner's pair, the smaller arg winning a tie: over lanes l ^ 1, l ^ 2 and 7 - l of a group
// of 8 lanes it leaves the group's minimum and the smallest index that has it on all eight.  Selects, no branches: the
// chain of a step is short only if the wave never splits.
#define F0_MIN_STEP(PERM)                                                  \
    {                                                                      \
        const float ov = __uint_as_float(PERM(__float_as_uint(v)));        \
        const int oa = (int)PERM((unsigned)arg);                           \
        const bool take = (ov < v) | ((ov == v) & (oa < arg));             \
        v = take ? ov : v;                                                 \
        arg = take ? oa : arg;                                             \
    }

__device__ inline void f0_group_min(float &v, int &arg) {
    F0_MIN_STEP(f0_dpp_quad_1032)
    F0_MIN_STEP(f0_dpp_quad_2301)
    F0_MIN_STEP(f0_dpp_half_mirror)
}

__device__ inline bool f0_cost_ok(float cst) { return (cst >= 0.f) & (cst <= F0_COST_LIMIT); }
__device__ inline bool f0_slot_available(bool unvoiced, float per, float cst) {
    return unvoiced | (f0_cost_ok(cst) & (per >= 1.f) & (per <= F0_COST_LIMIT));
}
// the minimum over a group of 8 lanes, on all eight.  No NaN comes here, so a compare and a select do (fminf would
// canonicalise its operands first)
__device__ inline float f0_group_smallest(float v) {
    float o = __uint_as_float(f0_dpp_quad_1032(__float_as_uint(v)));
    v = o < v ? o : v;
    o = __uint_as_float(f0_dpp_quad_2301(__float_as_uint(v)));
    v = o < v ? o : v;
    o = __uint_as_float(f0_dpp_half_mirror(__float_as_uint(v)));
    return o < v ? o : v;
}

__global__ __launch_bounds__(64) void f0_decode_kernel(DecodeArgs p) {
    __shared__ unsigned back[F0_DECODE_MAX_FRAMES];        // per frame 8 x 3 bits of back pointers; later the frame's state
    const int b = blockIdx.x, lane = threadIdx.x, i = lane & 7, j = lane >> 3;
    const int T = min(max(p.n_frames[b], 0), p.max_frames);
    if (T == 0) return;
    const long long base = (long long)b * p.max_frames * F0_SLOTS;
    const float *per = p.period + base, *cst = p.cost + base, *dpr = p.dprime + base;
    auto load = [&](int t) {
        const int tt = min(t, T - 1) * F0_SLOTS;            // (frames behind the end are loaded again and not used)
        return DecodeFrame{per[tt + i], cst[tt + i], per[tt + j], cst[tt + j]};
    };

    // frame 0: delta[i] = loc[i]
    DecodeFrame fr = load(0);
    float prev_p = fr.pi;
    const bool i_unvoiced = i == F0_SLOTS - 1, j_unvoiced = j == F0_SLOTS - 1, both_voiced = !i_unvoiced & !j_unvoiced;
    const float tr_fixed = i == j ? 0.f : p.w_switch;       // of the transitions that touch the unvoiced state
    bool prev_avail = f0_slot_available(i_unvoiced, fr.pi, fr.ci);
    float delta = f0_cost_ok(fr.ci) ? fr.ci : 0.f;

    DecodeFrame cur[F0_DECODE_AHEAD], nxt[F0_DECODE_AHEAD];
#pragma unroll
    for (int u = 0; u < F0_DECODE_AHEAD; ++u) cur[u] = load(1 + u);
    for (int t0 = 1; t0 < T; t0 += F0_DECODE_AHEAD) {
#pragma unroll
        for (int u = 0; u < F0_DECODE_AHEAD; ++u) nxt[u] = load(t0 + F0_DECODE_AHEAD + u);
#pragma unroll
        for (int u = 0; u < F0_DECODE_AHEAD; ++u) {
            const int t = t0 + u;
            if (t < T) {
                fr = cur[u];
                const bool avail_j = f0_slot_available(j_unvoiced, fr.pj, fr.cj);
                const float loc_j = f0_cost_ok(fr.cj) ? fr.cj : 0.f;
                const float jump = p.w_jump * (fabsf(fr.pj - prev_p) / (fr.pj + prev_p));
                const float tr = both_voiced ? jump : tr_fixed;
                const float v = (prev_avail & avail_j) ? delta + tr : INFINITY;   // (an unavailable end: tr may be anything)
                const float best = f0_group_smallest(v);
                const float nw = avail_j ? best + loc_j : INFINITY;
                // this lane's new[i] comes from group i (one ds_bpermute: the crossbar, no LDS memory); the group then
                // holds new[0 .. 7], and their minimum is the frame's m
                const float ni = __int_as_float(__builtin_amdgcn_ds_bpermute(32 * i, __float_as_int(nw)));
                delta = ni - f0_group_smallest(ni);
                // off the chain: the smallest i that has the minimum, from the wave's equality mask
                const unsigned long long hit = __ballot(v == best);
                const int arg = __ffs((unsigned)(hit >> (8 * j)) & 0xffu) - 1;
                prev_avail = f0_slot_available(i_unvoiced, fr.pi, fr.ci);
                prev_p = fr.pi;
                // the frame's back pointers, 3 bits per j, gathered over the eight groups
                typedef unsigned f0_pair __attribute__((ext_vector_type(2)));
                unsigned w = avail_j ? (unsigned)arg << (3 * j) : 0u;                                      // (arg is in 0 .. 7)
                w |= __builtin_amdgcn_update_dpp(0u, w, 0x128, 0xf, 0xf, true);                            // row_ror:8
                f0_pair r = __builtin_amdgcn_permlane16_swap(w, w, false, false);
                w = r[0] | r[1];
                r = __builtin_amdgcn_permlane32_swap(w, w, false, false);
                w = r[0] | r[1];
                if (lane == 0) back[t] = w;
            }
        }
#pragma unroll
        for (int u = 0; u < F0_DECODE_AHEAD; ++u) cur[u] = nxt[u];
    }

    // the last state: the smallest index of the minimum of delta (lanes 0 .. 7 hold delta[i])
    float v = prev_avail ? delta : INFINITY;
    int arg = i;
    f0_group_min(v, arg);
    if (lane == 0) {                                        // the walk back: one LDS read and one write per frame
        int s = arg;
        for (int t = T - 1; t >= 1; --t) {
            const unsigned w = back[t];
            back[t] = (unsigned)s;
            s = (int)((w >> (3 * s)) & 7u);
        }
        back[0] = (unsigned)s;
    }
    __syncthreads();
    const float sr = (float)p.sample_rate;
    for (int t = lane; t < T; t += 64) {
        const int s = (int)back[t];
        const long long o = (long long)b * p.max_frames + t;
        p.f0[o] = s < F0_SLOTS - 1 ? sr / per[t * F0_SLOTS + s] : 0.f;
        p.periodicity[o] = dpr[t * F0_SLOTS + s];
    }
}

const char *check_decode_f0(const DecodeArgs &a) {
    if (!a.period || !a.cost || !a.dprime || !a.n_frames || !a.f0 || !a.periodicity) return "null pointer";
    if (a.max_frames < 1) return "max_frames must be at least 1";
    if (a.max_frames > F0_DECODE_MAX_FRAMES) return "max_frames must be at most 16000 (the back pointers stay in LDS)";
    if (a.batch < 0) return "batch must not be negative";
    if (a.batch > 65535) return "batch must be at most 65535";
    if (!(a.w_jump >= 0.f && a.w_jump <= F0_COST_LIMIT)) return "w_jump must be in [0, 1e6]";
    if (!(a.w_switch >= 0.f && a.w_switch <= F0_COST_LIMIT)) return "w_switch must be in [0, 1e6]";
    if (a.sample_rate < 1) return "sample_rate must be at least 1";
    return nullptr;
}

void launch_decode_f0(const DecodeArgs &a, hipStream_t stream) {
    if (a.batch == 0) return;
    hipLaunchKernelGGL(f0_decode_kernel, dim3(a.batch), dim3(64), 0, stream, a);
}

}  // namespace mbx
