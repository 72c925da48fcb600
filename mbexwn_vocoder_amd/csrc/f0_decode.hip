// A decoded F0 contour: Viterbi over YIN candidates (include/mbexwn_contour.h: mbxc_f0_candidates, mbxc_decode_f0; DESIGN.md
// section 6i; the host definition is mbexwn_vocoder_amd/f0decode.py::candidates_host and ::viterbi_host).
//
// f0_candidates_kernel: one 256-thread block per (frame, item).  Up to d' it is the tracker's frame (f0_frame.h).  Then wave
// 0 alone (f0_frame_candidates of f0_frame.h, which the streaming kernel of f0_lag.hip ends in too): every lane scans its
// lags once and keeps, for each of the up to 16 ascending thresholds, the first lag below it;
// 16 first-index reductions over the wave; lane n < N walks pick_n on to its local minimum; the weight sums P (per distinct
// lag, in ascending n) and U (no pick), the ranks by counting, and lanes 0 .. 7 write the eight slots.
//
// f0_decode_kernel: one 64-lane wave per item.  Lane 8 j + i owns the transition i -> j.  The step is f0_viterbi_step of
// f0_viterbi.h, shared with the fixed-lag kernel of f0_lag.hip.  The chain of a step is: v =
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
#include "f0_viterbi.h"
#include "mbx_kernels.h"

#pragma clang fp contract(off)

namespace mbx {

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
    if (threadIdx.x >= 64) return;
    f0_frame_candidates(d, f.tau_min, TM, bad, s_energy, f.e_min, p.thresholds, p.weights, p.n_thresholds, p.n_cand,
                        ((long long)b * f.max_frames + k) * F0_SLOTS, p.period, p.cost, p.dprime);
}

const char *fill_f0_candidates(CandidateArgs &a, const float *thresholds, const float *weights) {
    if (!a.period || !a.cost || !a.dprime || !thresholds || !weights) return "null pointer";
    PitchArgs f = a.frame;                                  // the tracker's checks of the arguments the two share
    f.threshold = 0.f;
    f.f0 = a.period;
    f.periodicity = a.cost;
    if (const char *why = check_track_f0(f)) return why;
    return fill_f0_rule(a.thresholds, a.weights, a.n_thresholds, a.n_cand, thresholds, weights);
}

const char *fill_f0_rule(float *th, float *ww, int n_thresholds, int n_cand, const float *thresholds, const float *weights) {
    if (n_thresholds < 1 || n_thresholds > F0_MAX_THRESHOLDS) return "n_thresholds must be in 1 .. 16";
    if (n_cand < 1 || n_cand > F0_SLOTS - 1) return "n_cand must be in 1 .. 7";
    for (int nn = 0; nn < F0_MAX_THRESHOLDS; ++nn) {
        th[nn] = -INFINITY;
        ww[nn] = 0.f;
    }
    for (int nn = 0; nn < n_thresholds; ++nn) {
        if (!std::isfinite(thresholds[nn])) return "the thresholds must be finite";
        if (nn > 0 && !(thresholds[nn] > thresholds[nn - 1])) return "the thresholds must be strictly ascending";
        if (!std::isfinite(weights[nn]) || weights[nn] < 0.f) return "the weights must be finite and not negative";
        th[nn] = thresholds[nn];
        ww[nn] = weights[nn];
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
    const ViterbiLane ln(lane, p.w_jump, p.w_switch);
    bool prev_avail = f0_slot_available(ln.i_unvoiced, fr.pi, fr.ci);
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
                const unsigned w = f0_viterbi_step(fr, ln, delta, prev_p, prev_avail);
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
