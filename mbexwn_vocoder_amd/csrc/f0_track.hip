// F0 of every analysis frame from the audio: a YIN-type tracker (include/mbexwn_pitch.h: mbxp_track_f0; DESIGN.md section
// 6h; the host definition is mbexwn_vocoder_amd/f0track.py::track_f0_host).
//
//   y[i]   = x[c - L/2 + i], 0 outside the item            L = W + tau_max, c = centres[b][k] clamped to [0, n_b]
//   d[tau] = sum_j (y[s + j] - y[s + tau + j])^2           s = (tau_max - tau) >> 1, 0 <= j < W, 1 <= tau <= tau_max
//   d'[tau] = d[tau] tau / (d[1] + .. + d[tau])            the cumulative-mean-normalised difference function
//   pick   = first tau in [lo, hi] with d' < thr, walked down to its local minimum, refined by a parabola
//
// One 256-thread block per (frame, item).  The frame's L samples sit in LDS; each of the four waves takes every fourth pair
// of lags with a common s (so the first window is read once for two lags): lane l sums the W / 64 terms j = l + 64 k in
// order, and the wave adds the 64 partial sums in the order of the definition's halving tree with lane swaps and DPP, not
// through LDS (float addition commutes, so which partner is the left operand does not matter; lane 0 ends with the tree's
// value).  The running sum of d is one thread's sequential chain (it is the definition's order); the division and the two
// searches are parallel again.
// LDS-type: 1.5 four-byte LDS reads and 3 float operations per term, W tau_max terms per frame.  No MFMA.
//
// Host and device must give the same bits: every operation below is one separately rounded IEEE float32 operation -- plain
// operators with contraction switched off for this file (no fused multiply-add: numpy has none), the division the compiler's
// correctly rounded one.
#include <climits>
#include <cmath>

#include "mbx_kernels.h"

#pragma clang fp contract(off)

namespace mbx {

constexpr int F0_THREADS = 256;
constexpr int F0_WAVES = F0_THREADS / 64;
// a sample that is not finite, or so large that the sums below could overflow, makes its frame unvoiced (f0track.SAMPLE_LIMIT)
constexpr float F0_SAMPLE_LIMIT = 1e15f;

// the definition's lane sum from 64 partial sums: after the step with m, lane l < m holds a[l] + a[l + m] (the other lanes
// hold sums nobody reads).  All in the vector ALU: the two halves of the wave, then the rows of 16 lanes, meet through
// gfx950's lane swaps (v_permlane32_swap, v_permlane16_swap: with both operands the same register, one result holds the lower
// partner and the other the upper one on every lane); inside a row lane l reads lane l + m by DPP (row_shl).  The whole wave
// must be active.
__device__ inline float f0_lane_sum(float a) {
    typedef unsigned f0_pair __attribute__((ext_vector_type(2)));
    f0_pair r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(a), false, false);
    a = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(a), false, false);
    a = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    a = a + __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(a), 0x108, 0xf, 0xf, true));   // row_shl:8
    a = a + __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(a), 0x104, 0xf, 0xf, true));   // row_shl:4
    a = a + __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(a), 0x102, 0xf, 0xf, true));   // row_shl:2
    a = a + __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(a), 0x101, 0xf, 0xf, true));   // row_shl:1
    return a;
}

__global__ __launch_bounds__(F0_THREADS) void f0_track_kernel(PitchArgs p) {
    extern __shared__ __attribute__((aligned(16))) float f0_smem[];
    __shared__ float s_energy;
    const int k = blockIdx.x, b = blockIdx.y;
    if (k >= p.n_frames[b]) return;
    const int W = p.window, TM = p.tau_max, L = W + TM;
    float *y = f0_smem;                                     // (L) the frame; later (TM + 1) the running sums of d
    float *d = f0_smem + L;                                 // (TM + 1) d, then d'
    // length and centre from the device arrays, clamped to the item's row: a wrong entry must not address outside the buffer
    const long long n = min(max((long long)p.n_samples[b], 0LL), p.stride);
    const long long c = min(max(p.centres[(long long)b * p.max_frames + k], 0LL), n);
    const float *xb = p.audio + (long long)b * p.stride;
    const long long first = c - (L >> 1);
    int bad = 0;
    for (int i = threadIdx.x; i < L; i += F0_THREADS) {
        const long long s = first + i;
        const float v = (s >= 0 && s < n) ? xb[s] : 0.f;
        if (!(fabsf(v) <= F0_SAMPLE_LIMIT)) bad = 1;
        y[i] = v;
    }
    bad = __syncthreads_or(bad);

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int terms = W >> 6;
    // two lags per turn: tau_max - 2 j - 1 and tau_max - 2 j share s = j, hence the first window, which is read once for both
    // (tau = 0, the partner of tau = 1 when tau_max is odd, is computed and dropped: its second window is the first)
    for (int j = wave; 2 * j < TM; j += F0_WAVES) {
        const int tau = TM - 2 * j;                         // (the highest index is j + tau + W - 1 <= TM + W - 1 = L - 1)
        const float *u = y + j + lane, *v = u + tau;
        float x0 = u[0];
        float e1 = x0 - v[0], e0 = x0 - v[-1];
        float a1 = e1 * e1, a0 = e0 * e0;
        for (int kk = 1; kk < terms; ++kk) {
            x0 = u[64 * kk];
            e1 = x0 - v[64 * kk];
            e0 = x0 - v[64 * kk - 1];
            const float q1 = e1 * e1, q0 = e0 * e0;
            a1 = a1 + q1;
            a0 = a0 + q0;
        }
        a1 = f0_lane_sum(a1);
        a0 = f0_lane_sum(a0);
        if (lane == 0) {
            d[tau] = a1;
            if (tau > 1) d[tau - 1] = a0;
        }
    }
    if (wave == F0_WAVES - 1) {                             // the energy of the W samples about the centre
        const float *u = y + (TM >> 1) + lane;
        float a = u[0] * u[0];
        for (int kk = 1; kk < terms; ++kk) {
            const float q = u[64 * kk] * u[64 * kk];
            a = a + q;
        }
        a = f0_lane_sum(a);
        if (lane == 0) s_energy = a;
    }
    __syncthreads();                                        // the frame is no longer read: its space takes the running sums

    float *cs = y;
    if (threadIdx.x == 0) {
        float run = 0.f;
        d[0] = 1.f;
        for (int tau = 1; tau <= TM; ++tau) {
            run = run + d[tau];
            cs[tau] = run;
        }
    }
    __syncthreads();
    for (int tau = 1 + threadIdx.x; tau <= TM; tau += F0_THREADS) {
        const float ct = cs[tau];
        const float num = d[tau] * (float)tau;
        d[tau] = ct > 0.f ? num / ct : 1.f;
    }
    __syncthreads();
    if (wave != 0) return;

    // the first lag below the threshold, and the first lag of the minimum, over [lo, hi]: per lane, then over the wave
    const int lo = max(p.tau_min, 2), hi = TM - 1;
    int pick = INT_MAX, best = INT_MAX;
    float best_v = INFINITY;
    for (int tau = lo + lane; tau <= hi; tau += 64) {
        const float v = d[tau];
        if (v < p.threshold && pick == INT_MAX) pick = tau;
        if (v < best_v) {
            best_v = v;
            best = tau;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        pick = min(pick, __shfl_xor(pick, m, 64));
        const float ov = __shfl_xor(best_v, m, 64);
        const int oi = __shfl_xor(best, m, 64);
        if (ov < best_v || (ov == best_v && oi < best)) {
            best_v = ov;
            best = oi;
        }
    }
    if (lane != 0) return;
    float f0 = 0.f, per;
    if (pick == INT_MAX) {
        per = best == INT_MAX ? d[lo] : best_v;
    } else {
        int tau = pick;
        while (tau + 1 <= hi && d[tau + 1] < d[tau]) ++tau;
        per = d[tau];
        if (s_energy >= p.e_min) {
            const float a = d[tau - 1], bb = d[tau], g = d[tau + 1];
            const float den = (a - bb) + (g - bb);
            float off = 0.f;
            if (den > 0.f) {
                off = ((a - g) / den) * 0.5f;
                off = fminf(fmaxf(off, -1.f), 1.f);
            }
            f0 = (float)p.sample_rate / ((float)tau + off);
        }
    }
    if (bad) {
        f0 = 0.f;
        per = 1.f;
    }
    const long long o = (long long)b * p.max_frames + k;
    p.f0[o] = f0;
    p.periodicity[o] = per;
}

const char *check_track_f0(const PitchArgs &a) {
    if (!a.audio || !a.n_samples || !a.centres || !a.n_frames || !a.f0 || !a.periodicity) return "null pointer";
    if (a.sample_rate < 1) return "sample_rate must be at least 1";
    if (a.window < 64 || a.window > 2048 || a.window % 64 != 0) return "window must be a multiple of 64 in 64 .. 2048";
    if (a.tau_max < 2) return "tau_max must be at least 2";
    if (a.tau_min < 0) return "tau_min must not be negative";
    if (std::max(a.tau_min, 2) > a.tau_max - 1) return "max(tau_min, 2) must be at most tau_max - 1";
    if ((long long)a.window + a.tau_max > 4096) return "window + tau_max must be at most 4096 (the frame stays in LDS)";
    if (!(a.threshold == a.threshold) || !(a.e_min == a.e_min)) return "threshold and e_min must be numbers";
    if (a.max_frames < 1) return "max_frames must be at least 1";
    if (a.stride < 1) return "stride must be at least 1";
    if (a.batch < 0) return "batch must not be negative";
    if (a.batch > 65535) return "batch is larger than 65535, the y extent of a grid";
    return nullptr;
}

void launch_track_f0(const PitchArgs &a, hipStream_t stream) {
    if (a.batch == 0) return;
    const size_t smem = (size_t)(a.window + 2 * a.tau_max + 1) * sizeof(float);
    hipLaunchKernelGGL(f0_track_kernel, dim3(a.max_frames, a.batch), dim3(F0_THREADS), smem, stream, a);
}

}  // namespace mbx
