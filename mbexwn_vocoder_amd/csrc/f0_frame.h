// The part the F0 tracker (f0_track.hip), its streaming form (f0_stream.hip) and the candidates kernels of the decoder
// (f0_decode.hip, and f0_lag.hip for streams) share: one 256-thread block loads a frame into LDS (f0_frame_load, with the
// kernel's own fetch: F0RowFetch or F0RingFetch) and leaves its cumulative-mean-normalised difference function d' there
// (f0_frame_dprime; the host definition is mbexwn_vocoder_amd/f0track.py::difference_host); the two
// trackers then share the pick (f0_frame_pick), the two candidates kernels the candidates (f0_frame_candidates).
//
//   y[i]   = x[c - L/2 + i], 0 outside the item            L = W + tau_max, c = centres[b][k] clamped to [0, n_b]
//   d[tau] = sum_j (y[s + j] - y[s + tau + j])^2           s = (tau_max - tau) >> 1, 0 <= j < W, 1 <= tau <= tau_max
//   d'[tau] = d[tau] tau / (d[1] + .. + d[tau])            1 where the running sum is not positive
//
// Host and device must give the same bits: every operation is one separately rounded IEEE float32 operation.  This header
// sets `#pragma clang fp contract(off)` itself, and it holds for the rest of a file that includes this header.
#pragma once

#include <climits>
#include <cmath>

#include <hip/hip_runtime.h>

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

// The load of a frame into LDS: y[i] = fetch(i) for 0 <= i < L, where fetch(i) is sample c - L/2 + i of the sound or 0 outside
// it -- the item's row (f0_track.hip, f0_decode.hip) or a stream's ring (f0_stream.hip, f0_lag.hip); only the fetch differs between
// them.  The whole block calls it.  Returns, on every thread, whether the frame touches a sample that is not finite or above
// F0_SAMPLE_LIMIT.  Ends behind a __syncthreads().
template <typename Fetch>
__device__ inline int f0_frame_load(Fetch fetch, int L, float *y) {
    int bad = 0;
    for (int i = threadIdx.x; i < L; i += F0_THREADS) {
        const float v = fetch(i);
        if (!(fabsf(v) <= F0_SAMPLE_LIMIT)) bad = 1;
        y[i] = v;
    }
    return __syncthreads_or(bad);
}

// the fetch of an item row `xb` of n samples for the frame centred on c
struct F0RowFetch {
    const float *xb;
    long long n, first;
    __device__ F0RowFetch(const float *xb_, long long n_, long long c, int L) : xb(xb_), n(n_), first(c - (L >> 1)) {}
    __device__ float operator()(int i) const {
        const long long s = first + i;
        return (s >= 0 && s < n) ? xb[s] : 0.f;
    }
};

// the fetch from a stream's ring (sample s at ring[s & (ring_samples - 1)]) for the frame centred on c; n_total < 0: the
// stream is still open and only the start is an edge.  "Outside" is decided from the index alone and never touches the ring
struct F0RingFetch {
    const float *ring;
    long long mask, n_total, first;
    __device__ F0RingFetch(const float *ring_, int ring_samples, long long n_total_, long long c, int L)
        : ring(ring_), mask(ring_samples - 1), n_total(n_total_), first(c - (L >> 1)) {}
    __device__ float operator()(int i) const {
        const long long s = first + i;
        if (s < 0 || (n_total >= 0 && s >= n_total)) return 0.f;
        return ring[s & mask];
    }
};

// Everything behind the load, through to d'.  The whole block calls it, behind f0_frame_load.  `smem` holds W + 2 TM + 1
// floats, the first L = W + TM of them the frame: on return smem + W + TM is d' (TM + 1 entries, d'[0] = 1) and the W + TM
// floats in front of it are free; *s_energy (one __shared__ float) is the energy of the W samples about the centre.  Ends
// behind a __syncthreads().
__device__ inline void f0_frame_dprime(int W, int TM, float *smem, float *s_energy) {
    const int L = W + TM;
    float *y = smem;                                        // (L) the frame; later (TM + 1) the running sums of d
    float *d = smem + L;                                    // (TM + 1) d, then d'

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
        if (lane == 0) *s_energy = a;
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
}

// f0track.pick_host's refinement of a lag tau in [2, tau_max - 1]: float(tau) plus the vertex of the parabola through
// d'[tau - 1 .. tau + 1], clamped to [-1, 1]
__device__ inline float f0_refined_lag(const float *d, int tau) {
    const float a = d[tau - 1], bb = d[tau], g = d[tau + 1];
    const float den = (a - bb) + (g - bb);
    float off = 0.f;
    if (den > 0.f) {
        off = ((a - g) / den) * 0.5f;
        off = fminf(fmaxf(off, -1.f), 1.f);
    }
    return (float)tau + off;
}

// f0track.pick_host on the d' of a frame: the first lag in [max(tau_min, 2), TM - 1] below the threshold, walked on to its
// local minimum and refined.  ONE whole wave calls it (every lane active) behind f0_frame_dprime; the results are valid on
// lane 0.  `bad`: the frame touches a sample that is not finite -- unvoiced with periodicity 1.
__device__ inline void f0_frame_pick(const float *d, int tau_min, int TM, float threshold, float e_min, float energy,
                                     int sample_rate, int bad, float &f0, float &per) {
    const int lane = threadIdx.x & 63;
    // the first lag below the threshold, and the first lag of the minimum, over [lo, hi]: per lane, then over the wave
    const int lo = max(tau_min, 2), hi = TM - 1;
    int pick = INT_MAX, best = INT_MAX;
    float best_v = INFINITY;
    for (int tau = lo + lane; tau <= hi; tau += 64) {
        const float v = d[tau];
        if (v < threshold && pick == INT_MAX) pick = tau;
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
    f0 = 0.f;
    per = 1.f;
    if (lane != 0) return;
    if (pick == INT_MAX) {
        per = best == INT_MAX ? d[lo] : best_v;
    } else {
        int tau = pick;
        while (tau + 1 <= hi && d[tau + 1] < d[tau]) ++tau;
        per = d[tau];
        if (energy >= e_min) {
            f0 = (float)sample_rate / f0_refined_lag(d, tau);
        }
    }
    if (bad) {
        f0 = 0.f;
        per = 1.f;
    }
}

// f0decode.py::candidates_host on the d' of a frame: per threshold the tracker's pick, the weight sums
// per distinct lag, the n_cand heaviest lags by ascending lag in slots 0 .. 6 and "unvoiced" in slot 7, written to the three
// tables at out .. out + 7.  ONE whole wave calls it (every lane active) behind f0_frame_dprime: every lane scans its lags
// once and keeps, for each of the up to 16 ascending thresholds, the first lag below it; 16 first-index reductions over the
// wave; lane n < N walks pick_n on to its local minimum; the weight sums P (per distinct lag, in ascending n) and U (no
// pick), the ranks by counting, and lanes 0 .. 7 write the eight slots.  Thresholds from n_thresholds on are -inf.  The
// offline kernel (f0_decode.hip) and the streaming one (f0_lag.hip) both end in it: same d', same bits.
__device__ inline void f0_frame_candidates(const float *d, int tau_min, int TM, int bad, float energy, float e_min,
                                           const float (&thresholds)[F0_MAX_THRESHOLDS], const float (&weights)[F0_MAX_THRESHOLDS],
                                           int n_thresholds, int n_cand, long long out, float *period_out, float *cost_out,
                                           float *dprime_out) {
    const int lane = threadIdx.x & 63;
    // per threshold the first lag below it, and the first lag of the minimum, over [lo, hi]: per lane, then over the wave
    // (thresholds from n_thresholds on are -inf: nothing is below them)
    const int lo = max(tau_min, 2), hi = TM - 1, N = n_thresholds;
    int first[F0_MAX_THRESHOLDS];
#pragma unroll
    for (int nn = 0; nn < F0_MAX_THRESHOLDS; ++nn) first[nn] = INT_MAX;
    int best = INT_MAX;
    float best_v = INFINITY;
    for (int tau = lo + lane; tau <= hi; tau += 64) {
        const float v = d[tau];
#pragma unroll
        for (int nn = 0; nn < F0_MAX_THRESHOLDS; ++nn)
            if (v < thresholds[nn] && first[nn] == INT_MAX) first[nn] = tau;
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
    const bool usable = !bad && energy >= e_min;
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
        const float wm = weights[m];
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
    const int keep = leader && rank < n_cand;
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
    const long long o = out + lane;
    period_out[o] = period;
    cost_out[o] = cost;
    dprime_out[o] = dprime;
}

}  // namespace mbx
