// F0 of every analysis frame from the audio: a YIN-type tracker (include/mbexwn_pitch.h: mbxp_track_f0; DESIGN.md section
// 6h; the host definition is mbexwn_vocoder_amd/f0track.py::track_f0_host).
//
//   y[i]   = x[c - L/2 + i], 0 outside the item            L = W + tau_max, c = centres[b][k] clamped to [0, n_b]
//   d[tau] = sum_j (y[s + j] - y[s + tau + j])^2           s = (tau_max - tau) >> 1, 0 <= j < W, 1 <= tau <= tau_max
//   d'[tau] = d[tau] tau / (d[1] + .. + d[tau])            the cumulative-mean-normalised difference function
//   pick   = first tau in [lo, hi] with d' < thr, walked down to its local minimum, refined by a parabola
//
// One 256-thread block per (frame, item).  Everything is f0_frame.h's: the load of the frame with the row's fetch, d'
// (f0_frame_dprime, which the candidates kernel of f0_decode.hip calls too) and the pick (f0_frame_pick); the streaming
// tracker of f0_stream.hip runs the same two functions behind a fetch from its ring.
// The frame's L samples sit in LDS; each of the four waves takes every fourth pair of lags with a common s (so the first window is read once for two lags): lane l sums the W / 64 terms j = l + 64 k in
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

#include "f0_frame.h"
#include "mbx_kernels.h"

#pragma clang fp contract(off)

namespace mbx {

__global__ __launch_bounds__(F0_THREADS) void f0_track_kernel(PitchArgs p) {
    extern __shared__ __attribute__((aligned(16))) float f0_smem[];
    __shared__ float s_energy;
    const int k = blockIdx.x, b = blockIdx.y;
    if (k >= p.n_frames[b]) return;
    const int W = p.window, TM = p.tau_max, L = W + TM;
    float *d = f0_smem + L;                                 // (TM + 1) d'; f0_frame.h has the layout
    // length and centre from the device arrays, clamped to the item's row: a wrong entry must not address outside the buffer
    const long long n = min(max((long long)p.n_samples[b], 0LL), p.stride);
    const long long c = min(max(p.centres[(long long)b * p.max_frames + k], 0LL), n);
    const int bad = f0_frame_load(F0RowFetch(p.audio + (long long)b * p.stride, n, c, L), L, f0_smem);
    f0_frame_dprime(W, TM, f0_smem, &s_energy);
    if (threadIdx.x >= 64) return;
    float f0, per;
    f0_frame_pick(d, p.tau_min, TM, p.threshold, p.e_min, s_energy, p.sample_rate, bad, f0, per);
    if (threadIdx.x != 0) return;
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
