// The decoded F0 contour of sounds that are still arriving (include/mbexwn_live_contour.h: mbxv_f0_candidate_frames,
// mbxv_decode_f0_frames; the host definition is mbexwn_vocoder_amd/f0decode.py::candidates_host,
// ::viterbi_lag_host and ::LagDecoder).
//
// f0_stream_candidates_kernel: one 256-thread block per (stream, new frame).  It is f0_stream_kernel (f0_stream.hip) with
// another end: the same ring fetch (F0RingFetch), the same frame code up to d' (f0_frame.h), then f0_frame_candidates, the
// function the offline f0_candidates_kernel ends in -- so a frame carries the bits mbxc_f0_candidates gives at centre t * hop
// on the stream's whole sound.
//
// f0_lag_decode_kernel: one 64-lane wave per row of the descriptor table, lane 8 j + i owning the transition i -> j and the
// forward step that of f0_decode_kernel (f0_viterbi.h).  A stream's state row holds the counters, delta and the last
// frame's periods and costs in 32 words, then a ring of 256 frames: per frame one word (eight 3-bit back pointers and, from
// bit 24, the frame's best state), 8 periods and 8 dprimes.  The wave stages the last `lag` frames of the ring in LDS, then
// works in sub-chunks of at most 64 frames: the tables of the sub-chunk go to LDS (periods and dprimes straight into their
// ring places), the forward steps run, and then the lanes walk back in parallel, one output frame per lane: frame t starts
// from the best state of frame min(t + lag, done - 1) and follows at most `lag` pointers.  With lag <= 128 a walk reaches at
// most 128 + 64 frames back from the newest, which the ring of 256 holds.  At the end the ring places of the new frames and
// the 32 head words go back to the state row.  Every loop runs to a clamped count and the wave waits on nobody: a
// descriptor or a state row with wrong entries gives wrong values, never an access outside the buffers (`decided` is
// clamped to [done - lag, done], so a call writes at most n + lag outputs).
//
// A stream must appear in at most ONE row of a launch: two waves on one state row would race.
//
// Host and device must give the same bits: the two headers switch contraction off, and it stays off for this file.
#include <algorithm>
#include <climits>
#include <cmath>

#include "f0_frame.h"
#include "f0_viterbi.h"
#include "mbx_kernels.h"

#pragma clang fp contract(off)

namespace mbx {

static_assert((F0_LAG_RING & (F0_LAG_RING - 1)) == 0 && F0_LAG_RING >= F0_MAX_LAG + 1 + F0_LAG_CHUNK, "the ring holds a walk");

__global__ __launch_bounds__(F0_THREADS) void f0_stream_candidates_kernel(CandidateStreamArgs p) {
    extern __shared__ __attribute__((aligned(16))) float f0_smem[];
    __shared__ float s_energy;
    const PitchStreamArgs &f = p.ring;
    const StreamRow row{f.desc + 4LL * blockIdx.y};
    if (!row.has_frame(blockIdx.x, f.rings)) return;
    const long long n_total = row.n_total();
    const int W = f.window, TM = f.tau_max, L = W + TM;
    long long c = (row.first() + blockIdx.x) * f.hop;
    if (n_total >= 0) c = min(c, n_total);
    const int bad = f0_frame_load(F0RingFetch(f.rings.row(row.slot()), f.rings.ring_samples, n_total, c, L), L, f0_smem);
    f0_frame_dprime(W, TM, f0_smem, &s_energy);
    if (threadIdx.x >= 64) return;
    f0_frame_candidates(f0_smem + L, f.tau_min, TM, bad, s_energy, f.e_min, p.thresholds, p.weights, p.n_thresholds, p.n_cand,
                        ((long long)blockIdx.y * f.max_new_frames + blockIdx.x) * F0_SLOTS, p.period, p.cost, p.dprime);
}

const char *fill_f0_stream_candidates(CandidateStreamArgs &a, const float *thresholds, const float *weights) {
    if (!a.period || !a.cost || !a.dprime || !thresholds || !weights) return "NULL pointer";
    PitchStreamArgs f = a.ring;                             // the streaming tracker's checks of the arguments the two share
    f.threshold = 0.f;
    f.f0 = a.period;
    f.periodicity = a.cost;
    if (const char *why = check_f0_stream(f)) return why;
    return fill_f0_rule(a.thresholds, a.weights, a.n_thresholds, a.n_cand, thresholds, weights);
}

void launch_f0_stream_candidates(const CandidateStreamArgs &a, hipStream_t stream) {
    if (a.ring.n_streams == 0 || a.ring.max_new_frames == 0) return;
    const size_t smem = (size_t)(a.ring.window + 2 * a.ring.tau_max + 1) * sizeof(float);
    hipLaunchKernelGGL(f0_stream_candidates_kernel, dim3(a.ring.max_new_frames, a.ring.n_streams), dim3(F0_THREADS), smem,
                       stream, a);
}

// ------------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(64) void f0_lag_decode_kernel(LagDecodeArgs p) {
    __shared__ unsigned s_word[F0_LAG_RING];                // the ring, by frame & 255: pointers and best state
    __shared__ float s_per[F0_LAG_RING * F0_SLOTS], s_dpr[F0_LAG_RING * F0_SLOTS];
    __shared__ float s_cst[F0_LAG_CHUNK * F0_SLOTS];        // the costs of a sub-chunk
    constexpr int MASK = F0_LAG_RING - 1;
    const int r = blockIdx.x, lane = threadIdx.x;
    const StreamRow row{p.desc + 4LL * r};
    const long long slot = row.slot(), first = row.first(), n_total = row.n_total();
    if (slot < 0 || slot >= p.n_slots || first < 0 || first > (long long)INT_MAX - p.max_new_frames) return;
    unsigned *st = p.state + slot * F0_LAG_STATE_WORDS;
    if ((long long)(int)st[0] != first) return;             // not the stream's next frame: nothing is touched
    const int n = (int)min(max(row.n(), 0LL), (long long)p.max_new_frames), lag = p.lag;
    const bool closing = n_total >= 0 && first + n >= n_total / p.hop + 1;
    int done = (int)first;
    int decided = min(max((int)st[1], max(done - lag, 0)), done);
    const int decided0 = decided;
    unsigned *g_word = st + F0_LAG_HEAD;
    float *g_per = reinterpret_cast<float *>(g_word + F0_LAG_RING), *g_dpr = g_per + F0_LAG_RING * F0_SLOTS;

    // the frames a walk of this call may still read: the last min(done, lag)
    const int keep = min(done, lag);
    for (int q = lane; q < keep; q += 64) {
        const int sl = (done - keep + q) & MASK;
        s_word[sl] = g_word[sl];
    }
    for (int q = lane; q < keep * F0_SLOTS; q += 64) {
        const int sl = ((done - keep + (q >> 3)) & MASK) * F0_SLOTS + (q & 7);
        s_per[sl] = g_per[sl];
        s_dpr[sl] = g_dpr[sl];
    }
    const ViterbiLane ln(lane, p.w_jump, p.w_switch);
    const int i = ln.i, j = ln.j;
    float delta = __uint_as_float(st[2 + i]), prev_p = __uint_as_float(st[2 + F0_SLOTS + i]);
    float prev_c = __uint_as_float(st[2 + 2 * F0_SLOTS + i]);
    bool prev_avail = f0_slot_available(ln.i_unvoiced, prev_p, prev_c);

    const long long base = (long long)r * p.max_new_frames * F0_SLOTS;
    const float *per = p.period + base, *cst = p.cost + base, *dpr = p.dprime + base;
    const float sr = (float)p.sample_rate;
    int off = 0;
    do {
        const int m = min(F0_LAG_CHUNK, n - off);
        __syncthreads();                                    // the walk of the sub-chunk before has read the ring
        for (int q = lane; q < m * F0_SLOTS; q += 64) {
            const int sl = ((done + (q >> 3)) & MASK) * F0_SLOTS + (q & 7);
            s_per[sl] = per[off * F0_SLOTS + q];
            s_dpr[sl] = dpr[off * F0_SLOTS + q];
            s_cst[q] = cst[off * F0_SLOTS + q];
        }
        __syncthreads();
        for (int u = 0; u < m; ++u) {
            const int sl = ((done + u) & MASK) * F0_SLOTS;
            const DecodeFrame fr{s_per[sl + i], s_cst[u * F0_SLOTS + i], s_per[sl + j], s_cst[u * F0_SLOTS + j]};
            unsigned w = 0u;
            if (done + u == 0) {                            // (the whole wave) frame 0: delta[i] = loc[i]
                prev_avail = f0_slot_available(ln.i_unvoiced, fr.pi, fr.ci);
                const float loc = f0_cost_ok(fr.ci) ? fr.ci : 0.f;
                delta = prev_avail ? loc : INFINITY;
                prev_p = fr.pi;
            } else {
                w = f0_viterbi_step(fr, ln, delta, prev_p, prev_avail);
            }
            prev_c = fr.ci;
            const int best = f0_best_state(delta, prev_avail, i);
            if (lane == 0) s_word[(done + u) & MASK] = w | (unsigned)best << 24;
        }
        done += m;
        off += m;
        __syncthreads();
        // one decided frame per lane: from the best state of frame min(t + lag, done - 1) back to frame t
        const int target = (closing && off >= n) ? done : max(done - lag, 0);
        for (int t = decided + lane; t < target; t += 64) {
            const int e = min(t + lag, done - 1);
            int s = (int)(s_word[e & MASK] >> 24) & 7;
            for (int u = e; u > t; --u) s = (int)(s_word[u & MASK] >> (3 * s)) & 7;
            const int sl = (t & MASK) * F0_SLOTS + s;
            const long long o = (long long)r * p.max_out + (t - decided0);
            p.f0[o] = s < F0_SLOTS - 1 ? sr / s_per[sl] : 0.f;
            p.periodicity[o] = s_dpr[sl];
        }
        decided = max(decided, target);
    } while (off < n);

    // the state row: the ring places of the frames of this call, then the head
    __syncthreads();
    const int fresh = min(n, F0_LAG_RING);
    for (int q = lane; q < fresh; q += 64) {
        const int sl = (done - fresh + q) & MASK;
        g_word[sl] = s_word[sl];
    }
    for (int q = lane; q < fresh * F0_SLOTS; q += 64) {
        const int sl = ((done - fresh + (q >> 3)) & MASK) * F0_SLOTS + (q & 7);
        g_per[sl] = s_per[sl];
        g_dpr[sl] = s_dpr[sl];
    }
    if (lane < F0_SLOTS) {                                  // lanes 0 .. 7 hold slot i = lane
        st[2 + lane] = __float_as_uint(delta);
        st[2 + F0_SLOTS + lane] = __float_as_uint(prev_p);
        st[2 + 2 * F0_SLOTS + lane] = __float_as_uint(prev_c);
    }
    if (lane == 0) {
        st[0] = (unsigned)done;
        st[1] = (unsigned)decided;
    }
}

const char *check_lag_decode(const LagDecodeArgs &a) {
    if (!a.period || !a.cost || !a.dprime || !a.desc || !a.state || !a.f0 || !a.periodicity) return "NULL pointer";
    if (!row_count_fits(a.n_streams)) return "n_streams must lie in [0, 65535]";
    if (a.max_new_frames < 0) return "max_new_frames must not be negative";
    if (a.hop < 1) return "hop must be at least 1";
    if (a.n_slots < 1) return "n_slots must be at least 1";
    if (a.lag < 0 || a.lag > F0_MAX_LAG) return "lag must be in 0 .. 128";
    if ((long long)a.max_out < (long long)a.max_new_frames + a.lag) return "max_out must be at least max_new_frames + lag";
    if (!(a.w_jump >= 0.f && a.w_jump <= F0_COST_LIMIT)) return "w_jump must be in [0, 1e6]";
    if (!(a.w_switch >= 0.f && a.w_switch <= F0_COST_LIMIT)) return "w_switch must be in [0, 1e6]";
    if (a.sample_rate < 1) return "sample_rate must be at least 1";
    return nullptr;
}

void launch_lag_decode(const LagDecodeArgs &a, hipStream_t stream) {
    if (a.n_streams == 0) return;
    hipLaunchKernelGGL(f0_lag_decode_kernel, dim3(a.n_streams), dim3(64), 0, stream, a);
}

}  // namespace mbx
