// Align a recording's timing to a guide: DTW over log-mel frames (include/mbexwn_align.h: mbxg_local_cost, mbxg_align_path;
// DESIGN.md section 6k; the host definition is mbexwn_vocoder_amd/align.py::local_cost_host and ::path_host).
//
// align_cost_kernel: one 64-lane wave per (chunk of 64 band cells, guide row, item).  The up to 64 source rows of the chunk
// are one contiguous span of memory: the wave copies it, coalesced, into LDS rows of M | 1 floats (an odd stride: the 64
// lanes, each on a row of its own, read 64 different banks), and the guide row beside it.  Lane l then owns cell l: the
// mean of its source row, the mean of the guide row (every lane, from broadcast reads) and the cost, each with THE SUM of
// align.py -- four interleaved partial sums in ascending m, combined (s0 + s1) + (s2 + s3) -- which a lane executes as it
// stands.  Bandwidth-type work: M loads per cell from L2, everything else in LDS.
//
// align_path_kernel: one block per item, one thread per band cell (2 W + 1 <= 1024).  Rows i - 1 and i - 2 of D live in LDS
// (three rotating rows, so that ONE barrier per guide row is enough: row i writes the buffer row i - 3 used, which nobody
// reads any more; each row has an unreachable cell at either end, so that the three reads of a cell need no branch).  The row chain is latency bound -- its cost is the number of rows, not of cells -- so the quantised costs
// of the next eight rows are loaded while eight rows run, and the band centre c(i) moves by additions (quotient and
// remainder of (Tb - 1) / (Ta - 1)), never by a division.  Back pointers, one byte per cell, go to the workspace.  Thread 0
// then walks back from (Ta - 1, Tb - 1), leaving the nodes in descending order in the workspace, and the block writes them
// in ascending order.  Integer from end to end: host and device cannot disagree.
//
// No MFMA: the fixed order of the float32 sums forbids it, and the work is small.
#include <climits>
#include <cstdint>

#include "mbx_kernels.h"

#pragma clang fp contract(off)

namespace mbx {

constexpr int ALIGN_NO_CELL = 65535;                        // align.NO_CELL
constexpr int ALIGN_UNREACHED = INT_MAX;
constexpr int ALIGN_AHEAD = 8;                              // rows whose costs are in flight while as many rows run

// c(i) = (i (Tb - 1) + (Ta - 1) / 2) / max(Ta - 1, 1); fits 32 bits: i, Tb - 1 <= 65534 and 65534^2 + 32767 < 2^32
__device__ inline int align_band_centre(int i, int ta, int tb) {
    const unsigned den = (unsigned)max(ta - 1, 1);
    return (int)(((unsigned)i * (unsigned)(tb - 1) + (unsigned)(ta - 1) / 2u) / den);
}

// THE SUM of align.py over x[0 .. M) read through `at`
template <class At>
__device__ inline float align_sum4(int M, At at) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int m = 0;
    for (; m + 4 <= M; m += 4) {
        s0 = s0 + at(m);
        s1 = s1 + at(m + 1);
        s2 = s2 + at(m + 2);
        s3 = s3 + at(m + 3);
    }
    if (m < M) s0 = s0 + at(m);
    if (m + 1 < M) s1 = s1 + at(m + 1);
    if (m + 2 < M) s2 = s2 + at(m + 2);
    return (s0 + s1) + (s2 + s3);
}

__global__ __launch_bounds__(64) void align_cost_kernel(AlignCostArgs p) {
    extern __shared__ __attribute__((aligned(16))) float align_smem[];
    const int b = blockIdx.z, i = blockIdx.y, lane = threadIdx.x;
    const int ta = min(max(p.n_frames_a[b], 0), p.max_frames_a), tb = min(max(p.n_frames_b[b], 0), p.max_frames_b);
    if (i >= ta || tb < 1) return;
    const int M = p.n_mels, W = p.band, nb = 2 * W + 1, stride = M | 1;
    const int o0 = 64 * (int)blockIdx.x;                    // first band column of the chunk (< nb by the grid)
    const int j0 = align_band_centre(i, ta, tb) - W + o0;   // its source row; may lie outside the item
    float *rows = align_smem, *guide = align_smem + 64 * stride;
    // the source rows of the chunk that exist: [lo, hi) of the item
    const int lo = max(j0, 0), hi = min(min(j0 + 64, j0 + nb - o0), tb);
    if (hi > lo) {
        const float *src = p.mel_b + ((long long)b * p.max_frames_b + lo) * M;
        const int total = (hi - lo) * M;
        int r = lane / M, m = lane - r * M;                 // element `lane` of the span: row r, channel m
        const int dr = 64 / M, dm = 64 - dr * M;            // a step of 64 elements
        for (int e = lane; e < total; e += 64) {
            rows[(lo - j0 + r) * stride + m] = src[e];
            r += dr;
            m += dm;
            if (m >= M) {
                m -= M;
                ++r;
            }
        }
    }
    const float *ga = p.mel_a + ((long long)b * p.max_frames_a + i) * M;
    for (int m = lane; m < M; m += 64) guide[m] = ga[m];
    __syncthreads();
    const int o = o0 + lane, j = j0 + lane;
    if (o >= nb) return;
    int q = ALIGN_NO_CELL;
    if (j >= 0 && j < tb) {
        const float *row = rows + lane * stride;
        const float fm = (float)M;
        const float mean_a = align_sum4(M, [&](int m) { return guide[m]; }) / fm;
        const float mean_b = align_sum4(M, [&](int m) { return row[m]; }) / fm;
        const float d = align_sum4(M, [&](int m) { return fabsf((guide[m] - mean_a) - (row[m] - mean_b)); });
        const float dd = d < 2048.f ? d : 2048.f;           // also a NaN
        q = (int)rintf(dd * 8.f);
    }
    p.cost[((long long)b * p.max_frames_a + i) * nb + o] = (uint16_t)q;
}

const char *check_align_cost(const AlignCostArgs &a) {
    if (!a.mel_a || !a.mel_b || !a.n_frames_a || !a.n_frames_b || !a.cost) return "null pointer";
    if (a.batch < 0) return "batch must not be negative";
    if (a.batch > 65535) return "batch must be at most 65535";
    if (a.max_frames_a < 1 || a.max_frames_b < 1) return "max_frames_a and max_frames_b must be at least 1";
    if (a.max_frames_a > ALIGN_MAX_FRAMES || a.max_frames_b > ALIGN_MAX_FRAMES)
        return "max_frames_a and max_frames_b must be at most 65535 (the int32 path cost)";
    if (a.n_mels < 1 || a.n_mels > ALIGN_MAX_MELS) return "n_mels must be in 1 .. 240 (64 source rows stay in LDS)";
    if (a.band < 1 || a.band > ALIGN_MAX_BAND) return "band must be in 1 .. 511 frames";
    return nullptr;
}

void launch_align_cost(const AlignCostArgs &a, hipStream_t stream) {
    if (a.batch == 0) return;
    const int nb = 2 * a.band + 1;
    const size_t smem = (size_t)(64 * (a.n_mels | 1) + a.n_mels) * sizeof(float);
    hipLaunchKernelGGL(align_cost_kernel, dim3((nb + 63) / 64, a.max_frames_a, a.batch), dim3(64), smem, stream, a);
}

// ------------------------------------------------------------------------------------------------------------------------

size_t align_workspace_bytes(long long batch, long long max_frames_a, long long band) {
    const long long cells = batch * max_frames_a * (2 * band + 1);
    return (size_t)((cells + 3) / 4 * 4 + batch * max_frames_a * 4);
}

__global__ __launch_bounds__(1024) void align_path_kernel(AlignPathArgs p) {
    __shared__ int dist[3][2 * ALIGN_MAX_BAND + 4];        // cell o at [o + 1]; [0] and [nb + 1] stay unreachable
    __shared__ int s_count;
    const int b = blockIdx.x, o = threadIdx.x;
    const int ta = min(max(p.n_frames_a[b], 0), p.max_frames_a), tb = min(max(p.n_frames_b[b], 0), ALIGN_MAX_FRAMES);
    const int W = p.band, nb = 2 * W + 1;
    if (ta < 1 || tb < 1) {
        if (o == 0) {
            p.count[b] = 0;
            p.total[b] = -1;
        }
        return;
    }
    const bool cell = o < nb;                               // the block has nb threads rounded up to whole waves
    const uint16_t *cost = p.cost + (long long)b * p.max_frames_a * nb;
    uint8_t *back = p.workspace + (long long)b * p.max_frames_a * nb;
    uint32_t *rev = reinterpret_cast<uint32_t *>(p.workspace + ((long long)p.batch * p.max_frames_a * nb + 3) / 4 * 4)
                    + (long long)b * p.max_frames_a;
    dist[0][o + 1] = dist[1][o + 1] = dist[2][o + 1] = ALIGN_UNREACHED;   // o + 1 <= 1024: also the end [nb + 1]
    if (o == 0) dist[0][0] = dist[1][0] = dist[2][0] = ALIGN_UNREACHED;
    __syncthreads();
    auto load = [&](int i) { return cell ? (int)cost[(long long)min(i, ta - 1) * nb + o] : ALIGN_NO_CELL; };

    // c(i) by additions: num(i) = i (Tb - 1) + (Ta - 1) / 2 = c den + rem
    const int den = max(ta - 1, 1), step_q = (tb - 1) / den, step_r = (tb - 1) - step_q * den;
    int c0 = ((ta - 1) / 2) / den, rem = ((ta - 1) / 2) - c0 * den;   // c(0)
    int c1 = c0, c2 = c0;                                   // c(i - 1), c(i - 2)
    int cur[ALIGN_AHEAD], nxt[ALIGN_AHEAD];
#pragma unroll
    for (int u = 0; u < ALIGN_AHEAD; ++u) cur[u] = load(u);
    for (int i0 = 0; i0 < ta; i0 += ALIGN_AHEAD) {
#pragma unroll
        for (int u = 0; u < ALIGN_AHEAD; ++u) nxt[u] = load(i0 + ALIGN_AHEAD + u);
#pragma unroll
        for (int u = 0; u < ALIGN_AHEAD; ++u) {
            const int i = i0 + u;
            if (i < ta) {                                   // uniform over the block: the barrier below is reached by all
                const int q = cur[u];
                const int *row1 = dist[(i + 2) % 3], *row2 = dist[(i + 1) % 3];
                // three reads without a branch: an index outside the band lands on one of the two unreachable ends, and
                // the rows in front of row 0 (and row -1 for i = 1) still hold what they were initialised with
                const int o1 = o + (c0 - c1), o3 = o + (c0 - c2);
                const int p0 = row1[min(max(o1, 0), nb + 1)];           // (i - 1, j - 1): cell o1 - 1, at [o1]
                const int p1 = row1[min(max(o1 - 1, 0), nb + 1)];       // (i - 1, j - 2)
                const int p2 = row2[min(max(o3, 0), nb + 1)];           // (i - 2, j - 1)
                int best = p0, arg = 0;
                arg = p1 < best ? 1 : arg;
                best = min(best, p1);
                arg = p2 < best ? 2 : arg;
                best = min(best, p2);
                best = (i == 0 && o == W - c0) ? 0 : best;              // the cell (0, 0)
                const bool ok = best != ALIGN_UNREACHED && q != ALIGN_NO_CELL;
                if (cell) {
                    dist[i % 3][o + 1] = ok ? best + q : ALIGN_UNREACHED;
                    back[(long long)i * nb + o] = (uint8_t)(ok ? arg : 3);
                }
                c2 = c1;
                c1 = c0;
                c0 += step_q;
                rem += step_r;
                if (rem >= den) {
                    rem -= den;
                    ++c0;
                }
                __syncthreads();
            }
        }
#pragma unroll
        for (int u = 0; u < ALIGN_AHEAD; ++u) cur[u] = nxt[u];
    }
    // c1 is now c(Ta - 1).  The walk back: one thread, one dependent load per node (the block's own stores, made visible
    // by the barriers above)
    if (o == 0) {
        const int end = tb - 1 - c1 + W;
        const int total = (end >= 0 && end < nb) ? dist[(ta - 1) % 3][end + 1] : ALIGN_UNREACHED;
        int n = 0;
        if (total != ALIGN_UNREACHED) {
            int i = ta - 1, j = tb - 1;
            while (true) {
                rev[n++] = ((uint32_t)i << 16) | (uint32_t)j;
                if (i == 0 && j == 0) break;
                const int oo = j - align_band_centre(i, ta, tb) + W;
                const int step = (oo >= 0 && oo < nb) ? back[(long long)i * nb + oo] : 3;
                i -= step == 2 ? 2 : 1;
                j -= step == 1 ? 2 : 1;
                if (step == 3 || i < 0 || j < 0 || n >= ta) {   // cannot happen on a reachable path; never walk outside
                    n = 0;
                    break;
                }
            }
        }
        s_count = n;
        p.count[b] = n;
        p.total[b] = n > 0 ? total : -1;
    }
    __syncthreads();
    const int n = s_count;
    for (int k = o; k < n; k += blockDim.x) {
        const uint32_t node = rev[n - 1 - k];
        p.nodes_i[(long long)b * p.max_frames_a + k] = (int)(node >> 16);
        p.nodes_j[(long long)b * p.max_frames_a + k] = (int)(node & 0xffffu);
    }
}

const char *check_align_path(const AlignPathArgs &a) {
    if (!a.cost || !a.n_frames_a || !a.n_frames_b || !a.workspace || !a.nodes_i || !a.nodes_j || !a.count || !a.total)
        return "null pointer";
    if (a.batch < 0) return "batch must not be negative";
    if (a.batch > 65535) return "batch must be at most 65535";
    if (a.max_frames_a < 1) return "max_frames_a must be at least 1";
    if (a.max_frames_a > ALIGN_MAX_FRAMES) return "max_frames_a must be at most 65535 (the int32 path cost)";
    if (a.band < 1 || a.band > ALIGN_MAX_BAND) return "band must be in 1 .. 511 frames (one thread per band cell)";
    if (a.workspace_bytes < align_workspace_bytes(a.batch, a.max_frames_a, a.band))
        return "the workspace is smaller than mbxg_align_workspace_size says";
    if (reinterpret_cast<uintptr_t>(a.workspace) % 4 != 0) return "the workspace must be aligned to 4 bytes";
    return nullptr;
}

void launch_align_path(const AlignPathArgs &a, hipStream_t stream) {
    if (a.batch == 0) return;
    const int threads = (2 * a.band + 1 + 63) / 64 * 64;
    hipLaunchKernelGGL(align_path_kernel, dim3(a.batch), dim3(threads), 0, stream, a);
}

}  // namespace mbx
