// Look-ahead peak limiter (include/mbexwn_limiter.h; the definition is mbexwn_vocoder_amd/limiter.py).
//
// limit_tile          THE device function: the outputs [t0, t0 + cnt) of one item from the samples [t0 - h - H, t0 + cnt + 2h)
//                     inside it.  The needs of the span go to LDS as bit patterns (a minimum of non-negative floats is the
//                     minimum of their patterns); the sliding minimum over W = H + h + 1 is a table of doubling widths
//                     between two LDS spans -- log2(W) passes over the span, every one of them parallel over the block, where
//                     a van Herk scan would leave all but span / W threads idle -- and the last pass takes the minimum of
//                     two overlapping power-of-two windows and stores 1 - m; the FIR reads 2 h + 1 neighbours and the
//                     weights from LDS in the definition's order.  A span without a need below 1 skips all of that.
// limit_kernel        one block per (item, tile), the items' lengths in the kernel arguments; in place behind
//                     limit_margins_kernel, which saves what every tile reads outside itself
// limit_emit_kernel   one block per (descriptor row, tile), reading a ring store with masked indices, writing packed rows
//
// Both kernels call limit_tile with a fetch of their own: the operands and their order are the same, so are the bits.
// Contraction to fused multiply-adds is off for the whole file (the fmaf of the true peak is an explicit call).
#include <cmath>

#include "mbx_handle.h"
#include "resample_chain.h"
#include "ring_rows.h"
#include "../../include/mbexwn_limiter.h"

#pragma clang fp contract(off)

namespace mbx {

namespace {

constexpr int LIM_ITEMS = 32;                   // the items' lengths travel in the kernel arguments
constexpr int LIM_THREADS = 256;
constexpr int LIM_WAVES = LIM_THREADS / 64;
constexpr int LIM_TILE = MBXD_TILE;
constexpr int LIM_RED_WORDS = 16;               // the block's reductions: 3 words per wave
constexpr int LIM_MAX_TILES = 65535;            // of the emit launch; a longer row is walked
constexpr unsigned int ONE_BITS = 0x3F800000u, INF_BITS = 0x7F800000u;

static_assert(MBXD_STAT_WORDS == 4 && LIM_RED_WORDS >= 3 * LIM_WAVES, "mbexwn_limiter.h states the statistics");
static_assert(MBXD_LDS_WORDS * 4 <= 65536, "a block's LDS");

struct LimitItems {
    long long n[LIM_ITEMS];
};

__device__ __forceinline__ unsigned int lim_abs_bits(float v) { return __float_as_uint(v) & 0x7FFFFFFFu; }

// need of the definition from the bit pattern of d
__device__ __forceinline__ unsigned int lim_need_bits(unsigned int d_bits, float c) {
    const float d = __uint_as_float(d_bits);
    return d_bits < INF_BITS && d > c ? __float_as_uint(__fdiv_rn(c, d)) : ONE_BITS;
}

// `lds`: 2 * span_cap + 1 + (2 h + 1) + n_taps + LIM_RED_WORDS words, span_cap = LIM_TILE + 3 h + H >= cnt + 3 h + H.
// x(k): sample k of the item, asked for 0 <= k < n only.  store(i, y): output i, t0 <= i < t0 + cnt <= n.
// Every thread of the block calls it with the same arguments (it holds barriers).
template <bool TRUE_PEAK, class Fetch, class Store>
__device__ __forceinline__ void limit_tile(unsigned int *lds, int span_cap, const float *weights, int h, int H,
                                           const float *taps, int n_taps, long long n, long long t0, int cnt, float g0,
                                           float c, Fetch x, Store store, int *stats) {
    const int tid = threadIdx.x;
    unsigned int *A = lds;                                  // span_cap words
    unsigned int *B = lds + span_cap;                       // span_cap + 1 words
    float *ws = reinterpret_cast<float *>(lds + 2 * span_cap + 1);
    float *ts = ws + (2 * h + 1);
    int *red = reinterpret_cast<int *>(ts + n_taps);
    const int S = cnt + 3 * h + H;                          // needs of [k_lo, k_lo + S)
    const long long k_lo = t0 - h - H;
    __syncthreads();                                        // the tile before this one has read its LDS
    for (int j = tid; j <= 2 * h; j += LIM_THREADS) ws[j] = weights[j];
    bool below = false;
    if (TRUE_PEAK) {
        for (int j = tid; j < n_taps; j += LIM_THREADS) ts[j] = taps[j];
        __syncthreads();
        const int half = (n_taps - 1) / 2;
        // per sample k the four outputs v[4 k .. 4 k + 3] at four times the rate: A takes max(|u[k]|, |v[4 k .. 4 k + 3]|),
        // B (one to the right) the part of it that sample k + 1 sees too, max |v[4 k + 1 .. 4 k + 3]|
        for (int idx = tid - 1; idx < S; idx += LIM_THREADS) {
            const long long k = k_lo + idx;
            unsigned int own = 0, late = 0;
            if (k >= 0 && k < n) {
                own = lim_abs_bits(x(k) * g0);
                for (int ph = 0; ph < 4; ++ph) {
                    const unsigned int v = lim_abs_bits(resample_chain(4 * k + ph + half, n, 4, n_taps, [=](int i) { return ts[i]; },
                                                                       [=](long long j) { return x(j) * g0; }));
                    if (ph == 0) own = max(own, v);
                    else late = max(late, v);
                }
            }
            if (idx >= 0) A[idx] = max(own, late);
            B[idx + 1] = late;
        }
        __syncthreads();
        for (int idx = tid; idx < S; idx += LIM_THREADS) {
            const unsigned int need = lim_need_bits(max(A[idx], B[idx]), c);
            A[idx] = need;
            below |= need != ONE_BITS;
        }
    } else {
        for (int idx = tid; idx < S; idx += LIM_THREADS) {
            const long long k = k_lo + idx;
            const unsigned int need = k >= 0 && k < n ? lim_need_bits(lim_abs_bits(x(k) * g0), c) : ONE_BITS;
            A[idx] = need;
            below |= need != ONE_BITS;
        }
    }
    const bool limiting = __syncthreads_or(below);          // uniform; A and ws are visible behind it
    int low = (int)ONE_BITS, n_low = 0, n_clamp = 0;
    if (limiting) {
        const int W = H + h + 1;
        unsigned int *cur = A, *nxt = B;
        int size = 1;
        for (; 2 * size <= W; size *= 2) {                  // nxt[i] = min cur[i .. i + 2 size)
            for (int i = tid; i < S; i += LIM_THREADS) nxt[i] = i + size < S ? min(cur[i], cur[i + size]) : cur[i];
            __syncthreads();
            unsigned int *swap = cur;
            cur = nxt;
            nxt = swap;
        }
        // 1 - m over [t0 - h, t0 + cnt + h): entry e is the window cur[e .. e + W) = two windows of `size`
        float *slack = reinterpret_cast<float *>(nxt);
        const int shift = W - size;
        for (int e = tid; e < cnt + 2 * h; e += LIM_THREADS) slack[e] = 1.f - __uint_as_float(min(cur[e], cur[e + shift]));
        __syncthreads();
        for (int i = tid; i < cnt; i += LIM_THREADS) {
            float acc = 0.f;
            for (int j = 0; j <= 2 * h; ++j) acc = acc + ws[j] * slack[i + j];
            const float g = 1.f - acc;
            const float y = (x(t0 + i) * g0) * g;
            const float out = y > c ? c : (y < -c ? -c : y);
            store(t0 + i, out);
            low = min(low, (int)__float_as_uint(g));
            n_low += g < 1.f;
            n_clamp += (y > c) | (y < -c);
        }
    } else {
        for (int i = tid; i < cnt; i += LIM_THREADS) {      // g == 1: u * 1 has the bits of u
            const float y = x(t0 + i) * g0;
            store(t0 + i, y > c ? c : (y < -c ? -c : y));
            n_clamp += (y > c) | (y < -c);
        }
    }
    if (!stats) return;                                     // uniform
    for (int off = 1; off < 64; off <<= 1) {
        low = min(low, __shfl_xor(low, off));
        n_low += __shfl_xor(n_low, off);
        n_clamp += __shfl_xor(n_clamp, off);
    }
    if ((tid & 63) == 0) {
        red[3 * (tid >> 6)] = low;
        red[3 * (tid >> 6) + 1] = n_low;
        red[3 * (tid >> 6) + 2] = n_clamp;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < LIM_WAVES; ++w) {
            low = min(low, red[3 * w]);
            n_low += red[3 * w + 1];
            n_clamp += red[3 * w + 2];
        }
        if (low != (int)ONE_BITS) atomicMin(stats, low);
        if (n_low) atomicAdd(stats + 1, n_low);
        if (n_clamp) atomicAdd(stats + 2, n_clamp);
    }
}

__global__ __launch_bounds__(64) void limit_stats_kernel(int *stats, int items) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i < items) {
        stats[4 * i] = (int)ONE_BITS;
        stats[4 * i + 1] = stats[4 * i + 2] = stats[4 * i + 3] = 0;
    }
}

// In place a tile must not read what its neighbours may have overwritten: a launch in front of the limiter's saves, per
// (item, tile), the samples the tile reads outside itself -- `left` in front of it, `right` behind it -- and the limiter
// then reads its own tile from the audio (which no other block writes) and everything else from there.  The values are
// the same, so are the bits.  reach: what the true peak's chain reads beyond the span of needs (0 without taps).
__host__ __device__ inline int limit_reach(int n_taps) { return n_taps > 0 ? n_taps / 4 + 2 : 0; }

__global__ __launch_bounds__(LIM_THREADS) void limit_margins_kernel(const float *audio, long long stride, int h, int H, int reach,
                                                                    float *margins, long long tiles_cap, LimitItems it) {
    const int item = blockIdx.y;
    const long long n = it.n[item];
    const long long t0 = (long long)blockIdx.x * LIM_TILE;
    if (t0 >= n) return;
    const int cnt = (int)min((long long)LIM_TILE, n - t0);
    const int left = h + H + reach, right = 2 * h + reach;
    const float *src = audio + (long long)item * stride;
    float *mg = margins + ((long long)item * tiles_cap + blockIdx.x) * (left + right);
    for (int idx = threadIdx.x; idx < left + right; idx += LIM_THREADS) {
        const long long k = idx < left ? t0 - left + idx : t0 + cnt + (idx - left);
        if (k >= 0 && k < n) mg[idx] = src[k];
    }
}

template <bool TRUE_PEAK, bool IN_PLACE>
__global__ __launch_bounds__(LIM_THREADS) void limit_kernel(const float *audio, long long stride, const float *gains, float c,
                                                            int h, int H, const float *weights, const float *taps, int n_taps,
                                                            float *out, long long out_stride, int *stats, const float *margins,
                                                            long long tiles_cap, LimitItems it) {
    extern __shared__ unsigned int limit_lds[];
    const int item = blockIdx.y;
    const long long n = it.n[item];
    const long long t0 = (long long)blockIdx.x * LIM_TILE;
    if (t0 >= n) return;                                    // uniform over the block: before any barrier
    const int cnt = (int)min((long long)LIM_TILE, n - t0);
    const float *src = audio + (long long)item * stride;
    float *dst = out + (long long)item * out_stride;
    const auto store = [=](long long i, float y) { dst[i] = y; };
    if (IN_PLACE) {
        const int left = h + H + limit_reach(n_taps), right = 2 * h + limit_reach(n_taps);
        const float *mg = margins + ((long long)item * tiles_cap + blockIdx.x) * (left + right);
        const long long end = t0 + cnt;
        limit_tile<TRUE_PEAK>(limit_lds, LIM_TILE + 3 * h + H, weights, h, H, taps, n_taps, n, t0, cnt, gains[item], c,
                              [=](long long k) { return k < t0 ? mg[k - t0 + left] : (k >= end ? mg[left + (k - end)] : src[k]); },
                              store, stats + MBXD_STAT_WORDS * item);
    } else {
        limit_tile<TRUE_PEAK>(limit_lds, LIM_TILE + 3 * h + H, weights, h, H, taps, n_taps, n, t0, cnt, gains[item], c,
                              [=](long long k) { return src[k]; }, store, stats + MBXD_STAT_WORDS * item);
    }
}

struct LimitEmitArgs {
    RingStore rings;
    const long long *desc;
    int n_rows, max_new;
    float c;
    int h, H;
    const float *weights;
    float *out;
    long long out_floats;
    int *stats;
};

__global__ __launch_bounds__(LIM_THREADS) void limit_emit_kernel(LimitEmitArgs p) {
    extern __shared__ unsigned int limit_lds[];
    const EmitRow row = EmitRow::of(p.desc + 6LL * blockIdx.y);
    const long long first = row.first_out, n_new = row.n_new;
    const float g0 = __uint_as_float((unsigned int)(row.word5 & 0xFFFFFFFFLL));
    // all uniform over the block
    if (!row.fits(p.rings, p.out_floats) || n_new <= 0 || first > (1LL << 62) - n_new) return;
    const long long end = first + n_new;
    // an open stream: the caller asks for outputs whose samples are there, the last of them reads sample end + 2 h - 1
    const long long n = row.n_total >= 0 ? row.n_total : end + 2LL * p.h;
    if (end > n) return;
    const float *ring = p.rings.row(row.slot);
    const long long mask = p.rings.mask();
    float *dst = p.out + row.out_offset;
    int *stats = p.stats ? p.stats + MBXD_STAT_WORDS * row.slot : nullptr;
    for (long long t0 = first + (long long)blockIdx.x * LIM_TILE; t0 < end; t0 += (long long)gridDim.x * LIM_TILE) {
        const int cnt = (int)min((long long)LIM_TILE, end - t0);
        limit_tile<false>(limit_lds, LIM_TILE + 3 * p.h + p.H, p.weights, p.h, p.H, nullptr, 0, n, t0, cnt, g0, p.c,
                          [=](long long k) { return ring[k & mask]; }, [=](long long i, float y) { dst[i - first] = y; }, stats);
    }
}

long long lds_words(int h, int H, int n_taps) {
    return 2LL * (LIM_TILE + 3LL * h + H) + 1 + (2LL * h + 1) + n_taps + LIM_RED_WORDS;
}

const char *check_window(float c, int h, int H, const float *weights, int n_taps) {
    if (!(c > 0.f) || !std::isfinite(c)) return "the ceiling must be finite and positive";
    if (h < 1 || H < h) return "the window needs 1 <= h <= hold";
    if (!weights) return "null pointer to the weights";
    if (lds_words(h, H, n_taps) > MBXD_LDS_WORDS)
        return "the window is too long: 2 * (MBXD_TILE + 3 h + hold) + 2 h + n_taps + 18 exceeds MBXD_LDS_WORDS";
    return nullptr;
}

long long margin_floats(long long stride, int batch, int h, int H, int n_taps) {
    const long long tiles = (stride + LIM_TILE - 1) / LIM_TILE;
    return (long long)batch * tiles * (3LL * h + H + 2LL * limit_reach(n_taps));
}

template <bool TRUE_PEAK, bool IN_PLACE>
void launch_limit(dim3 grid, size_t smem, hipStream_t stream, const float *audio, long long stride, const float *gains, float c,
                  int h, int H, const float *weights, const float *taps, int n_taps, float *out, long long out_stride, int *stats,
                  const float *margins, long long tiles_cap, const LimitItems &it) {
    hipLaunchKernelGGL((limit_kernel<TRUE_PEAK, IN_PLACE>), grid, dim3(LIM_THREADS), smem, stream, audio, stride, gains, c, h, H,
                       weights, taps, n_taps, out, out_stride, stats, margins, tiles_cap, it);
}

}  // namespace

}  // namespace mbx

using namespace mbx_host;

static mbx_status refuse_limit(const char *stage, const char *why) {
    return fail(MBX_ERR_INVALID_ARGUMENT, std::string(stage) + ": " + why);
}

extern "C" {

mbx_status mbxd_limit(const float *audio, int64_t stride, int32_t batch, const int64_t *n_samples, const float *gains,
                      float ceiling, int32_t h, int32_t hold, const float *weights, const float *taps, int32_t n_taps,
                      float *out, int64_t out_stride, int32_t *stats, float *workspace, int64_t workspace_floats,
                      void *hip_stream) {
    if (batch < 0 || (batch > 0 && !n_samples)) return refuse_limit("limit", "need batch >= 0 and the host array of sample counts");
    if (stride < 0 || out_stride < 0) return refuse_limit("limit", "the strides must not be negative");
    long long longest = 0;
    for (int b = 0; b < batch; ++b) {
        if (n_samples[b] < 0 || n_samples[b] > std::min(stride, out_stride))
            return refuse_limit("limit", "every item needs 0 <= n_samples <= min(stride, out_stride)");
        longest = std::max<long long>(longest, n_samples[b]);
    }
    if (taps && n_taps < 1) return refuse_limit("limit", "n_taps must be at least 1");
    if (!taps) n_taps = 0;
    if (const char *why = mbx::check_window(ceiling, h, hold, weights, n_taps)) return refuse_limit("limit", why);
    if ((longest + mbx::LIM_TILE - 1) / mbx::LIM_TILE > 0x7FFFFFFFLL) return refuse_limit("limit", "more tiles than one launch holds");
    if (batch == 0) return MBX_OK;
    if (!audio || !gains || !out || !stats) return refuse_limit("limit", "null device pointer");
    const bool in_place = out == audio;
    if (in_place) {
        if (out_stride != stride) return refuse_limit("limit", "in place needs out_stride == stride");
        if (!workspace || workspace_floats < mbx::margin_floats(stride, batch, h, hold, n_taps))
            return refuse_limit("limit", "in place needs a workspace of mbxd_limit_workspace_floats floats: a tile reads the "
                                         "samples of its neighbours");
        const float *ws_end = workspace + workspace_floats;
        if (workspace < audio + (long long)batch * stride && audio < ws_end)
            return refuse_limit("limit", "the workspace must not overlap the audio");
    } else if (out < audio + (long long)batch * stride && audio < out + (long long)batch * out_stride) {
        return refuse_limit("limit", "out must be audio itself or must not overlap it");
    }
    const long long tiles_cap = (stride + mbx::LIM_TILE - 1) / mbx::LIM_TILE;
    const int reach = mbx::limit_reach(n_taps);
    const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const size_t smem = (size_t)mbx::lds_words(h, hold, n_taps) * sizeof(unsigned int);
    hipLaunchKernelGGL(mbx::limit_stats_kernel, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, stream, stats, batch);
    for (int b0 = 0; b0 < batch; b0 += mbx::LIM_ITEMS) {
        const int items = std::min(batch - b0, mbx::LIM_ITEMS);
        mbx::LimitItems it{};
        long long most = 0;
        for (int i = 0; i < items; ++i) most = std::max<long long>(most, it.n[i] = n_samples[b0 + i]);
        if (most == 0) continue;
        const dim3 grid((unsigned)((most + mbx::LIM_TILE - 1) / mbx::LIM_TILE), (unsigned)items), block(mbx::LIM_THREADS);
        const float *src = audio + (long long)b0 * stride;
        float *dst = out + (long long)b0 * out_stride;
        int *st = stats + (long long)b0 * MBXD_STAT_WORDS;
        float *mg = in_place ? workspace + (long long)b0 * tiles_cap * (3LL * h + hold + 2LL * reach) : nullptr;
        if (in_place)
            hipLaunchKernelGGL(mbx::limit_margins_kernel, grid, block, 0, stream, src, stride, h, hold, reach, mg, tiles_cap, it);
        auto launch = taps ? (in_place ? mbx::launch_limit<true, true> : mbx::launch_limit<true, false>)
                           : (in_place ? mbx::launch_limit<false, true> : mbx::launch_limit<false, false>);
        launch(grid, smem, stream, src, stride, gains + b0, ceiling, h, hold, weights, taps, n_taps, dst, out_stride, st, mg,
               tiles_cap, it);
    }
    return launch_status("kernel launch: ");
}

size_t mbxd_limit_workspace_floats(int64_t stride, int32_t batch, int32_t h, int32_t hold, int32_t n_taps) {
    if (stride < 0 || batch < 0 || h < 1 || hold < h || n_taps < 0) return 0;
    return (size_t)mbx::margin_floats(stride, batch, h, hold, n_taps);
}

mbx_status mbxd_limit_emit(const float *rings, int32_t n_slots, int32_t ring_samples, const int64_t *desc, int32_t n_rows,
                           int32_t max_new, float ceiling, int32_t h, int32_t hold, const float *weights, float *out,
                           int64_t out_floats, int32_t *stats, void *hip_stream) {
    const mbx::LimitEmitArgs args{{rings, n_slots, ring_samples}, reinterpret_cast<const long long *>(desc), n_rows, max_new,
                                  ceiling, h, hold, weights, out, out_floats, stats};
    if (!rings || !desc || !out) return refuse_limit("limit emit", "NULL pointer");
    if (!mbx::row_count_fits(n_rows)) return refuse_limit("limit emit", "n_rows must lie in [0, 65535]");
    if (max_new < 0) return refuse_limit("limit emit", "max_new must not be negative");
    if (!mbx::ring_store_ok(args.rings)) return refuse_limit("limit emit", "n_slots must be at least 1 and ring_samples a power of two");
    if (out_floats < 0) return refuse_limit("limit emit", "out_floats must not be negative");
    if (const char *why = mbx::check_window(ceiling, h, hold, weights, 0)) return refuse_limit("limit emit", why);
    if (n_rows == 0 || max_new == 0) return MBX_OK;
    const long long want = ((long long)max_new + mbx::LIM_TILE - 1) / mbx::LIM_TILE;
    const dim3 grid((unsigned)std::min<long long>(want, mbx::LIM_MAX_TILES), (unsigned)n_rows);
    hipLaunchKernelGGL(mbx::limit_emit_kernel, grid, dim3(mbx::LIM_THREADS), (size_t)mbx::lds_words(h, hold, 0) * sizeof(unsigned int),
                       static_cast<hipStream_t>(hip_stream), args);
    return launch_status("kernel launch: ");
}

}  // extern "C"
