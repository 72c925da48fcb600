// Level control of whole items (include/mbexwn_level.h; the definition is mbexwn_vocoder_amd/level.py):
// BS.1770 hop energies, block powers and gates, sample and 4x true peak, one gain per item, and the product.
//
// level_hops_kernel   one thread per (item, hop): a float64 dependent chain of 3 * hop steps through two biquads (2 * hop
//                     steps of warm-up from zero state, then the hop itself).  Latency-type: the parallelism is items x hops
//                     (1600 chains at 16 x 10 s), 64-thread blocks so that the waves spread over the CUs.  The second biquad's
//                     step depends on the first's y of the same sample only, so the critical path is one biquad's recurrence.
// level_peak_kernel   one 256-thread block per (item, tile of 4096 samples): max |x| and, with taps, max |y| over the 16384
//                     outputs of the tile at four times the rate -- resample_chain.h's fmaf chain with the tile's input span
//                     and the taps in LDS, y never stored.  Maxima of non-negative float bit patterns: wave and block reduce,
//                     then one atomicMax on the uint per block, so the launch geometry cannot change the result.
// level_gate_kernel   one 64-thread block per item: the block powers in parallel, then the two gates and their ascending
//                     sums by one thread, the powers staged through LDS in chunks.
// level_gains_kernel  one thread per item, the targets in the kernel arguments;  level_apply_kernel  one float32 product per sample.
//
// The float64 expressions are the definition's, every product and sum rounded on its own: contraction to fused multiply-adds
// is off for the whole file (the fmaf of the true peak is an explicit call and stays one).
#include "mbx_handle.h"
#include "resample_chain.h"
#include "../../include/mbexwn_level.h"

#pragma clang fp contract(off)

namespace mbx {

namespace {

constexpr int LEVEL_ITEMS = 32;                 // the items' lengths, hops, coefficients and targets travel in the kernel arguments
constexpr int HOP_THREADS = 64;
constexpr int HOP_CHUNK = 16;                   // samples a thread of the hop kernel holds in registers, twice
constexpr int PEAK_THREADS = 256;
constexpr int PEAK_TILE = 4096;                 // input samples per block: 16384 outputs at four times the rate
constexpr int GATE_THREADS = 64;
constexpr int GATE_CHUNK = 2048;                // block powers staged in LDS at a time
constexpr int APPLY_THREADS = 256;
constexpr int APPLY_TILE = 2048;
constexpr int REC_COUNT = 8, REC_ABS = 12, REC_PEAK = 16, REC_TRUE = 20;   // byte offsets inside a record

static_assert(MBXL_RECORD_BYTES == 24 && MBXL_COEF_DOUBLES == 10, "mbexwn_level.h states the record and the coefficient row");

struct LevelItems {
    long long n[LEVEL_ITEMS];
    int hop[LEVEL_ITEMS];
};

// UNIT: b0 == 1 and b2 == 1 (the high-pass); 1 * x has the bits of x, so the two products are left out
struct LevelCoefs {                              // the items' coefficient rows, in the kernel arguments too
    double c[LEVEL_ITEMS][MBXL_COEF_DOUBLES];
};

struct LevelTargets {
    double power[LEVEL_ITEMS];
};

struct Biquad {
    double b0, b1, b2, a1, a2, s1, s2;
    template <bool UNIT>
    __device__ __forceinline__ double step(double x) {
        const double y = (UNIT ? x : b0 * x) + s1;
        s1 = (b1 * x - a1 * y) + s2;
        s2 = (UNIT ? x : b2 * x) - a2 * y;
        return y;
    }
};

// e of one hop: `warm` steps of warm-up from p[0], then the hop's own; p[0 .. total) is the item's
template <bool UNIT>
__device__ __forceinline__ double hop_energy(const float *p, int warm, int total, const double *c) {
    Biquad shelf{c[0], c[1], c[2], c[3], c[4], 0.0, 0.0}, high{c[5], c[6], c[7], c[8], c[9], 0.0, 0.0};
    // The samples come HOP_CHUNK at a time, the next chunk's loads in flight while this one is filtered: a lane walks its own
    // cache lines, and a load per step would put the memory latency into the chain.  Nothing behind p[total) is read; the
    // steps behind it in the last chunk work on zeros and their results are dropped.
    float cur[HOP_CHUNK], nxt[HOP_CHUNK];
    auto load = [=](float *dst, int k) {
        if (k + HOP_CHUNK <= total) {
#pragma unroll
            for (int i = 0; i < HOP_CHUNK; ++i) dst[i] = p[k + i];
        } else {
#pragma unroll
            for (int i = 0; i < HOP_CHUNK; ++i) dst[i] = k + i < total ? p[k + i] : 0.f;
        }
    };
    load(cur, 0);
    double e = 0.0;
    int k = 0;
    for (; k + HOP_CHUNK <= warm; k += HOP_CHUNK) {         // chunks inside the warm-up: no energy
        load(nxt, k + HOP_CHUNK);
#pragma unroll
        for (int i = 0; i < HOP_CHUNK; ++i) high.step<UNIT>(shelf.step<false>((double)cur[i]));
#pragma unroll
        for (int i = 0; i < HOP_CHUNK; ++i) cur[i] = nxt[i];
    }
    for (; k < total; k += HOP_CHUNK) {
        load(nxt, k + HOP_CHUNK);
#pragma unroll
        for (int i = 0; i < HOP_CHUNK; ++i) {
            const double y = high.step<UNIT>(shelf.step<false>((double)cur[i]));
            const double sq = y * y;
            e = e + (k + i >= warm && k + i < total ? sq : 0.0);    // e >= +0: adding +0 leaves its bits
        }
#pragma unroll
        for (int i = 0; i < HOP_CHUNK; ++i) cur[i] = nxt[i];
    }
    return e;
}

__global__ __launch_bounds__(HOP_THREADS) void level_hops_kernel(const float *audio, long long stride, LevelCoefs coefs,
                                                                 double *work, int hops_cap, LevelItems it) {
    const int item = blockIdx.y;
    const int hop = it.hop[item];
    const long long hops = it.n[item] / hop;
    const long long h = (long long)blockIdx.x * HOP_THREADS + threadIdx.x;
    if (h >= hops) return;
    const double *c = coefs.c[item];
    const long long first = h * hop;                        // first + hop <= hops * hop <= n_samples <= stride
    // The zeros in front of the item leave the zero state as it is (a zero's sign reaches no sum that is not zero), so the
    // chain starts at the item's first sample where the warm-up would start in front of it.
    const long long start = max(first - 2LL * hop, 0LL);
    const int warm = (int)(first - start), total = warm + hop;      // hop <= 2^28 (check_measure)
    const float *p = audio + (long long)item * stride + start;
    const bool unit = c[5] == 1.0 && c[7] == 1.0;           // uniform over the block
    work[(long long)item * 2 * hops_cap + h] = unit ? hop_energy<true>(p, warm, total, c) : hop_energy<false>(p, warm, total, c);
}

__device__ __forceinline__ unsigned int abs_bits(float v) { return __float_as_uint(v) & 0x7FFFFFFFu; }

template <bool TRUE_PEAK>
__global__ __launch_bounds__(PEAK_THREADS) void level_peak_kernel(const float *audio, long long stride, const float *taps,
                                                                  int n_taps, int span_cap, unsigned char *records,
                                                                  LevelItems it) {
    extern __shared__ float level_smem[];
    __shared__ unsigned int part[2][PEAK_THREADS / 64];
    float *xs = level_smem;                                 // span_cap floats
    float *ts = level_smem + span_cap;                      // n_taps floats
    const int item = blockIdx.y, tid = threadIdx.x;
    const long long n = it.n[item];
    const long long j0 = (long long)blockIdx.x * PEAK_TILE;
    if (j0 >= n) return;                                    // uniform over the block: before any barrier
    const float *xb = audio + (long long)item * stride;
    const int cnt = (int)min((long long)PEAK_TILE, n - j0);
    unsigned int m = 0, mt = 0;
    for (int i = tid; i < cnt; i += PEAK_THREADS) m = max(m, abs_bits(xb[j0 + i]));
    if (TRUE_PEAK) {
        constexpr int UP = 4;
        const int half = (n_taps - 1) / 2;
        const long long k0 = j0 * UP, k_last = (j0 + cnt) * UP - 1;
        // input span of the tile, as resample_poly.hip takes it (down = 1)
        const long long c_first = k0 + half - (n_taps - 1);
        const long long j_lo = c_first > 0 ? (c_first + UP - 1) / UP : 0;
        const long long j_hi = min(n - 1, (k_last + half) / UP);
        const int span = (int)min(j_hi - j_lo + 1, (long long)span_cap);
        for (int i = tid; i < span; i += PEAK_THREADS) xs[i] = xb[j_lo + i];
        for (int i = tid; i < n_taps; i += PEAK_THREADS) ts[i] = taps[i];
        __syncthreads();
        for (long long k = k0 + tid; k <= k_last; k += PEAK_THREADS)
            mt = max(mt, abs_bits(resample_chain(k + half, n, UP, n_taps, [=](int idx) { return ts[idx]; },
                                                 [=](long long j) { return xs[(int)(j - j_lo)]; })));
    }
    mt = max(mt, m);
    for (int off = 1; off < 64; off <<= 1) {
        m = max(m, (unsigned int)__shfl_xor((int)m, off));
        mt = max(mt, (unsigned int)__shfl_xor((int)mt, off));
    }
    if ((tid & 63) == 0) {
        part[0][tid >> 6] = m;
        part[1][tid >> 6] = mt;
    }
    __syncthreads();
    if (tid == 0) {                                         // one pair of atomics per block: they serialise per item
        for (int w = 1; w < PEAK_THREADS / 64; ++w) {
            m = max(m, part[0][w]);
            mt = max(mt, part[1][w]);
        }
        unsigned char *rec = records + (long long)item * MBXL_RECORD_BYTES;
        atomicMax(reinterpret_cast<unsigned int *>(rec + REC_PEAK), m);
        atomicMax(reinterpret_cast<unsigned int *>(rec + REC_TRUE), mt);
    }
}

__global__ __launch_bounds__(GATE_THREADS) void level_gate_kernel(double *work, int hops_cap, double abs_gate,
                                                                  unsigned char *records, LevelItems it) {
    __shared__ double zs[GATE_CHUNK];
    __shared__ double threshold;
    const int item = blockIdx.x, tid = threadIdx.x;
    const int hop = it.hop[item];
    const long long hops = it.n[item] / hop;
    const long long blocks = hops >= 4 ? hops - 3 : 0;
    const double *e = work + (long long)item * 2 * hops_cap;
    double *z = work + ((long long)item * 2 + 1) * hops_cap;
    const double den = (double)(4LL * hop);
    for (long long j = tid; j < blocks; j += GATE_THREADS) z[j] = (((e[j] + e[j + 1]) + e[j + 2]) + e[j + 3]) / den;
    __syncthreads();
    // two passes of ascending sums by thread 0, the powers staged through LDS: first the absolutely gated blocks, which
    // give the relative threshold, then the blocks above both
    double total = 0.0;
    long long count = 0, n_abs = 0;
    for (int pass = 0; pass < 2; ++pass) {
        total = 0.0;
        count = 0;
        for (long long base = 0; base < blocks; base += GATE_CHUNK) {
            const int len = (int)min((long long)GATE_CHUNK, blocks - base);
            for (int i = tid; i < len; i += GATE_THREADS) zs[i] = z[base + i];
            __syncthreads();
            if (tid == 0) {
                const double limit = pass ? threshold : abs_gate;
                for (int i = 0; i < len; ++i) {
                    const double v = zs[i];
                    if (v > abs_gate && v > limit) {
                        total = total + v;
                        ++count;
                    }
                }
            }
            __syncthreads();
        }
        if (pass == 0) {
            if (tid == 0) threshold = count > 0 ? 0.1 * (total / (double)count) : 0.0;
            n_abs = count;
            __syncthreads();
        }
    }
    if (tid == 0) {
        unsigned char *rec = records + (long long)item * MBXL_RECORD_BYTES;
        *reinterpret_cast<double *>(rec) = count > 0 ? total / (double)count : 0.0;
        *reinterpret_cast<int *>(rec + REC_COUNT) = (int)count;
        *reinterpret_cast<int *>(rec + REC_ABS) = (int)n_abs;
    }
}

__global__ __launch_bounds__(64) void level_gains_kernel(const unsigned char *records, int batch, LevelTargets targets,
                                                         const unsigned char *other, double ceiling, int has_ceiling,
                                                         int true_peak, float *gains) {
    const int b = threadIdx.x;                              // one block per launch: at most LEVEL_ITEMS items
    if (b >= batch) return;
    const unsigned char *rec = records + (long long)b * MBXL_RECORD_BYTES;
    const double power = *reinterpret_cast<const double *>(rec);
    const int count = *reinterpret_cast<const int *>(rec + REC_COUNT);
    const float pk = *reinterpret_cast<const float *>(rec + (true_peak ? REC_TRUE : REC_PEAK));
    float out = 1.f;
    if (pk == pk && pk != 0.f) {
        double target = targets.power[b];
        if (other) {
            const unsigned char *src = other + (long long)b * MBXL_RECORD_BYTES;
            target = *reinterpret_cast<const int *>(src + REC_COUNT) > 0 ? *reinterpret_cast<const double *>(src) : 0.0;
        }
        const double peak = (double)pk;
        double g = 1.0;
        if (target > 0.0 && count > 0 && power > 0.0) g = sqrt(target / power);
        if (has_ceiling && g * peak > ceiling) g = ceiling / peak;
        out = (float)g;
    }
    gains[b] = out;
}

__global__ __launch_bounds__(APPLY_THREADS) void level_apply_kernel(const float *audio, long long stride, const float *gains,
                                                                    float *out, long long out_stride, LevelItems it) {
    const int item = blockIdx.y;
    const long long n = it.n[item];
    const long long i0 = (long long)blockIdx.x * APPLY_TILE;
    if (i0 >= n) return;
    const long long i1 = min(i0 + APPLY_TILE, n);
    const float g = gains[item];
    const float *src = audio + (long long)item * stride;
    float *dst = out + (long long)item * out_stride;
    for (long long i = i0 + threadIdx.x; i < i1; i += APPLY_THREADS) dst[i] = src[i] * g;
}

const char *check_counts(int batch, const int64_t *n_samples, long long stride) {
    if (batch < 0 || (batch > 0 && !n_samples)) return "need batch >= 0 and the host array of sample counts";
    if (stride < 0) return "the stride must not be negative";
    for (int b = 0; b < batch; ++b)
        if (n_samples[b] < 0 || n_samples[b] > stride) return "every item needs 0 <= n_samples <= stride";
    return nullptr;
}

const char *check_measure(const float *audio, long long stride, int batch, const int64_t *n_samples, const int32_t *hops,
                          const double *coefs, const double *abs_gate, const float *taps, int n_taps, const double *workspace,
                          int hops_cap, const void *records) {
    if (const char *why = check_counts(batch, n_samples, stride)) return why;
    if (batch > 0 && !hops) return "need the host array of hop lengths";
    if (batch > 0 && !coefs) return "need the host array of coefficient rows";
    if (!abs_gate) return "null pointer to the absolute gate";
    if (hops_cap < 1) return "the workspace needs hops_cap >= 1";
    long long tiles = 0;
    for (int b = 0; b < batch; ++b) {
        if (hops[b] < 1 || hops[b] > (1 << 28)) return "every item needs 1 <= hop <= 2^28";
        if (n_samples[b] / hops[b] > hops_cap) return "the workspace is too small: an item has more hops than hops_cap";
        tiles = std::max(tiles, (long long)((n_samples[b] + PEAK_TILE - 1) / PEAK_TILE));
    }
    if (tiles > 0x7FFFFFFFLL) return "more tiles than one launch holds";
    if (taps && (n_taps < 1 || n_taps > MBXL_MAX_TAPS)) return "n_taps must lie in [1, MBXL_MAX_TAPS]";
    if (batch > 0 && (!audio || !workspace || !records)) return "null device pointer";
    return nullptr;
}

LevelItems chunk_items(int b0, int items, const int64_t *n_samples, const int32_t *hops, long long *longest) {
    LevelItems it{};
    *longest = 0;
    for (int i = 0; i < items; ++i) {
        it.n[i] = n_samples[b0 + i];
        it.hop[i] = hops ? hops[b0 + i] : 1;
        *longest = std::max(*longest, it.n[i]);
    }
    return it;
}

void launch_measure(const float *audio, long long stride, int batch, const int64_t *n_samples, const int32_t *hops,
                    const double *coefs, double abs_gate, const float *taps, int n_taps, double *workspace, int hops_cap,
                    unsigned char *records, hipStream_t stream) {
    const int span_cap = taps ? (4 * PEAK_TILE - 1 + n_taps - 1) / 4 + 2 : 0;
    const size_t smem = taps ? (size_t)(span_cap + n_taps) * sizeof(float) : 0;
    for (int b0 = 0; b0 < batch; b0 += LEVEL_ITEMS) {
        const int items = std::min(batch - b0, LEVEL_ITEMS);
        long long longest = 0, most_hops = 0;
        const LevelItems it = chunk_items(b0, items, n_samples, hops, &longest);
        LevelCoefs rows{};
        for (int i = 0; i < items; ++i) {
            most_hops = std::max(most_hops, it.n[i] / it.hop[i]);
            std::copy(coefs + (long long)(b0 + i) * MBXL_COEF_DOUBLES, coefs + (long long)(b0 + i + 1) * MBXL_COEF_DOUBLES, rows.c[i]);
        }
        const float *xa = audio + (long long)b0 * stride;
        double *work = workspace + (long long)b0 * 2 * hops_cap;
        unsigned char *rec = records + (long long)b0 * MBXL_RECORD_BYTES;
        if (most_hops > 0)
            hipLaunchKernelGGL(level_hops_kernel, dim3((unsigned)((most_hops + HOP_THREADS - 1) / HOP_THREADS), (unsigned)items),
                               dim3(HOP_THREADS), 0, stream, xa, stride, rows, work, hops_cap, it);
        if (longest > 0) {
            const dim3 grid((unsigned)((longest + PEAK_TILE - 1) / PEAK_TILE), (unsigned)items), block(PEAK_THREADS);
            if (taps)
                hipLaunchKernelGGL((level_peak_kernel<true>), grid, block, smem, stream, xa, stride, taps, n_taps, span_cap, rec, it);
            else
                hipLaunchKernelGGL((level_peak_kernel<false>), grid, block, 0, stream, xa, stride, taps, 0, 0, rec, it);
        }
        hipLaunchKernelGGL(level_gate_kernel, dim3((unsigned)items), dim3(GATE_THREADS), 0, stream, work, hops_cap, abs_gate, rec, it);
    }
}

}  // namespace

}  // namespace mbx

using namespace mbx_host;

static mbx_status refuse_level(const char *stage, const char *why) {
    return fail(MBX_ERR_INVALID_ARGUMENT, std::string(stage) + ": " + why);
}

extern "C" {

mbx_status mbxl_measure(const float *audio, int64_t stride, int32_t batch, const int64_t *n_samples, const int32_t *hops,
                        const double *coefs, const double *abs_gate, const float *taps, int32_t n_taps, double *workspace,
                        int32_t hops_cap, void *records, void *hip_stream) {
    if (const char *why = mbx::check_measure(audio, stride, batch, n_samples, hops, coefs, abs_gate, taps, n_taps, workspace,
                                             hops_cap, records))
        return refuse_level("level measure", why);
    if (batch == 0) return MBX_OK;
    const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipMemsetAsync(records, 0, (size_t)batch * MBXL_RECORD_BYTES, stream));    // the peaks are maxima from 0
    mbx::launch_measure(audio, stride, batch, n_samples, hops, coefs, *abs_gate, taps, n_taps, workspace, hops_cap,
                        static_cast<unsigned char *>(records), stream);
    return launch_status("kernel launch: ");
}

mbx_status mbxl_gains(const void *records, int32_t batch, const double *targets, const void *target_records,
                      const double *ceiling, int32_t true_peak, float *gains, void *hip_stream) {
    if (batch < 0) return refuse_level("level gains", "need batch >= 0");
    if (ceiling && !(*ceiling > 0.0)) return refuse_level("level gains", "the ceiling must be positive");
    if (batch == 0) return MBX_OK;
    if (!targets) return refuse_level("level gains", "need the host array of target powers");
    if (!records || !gains) return refuse_level("level gains", "null device pointer");
    const unsigned char *rec = static_cast<const unsigned char *>(records);
    const unsigned char *other = static_cast<const unsigned char *>(target_records);
    for (int b0 = 0; b0 < batch; b0 += mbx::LEVEL_ITEMS) {
        const int items = std::min(batch - b0, mbx::LEVEL_ITEMS);
        mbx::LevelTargets tt{};
        std::copy(targets + b0, targets + b0 + items, tt.power);
        hipLaunchKernelGGL(mbx::level_gains_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(hip_stream),
                           rec + (long long)b0 * MBXL_RECORD_BYTES, items, tt,
                           other ? other + (long long)b0 * MBXL_RECORD_BYTES : nullptr, ceiling ? *ceiling : 0.0,
                           ceiling ? 1 : 0, true_peak ? 1 : 0, gains + b0);
    }
    return launch_status("kernel launch: ");
}

mbx_status mbxl_apply(const float *audio, int64_t stride, int32_t batch, const int64_t *n_samples, const float *gains,
                      float *out, int64_t out_stride, void *hip_stream) {
    if (const char *why = mbx::check_counts(batch, n_samples, std::min(stride, out_stride)))
        return refuse_level("level apply", why);
    if (batch == 0) return MBX_OK;
    if (!audio || !gains || !out) return refuse_level("level apply", "null device pointer");
    if (out == audio && out_stride != stride) return refuse_level("level apply", "in place needs out_stride == stride");
    const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    for (int b0 = 0; b0 < batch; b0 += mbx::LEVEL_ITEMS) {
        const int items = std::min(batch - b0, mbx::LEVEL_ITEMS);
        long long longest = 0;
        const mbx::LevelItems it = mbx::chunk_items(b0, items, n_samples, nullptr, &longest);
        if (longest > 0)
            hipLaunchKernelGGL(mbx::level_apply_kernel,
                               dim3((unsigned)((longest + mbx::APPLY_TILE - 1) / mbx::APPLY_TILE), (unsigned)items),
                               dim3(mbx::APPLY_THREADS), 0, stream, audio + (long long)b0 * stride, stride, gains + b0,
                               out + (long long)b0 * out_stride, out_stride, it);
    }
    return launch_status("kernel launch: ");
}

}  // extern "C"
