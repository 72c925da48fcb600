// Streaming polyphase FIR resampler (include/mbexwn_live_resample.h): the resampler of resample_poly.hip for sounds that are
// still arriving, from a ring at the input rate straight into the model-rate ring the streaming analysis reads -- and, on the
// way out (include/mbexwn_live_out.h), from a ring of model-rate samples that are still being produced into packed rows at
// the output rate, ready for one copy back.  Both are one body, resample_stream_row; only where an output is stored differs.
//
// Output k of a stream is resample_chain.h's chain, the one function the offline kernel calls too: only the fetch differs
// (sample j of the stream at in_rings[in_slot][j & (in_ring_samples - 1)] instead of the item's row).  While a stream is
// open its length is unknown (n_total_in < 0): there is no clip at the end, and the host asks for no output whose newest
// sample, jh = (k * down + half) / up, has not arrived.  Once the length is known the trailing clip is the offline one.
//
// One 256-thread block per (descriptor row, tile of RSS_TILE outputs), thread t takes output first_out + tile * RSS_TILE + t;
// a row with more tiles than the launch has blocks is finished by striding.  RSS_TILE is 256, not the 1024 of the offline
// kernel: a live tick is 64 streams x 1920 outputs, which is 128 blocks at 1024 and 512 at 256 on 256 CUs.  The tap table is
// staged in LDS when it fits the default 64 KB (6 480 taps at 44.1 kHz, 14 400 at 11.025 kHz), else read from global memory
// (72 000 taps at 12 345 Hz); the input span is read from the ring as it is (neighbouring outputs read neighbouring
// samples, and the ring of a tick is cache-resident).  Neither choice, nor the tile, moves a bit: the chain of an output
// depends on k, the filter and the stream's length alone.  Plain vector code, 45 to 180 multiply-adds per output, no MFMA.
//
// A wrong descriptor row must not address outside the caller's buffers: a row that names a slot outside a store, a negative
// first_out or one so large that k * down + half would leave 62 bits is skipped; n_out_new is clipped to the ring (into
// rings) or the row is skipped when it does not fit `out` (packed rows); every ring access is masked; the chain's trip count
// is bounded by n_taps / up + 1.
#include <algorithm>

#include "mbx_kernels.h"
#include "resample_chain.h"

namespace mbx {

constexpr int RSS_THREADS = 256;
constexpr int RSS_TILE = RSS_THREADS;             // outputs per block and pass
constexpr int RSS_MAX_TILES = 4096;               // blocks per row; the kernel strides over what is left
constexpr int RSS_LDS_BYTES = 64 * 1024;          // the default dynamic LDS limit: no function attribute needed

// The rows of one block: stage the taps, then one chain per output of the block's tiles.  `store(k, value)` is where output k of
// the stream goes -- the one thing the two kernels below differ in, as the fetches are the one thing resample_chain's callers
// differ in.  Every return is uniform over the block and in front of the barrier.
template <bool T_LDS, class Store>
__device__ __forceinline__ void resample_stream_row(const float *in_rings, int n_in_slots, int in_ring_samples, int up, int down,
                                                    const float *taps, int n_taps, long long in_slot, long long first_out,
                                                    long long n_new, long long n_total, Store store) {
    extern __shared__ float rss_smem[];
    const int half = (n_taps - 1) / 2;
    if (in_slot < 0 || in_slot >= n_in_slots || first_out < 0) return;
    if ((long long)blockIdx.x * RSS_TILE >= n_new) return;
    if (first_out > (0x3FFFFFFFFFFFFFFFLL - half) / down - n_new) return;
    const int tid = threadIdx.x;
    if (T_LDS) {
        for (int i = tid; i < n_taps; i += RSS_THREADS) rss_smem[i] = taps[i];
        __syncthreads();
    }
    const float *tsrc = T_LDS ? rss_smem : taps;
    const float *ring = in_rings + in_slot * in_ring_samples;
    const long long in_mask = in_ring_samples - 1;
    const long long n = n_total < 0 ? RESAMPLE_OPEN : n_total;
    for (long long o = (long long)blockIdx.x * RSS_TILE + tid; o < n_new; o += (long long)gridDim.x * RSS_TILE) {
        const long long k = first_out + o;
        store(k, resample_chain(k * down + half, n, up, n_taps, [=](int idx) { return tsrc[idx]; },
                                [=](long long j) { return ring[j & in_mask]; }));
    }
}

// into the model-rate ring store (mbxr_resample_rings): output k at out_rings[out_slot][k & (out_ring_samples - 1)]
template <bool T_LDS>
__global__ __launch_bounds__(RSS_THREADS) void resample_stream_kernel(ResampleStreamArgs p) {
    const long long *d = p.desc + 6LL * blockIdx.y;
    const long long in_slot = d[0], out_slot = d[1], first_out = d[2], n_total = d[4];
    const long long n_new = min(d[3], (long long)p.out_rings.ring_samples);     // one call never writes more than the ring holds
    if (!p.out_rings.has(out_slot)) return;
    float *out = p.out_rings.row(out_slot);
    const long long out_mask = p.out_rings.mask();
    resample_stream_row<T_LDS>(p.in_rings.data, p.in_rings.n_slots, p.in_rings.ring_samples, p.up, p.down, p.taps, p.n_taps,
                               in_slot, first_out, n_new, n_total, [=](long long k, float v) { out[k & out_mask] = v; });
}

// into packed rows (mbxo_resample_emit, include/mbexwn_live_out.h): output first_out + i at out[out_offset + i]
template <bool T_LDS>
__global__ __launch_bounds__(RSS_THREADS) void resample_emit_kernel(ResampleEmitArgs p) {
    const EmitRow row = EmitRow::of(p.desc + 6LL * blockIdx.y);
    if (!row.fits(p.in_rings, p.out_floats)) return;
    float *out = p.out + row.out_offset;
    const long long first_out = row.first_out;
    resample_stream_row<T_LDS>(p.in_rings.data, p.in_rings.n_slots, p.in_rings.ring_samples, p.up, p.down, p.taps, p.n_taps,
                               row.slot, first_out, row.n_new, row.n_total, [=](long long k, float v) { out[k - first_out] = v; });
}

const char *check_resample_stream(const ResampleStreamArgs &a) {
    if (!a.in_rings.data || !a.desc || !a.taps || !a.out_rings.data) return "NULL pointer";
    if (!row_count_fits(a.n_rows)) return "n_rows must lie in [0, 65535]";
    if (a.max_new_out < 0) return "max_new_out must not be negative";
    if (a.up < 1 || a.down < 1 || a.n_taps < 1) return "up, down and n_taps must be at least 1";
    if (!ring_store_ok(a.in_rings)) return "n_in_slots must be at least 1 and in_ring_samples a power of two";
    return ring_store_ok(a.out_rings) ? nullptr : "n_out_slots must be at least 1 and out_ring_samples a power of two";
}

const char *check_resample_emit(const ResampleEmitArgs &a) {
    if (!a.in_rings.data || !a.desc || !a.taps || !a.out) return "NULL pointer";
    if (!row_count_fits(a.n_rows)) return "n_rows must lie in [0, 65535]";
    if (a.max_new_out < 0) return "max_new_out must not be negative";
    if (a.up < 1 || a.down < 1 || a.n_taps < 1) return "up, down and n_taps must be at least 1";
    if (a.out_floats < 0) return "out_floats must not be negative";
    return ring_store_ok(a.in_rings) ? nullptr : "n_in_slots must be at least 1 and in_ring_samples a power of two";
}

// one block per (row, tile of the longest row), at most RSS_MAX_TILES tiles; the taps in LDS when they fit
template <class Args>
static void rss_launch(void (*taps_in_lds)(Args), void (*taps_in_global)(Args), const Args &a, long long max_new,
                       hipStream_t stream) {
    const long long want = (max_new + RSS_TILE - 1) / RSS_TILE;
    const int tiles = (int)std::min<long long>(std::max<long long>(want, 1), RSS_MAX_TILES);
    const dim3 grid(tiles, a.n_rows), block(RSS_THREADS);
    const size_t tap_bytes = (size_t)a.n_taps * sizeof(float);
    if (tap_bytes <= (size_t)RSS_LDS_BYTES)
        hipLaunchKernelGGL(taps_in_lds, grid, block, tap_bytes, stream, a);
    else
        hipLaunchKernelGGL(taps_in_global, grid, block, 0, stream, a);
}

void launch_resample_stream(const ResampleStreamArgs &a, hipStream_t stream) {
    if (a.n_rows == 0 || a.max_new_out == 0) return;
    rss_launch(resample_stream_kernel<true>, resample_stream_kernel<false>, a, std::min(a.max_new_out, a.out_rings.ring_samples), stream);
}

void launch_resample_emit(const ResampleEmitArgs &a, hipStream_t stream) {
    if (a.n_rows == 0 || a.max_new_out == 0) return;
    rss_launch(resample_emit_kernel<true>, resample_emit_kernel<false>, a, a.max_new_out, stream);
}

}  // namespace mbx
