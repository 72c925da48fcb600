// Streaming audio -> log-mel analysis (include/mbexwn_live.h): the analysis of mel_analysis.hip for sounds that are still
// arriving.
//
// Frame t of the offline kernel depends only on samples [t*hop - win/2, t*hop - win/2 + win) of the reflect-padded item.
// Every stream keeps its last ring_samples samples in a ring (sample s of the stream at ring[slot][s & (ring_samples - 1)]);
//   ring_append_kernel   writes a tick's new samples of every stream into the rings,
//   mel_stream_kernel    computes the frames that became ready from the rings, by absolute sample index.
// The frame's arithmetic is mel_frame.h's body, the one function the offline kernel calls too: only the fetch of a sample
// differs (ring instead of the item's row), and the index it fetches is the offline kernel's.  While a stream is open its
// length is unknown (n_total < 0): only the fold about sample 0 applies, and the host asks for no frame whose window passes
// the newest sample.  Once the length is known the reflection is numpy's, of any depth, as offline.
//
// Both kernels are plain vector code.  A descriptor that names a slot outside the ring store, or samples outside the packed
// buffer, is skipped: a wrong entry must not address outside the caller's buffers.
#include <algorithm>
#include <cmath>

#include "mbx_kernels.h"
#include "mel_frame.h"

namespace mbx {

constexpr int RING_APPEND_THREADS = 256;
constexpr int RING_APPEND_MAX_BLOCKS = 1024;      // per stream; the kernel strides over what is left

__global__ __launch_bounds__(RING_APPEND_THREADS) void ring_append_kernel(RingAppendArgs p) {
    const long long *d = p.desc + 4LL * blockIdx.y;
    const long long slot = d[0], start = d[1], offset = d[3];
    // one call never writes more than the ring holds of a stream
    const long long count = min(d[2], (long long)p.rings.ring_samples);
    if (count <= 0 || !p.rings.has(slot) || start < 0 || offset < 0 || offset > p.packed_samples - count) return;
    float *ring = p.rings.row(slot);
    const float *src = p.packed + offset;
    const long long mask = p.rings.mask();
    for (long long i = (long long)blockIdx.x * RING_APPEND_THREADS + threadIdx.x; i < count;
         i += (long long)gridDim.x * RING_APPEND_THREADS)
        ring[(start + i) & mask] = src[i];
}

__global__ __launch_bounds__(FFT_THREADS) void mel_stream_kernel(MelStreamArgs p, float log_eps) {
    extern __shared__ float2 smem[];
    const StreamRow row{p.desc + 4LL * blockIdx.y};
    if (!row.has_frame(blockIdx.x, p.rings)) return;
    const long long t = row.first() + blockIdx.x, n_total = row.n_total();
    const float *ring = p.rings.row(row.slot());
    const long long mask = p.rings.mask();
    const MelFrameTables tabs{p.win, p.fft_size, p.n_mels, p.window, p.twiddle, p.basis, p.bin_lo, p.bin_hi, p.eps, log_eps};
    const long long first = t * p.hop - p.win / 2;
    auto fetch = [=](int j, float &x) {
        long long s = first + j;
        if (n_total < 0) {
            if (s < 0) s = -s;                               // the stream is open: only the start is an edge
        } else {
            // numpy "reflect" of any depth at the stream's final length, as the offline kernel folds
            const long long period = 2 * (n_total - 1);
            if (period > 0) {
                if (s < 0 || s >= n_total) {
                    s %= period;
                    if (s < 0) s += period;
                    if (s >= n_total) s = period - s;
                }
            } else {
                s = 0;
            }
            if (n_total < 1) return false;                   // an empty stream is one frame of silence, as offline
        }
        x = ring[s & mask];
        return true;
    };
    mel_frame_body(tabs, smem, fetch, p.out + ((long long)blockIdx.y * p.max_new_frames + blockIdx.x) * p.n_mels);
}

const char *check_ring_append(const RingAppendArgs &a) {
    if (!a.packed || !a.desc || !a.rings.data) return "NULL pointer";
    if (!row_count_fits(a.n_streams)) return "n_streams must lie in [0, 65535]";
    if (a.packed_samples < 0 || a.max_count < 0) return "packed_samples and max_count must not be negative";
    return ring_store_ok(a.rings) ? nullptr : "n_slots must be at least 1 and ring_samples a power of two";
}

void launch_ring_append(const RingAppendArgs &a, hipStream_t stream) {
    if (a.n_streams == 0 || a.max_count == 0) return;
    const long long want = ((long long)std::min(a.max_count, a.rings.ring_samples) + RING_APPEND_THREADS - 1) / RING_APPEND_THREADS;
    const int blocks = (int)std::min<long long>(std::max<long long>(want, 1), RING_APPEND_MAX_BLOCKS);
    hipLaunchKernelGGL(ring_append_kernel, dim3(blocks, a.n_streams), dim3(RING_APPEND_THREADS), 0, stream, a);
}

const char *check_mel_stream(const MelStreamArgs &a) {
    if (!a.rings.data || !a.desc || !a.window || !a.twiddle || !a.basis || !a.bin_lo || !a.bin_hi || !a.out) return "NULL pointer";
    if (!row_count_fits(a.n_streams)) return "n_streams must lie in [0, 65535]";
    if (a.max_new_frames < 0) return "max_new_frames must not be negative";
    // the bounds of launch_mel_analysis
    if (a.fft_size < 8 || a.fft_size > 2048 || !power_of_two(a.fft_size)) return "fft_size must be a power of two in [8, 2048]";
    if (a.win < 2 || a.win > a.fft_size) return "win must lie in [2, fft_size]";
    if (a.hop < 1 || a.n_mels < 1) return "hop and n_mels must be at least 1";
    return ring_store_ok(a.rings, a.win) ? nullptr : "n_slots must be at least 1 and ring_samples a power of two, at least win";
}

void launch_mel_stream(const MelStreamArgs &a, hipStream_t stream) {
    if (a.n_streams == 0 || a.max_new_frames == 0) return;
    const float log_eps = (float)log((double)a.eps);
    hipLaunchKernelGGL(mel_stream_kernel, dim3(a.max_new_frames, a.n_streams), dim3(FFT_THREADS), mel_frame_smem(a.fft_size),
                       stream, a, log_eps);
}

}  // namespace mbx
