// Log-mel frames at arbitrary centre samples: the analysis of a time-stretched sound (include/mbexwn_warp.h:
// mbxw_mel_frames_at; the time map that gives the centres is mbexwn_vocoder_amd/timemap.py, the host definition
// analysis.py::compute_log_mel_at).
//
//   frame k of item b = win * x_reflect[c - win/2 .. + win), c = centres[b][k] clamped to [0, n_b]
//
// mel_analysis.hip with the frame's position read from a table instead of t * hop: one 256-thread block per (frame, item),
// the same closed-form numpy "reflect" fold (in 64-bit: a centre is an int64), then mel_frame.h's body, unchanged.  A frame
// with the same win samples in front of it therefore carries the bits of mel_analysis_kernel's row.  Bandwidth-type: reads
// win samples per frame (from L2 where frames overlap) and writes n_mels floats.  No MFMA.
#include <cmath>

#include "mbx_kernels.h"
#include "mel_frame.h"

namespace mbx {

__global__ __launch_bounds__(FFT_THREADS) void mel_warp_kernel(MelWarpArgs p) {
    extern __shared__ float2 smem[];
    const int k = blockIdx.x, b = blockIdx.y;
    if (k >= p.n_frames[b]) return;
    // length and centre from the device arrays, clamped to the item's row: a wrong entry must not address outside the buffer
    const long long n = min(max((long long)p.n_samples[b], 0LL), p.stride);
    const long long c = min(max(p.centres[(long long)b * p.max_frames + k], 0LL), n);
    const float *xb = p.audio + (long long)b * p.stride;
    const MelFrameTables tabs{p.win, p.fft_size, p.n_mels, p.window, p.twiddle, p.basis, p.bin_lo, p.bin_hi, p.eps, p.log_eps};
    const long long first = c - p.win / 2;
    const long long period = 2 * (n - 1);
    // sample j of the reflect-padded signal: the fold of mel_analysis_kernel (period 2 (n - 1), any depth; n = 1 repeats
    // its one sample).  The fold is the identity inside the item, so only a sample outside it pays the 64-bit remainder
    auto fetch = [=](int j, float &x) {
        long long s = first + j;
        if (s < 0 || s >= n) {
            if (period > 0) {
                s %= period;
                if (s < 0) s += period;
                if (s >= n) s = period - s;
            } else {
                s = 0;
            }
        }
        if (n < 1) return false;                            // an empty item is silence: log(eps) rows
        x = xb[s];
        return true;
    };
    mel_frame_body(tabs, smem, fetch, p.out + ((long long)b * p.max_frames + k) * p.n_mels);
}

const char *check_mel_warp(const MelWarpArgs &a) {
    if (!a.audio || !a.n_samples || !a.centres || !a.n_frames || !a.window || !a.twiddle || !a.basis || !a.bin_lo ||
        !a.bin_hi || !a.out)
        return "null pointer";
    if (a.fft_size < 8 || a.fft_size > 2048 || (a.fft_size & (a.fft_size - 1)) != 0)
        return "fft_size must be a power of two in 8 .. 2048";
    if (a.win < 2 || a.win > a.fft_size) return "win must lie in 2 .. fft_size";
    if (a.n_mels < 1) return "n_mels must be at least 1";
    if (a.max_frames < 1) return "max_frames must be at least 1";
    if (a.stride < 1) return "stride must be at least 1";
    if (a.batch < 0) return "batch must not be negative";
    if (a.batch > 65535) return "batch is larger than 65535, the y extent of a grid";
    return nullptr;
}

void launch_mel_warp(const MelWarpArgs &a, hipStream_t stream) {
    if (a.batch == 0) return;
    MelWarpArgs k = a;
    k.log_eps = (float)log((double)a.eps);
    hipLaunchKernelGGL(mel_warp_kernel, dim3(a.max_frames, a.batch), dim3(FFT_THREADS), mel_frame_smem(a.fft_size), stream, k);
}

}  // namespace mbx
