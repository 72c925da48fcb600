// Audio -> log-mel analysis: the step in front of the hot path.
//
// restates, for the configuration the reference's CLI uses (no band limiting, do_post=False):
//   compute_mel_spectrogram_internal   reference MBExWN_NVoc/vocoder/model/preprocess.py:417-572
//   calc_stft (magnitude, centred)     reference MBExWN_NVoc/sig_proc/spec/stft.py:14-96
//     frame t = win * x_reflect[t*hop - win/2 .. + win), zero-extended to fft_size, |rFFT|
//   mel = |X| . basis^T, log(max(mel, eps))
// The window (symmetric Hann, reference Mwindows.py:60-67) and the Slaney mel basis are tables of the host module
// (analysis.py), which also is the float64-transform oracle this kernel is tested against.
//
// One 256-thread block per (item, frame), the frame's arithmetic in mel_frame.h (shared with mel_stream.hip): windowed frame -> real FFT (complex Stockham FFT of fft_size/2 points in LDS,
// fft_lds.h) -> magnitudes in LDS -> one wavefront per mel channel sums its triangle (bins [lo, hi] of the dense basis
// row) -> log.  Bandwidth-type: reads hop samples and writes mel_channels floats per frame.
#include <cmath>

#include "mbx_kernels.h"
#include "mel_frame.h"

namespace mbx {

__global__ __launch_bounds__(FFT_THREADS) void mel_analysis_kernel(MelAnalysisArgs p) {
    extern __shared__ float2 smem[];
    const int t = blockIdx.x, b = blockIdx.y;
    // item length from the device array, clamped to the item's row: a wrong entry must not address outside the buffer
    const int n = p.n_samples ? min(max(p.n_samples[b], 0), p.max_samples) : p.max_samples;
    const int frames = n / p.hop + 1;
    if (t >= frames) return;
    const float *xb = p.audio + (long long)b * p.audio_bstride;
    const MelFrameTables tabs{p.win, p.fft_size, p.n_mels, p.window, p.twiddle, p.basis, p.bin_lo, p.bin_hi, p.eps, p.log_eps};
    const int first = t * p.hop - p.win / 2;
    // sample j of the reflect-padded signal (numpy "reflect": no repeated edge sample)
    auto fetch = [=](int j, float &x) {
        // numpy "reflect" of any depth: the padded signal has period 2 (n - 1), so an item shorter than half a
        // window folds as often as it needs (closed form, no data-dependent loop); n = 1 repeats its one sample
        int s = first + j;
        const int period = 2 * (n - 1);
        if (period > 0) {
            s %= period;
            if (s < 0) s += period;
            if (s >= n) s = period - s;
        } else {
            s = 0;
        }
        if (n < 1) return false;                            // an empty item is one frame of silence: log(eps) rows
        x = xb[s];
        return true;
    };
    mel_frame_body(tabs, smem, fetch, p.out + ((long long)b * p.max_frames + t) * p.n_mels);
}

bool launch_mel_analysis(const MelAnalysisArgs &a, hipStream_t stream) {
    const bool ok = a.fft_size >= 8 && a.fft_size <= 2048 && (a.fft_size & (a.fft_size - 1)) == 0 && a.win >= 2 &&
                    a.win <= a.fft_size && a.hop >= 1 && a.n_mels >= 1 && a.max_samples >= a.win / 2 + 1 && a.audio &&
                    a.window && a.twiddle && a.basis && a.bin_lo && a.bin_hi && a.out && a.max_frames >= a.max_samples / a.hop + 1;
    if (!ok) return false;
    if (a.batch <= 0) return true;
    const size_t smem = mel_frame_smem(a.fft_size);
    MelAnalysisArgs k = a;
    k.log_eps = (float)log((double)a.eps);
    hipLaunchKernelGGL(mel_analysis_kernel, dim3(a.max_samples / a.hop + 1, a.batch), dim3(FFT_THREADS), smem, stream, k);
    return true;
}

}  // namespace mbx
