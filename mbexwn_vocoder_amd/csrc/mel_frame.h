// One log-mel frame inside a 256-thread block: window multiply -> real FFT in LDS (fft_lds.h) -> magnitudes -> per-wave
// triangle sums -> log.  The body of the offline analysis (mel_analysis.hip) and of the streaming one (mel_stream.hip): both
// kernels call THIS function, parametrised only by how sample j of the frame is fetched, so that a frame computed from a
// ring of recent samples carries the bits of the same frame computed from the whole sound.
#pragma once
#include "fft_lds.h"

namespace mbx {

struct MelFrameTables {
    int win, fft_size, n_mels;
    const float *window;          // (win)
    const float *twiddle;         // (fft_size/2, 2): exp(-2 pi i m / fft_size)
    const float *basis;           // (n_mels, fft_size/2 + 1) dense rows
    const int *bin_lo, *bin_hi;   // (n_mels) first / last non-zero bin of a row
    float eps, log_eps;           // log_eps: the float32 nearest to log(eps)
};

// dynamic LDS the body needs: two FFT buffers and the twiddles (fft_size/2 float2 each) and fft_size/2 + 1 magnitudes
inline size_t mel_frame_smem(int fft_size) {
    const int nc = fft_size / 2;
    return sizeof(float2) * (size_t)(3 * nc) + sizeof(float) * (size_t)(nc + 1);
}

// fetch(j, &x): sample j (0 <= j < win) of the frame into x; false: there is none (the frame position is silence).
// ob: the n_mels outputs of the frame.  Called by all FFT_THREADS threads of the block.
template <class Fetch>
__device__ __forceinline__ void mel_frame_body(const MelFrameTables &p, float2 *smem, Fetch fetch, float *ob) {
    const int nc = p.fft_size / 2;
    float2 *a = smem, *bq = smem + nc, *tw = smem + 2 * nc;
    float *mag = reinterpret_cast<float *>(smem + 3 * nc);            // nc + 1 magnitudes
    const int tid = threadIdx.x;
    for (int i = tid; i < nc; i += FFT_THREADS) tw[i] = reinterpret_cast<const float2 *>(p.twiddle)[i];
    // frame samples j = 2m, 2m+1, zero-extended from win to fft_size
    for (int m = tid; m < nc; m += FFT_THREADS) {
        float v[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int j = 2 * m + q;
            float val = 0.f;
            if (j < p.win) {
                float x;
                if (fetch(j, x)) val = p.window[j] * x;
            }
            v[q] = val;
        }
        a[m] = make_float2(v[0], v[1]);
    }
    __syncthreads();
    const float2 *z = fft_lds<false>(a, bq, tw, nc, tid);
    for (int k = tid; k <= nc; k += FFT_THREADS) {
        const float2 x = real_bin(z, tw, k, nc);
        mag[k] = sqrtf(x.x * x.x + x.y * x.y);
    }
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6;
    for (int m = wave; m < p.n_mels; m += FFT_THREADS / 64) {
        const float *row = p.basis + (long long)m * (nc + 1);
        float acc = 0.f;
        for (int k = p.bin_lo[m] + lane; k <= p.bin_hi[m]; k += 64) acc = fmaf(mag[k], row[k], acc);
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
        // the floor is the float32 NEAREST to log(eps) (logf(eps) of the device library is its other neighbour)
        if (lane == 0) ob[m] = acc > p.eps ? logf(acc) : p.log_eps;
    }
}

}  // namespace mbx
