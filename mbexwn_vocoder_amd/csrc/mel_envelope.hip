// Formant shift: the mel envelope of a frame read at f / phi (include/mbexwn_envelope.h: mbxe_warp_envelope; DESIGN.md
// section 6g; the host definition is mbexwn_vocoder_amd/envelope.py::warp_envelope_host).
//
//   out[b][t][m] = E_t(c[m] / phi[b][t]),   E_t = piecewise linear in Hz through (c[j], x[b][t][j]), held outside [c[0], c[n-1]]
//
// One thread per (frame, channel), as many whole frames per 256-thread block as fit (n_mels > 256: one frame, in turns); the
// centre table and the block's rows in LDS, the interval by a binary search over the table.  Bandwidth-type and, at every size
// the project runs, launch-bound: 2 B T n floats moved, ~log2(n) LDS reads and one division per element.  No MFMA.
//
// Host and device must give the same bits: every operation below is one separately rounded IEEE float32 operation -- plain
// operators with contraction switched off for this file (no fused multiply-add: numpy has none), the division the compiler's
// correctly rounded one.
#include "mbx_kernels.h"

#pragma clang fp contract(off)

namespace mbx {

constexpr int ENV_THREADS = 256;

__global__ __launch_bounds__(ENV_THREADS) void mel_envelope_kernel(EnvelopeArgs p) {
    extern __shared__ __attribute__((aligned(16))) float env_smem[];
    const int n = p.n_mels, b = blockIdx.y;
    const int t0 = blockIdx.x * p.frames_per_block;
    const int rows = min(p.frames_per_block, p.max_frames - t0);        // (> 0: the grid covers max_frames exactly)
    const int nf = p.n_frames ? min(max(p.n_frames[b], 0), p.max_frames) : p.max_frames;
    float *sc = env_smem, *sx = env_smem + n;
    const long long base = (long long)b * p.bstride + (long long)t0 * n;
    const float *xb = p.mel + base;
    for (int i = threadIdx.x; i < n; i += ENV_THREADS) sc[i] = p.centres[i];
    for (int i = threadIdx.x; i < rows * n; i += ENV_THREADS) sx[i] = xb[i];
    __syncthreads();
    float *ob = p.out + base;
    for (int idx = threadIdx.x; idx < rows * n; idx += ENV_THREADS) {
        const int r = idx / n, m = idx - r * n, t = t0 + r;
        const float *x = sx + r * n;
        float y = x[m];                                                   // rows behind the item's end and phi == 1: a copy
        const float phi = t < nf ? p.factors[(long long)b * p.max_frames + t] : 1.f;
        if (phi != 1.f) {
            const float f = sc[m] / phi;
            int lo = 0, hi = n;                                           // k = number of centres <= f (a NaN gives 0)
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (sc[mid] <= f) lo = mid + 1;
                else hi = mid;
            }
            if (lo == 0) {
                y = x[0];
            } else if (lo == n) {
                y = x[n - 1];
            } else {
                const int i = lo - 1;
                const float w = (f - sc[i]) / (sc[i + 1] - sc[i]);
                const float d = x[i + 1] - x[i];
                const float wd = w * d;
                y = x[i] + wd;
            }
        }
        ob[idx] = y;
    }
}

const char *check_envelope(const EnvelopeArgs &a) {
    if (!a.mel || !a.centres || !a.factors || !a.out) return "null pointer";
    if (a.n_mels < 2) return "n_mels must be at least 2";
    if (a.n_mels > 4096) return "n_mels must be at most 4096 (one row and the centre table stay in LDS)";
    if (a.max_frames < 1) return "max_frames must be at least 1";
    if (a.batch < 0) return "batch must not be negative";
    if (a.batch > 65535) return "batch is larger than 65535, the y extent of a grid";
    if (a.bstride < (long long)a.max_frames * a.n_mels) return "the item stride must be at least max_frames * n_mels";
    if (a.batch > 0) {
        const uintptr_t bytes = (uintptr_t)((long long)(a.batch - 1) * a.bstride + (long long)a.max_frames * a.n_mels) * sizeof(float);
        const uintptr_t in = reinterpret_cast<uintptr_t>(a.mel), out = reinterpret_cast<uintptr_t>(a.out);
        if (out < in + bytes && in < out + bytes) return "out must not alias mel";
    }
    return nullptr;
}

void launch_envelope(const EnvelopeArgs &a, hipStream_t stream) {
    if (a.batch == 0) return;
    EnvelopeArgs k = a;
    k.frames_per_block = std::max(1, std::min(ENV_THREADS / a.n_mels, a.max_frames));
    const int blocks = (a.max_frames + k.frames_per_block - 1) / k.frames_per_block;
    const size_t smem = (size_t)(a.n_mels + k.frames_per_block * a.n_mels) * sizeof(float);
    hipLaunchKernelGGL(mel_envelope_kernel, dim3(blocks, a.batch), dim3(ENV_THREADS), smem, stream, k);
}

}  // namespace mbx
