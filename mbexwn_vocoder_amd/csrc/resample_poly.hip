// Polyphase FIR resampler of a ragged batch: the step in front of the mel analysis (include/mbexwn_audio.h).
//
// restates the indexing of scipy.signal.resample_poly, which the reference's resampler ends in
// (reference MBExWN_NVoc/sig_proc/resample.py:64; the filter design, :31-63, is host work: resample.py::reference_filter):
//   half = (n_taps - 1) / 2,  c_k = k * down + half   (64-bit: down = 147 passes 2^31 after ten minutes of 44.1 kHz audio)
//   y[k] = sum_j g[c_k - j * up] x[j],  0 <= j < n, tap index in [0, n_taps),  0 <= k < ceil(n * up / down)
// With jh = c_k / up and ph = c_k % up the terms are g[ph + i * up] x[jh - i], i = 0 .. (n_taps - 1 - ph) / up.
//
// One 256-thread block per (item, tile of RS_TILE outputs), thread t takes outputs k0 + t + 256 q (coalesced stores).
// The block stages the input span of its tile in LDS and the tap table too when both fit in 64 KB (the rates that
// occur: 6 480 taps at 44.1 kHz, 14 400 at 11.025 kHz); a table that does not fit (an odd rate: 72 000 taps at 12 345 Hz)
// or a span that does not (decimation by more than 7) is read from global memory instead.  Bandwidth-type: 45 to 180
// multiply-adds per output, no MFMA.
//
// Every output is one fmaf chain over ascending j whose bounds follow from k and the item's own length, so its bits do
// not depend on the batch, on max_samples or on the tile it falls in -- nor on where the operands are read from.
#include "mbx_kernels.h"
#include "resample_chain.h"

namespace mbx {

constexpr int RS_THREADS = 256;
constexpr int RS_LDS_BYTES = 64 * 1024;          // the default dynamic LDS limit: no function attribute needed

template <bool X_LDS, bool T_LDS>
__global__ __launch_bounds__(RS_THREADS) void resample_poly_kernel(ResampleArgs p) {
    extern __shared__ float rs_smem[];
    float *xs = rs_smem;                                   // X_LDS: span_cap floats
    float *ts = rs_smem + (X_LDS ? p.span_cap : 0);        // T_LDS: n_taps floats
    const int b = (int)(blockIdx.x / (unsigned)p.tiles), tile = (int)(blockIdx.x % (unsigned)p.tiles);
    // item length from the device array, clamped to the item's row: a wrong entry must not address outside the buffer
    const int n = p.n_samples ? min(max(p.n_samples[b], 0), p.max_samples) : p.max_samples;
    const long long n_out = ((long long)n * p.up + p.down - 1) / p.down;
    const long long k0 = (long long)tile * RS_TILE;
    if (k0 >= n_out) return;                               // uniform over the block: before any barrier
    const int tid = threadIdx.x;
    const int half = (p.n_taps - 1) / 2;
    const float *xb = p.audio + (long long)b * p.max_samples;
    const long long k_last = min(k0 + RS_TILE, n_out) - 1;
    // input span of the tile: j_lo = first sample the first output reaches, j_hi = last sample the last output reaches
    const long long c_first = k0 * p.down + half - (p.n_taps - 1);
    const long long j_lo = c_first > 0 ? (c_first + p.up - 1) / p.up : 0;
    const long long j_hi = min((long long)n - 1, (k_last * p.down + half) / p.up);
    if (X_LDS) {
        const int span = (int)min(j_hi - j_lo + 1, (long long)p.span_cap);
        for (int i = tid; i < span; i += RS_THREADS) xs[i] = xb[j_lo + i];
    }
    if (T_LDS)
        for (int i = tid; i < p.n_taps; i += RS_THREADS) ts[i] = p.taps[i];
    if (X_LDS || T_LDS) __syncthreads();
    const float *tsrc = T_LDS ? ts : p.taps;
    float *ob = p.out + (long long)b * p.max_out;
    // the chain is resample_chain.h's, shared with the streaming kernel; here j lies in [j_lo, j_hi]
    for (long long k = k0 + tid; k <= k_last; k += RS_THREADS)
        ob[k] = resample_chain(k * p.down + half, n, p.up, p.n_taps, [=](int idx) { return tsrc[idx]; },
                               [=](long long j) { return X_LDS ? xs[(int)(j - j_lo)] : xb[j]; });
}

const char *check_resample_poly(const ResampleArgs &a) {
    if (!a.audio || !a.taps || !a.out) return "null pointer";
    if (a.batch < 1 || a.up < 1 || a.down < 1 || a.n_taps < 1) return "batch, up, down and n_taps must be at least 1";
    if (a.max_samples < 0) return "max_samples must not be negative";
    const long long need = ((long long)a.max_samples * a.up + a.down - 1) / a.down;
    if ((long long)a.max_out < need) return "max_out is smaller than ceil(max_samples * up / down)";
    const long long tiles = (need + RS_TILE - 1) / RS_TILE;
    if (tiles * a.batch > 0x7FFFFFFFLL) return "more tiles than one launch holds";
    return nullptr;
}

void launch_resample_poly(const ResampleArgs &a, hipStream_t stream) {
    ResampleArgs k = a;
    const long long need = ((long long)a.max_samples * a.up + a.down - 1) / a.down;
    k.tiles = (int)((need + RS_TILE - 1) / RS_TILE);
    if (k.tiles == 0) return;
    // the widest span a tile can reach: RS_TILE outputs advance (RS_TILE - 1) * down tap positions, n_taps - 1 more behind
    const long long span_cap = ((long long)(RS_TILE - 1) * a.down + a.n_taps - 1) / a.up + 2;
    const bool x_lds = span_cap * (long long)sizeof(float) <= RS_LDS_BYTES / 2;
    k.span_cap = x_lds ? (int)span_cap : 0;
    const size_t x_bytes = x_lds ? (size_t)span_cap * sizeof(float) : 0;
    const bool t_lds = x_bytes + (size_t)a.n_taps * sizeof(float) <= (size_t)RS_LDS_BYTES;
    const size_t smem = x_bytes + (t_lds ? (size_t)a.n_taps * sizeof(float) : 0);
    const dim3 grid((unsigned)((long long)k.tiles * a.batch)), block(RS_THREADS);
    if (x_lds && t_lds)
        hipLaunchKernelGGL((resample_poly_kernel<true, true>), grid, block, smem, stream, k);
    else if (x_lds)
        hipLaunchKernelGGL((resample_poly_kernel<true, false>), grid, block, smem, stream, k);
    else if (t_lds)
        hipLaunchKernelGGL((resample_poly_kernel<false, true>), grid, block, smem, stream, k);
    else
        hipLaunchKernelGGL((resample_poly_kernel<false, false>), grid, block, smem, stream, k);
}

}  // namespace mbx
