// One output of the polyphase FIR resampler: the fmaf chain both resamplers evaluate (resample_poly.hip on whole items,
// resample_stream.hip on sounds that are still arriving), as mel_frame.h is the one body of the two mel analyses.
//
//   c = k * down + half (64-bit),  jh = c / up,  ph = c % up
//   y[k] = sum_i g[ph + i * up] x[jh - i]  over  i = min((n_taps - 1 - ph) / up, jh)  down to  max(0, jh - (n - 1)):
// ascending j = jh - i, acc from 0.f, one fmaf per term.  A term past either end of the sound is left out, not multiplied
// by a zero.  `n` is the sound's length; a caller that does not know it yet passes RESAMPLE_OPEN and asks only for outputs
// with jh in front of the newest sample.  `tap(int index)` and `x(long long j)` are the fetches: where the operands are read
// from is the caller's business and moves no bit.  The trip count is at most n_taps / up + 1, whatever c and n are.
#pragma once

namespace mbx {

constexpr long long RESAMPLE_OPEN = 0x7FFFFFFFFFFFFFFFLL;      // "the length is not known yet": no clip at the end

template <class Tap, class Fetch>
__device__ __forceinline__ float resample_chain(long long c, long long n, int up, int n_taps, Tap tap, Fetch x) {
    const long long jh = c / up;
    const int ph = (int)(c - jh * up);
    float acc = 0.f;
    if (ph < n_taps) {
        const long long i_hi = min((long long)((n_taps - 1 - ph) / up), jh);      // tap index < n_taps, j >= 0
        const long long i_lo = max(0LL, jh - (n - 1));                              // j <= n - 1
        for (long long i = i_hi; i >= i_lo; --i)                                    // ascending j
            acc = fmaf(tap(ph + (int)i * up), x(jh - i), acc);
    }
    return acc;
}

}  // namespace mbx
