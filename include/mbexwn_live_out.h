/*
 * mbexwn_live_out.h -- the streaming output resampler of libmbexwn_hip.so (prefix mbxo_): audio out at any rate
 * (csrc/resample_stream.hip).
 *
 * It lives in the same shared library as include/mbexwn.h, include/mbexwn_audio.h, include/mbexwn_live.h,
 * include/mbexwn_live_resample.h and include/mbexwn_flac.h, returns the same mbx_status codes and leaves its message in the
 * same thread-local mbx_last_error().  It is declared in a header of its own because the export lists of the other headers
 * (and MBX_ABI_VERSION) are pinned by the suite's contract tests; this header adds to the library without changing those
 * lists.
 *
 * Conventions as in mbexwn_live_resample.h: no handle; the caller owns all buffers, every pointer is a device pointer; a
 * call only enqueues work on `hip_stream` (NULL: the default stream) of the CURRENT device, never allocates, never
 * synchronises and reads no environment variable.
 *
 * The input is a ring store at the model rate, laid out as mbexwn_live.h describes: `in_rings` (n_in_slots,
 * in_ring_samples), sample j of the stream in slot s at in_rings[s][j & (in_ring_samples - 1)], the length a power of two
 * (mbxl_ring_append fills it, from wherever the synthesis left its audio).  The output is not a ring: every row of the
 * call writes its new outputs side by side into `out`, ready for one device-to-host copy.
 *
 * The filter: `taps` (n_taps) float32 is the anti-aliasing FIR times the gain `up`, and up / down the reduced ratio of
 * the output rate to the model rate -- the arguments of mbxa_resample_poly for model rate -> output rate.  With
 * half = (n_taps - 1) / 2, output k is
 *
 *     c = k * down + half (64-bit),  jh = c / up,  ph = c % up
 *     y[k] = sum_i taps[ph + i * up] * x[jh - i],   i = min((n_taps - 1 - ph) / up, jh)  down to  max(0, jh - (n - 1))
 *
 * one float32 fmaf chain over ascending j = jh - i from 0.f, n the stream's final length in model-rate samples.  While
 * the stream is open n is unknown and the lower bound of i is 0: output k is final once jh <= have - 1, that is
 * k * down + half <= have * up - 1 with `have` samples appended; the caller asks for no other output.  Output k reads the
 * samples from max(0, ceil((k * down + half - (n_taps - 1)) / up)) to jh: the caller keeps in_ring_samples large enough
 * that none of them has been overwritten.
 *
 * THE PROMISE: output k of a stream, computed from a ring that holds the samples it reads, carries exactly the bits of
 * output k of mbxa_resample_poly on the stream's whole model-rate sound with the same taps -- both kernels run one device
 * function on the same operand values in the same order; the tile, the launch shape, where the taps are staged and where
 * the output is stored move no bit.
 */
#ifndef MBEXWN_LIVE_OUT_H
#define MBEXWN_LIVE_OUT_H

#include "mbexwn.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Resample the new outputs of every stream of a tick from the model-rate rings into packed rows at the output rate.  One
 * 256-thread block per (row, tile of 256 outputs).
 *
 *   in_rings        (n_in_slots, in_ring_samples) float32
 *   desc            (n_rows, 6) int64, one row per stream:
 *                     [0] in_slot     row of `in_rings`
 *                     [1] first_out   index, in its stream, of the first output to produce
 *                     [2] n_out_new   outputs to produce; 0 (or less) produces nothing
 *                     [3] n_total_in  the stream's final length in model-rate samples once it is known, else any negative
 *                                     value
 *                     [4] out_offset  where the row's outputs start in `out`, in floats
 *                     [5] reserved, 0
 *   max_new_out     the largest n_out_new among the rows; it sizes the launch only (a larger one is still produced whole)
 *   up, down, taps, n_taps: the filter, as for mbxa_resample_poly (mbexwn_audio.h)
 *   out             (out_floats) float32
 *
 * Output first_out + i goes to out[out_offset + i] for 0 <= i < n_out_new, and nothing else of `out` is written.  With
 * n_total_in >= 0 the terms past the end of the sound are left out of the chain (the caller asks for outputs below
 * ceil(n_total_in * up / down)).  A row whose in_slot is outside [0, n_in_slots), whose first_out is negative or so large
 * that (first_out + n_out_new) * down + half leaves 62 bits, whose out_offset is negative or whose out_offset + n_out_new
 * exceeds out_floats is skipped, not followed.  Every ring access is masked with the ring's length, and an output reads at
 * most n_taps / up + 1 samples.  Two rows of one call must not overlap in `out`: that is the caller's duty.  in_rings and
 * out must not overlap.
 *
 * Refused before any launch with MBX_ERR_INVALID_ARGUMENT (the message starts with "resample emit:"): a NULL pointer;
 * n_rows outside [0, 65535]; max_new_out below 0; up, down or n_taps below 1; n_in_slots below 1; in_ring_samples not a
 * power of two; out_floats below 0.
 */
mbx_status mbxo_resample_emit(const float *in_rings, int32_t n_in_slots, int32_t in_ring_samples, const int64_t *desc,
                              int32_t n_rows, int32_t max_new_out, int32_t up, int32_t down, const float *taps, int32_t n_taps,
                              float *out, int64_t out_floats, void *hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* MBEXWN_LIVE_OUT_H */
