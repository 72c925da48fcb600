/*
 * mbexwn_live_resample.h -- the streaming resampler of libmbexwn_hip.so (prefix mbxr_): live streams at any input rate
 * (csrc/resample_stream.hip).
 *
 * It lives in the same shared library as include/mbexwn.h, include/mbexwn_audio.h and include/mbexwn_live.h, returns the
 * same mbx_status codes and leaves its message in the same thread-local mbx_last_error().  It is declared in a header of
 * its own because the export lists of the other three headers (and MBX_ABI_VERSION) are pinned by the suite's contract
 * tests; this header adds to the library without changing those lists.
 *
 * Conventions as in mbexwn_live.h: no handle; the caller owns all buffers, every pointer is a device pointer; a call only
 * enqueues work on `hip_stream` (NULL: the default stream) of the CURRENT device, never allocates, never synchronises and
 * reads no environment variable.
 *
 * Two ring stores, both laid out as mbexwn_live.h describes: `in_rings` (n_in_slots, in_ring_samples) holds the arriving
 * samples at the input rate (sample j of the stream in slot s at in_rings[s][j & (in_ring_samples - 1)]; mbxl_ring_append
 * fills it), `out_rings` (n_out_slots, out_ring_samples) is the model-rate store mbxl_mel_frames reads (output k of the
 * stream in slot s at out_rings[s][k & (out_ring_samples - 1)]).  Both lengths are powers of two.
 *
 * The filter: `taps` (n_taps) float32 is the anti-aliasing FIR times the gain `up`, and up / down the reduced ratio of
 * the model rate to the input rate -- the arguments of mbxa_resample_poly.  With half = (n_taps - 1) / 2, output k is
 *
 *     c = k * down + half (64-bit),  jh = c / up,  ph = c % up
 *     y[k] = sum_i taps[ph + i * up] * x[jh - i],   i = min((n_taps - 1 - ph) / up, jh)  down to  max(0, jh - (n - 1))
 *
 * one float32 fmaf chain over ascending j = jh - i from 0.f, n the stream's final length in input samples.  While the
 * stream is open n is unknown and the lower bound of i is 0: output k is final once jh <= have - 1, that is
 * k * down + half <= have * up - 1 with `have` input samples appended; the caller asks for no other output.  Output k reads
 * the input samples from max(0, ceil((k * down + half - (n_taps - 1)) / up)) to jh: the caller keeps in_ring_samples large
 * enough that none of them has been overwritten.
 *
 * THE PROMISE: output k of a stream, computed from a ring that holds the samples it reads, carries exactly the bits of
 * output k of mbxa_resample_poly on the stream's whole sound with the same taps -- both kernels run one device function on
 * the same operand values in the same order; the tile, the launch shape and where the taps are staged move no bit.
 */
#ifndef MBEXWN_LIVE_RESAMPLE_H
#define MBEXWN_LIVE_RESAMPLE_H

#include "mbexwn.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Resample the new outputs of every stream of a tick from the input-rate rings into the model-rate rings.  One 256-thread
 * block per (row, tile of 256 outputs).
 *
 *   in_rings        (n_in_slots, in_ring_samples) float32
 *   desc            (n_rows, 6) int64, one row per stream:
 *                     [0] in_slot     row of `in_rings`
 *                     [1] out_slot    row of `out_rings`
 *                     [2] first_out   index, in its stream, of the first output to produce
 *                     [3] n_out_new   outputs to produce; 0 (or less) produces nothing
 *                     [4] n_total_in  the stream's final length in input samples once it is known, else any negative value
 *                     [5] reserved, 0
 *   max_new_out     the largest n_out_new among the rows; it sizes the launch only (a larger one is still produced whole)
 *   up, down, taps, n_taps: the filter, as for mbxa_resample_poly (mbexwn_audio.h)
 *   out_rings       (n_out_slots, out_ring_samples) float32
 *
 * Output first_out + i goes to out_rings[out_slot][(first_out + i) & (out_ring_samples - 1)] for
 * 0 <= i < min(n_out_new, out_ring_samples): one call never writes more than out_ring_samples outputs of a stream, and
 * nothing outside the stream's own row.  With n_total_in >= 0 the terms past the end of the sound are left out of the chain
 * (the caller asks for outputs below ceil(n_total_in * up / down)).  A row whose in_slot is outside [0, n_in_slots), whose
 * out_slot is outside [0, n_out_slots), whose first_out is negative or so large that (first_out + n_out_new) * down + half
 * leaves 62 bits is skipped.  Every ring access is masked with the ring's length, and an output reads at most
 * n_taps / up + 1 samples.  Two rows of one call must not name the same out_slot; in_rings and out_rings must not overlap.
 *
 * Refused before any launch with MBX_ERR_INVALID_ARGUMENT: a NULL pointer; n_rows outside [0, 65535]; max_new_out below 0;
 * up, down or n_taps below 1; n_in_slots or n_out_slots below 1; in_ring_samples or out_ring_samples not a power of two.
 */
mbx_status mbxr_resample_rings(const float *in_rings, int32_t n_in_slots, int32_t in_ring_samples, const int64_t *desc,
                               int32_t n_rows, int32_t max_new_out, int32_t up, int32_t down, const float *taps, int32_t n_taps,
                               float *out_rings, int32_t n_out_slots, int32_t out_ring_samples, void *hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* MBEXWN_LIVE_RESAMPLE_H */
