/*
 * mbexwn_audio.h -- audio-side entry points of libmbexwn_hip.so (prefix mbxa_).
 *
 * They live in the same shared library as include/mbexwn.h, return the same mbx_status codes and leave their message in
 * the same thread-local mbx_last_error().  They are declared in a header of their own because the export list of mbexwn.h
 * (and with it MBX_ABI_VERSION) is pinned by the suite's contract tests; this header adds to the library without changing
 * that list.
 *
 * Conventions as in mbexwn.h: the caller owns all buffers, every pointer is a device pointer unless said otherwise, a call
 * only enqueues work on `hip_stream` (NULL: the default stream) of the CURRENT device, never allocates, never synchronises
 * and reads no environment variable.
 */
#ifndef MBEXWN_AUDIO_H
#define MBEXWN_AUDIO_H

#include "mbexwn.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Polyphase FIR resampling by up / down of a ragged batch (csrc/resample_poly.hip), indexed as scipy.signal.resample_poly:
 *
 *     half = (n_taps - 1) / 2
 *     out[b][k] = sum_j taps[k * down + half - j * up] * audio[b][j]          0 <= k < ceil(n_b * up / down)
 *
 * over 0 <= j < n_b with the tap index inside [0, n_taps).  The products k * down are 64-bit.
 *
 *   audio      (batch, max_samples) float32
 *   n_samples  (batch) int32 item lengths, or NULL: every item has max_samples.  An entry is clamped to [0, max_samples]
 *              in the kernel.
 *   taps       (n_taps) float32 in natural order, the gain `up` included (scipy's h = window * up)
 *   out        (batch, max_out) float32.  Item b writes exactly out[b][0 .. ceil(n_b * up / down)); the rest of its row
 *              is not touched, and an item with n_b = 0 writes nothing.
 *
 * An output sample is a float32 fmaf chain over ascending j: its bits depend on k, the item's samples and its length
 * alone -- not on the batch, on max_samples, on max_out or on the tile of the launch it falls in.
 *
 * Refused before any launch with MBX_ERR_INVALID_ARGUMENT: a NULL pointer other than n_samples; batch, up, down or n_taps
 * below 1; max_samples below 0; max_out < ceil(max_samples * up / down); more tiles than one launch can hold (2^31 - 1).
 */
mbx_status mbxa_resample_poly(const float *audio, const int32_t *n_samples, int32_t batch, int32_t max_samples,
                              int32_t up, int32_t down, const float *taps, int32_t n_taps,
                              float *out, int32_t max_out, void *hip_stream);

/* outputs per block of mbxa_resample_poly's launch (for tests that straddle a tile edge) */
#define MBXA_RESAMPLE_TILE 1024

#ifdef __cplusplus
}
#endif

#endif /* MBEXWN_AUDIO_H */
