/*
 * mbexwn_live.h -- streaming audio-side entry points of libmbexwn_hip.so (prefix mbxl_): the mel analysis of sounds that
 * are still arriving (csrc/mel_stream.hip).
 *
 * They live in the same shared library as include/mbexwn.h and include/mbexwn_audio.h, return the same mbx_status codes
 * and leave their message in the same thread-local mbx_last_error().  They are declared in a header of their own because
 * the export lists of the other two headers (and MBX_ABI_VERSION) are pinned by the suite's contract tests; this header adds
 * to the library without changing those lists.
 *
 * Conventions as in mbexwn_audio.h: no handle; the caller owns all buffers, every pointer is a device pointer; a call only
 * enqueues work on `hip_stream` (NULL: the default stream) of the CURRENT device, never allocates, never synchronises and
 * reads no environment variable.
 *
 * The ring store: `rings` is (n_slots, ring_samples) float32, ring_samples a power of two.  Sample s (counted from the
 * start of its stream, 0-based) of the stream in slot k lives at rings[k][s & (ring_samples - 1)].  The caller decides which
 * stream owns which slot and keeps ring_samples large enough that no sample a frame still needs has been overwritten.
 *
 * THE PROMISE: row t of a stream, computed by mbxl_mel_frames from a ring that holds the samples frame t reads, carries
 * exactly the bits of row t of mbx_mel_analysis on the stream's whole sound with the same tables -- both kernels run one
 * device function on the same sample values in the same order.  For a stream that is still open this holds for every frame
 * whose window ends at or before the newest sample: (t * hop - win / 2 + win) <= samples appended.
 */
#ifndef MBEXWN_LIVE_H
#define MBEXWN_LIVE_H

#include "mbexwn.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Append the new samples of every stream of a tick to the rings.
 *
 *   packed          (packed_samples) float32: the new samples of all streams, back to back in any order
 *   desc            (n_streams, 4) int64, one row per stream:
 *                     [0] slot       row of `rings`
 *                     [1] abs_start  index, in its stream, of the first sample of this append
 *                     [2] count      samples to append; 0 (or less) writes nothing
 *                     [3] offset     of the stream's first new sample in `packed`
 *   max_count       the largest count among the rows; it sizes the launch only (a larger count is still appended whole)
 *   rings           (n_slots, ring_samples) float32
 *
 * Sample abs_start + i goes to rings[slot][(abs_start + i) & (ring_samples - 1)] for 0 <= i < min(count, ring_samples):
 * one call never writes more than ring_samples samples of a stream, and nothing outside the stream's own row.  A row whose
 * slot is outside [0, n_slots), whose abs_start is negative or whose samples do not lie inside `packed` is skipped.  Two
 * rows of one call must not name the same slot.
 *
 * Refused before any launch with MBX_ERR_INVALID_ARGUMENT: a NULL pointer; n_streams outside [0, 65535]; packed_samples or
 * max_count below 0; n_slots below 1; ring_samples not a power of two.
 */
mbx_status mbxl_ring_append(const float *packed, int64_t packed_samples, const int64_t *desc, int32_t n_streams,
                            int32_t max_count, float *rings, int32_t n_slots, int32_t ring_samples, void *hip_stream);

/*
 * Log-mel frames of every stream of a tick, from the rings.  One 256-thread block per (stream, new frame).
 *
 *   desc            (n_streams, 4) int64, one row per stream:
 *                     [0] slot         row of `rings`
 *                     [1] first_frame  index, in its stream, of the first frame to compute
 *                     [2] n_frames     frames to compute, at most max_new_frames; 0 (or less) computes nothing
 *                     [3] n_total      the stream's final length in samples once it is known, else any negative value
 *   win, hop, fft_size, n_mels, window, twiddle, basis, bin_lo, bin_hi, eps: as for mbx_mel_analysis (mbexwn.h)
 *   out             (n_streams, max_new_frames, n_mels) float32; frame first_frame + i of row r of desc goes to out[r][i].
 *                   Rows beyond a stream's n_frames are not written.
 *
 * Frame t reads the samples t * hop - win / 2 + j, 0 <= j < win, of its stream by absolute index.  With n_total >= 0 an
 * index outside [0, n_total) is reflected as numpy's "reflect" padding does, as often as it takes (n_total = 1 repeats the
 * one sample, n_total = 0 is one frame of silence): what mbx_mel_analysis does with an item of that length.  With
 * n_total < 0 the stream is open and only a negative index is folded (s -> -s); the caller asks for no frame that would read
 * past the newest sample.  A row whose slot is outside [0, n_slots) or whose first_frame is negative is skipped.
 *
 * Refused before any launch with MBX_ERR_INVALID_ARGUMENT: a NULL pointer; n_streams outside [0, 65535]; max_new_frames
 * below 0; n_slots below 1; fft_size not a power of two in [8, 2048]; win outside [2, fft_size]; hop or n_mels below 1;
 * ring_samples not a power of two or below win.
 */
mbx_status mbxl_mel_frames(const float *rings, int32_t n_slots, int32_t ring_samples, const int64_t *desc, int32_t n_streams,
                           int32_t max_new_frames, int32_t win, int32_t hop, int32_t fft_size, int32_t n_mels,
                           const float *window, const float *twiddle, const float *basis, const int32_t *bin_lo,
                           const int32_t *bin_hi, float eps, float *out, void *hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* MBEXWN_LIVE_H */
