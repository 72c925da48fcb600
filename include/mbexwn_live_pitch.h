/*
 * mbexwn_live_pitch.h -- streaming F0 tracking of libmbexwn_hip.so (prefix mbxt_): the tracker of include/mbexwn_pitch.h
 * for sounds that are still arriving (csrc/f0_stream.hip), on the ring store of include/mbexwn_live.h.  A live stream can
 * then sing with the pitch that is in the sound instead of the F0-net's guess.
 *
 * It lives in the same shared library as include/mbexwn.h and the other mbexwn_*.h headers, returns the same mbx_status
 * codes and leaves its message in the same thread-local mbx_last_error().  It is declared in a header of its own because the
 * export lists of the other headers (and MBX_ABI_VERSION) are pinned by the suite's contract tests; this header adds to the
 * library without changing those lists.
 *
 * Conventions as in mbexwn_live.h: no handle; the caller owns all buffers, every pointer is a device pointer; a call only
 * enqueues work on `hip_stream` (NULL: the default stream) of the CURRENT device, never allocates, never synchronises and
 * reads no environment variable.  The ring store is that header's: sample s of the stream in slot k lives at
 * rings[k][s & (ring_samples - 1)].
 *
 * THE PROMISE: f0 and periodicity of frame t of a stream, computed from a ring that holds the samples the frame reads, carry
 * exactly the bits mbxp_track_f0 gives at centre t * hop on the stream's whole sound with the same parameters -- both
 * kernels run the same device functions on the same sample values in the same order; only the fetch of a sample differs.
 * The rule "a frame that touches a sample that is not finite, or above 1e15 in magnitude, is unvoiced with periodicity 1" is
 * included.  For a stream that is still open this holds for every frame that ends at or before the newest sample:
 * (t * hop - L / 2 + L) <= samples appended, with L = window + tau_max.
 */
#ifndef MBEXWN_LIVE_PITCH_H
#define MBEXWN_LIVE_PITCH_H

#include "mbexwn.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * F0 and periodicity of the new frames of every stream of a tick, from the rings.  One 256-thread block per (stream, new
 * frame).
 *
 *   rings, n_slots, ring_samples   the ring store of mbexwn_live.h
 *   desc            (n_streams, 4) int64, one row per stream -- the table mbxl_mel_frames reads, so one upload serves both:
 *                     [0] slot         row of `rings`
 *                     [1] first_frame  index, in its stream, of the first frame to compute
 *                     [2] n_frames     frames to compute, at most max_new_frames; 0 (or less) computes nothing
 *                     [3] n_total      the stream's final length in samples once it is known, else any negative value
 *   hop             samples between the centres of neighbouring frames
 *   sample_rate, window, tau_min, tau_max, threshold, e_min: as for mbxp_track_f0 (mbexwn_pitch.h)
 *   f0, periodicity (n_streams, max_new_frames) float32 each; frame first_frame + i of row r of desc goes to [r][i].  Rows at
 *                   or behind a stream's n_frames are not written.
 *
 * Frame t = first_frame + i has centre c = t * hop, clamped to [0, n_total] once the length is known, and reads the samples
 * c - L / 2 + j, 0 <= j < L = window + tau_max, of its stream by absolute index.  An index below 0 is the value 0 and is
 * never fetched; with n_total >= 0 so is an index at or above n_total.  There is no reflection, as offline.  With n_total < 0
 * the stream is open and the caller asks for no frame that would read past the newest sample.  A row whose slot is outside
 * [0, n_slots) or whose first_frame is negative is skipped.
 *
 * Refused before any launch with MBX_ERR_INVALID_ARGUMENT and a message starting "f0 frames:": a NULL pointer (all but
 * hip_stream); n_streams outside [0, 65535]; max_new_frames below 0; n_slots below 1; hop below 1; sample_rate, window,
 * tau_min, tau_max, threshold or e_min that mbxp_track_f0 refuses; ring_samples not a power of two or below
 * window + tau_max.  n_streams == 0 or max_new_frames == 0 is nothing to do.
 */
mbx_status mbxt_f0_frames(const float *rings, int32_t n_slots, int32_t ring_samples, const int64_t *desc, int32_t n_streams,
                          int32_t max_new_frames, int32_t hop, int32_t sample_rate, int32_t window, int32_t tau_min,
                          int32_t tau_max, float threshold, float e_min, float *f0, float *periodicity, void *hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* MBEXWN_LIVE_PITCH_H */
