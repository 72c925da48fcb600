/*
 * mbexwn_live_contour.h -- a decoded F0 contour for sounds that are still arriving, of libmbexwn_hip.so (prefix mbxv_): the
 * Viterbi decoder of include/mbexwn_contour.h with a FIXED LAG (csrc/f0_lag.hip), on the ring store of
 * include/mbexwn_live.h and the descriptor table of include/mbexwn_live_pitch.h.  Frame t of a stream is decided once frame
 * t + lag has been seen, by walking the back pointers from the best state of frame t + lag.
 *
 * It lives in the same shared library as include/mbexwn.h and the other mbexwn_*.h headers, returns the same mbx_status
 * codes and leaves its message in the same thread-local mbx_last_error().  It is declared in a header of its own because the
 * export lists of the other headers (and MBX_ABI_VERSION) are pinned by the suite's contract tests; this header adds to the
 * library without changing those lists.
 *
 * Conventions as in mbexwn_live_pitch.h: no handle; the caller owns all buffers, every pointer is a device pointer -- but
 * `thresholds` and `weights` of mbxv_f0_candidate_frames, which are HOST pointers; a call only enqueues work on `hip_stream`
 * (NULL: the default stream) of the CURRENT device, never allocates, never synchronises and reads no environment variable.
 *
 * THE DEFINITION is mbexwn_vocoder_amd/f0decode.py, in numpy float32: candidates_host for the tables, viterbi_lag_host for
 * the contour, LagDecoder for the state a stream keeps between calls.  Both entry points give its bits.
 *
 * A STREAM APPEARS IN AT MOST ONE ROW of the descriptor table of a launch: mbxv_decode_f0_frames advances the stream's state
 * row, one wave per row of the table, and two rows on one state would race.
 */
#ifndef MBEXWN_LIVE_CONTOUR_H
#define MBEXWN_LIVE_CONTOUR_H

#include "mbexwn.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The candidate tables of the new frames of every stream of a tick, from the rings.  One 256-thread block per (stream, new
 * frame).
 *
 *   rings, n_slots, ring_samples, desc, n_streams, max_new_frames, hop: as for mbxt_f0_frames (mbexwn_live_pitch.h); `desc`
 *                   is the (n_streams, 4) int64 table [slot, first_frame, n_frames, n_total] that mbxl_mel_frames reads too
 *   sample_rate, window, tau_min, tau_max, e_min, thresholds, weights, n_thresholds, n_cand: as for mbxc_f0_candidates
 *                   (mbexwn_contour.h); thresholds and weights are HOST pointers, read before the call returns
 *   period, cost, dprime   (n_streams, max_new_frames, 8) float32 each; frame first_frame + i of row r goes to [r][i][0 .. 7].
 *                   Rows at or behind a stream's n_frames are not written.
 *
 * THE PROMISE: the slot row [r][i] carries exactly the bits mbxc_f0_candidates gives at centre (first_frame + i) * hop on the
 * stream's whole sound with the same parameters -- both kernels run the same device functions on the same sample values in
 * the same order; only the fetch of a sample differs.  How a frame reads its samples, which rows are skipped (a slot outside
 * [0, n_slots), a negative first_frame) and when a frame of an open stream is ready are the rules of mbxt_f0_frames.
 *
 * Refused before any launch with MBX_ERR_INVALID_ARGUMENT and a message starting "f0 candidate frames:": a NULL pointer (all
 * but hip_stream); whatever mbxt_f0_frames refuses of the arguments the two share; n_thresholds outside 1 .. 16; n_cand
 * outside 1 .. 7; thresholds that are not finite and strictly ascending; weights that are not finite or negative.
 * n_streams == 0 or max_new_frames == 0 is nothing to do.
 */
mbx_status mbxv_f0_candidate_frames(const float *rings, int32_t n_slots, int32_t ring_samples, const int64_t *desc,
                                    int32_t n_streams, int32_t max_new_frames, int32_t hop, int32_t sample_rate, int32_t window,
                                    int32_t tau_min, int32_t tau_max, float e_min, const float *thresholds, const float *weights,
                                    int32_t n_thresholds, int32_t n_cand, float *period, float *cost, float *dprime,
                                    void *hip_stream);

/*
 * The 32-bit words of one stream's decoder state: 32 words of counters, delta and the last frame's periods and costs, then a
 * ring of 256 frames of 17 words (the pointer word with the frame's best state, 8 periods, 8 dprimes).
 */
size_t mbxv_lag_state_words(void);

/*
 * Continue the Viterbi recursion of every stream of a tick over its new frames and hand out the frames that became decided.
 * One 64-lane wave per row of `desc`.
 *
 *   period, cost, dprime   (n_streams, max_new_frames, 8) float32: the tables of mbxv_f0_candidate_frames of the same tick,
 *                   or any tables of that shape
 *   desc            the (n_streams, 4) int64 table; row r advances its stream by n = clamp(desc[r][2], 0, max_new_frames)
 *                   frames, read from [r][0 .. n)
 *   state           (n_slots, mbxv_lag_state_words()) 32-bit words; row desc[r][0] belongs to the stream of row r.  A
 *                   zero-filled row is a stream with no frame yet: zero a slot's row when a stream takes it
 *   lag             frames of look-ahead, 0 .. 128; the same value in every call of a stream
 *   sample_rate, w_jump, w_switch: as for mbxc_decode_f0 (mbexwn_contour.h)
 *   f0, periodicity (n_streams, max_out) float32 each, max_out >= max_new_frames + lag: the frames of row r that became
 *                   decided go to [r][0 ..], in order.  Entries behind the decided count are not written.
 *
 * With `done` the frames a stream has seen after the call, the decided frames are those below done - lag; if the stream is
 * final -- desc[r][3] >= 0 and desc[r][1] + n >= desc[r][3] / hop + 1 -- all of them.  The caller knows the count from the
 * same rule (f0decode.lag_frames_decided); it is at most n + lag.  Frame t takes the state the back pointers lead to from
 * the best state of frame min(t + lag, done - 1).  There is no limit on the frames of a stream or of a call: nothing but the
 * ring is kept.
 *
 * A row is skipped, its state and outputs untouched, if its slot is outside [0, n_slots), if first_frame is negative (or
 * above INT32_MAX - max_new_frames), or if first_frame is not the `done` of the state.
 *
 * Refused before any launch with MBX_ERR_INVALID_ARGUMENT and a message starting "decode f0 frames:": a NULL pointer (all
 * but hip_stream); n_streams outside [0, 65535]; max_new_frames below 0; hop below 1; n_slots below 1; lag outside 0 .. 128;
 * max_out below max_new_frames + lag; w_jump or w_switch outside [0, 1e6] (or NaN); sample_rate below 1.  n_streams == 0 is
 * nothing to do; max_new_frames == 0 still decides the frames of a stream that became final.
 */
mbx_status mbxv_decode_f0_frames(const float *period, const float *cost, const float *dprime, const int64_t *desc,
                                 int32_t n_streams, int32_t max_new_frames, int32_t hop, void *state, int32_t n_slots,
                                 int32_t lag, int32_t sample_rate, float w_jump, float w_switch, float *f0, float *periodicity,
                                 int32_t max_out, void *hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* MBEXWN_LIVE_CONTOUR_H */
