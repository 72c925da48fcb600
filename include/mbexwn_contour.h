/*
 * mbexwn_contour.h -- a decoded F0 contour of libmbexwn_hip.so (prefix mbxc_): Viterbi over YIN candidates
 * (csrc/f0_decode.hip).  mbxp_track_f0 of include/mbexwn_pitch.h decides every frame on its own, and one frame whose d' at
 * half the period dips below the threshold is an octave jump.  Here every frame offers up to seven lags and an "unvoiced"
 * state, and one path over the whole item is chosen.  The result has the shape and meaning of the tracker's: f0 in Hz per
 * frame, 0 = unvoiced, and a periodicity.
 *
 * It lives in the same shared library as include/mbexwn.h and the other mbexwn_*.h headers, returns the same mbx_status
 * codes and leaves its message in the same thread-local mbx_last_error().  It is declared in a header of its own because the
 * export lists of the other headers (and MBX_ABI_VERSION) are pinned by the suite's contract tests; this header adds to the
 * library without changing those lists.
 *
 * Conventions as in mbexwn_pitch.h: no handle; the caller owns all buffers, and every pointer is a device pointer EXCEPT
 * `thresholds` and `weights` of mbxc_f0_candidates, which are host pointers; a call only enqueues work on `hip_stream`
 * (NULL: the default stream) of the CURRENT device, never allocates, never synchronises and reads no environment variable.
 *
 * THE DEFINITION is mbexwn_vocoder_amd/f0decode.py (numpy float32): candidates_host and viterbi_host,
 * and the kernels give their bits.  It works like pYIN, but with linear costs, so that every operation is one rounded
 * float32 operation (no logarithm, no fused multiply-add) and every sum has one fixed order.
 *
 * Stage 1, per frame.  d', the energy E and the "bad" flag are the tracker's (mbexwn_pitch.h), lo = max(tau_min, 2), hi =
 * tau_max - 1.  A frame is usable if it is not bad and E >= e_min.  For every threshold theta_n, ascending, pick_n is the
 * tracker's pick with that threshold: the smallest lag in [lo, hi] with d' < theta_n, moved on while tau + 1 <= hi and
 * d'[tau + 1] < d'[tau]; none if the frame is not usable or no lag is below.  P[tau] is the float32 sum of weights[n] over
 * the n with pick_n == tau, added in ascending n; U the same over the n without a pick.  Every lag that is some pick_n is a
 * candidate.  The n_cand candidates with the largest P are kept (the smaller lag wins a tie) and listed by ascending lag in
 * slots 0 .. count - 1: period = float(tau) + off with the tracker's parabola and clamp, cost = max(1 - P, 0), dprime =
 * d'[tau].  An unused slot below 7 holds period 0, cost +inf, dprime 1.  Slot 7 is "unvoiced": period 0, cost = max(1 - U,
 * 0), dprime = d' at the first index of its minimum over [lo, hi], and 1 for a bad frame.
 *
 * Stage 2, per item of T frames.  Slot k < 7 of a frame is available iff 0 <= cost <= 1e6 and 1 <= period <= 1e6 (both
 * false for NaN); slot 7 always is, and its local cost is cost if 0 <= cost <= 1e6, else 0.  Frame 0: delta[j] = loc[j].
 * Frame t > 0, for every available j: v = delta[i] + tr(i, j) over the available i of frame t - 1 in ascending order, the
 * smallest kept with strict <, so the smallest i wins a tie; new[j] = best + loc[j].  Then m = min(new) over the available
 * slots and delta[j] = new[j] - m.  tr(i, j) = w_jump * (|p_j - p_i| / (p_j + p_i)) between two lags, 0 between two
 * unvoiced states, w_switch otherwise.  The last state is the smallest index of the minimum of delta; the back pointers
 * give the path.  f0 = float(sample_rate) / period, 0 for slot 7; periodicity is the slot's dprime.
 */
#ifndef MBEXWN_CONTOUR_H
#define MBEXWN_CONTOUR_H

#include "mbexwn.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Stage 1 for a ragged batch: the candidate tables of the frame of item b centred on centres[b][k], 0 <= k < n_frames[b].
 *
 *   audio .. e_min   as for mbxp_track_f0 (include/mbexwn_pitch.h), with the same clamps in the kernel: n_samples to
 *               [0, stride], centres to [0, n_samples[b]]; one 256-thread block per frame and item
 *   thresholds, weights   HOST pointers to n_thresholds floats each.  They are read and checked before the call returns and
 *               go to the kernel by value: the caller may free or change them as soon as the call is back.
 *   n_thresholds 1 .. 16
 *   n_cand      1 .. 7: the lags a frame keeps at most
 *   period, cost, dprime   (batch, max_frames, 8) float32 each.  Rows k >= n_frames[b] are not written.
 *
 * Refused before any launch with MBX_ERR_INVALID_ARGUMENT and a message starting "f0 candidates:": a NULL pointer (all but
 * hip_stream); everything mbxp_track_f0 refuses about the arguments the two share; n_thresholds outside 1 .. 16; thresholds
 * that are not finite and strictly ascending; weights that are not finite or negative; n_cand outside 1 .. 7.
 * batch == 0 is nothing to do.
 */
mbx_status mbxc_f0_candidates(const float *audio, int64_t stride, int32_t batch, const int32_t *n_samples,
                              const int64_t *centres, const int32_t *n_frames, int32_t max_frames,
                              int32_t sample_rate, int32_t window, int32_t tau_min, int32_t tau_max, float e_min,
                              const float *thresholds, const float *weights, int32_t n_thresholds, int32_t n_cand,
                              float *period, float *cost, float *dprime, void *hip_stream);

/*
 * Stage 2 for a ragged batch: one 64-lane wave per item walks its frames in order.
 *
 *   period, cost, dprime   (batch, max_frames, 8) float32: the tables of stage 1, or a caller's own.  Entries that are NaN,
 *               infinite, negative or above 1e6 make a slot unavailable (slot 7: its local cost 0); they never reach f0.
 *   n_frames    (batch) int32, clamped in the kernel to [0, max_frames].  An item with 0 frames writes nothing.
 *   max_frames  1 .. 16000: the back pointers of an item, 4 bytes per frame, stay in 64 000 bytes of LDS
 *   batch       0 .. 65535
 *   sample_rate of the audio the periods count samples of, in Hz
 *   w_jump, w_switch   the weights of tr(i, j), each in [0, 1e6]
 *   f0, periodicity   (batch, max_frames) float32.  Rows k >= n_frames[b] are not written.
 *
 * Refused before any launch with MBX_ERR_INVALID_ARGUMENT and a message starting "decode f0:": a NULL pointer (all but
 * hip_stream); max_frames < 1 or > 16000; batch < 0 or > 65535; w_jump or w_switch that is NaN, negative or above 1e6;
 * sample_rate < 1.  batch == 0 is nothing to do.
 */
mbx_status mbxc_decode_f0(const float *period, const float *cost, const float *dprime, const int32_t *n_frames,
                          int32_t max_frames, int32_t batch, int32_t sample_rate, float w_jump, float w_switch,
                          float *f0, float *periodicity, void *hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* MBEXWN_CONTOUR_H */
