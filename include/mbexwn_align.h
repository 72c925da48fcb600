/*
 * mbexwn_align.h -- timing alignment of libmbexwn_hip.so (prefix mbxg_): dynamic time warping of two log-mel sequences
 * (csrc/mel_align.hip).  Given the log-mel of a guide and of a source it finds, for every frame of the guide, the frame of
 * the source that belongs there; the host turns that path into the centre samples mbxw_mel_frames_at (mbexwn_warp.h) takes,
 * and the source comes out with the guide's timing.
 *
 * It lives in the same shared library as include/mbexwn.h and the other mbexwn_*.h headers, returns the same mbx_status
 * codes and leaves its message in the same thread-local mbx_last_error().  It is declared in a header of its own because the
 * export lists of the other headers (and MBX_ABI_VERSION) are pinned by the suite's contract tests; this header adds to the
 * library without changing those lists.
 *
 * Conventions as in mbexwn_contour.h: no handle; the caller owns all buffers, and every pointer is a device pointer; a call
 * only enqueues work on `hip_stream` (NULL: the default stream) of the CURRENT device, never allocates, never synchronises
 * and reads no environment variable.  Batches are ragged: item b has n_frames_a[b] guide frames and n_frames_b[b] source
 * frames, clamped in the kernels to [0, max_frames_a] and [0, max_frames_b].
 *
 * THE DEFINITION is mbexwn_vocoder_amd/align.py (numpy): local_cost_host and path_host, and the kernels
 * give their bits.  Every float32 operation is one rounded operation (no fused multiply-add, no logarithm); THE SUM of M
 * values is four interleaved partial sums (x[m] goes to sum m % 4, ascending m, each from +0) combined (s0 + s1) + (s2 + s3).
 *
 * Features: F[t][m] = X[t][m] - SUM(X[t][:]) / float(M).  Local cost: d(i, j) = SUM_m |FA[i][m] - FB[j][m]|, quantised q =
 * rint((d < 2048 ? d : 2048) * 8), 0 .. 16384 (a NaN cost is 16384).  Band: c(i) = (i (Tb - 1) + (Ta - 1) / 2) / max(Ta - 1,
 * 1) in integers; cell (i, j) exists iff |j - c(i)| <= band.  Column o of row i of a band table is j = c(i) - band + o; a
 * column whose j lies outside [0, Tb) holds 65535.
 *
 * Recursion, int32: steps (1, 1), (1, 2), (2, 1) in (guide, source) frames.  D[0][0] = q[0][0]; D[i][j] = q[i][j] +
 * min(D[i-1][j-1], D[i-1][j-2], D[i-2][j-1]) over the predecessors that exist, the first of that order winning a tie; a cell
 * without one is unreachable.  The path is walked back from (Ta - 1, Tb - 1) to (0, 0).  An unreachable end -- the length
 * ratio is outside about [1/2, 2], or the band is too narrow -- gives count 0 and total -1.
 */
#ifndef MBEXWN_ALIGN_H
#define MBEXWN_ALIGN_H

#include "mbexwn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MBXG_MAX_FRAMES 65535 /* per item and side: at most 65535 nodes of at most 16384 each stay below 2^31 */
#define MBXG_MAX_BAND 511     /* mbxg_align_path: one thread per band cell, 2 band + 1 <= 1024 */
#define MBXG_MAX_MELS 240     /* mbxg_local_cost: 64 source rows and the guide row stay in 64 KiB of LDS */

/*
 * The quantised band costs of a ragged batch: one 64-lane wave per 64 band cells of a guide row.
 *
 *   mel_a       (batch, max_frames_a, n_mels) float32: the guides' log-mel
 *   mel_b       (batch, max_frames_b, n_mels) float32: the sources' log-mel
 *   n_frames_a, n_frames_b   (batch) int32
 *   batch       0 .. 65535
 *   max_frames_a, max_frames_b   1 .. 65535
 *   n_mels      1 .. 240
 *   band        1 .. 511 frames
 *   cost        (batch, max_frames_a, 2 band + 1) uint16.  Rows i >= n_frames_a[b] are not written; an item whose
 *               n_frames_b[b] is below 1 writes nothing.
 *
 * Refused before any launch with MBX_ERR_INVALID_ARGUMENT and a message starting "local cost:": a NULL pointer (all but
 * hip_stream) and every size outside the ranges above.  batch == 0 is nothing to do.
 */
mbx_status mbxg_local_cost(const float *mel_a, const float *mel_b, const int32_t *n_frames_a, const int32_t *n_frames_b,
                           int32_t batch, int32_t max_frames_a, int32_t max_frames_b, int32_t n_mels, int32_t band,
                           uint16_t *cost, void *hip_stream);

/*
 * The bytes of workspace mbxg_align_path needs: one byte of back pointer per band cell, batch * max_frames_a * (2 band + 1)
 * rounded up to a multiple of 4, and 4 bytes per guide frame for the nodes in walking order.  0 for an argument outside the
 * ranges of mbxg_align_path.
 */
size_t mbxg_align_workspace_size(int32_t batch, int32_t max_frames_a, int32_t band);

/*
 * The recursion and the walk back for a ragged batch: one block per item, one thread per band cell, one barrier per guide
 * row.
 *
 *   cost        (batch, max_frames_a, 2 band + 1) uint16: the table of mbxg_local_cost, or a caller's own with the same
 *               layout (values above 16384 other than 65535 are the caller's risk of an int32 overflow, not of a fault)
 *   n_frames_a, n_frames_b   (batch) int32
 *   batch       0 .. 65535
 *   max_frames_a   1 .. 65535
 *   band        1 .. 511
 *   workspace, workspace_bytes   at least mbxg_align_workspace_size(batch, max_frames_a, band) bytes, aligned to 4; its
 *               content before and after the call means nothing
 *   nodes_i, nodes_j   (batch, max_frames_a) int32: the nodes (i_k, j_k) of item b in ascending order in entries 0 ..
 *               count[b] - 1.  Entries from count[b] on are not written.
 *   count       (batch) int32: the nodes of the path; 0 for an item that cannot be aligned or has no frames
 *   total       (batch) int32: D at the end cell; -1 where count is 0
 *
 * Refused before any launch with MBX_ERR_INVALID_ARGUMENT and a message starting "align path:": a NULL pointer (all but
 * hip_stream), every size outside the ranges above, a workspace that is too small or not aligned to 4 bytes.  batch == 0
 * is nothing to do.
 */
mbx_status mbxg_align_path(const uint16_t *cost, const int32_t *n_frames_a, const int32_t *n_frames_b, int32_t batch,
                           int32_t max_frames_a, int32_t band, uint8_t *workspace, size_t workspace_bytes,
                           int32_t *nodes_i, int32_t *nodes_j, int32_t *count, int32_t *total, void *hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* MBEXWN_ALIGN_H */
