/*
 * mbexwn_limiter.h -- the look-ahead peak limiter of libmbexwn_hip.so (prefix mbxd_), on whole items and on the ring store
 * of live streams (csrc/limiter.hip).  The stage behind the level stage of mbexwn_level.h, or the last stage of a stream.
 *
 * It lives in the same shared library as include/mbexwn.h and the headers beside it, returns the same mbx_status codes and
 * leaves its message in the same thread-local mbx_last_error().  It is declared in a header of its own because the export
 * lists of the other headers (and MBX_ABI_VERSION) are pinned by the suite's contract tests.
 *
 * Conventions as in mbexwn_level.h: no handle; the caller owns all buffers; every pointer is a device pointer unless it is
 * called a HOST array below (read before the call returns, it travels in the kernel arguments); a call only enqueues work on
 * `hip_stream` (NULL: the default stream) of the CURRENT device, never allocates, never synchronises and reads no
 * environment variable.
 *
 * THE DEFINITION is mbexwn_vocoder_amd/limiter.py (its host functions), DESIGN.md section 6n.  In float32, every product
 * and every sum rounded on its own (no fused multiply-add), for an item x[0 .. n), a gain g0, a ceiling c, a window
 * 1 <= h <= hold and weights w[0 .. 2 h]:
 *
 *   u[k]    = x[k] * g0
 *   need[k] = c / d[k] (correctly rounded) where d[k] is finite and > c, else 1; 1 outside [0, n).  d[k] = |u[k]|, or, with
 *             taps, the maximum of the bit patterns of |u[k]| and |v[q]|, q in [4 k - 3, 4 k + 3] inside [0, 4 n), v the
 *             output of mbxa_resample_poly(up = 4, down = 1) on u with the same taps (that resampler's fmaf chain)
 *   m[i]    = min(need[k], k in [i - hold, i + h])
 *   g[i]    = 1 - acc;  acc from 0, for j = -h .. h ascending  acc = acc + w[j + h] * (1 - m[i + j])
 *   y[i]    = u[i] * g[i];  y > c gives c, y < -c gives -c (a NaN stays a NaN)
 *
 * Output i is a function of the samples [i - h - hold, i + 2 h] alone, the minimum is exact and the sum has a fixed order:
 * the tile, the launch shape and where the operands are staged move no bit.
 *
 * STATISTICS: MBXD_STAT_WORDS int32 per item -- [0] the smallest bit pattern, as a signed integer, of g (from that of
 * 1.0f), [1] the samples with g < 1, [2] the samples the clamp changed, [3] 0.  Integer atomics only.
 */
#ifndef MBEXWN_LIMITER_H
#define MBEXWN_LIMITER_H

#include "mbexwn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MBXD_STAT_WORDS 4
#define MBXD_TILE 2048         /* outputs per block */
/*
 * LDS words of a block: two spans of needs, the weights, the taps and the block's reductions,
 *   2 * (MBXD_TILE + 3 h + hold) + 1 + (2 h + 1) + n_taps + 16 <= MBXD_LDS_WORDS.
 * 64000 bytes: two blocks are resident in the 160 KB of a compute unit.  A longer window is refused.
 */
#define MBXD_LDS_WORDS 16000

/*
 * Limit every item of a batch.  One 256-thread block per (item, tile of MBXD_TILE outputs); a tile whose span holds no
 * need below 1 writes u (the same bits by the definition).
 *
 *   audio       (batch, stride) float32: item b is audio[b * stride .. b * stride + n_samples[b]); nothing behind an item's
 *               end is read
 *   n_samples   HOST array of `batch` counts, each in [0, min(stride, out_stride)]
 *   gains       float32 (batch): g0 of every item (what mbxl_gains writes)
 *   ceiling     c: finite, > 0
 *   h, hold     the window, 1 <= h <= hold
 *   weights     float32 (2 h + 1)
 *   taps        NULL, or float32 (n_taps): the taps of the 4x resampler already scaled by 4, as mbxl_measure takes them
 *   out         (batch, out_stride) float32; nothing behind an item's end is written.  `out` is either `audio` itself with
 *               out_stride == stride -- in place -- or does not overlap it
 *   stats       int32 (batch, MBXD_STAT_WORDS): set by this call
 *   workspace   in place only (else NULL is fine): workspace_floats >= mbxd_limit_workspace_floats(...) floats that do not
 *               overlap the audio.  A tile reads h + hold samples in front of itself and 2 h behind (n_taps / 4 + 2 more
 *               on either side with taps), and one launch cannot order those reads against its neighbours' stores: in place
 *               a launch in front of the limiter's saves them per (item, tile), and the limiter reads them from there.
 *               The operands and their order are the same, so in place gives the bits of out of place.
 *
 * Refused before any launch with MBX_ERR_INVALID_ARGUMENT (the message starts with "limit:"): batch < 0, a NULL pointer
 * (taps excepted), a negative stride, a count outside its range, a ceiling that is not finite and positive, a window outside
 * 1 <= h <= hold or too long for MBXD_LDS_WORDS, n_taps < 1 with taps, an `out` that overlaps `audio` without being it, in
 * place another out_stride, no workspace, one too small or one that overlaps the audio.  batch == 0 is nothing to do.
 */
mbx_status mbxd_limit(const float *audio, int64_t stride, int32_t batch, const int64_t *n_samples, const float *gains,
                      float ceiling, int32_t h, int32_t hold, const float *weights, const float *taps, int32_t n_taps,
                      float *out, int64_t out_stride, int32_t *stats, float *workspace, int64_t workspace_floats,
                      void *hip_stream);

/*
 * The floats of the workspace of mbxd_limit in place: batch * ceil(stride / MBXD_TILE) * (3 h + hold + 2 reach), reach = 0
 * without taps, else n_taps / 4 + 2.  0 for arguments mbxd_limit refuses.
 */
size_t mbxd_limit_workspace_floats(int64_t stride, int32_t batch, int32_t h, int32_t hold, int32_t n_taps);

/*
 * The same device function over a ring store laid out as mbexwn_live.h describes: `rings` (n_slots, ring_samples), sample j
 * of the stream in slot s at rings[s][j & (ring_samples - 1)], the length a power of two.  The output is packed rows.
 *
 *   desc        (n_rows, 6) int64, one row per stream:
 *                 [0] slot        row of `rings` (and of `stats`)
 *                 [1] first_out   index, in its stream, of the first output to produce
 *                 [2] n_new       outputs to produce; 0 (or less) produces nothing
 *                 [3] n_total     the stream's final length once it is known, else any negative value
 *                 [4] out_offset  where the row's outputs start in `out`, in floats
 *                 [5] the stream's g0 as float32 bits in the low 32 bits
 *   max_new     the largest n_new among the rows; it sizes the launch only
 *   stats       NULL, or int32 (n_slots, MBXD_STAT_WORDS): the row's statistics are merged into those of its slot (the
 *               caller sets a slot to {bits of 1.0f, 0, 0, 0} when a stream opens)
 *
 * Output i is final once the stream has i + 2 h + 1 samples, or is closed; the caller asks for no other output.  Output i
 * reads the samples [i - h - hold, i + 2 h] inside the stream: the caller keeps ring_samples large enough that none of
 * them has been overwritten.  Every ring access is masked with the ring's length.  A row whose slot is outside
 * [0, n_slots), whose first_out or out_offset is negative, whose first_out + n_new leaves 62 bits or whose
 * out_offset + n_new exceeds out_floats is skipped, not followed.  rings and out must not overlap.
 *
 * THE PROMISE: output i of a stream, from a ring that holds the samples it reads, carries the bits of output i of
 * mbxd_limit (taps NULL) on the stream's whole sound -- both kernels run one device function on the same operands in the
 * same order.
 *
 * Refused before any launch (the message starts with "limit emit:"): a NULL pointer (stats excepted); n_rows outside
 * [0, 65535]; max_new below 0; n_slots below 1; ring_samples not a power of two; out_floats below 0; the ceiling and the
 * window as for mbxd_limit.
 */
mbx_status mbxd_limit_emit(const float *rings, int32_t n_slots, int32_t ring_samples, const int64_t *desc, int32_t n_rows,
                           int32_t max_new, float ceiling, int32_t h, int32_t hold, const float *weights, float *out,
                           int64_t out_floats, int32_t *stats, void *hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* MBEXWN_LIMITER_H */
