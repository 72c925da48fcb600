/*
 * mbexwn_pitch.h -- F0 tracking of libmbexwn_hip.so (prefix mbxp_): the fundamental frequency of every analysis frame of a
 * sound, from the sound itself (csrc/f0_track.hip).  It is the independent source of the per-frame `f0` that the pitch
 * control of include/mbexwn.h takes: a contour that can be written to a file, edited, and given back to the synthesis, and
 * that does not share the octave errors of the model's own F0-net.
 *
 * It lives in the same shared library as include/mbexwn.h and the other mbexwn_*.h headers, returns the same mbx_status
 * codes and leaves its message in the same thread-local mbx_last_error().  It is declared in a header of its own because the
 * export lists of the other headers (and MBX_ABI_VERSION) are pinned by the suite's contract tests; this header adds to the
 * library without changing those lists.
 *
 * Conventions as in mbexwn_warp.h: no handle; the caller owns all buffers, every pointer is a device pointer; a call only
 * enqueues work on `hip_stream` (NULL: the default stream) of the CURRENT device, never allocates, never synchronises and
 * reads no environment variable.
 *
 * THE DEFINITION is mbexwn_vocoder_amd/f0track.py::track_f0_host (numpy float32), and the kernel gives
 * its bits: a YIN-type tracker.  With L = window + tau_max, the frame with centre c holds y[i] = x[c - L/2 + i] (0 outside
 * the item: no reflection, which would manufacture periodicity).  For every lag 1 <= tau <= tau_max the difference function
 * d[tau] sums (y[s + j] - y[s + tau + j])^2 over 0 <= j < window with s = (tau_max - tau) >> 1, so that both windows lie
 * symmetrically about the centre; d'[tau] = d[tau] tau / (d[1] + .. + d[tau]) is its cumulative-mean normalisation.  The
 * pick is the first lag in [max(tau_min, 2), tau_max - 1] with d' < threshold, walked on to the local minimum and refined by
 * a parabola through its neighbours; f0 = sample_rate / lag.  A frame without a pick, or whose energy over the window about
 * the centre is below e_min, or that touches a sample that is not finite (or above 1e15 in magnitude), has f0 = 0: unvoiced.
 * Every sum has one fixed order and every operation is one rounded float32 operation (no fused multiply-add).
 */
#ifndef MBEXWN_PITCH_H
#define MBEXWN_PITCH_H

#include "mbexwn.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * F0 and periodicity of a ragged batch at given centre samples: f0[b][k], periodicity[b][k] of the frame of item b centred
 * on centres[b][k], for 0 <= k < n_frames[b].
 *
 *   audio       (batch, stride) float32.  Item b is its first n_samples[b] samples; nothing behind them is read.
 *   n_samples   (batch) int32, clamped in the kernel to [0, stride].  An empty item is silence: unvoiced, periodicity 1.
 *   centres     (batch, max_frames) int64, clamped in the kernel to [0, n_samples[b]]: a wrong entry must not address outside
 *               the row.  Any order; equal neighbours repeat a frame.  The table of the mel analysis (t * hop, or the warped
 *               centres given to mbxw_mel_frames_at) puts the contour on the mel's frame grid.
 *   n_frames    (batch) int32: rows k >= n_frames[b] of the outputs are not written.  max_frames sizes the grid (one
 *               256-thread block per frame and item), so an entry above it counts as max_frames.
 *   sample_rate of the audio, in Hz
 *   window      the integration length W: a multiple of 64 in 64 .. 2048
 *   tau_min, tau_max   the lag range in samples: 0 <= tau_min, 2 <= tau_max, max(tau_min, 2) <= tau_max - 1, and
 *               window + tau_max <= 4096 (the frame stays in LDS)
 *   threshold   on d' (0.15 is the usual value; 0 or less: never a pick, periodicity is then the minimum of d')
 *   e_min       the least sum of squares of the W samples about the centre that a voiced frame has
 *   f0          (batch, max_frames) float32, Hz; 0 = unvoiced
 *   periodicity (batch, max_frames) float32: d' at the pick (or at its minimum without one); small = periodic, 1 = silence
 *
 * mbexwn_vocoder_amd/f0track.py::params derives window .. e_min from a frequency range.
 *
 * Refused before any launch with MBX_ERR_INVALID_ARGUMENT and a message starting "track f0:": a NULL pointer (all but
 * hip_stream); sample_rate < 1; a window, tau_min or tau_max outside the ranges above; a threshold or e_min that is NaN;
 * max_frames < 1, stride < 1; batch < 0 or batch > 65535.  batch == 0 is nothing to do.
 */
mbx_status mbxp_track_f0(const float *audio, int64_t stride, int32_t batch, const int32_t *n_samples,
                         const int64_t *centres, const int32_t *n_frames, int32_t max_frames,
                         int32_t sample_rate, int32_t window, int32_t tau_min, int32_t tau_max,
                         float threshold, float e_min, float *f0, float *periodicity, void *hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* MBEXWN_PITCH_H */
