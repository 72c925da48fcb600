/*
 * mbexwn_envelope.h -- the formant shift of libmbexwn_hip.so (prefix mbxe_): the spectral envelope a log-mel row describes,
 * moved along the frequency axis frame by frame (csrc/mel_envelope.hip): the kernel on its own (mbxe_warp_envelope), and the
 * forward pass with it (mbxe_forward), in which the VTF-net and the WaveNet conditioning read the warped rows while the F0-net
 * keeps the original ones, so that the formants move and the pitch contour keeps its bits.
 *
 * It lives in the same shared library as include/mbexwn.h and the other mbexwn_*.h headers, returns the same mbx_status
 * codes and leaves its message in the same thread-local mbx_last_error().  It is declared in a header of its own because the
 * export lists of the other headers (and MBX_ABI_VERSION) are pinned by the suite's contract tests; this header adds to the
 * library without changing those lists.  For the same reason the forward with a formant shift is an entry point of this header
 * and not three more fields of mbx_forward_options: the layout of that struct is pinned as well.
 *
 * Conventions of mbxe_warp_envelope as in mbexwn_audio.h: no handle; the caller owns all buffers, every pointer is a device pointer; a call only
 * enqueues work on `hip_stream` (NULL: the default stream) of the CURRENT device, never allocates, never synchronises and
 * reads no environment variable.
 *
 * THE DEFINITION (mbexwn_vocoder_amd/envelope.py::warp_envelope_host restates it in numpy float32 and
 * gives the same bits).  n = n_mels, c[0..n) = the channel centre frequencies in Hz, strictly increasing
 * (envelope.py::channel_centres).  A row x[0..n) of log amplitudes is an envelope that is linear in Hz between the points
 * (c[m], x[m]) and constant outside [c[0], c[n-1]].  For a frame with factor phi (finite, > 0; phi > 1 moves formants up) the
 * new row is the old envelope read at c[m] / phi:
 *
 *   phi == 1.0f:  out[m] = x[m], a copy without arithmetic.
 *   otherwise     f = c[m] / phi;  k = the number of centres <= f;
 *                 k == 0:  out[m] = x[0];    k == n:  out[m] = x[n-1];
 *                 else     i = k - 1,  w = (f - c[i]) / (c[i+1] - c[i]),  out[m] = x[i] + w * (x[i+1] - x[i]).
 *
 * Every operation is one correctly rounded IEEE float32 operation; no fused multiply-add, no log, no exp.  The overall level
 * is not compensated: a warp changes the energy of a frame.
 */
#ifndef MBEXWN_ENVELOPE_H
#define MBEXWN_ENVELOPE_H

#include "mbexwn.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The warped rows of a ragged batch: out[b][t][:] = row t of item b read at f / factors[b][t], for 0 <= t < n_frames[b]; the
 * rows at or behind n_frames[b] are copied unwarped, so that out is defined everywhere.
 *
 *   mel               (batch, max_frames, n_mels) float32; item b starts row_stride_items floats behind item b - 1
 *   row_stride_items  floats between the items of mel and of out (>= max_frames * n_mels; larger: a window of a longer buffer)
 *   n_frames          (batch) int32, clamped in the kernel to [0, max_frames]; NULL: every item has max_frames frames
 *   centres           (n_mels) float32 Hz, strictly increasing (not checked)
 *   factors           (batch, max_frames) float32, dense; finite and positive (not checked: a NaN reads x[0], nothing is
 *                     addressed outside a row).  Entries at or behind n_frames[b] are not read.
 *   out               laid out like mel; only the max_frames * n_mels floats of every item are written
 *
 * Refused before any launch with MBX_ERR_INVALID_ARGUMENT and a message starting "warp envelope:": a NULL pointer (all but
 * n_frames and hip_stream); n_mels < 2 or > 4096; max_frames < 1; row_stride_items < max_frames * n_mels; batch < 0 or
 * batch > 65535; out overlapping mel.  batch == 0 is nothing to do.
 */
mbx_status mbxe_warp_envelope(const float *mel, int64_t row_stride_items, int32_t batch, const int32_t *n_frames,
                              int32_t max_frames, int32_t n_mels, const float *centres, const float *factors, float *out,
                              void *hip_stream);

/*
 * mbx_forward_ex with a formant shift: every argument up to `options` as there (options may be NULL: a plain mbx_forward),
 * then
 *
 *   env_factor    device (batch, max_frames) factor per mel frame, > 1 moves formants up; NULL: none
 *   env_centres   device (mel_channels) centre frequencies of the mel channels in Hz, strictly increasing
 *   env_mel       device scratch of the caller, (batch, max_frames, mel_channels) with the strides of mel; it must not
 *                 overlap mel.  It is the caller's so that mbx_workspace_size and the workspace contract stay as they are.
 *
 * The mel-rate chains that describe the spectral envelope -- the VTF-net, the conditioning chain of the WaveNet and of every
 * further WaveNet block -- read the warped copy of the mel rows, the F0-net keeps reading the rows as they came (its float64
 * variant with its alignment rule included).  The warp runs behind the RMS normalisation, on the rows the chains read (the
 * normalised mel of an RMS-normalised model), over the whole window of max_frames frames in every call -- streaming windows
 * included: a frame's factor travels with the frame, so the rows a stream's front-end ring keeps (fe_store) are those of the
 * whole-utterance run.  Rows at or behind n_frames[b] are copied.  The stage "mel_env" (mbx_stage) is env_mel after such a
 * call, and unknown after a call without.  The overall level is not compensated.
 *
 * All three or none, otherwise MBX_ERR_INVALID_ARGUMENT.  With all three NULL the call is mbx_forward_ex (mbx_forward without
 * options): the same launches, the same bits.  Like the forwards of mbexwn.h it only enqueues work and can be captured.
 */
mbx_status mbxe_forward(mbx_handle *handle, const float *mel, const int32_t *n_frames, int32_t batch, int32_t max_frames,
                        const float *noise, float *audio, void *workspace, size_t workspace_bytes,
                        const mbx_forward_options *options, const float *env_factor, const float *env_centres, float *env_mel,
                        void *hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* MBEXWN_ENVELOPE_H */
