/*
 * mbexwn_level.h -- level control of whole items in libmbexwn_hip.so (prefix mbxl_, shared with the ring entry points of
 * mbexwn_live.h; no name occurs twice): ITU-R BS.1770 integrated loudness, sample and 4x true peak, one static gain per
 * item, on the device (csrc/level.hip).  The stage between the forward, or the output resampler, and the FLAC encoders.
 *
 * It lives in the same shared library as include/mbexwn.h and the headers beside it, returns the same mbx_status codes and
 * leaves its message in the same thread-local mbx_last_error().  It is declared in a header of its own because the export
 * lists of the other headers (and MBX_ABI_VERSION) are pinned by the suite's contract tests.
 *
 * Conventions as in mbexwn_flac.h: no handle; the caller owns all buffers; every pointer is a device pointer unless it is
 * called a HOST pointer or a HOST array below (those are read before the call returns and travel in the kernel arguments,
 * so nothing small has to be uploaded); a call only enqueues work on `hip_stream` (NULL: the default stream) of the CURRENT
 * device, never allocates, never synchronises and reads no environment variable.
 *
 * THE DEFINITION is mbexwn_vocoder_amd/level.py (its host functions), DESIGN.md section 6m.  In float64, every product and
 * every sum rounded on its own (no fused multiply-add):
 *
 *   hop energies    item b has H = n_samples[b] / hops[b] hops (integer division; the tail is not measured).  Hop h is
 *                   filtered on its own: from zero state 2 * hop samples in front of its first sample (zeros in front of
 *                   the item), two biquads in transposed direct form II on x = (double)sample,
 *                     y = b0 x + s1;  s1 = (b1 x - a1 y) + s2;  s2 = b2 x - a2 y
 *                   the first (coefficients 0-4 of the item's row: b0 b1 b2 a1 a2) feeding the second (5-9);
 *                   e[h] = sum of y^2 of the second over the hop's own samples, ascending, from 0
 *   block powers    z[j] = (((e[j] + e[j+1]) + e[j+2]) + e[j+3]) / (4 hop),  j = 0 .. H - 4
 *   gates           absolute z > *abs_gate; relative z > 0.1 * (ascending sum of the absolutely gated z / their number)
 *   P, count        the ascending sum of the z that pass both gates / their number `count`; count == 0: P = 0
 *   sample peak     max |x| as the maximum of the bit patterns of |x| (a NaN item shows as NaN), 0 for no samples
 *   true peak       the maximum (of bit patterns) of the sample peak and of |y[k]|, 0 <= k < 4 n, y the output of
 *                   mbxa_resample_poly(up = 4, down = 1) with the same taps: the fmaf chain of that resampler, never stored
 *   gain            g = 1 for a NaN or zero peak.  Else g = sqrt(Pt / P) for a target Pt > 0 and count > 0, P > 0, else 1;
 *                   if g * (double)peak > ceiling then g = ceiling / (double)peak; rounded to float32
 *   apply           out = audio * g, one float32 product per sample
 *
 * A RECORD is MBXL_RECORD_BYTES bytes, 8-byte aligned: double P at byte 0; int32 count at 8; int32 number of absolutely
 * gated blocks at 12; float sample peak at 16; float true peak at 20 (the sample peak when no taps were given).
 */
#ifndef MBEXWN_LEVEL_H
#define MBEXWN_LEVEL_H

#include "mbexwn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MBXL_RECORD_BYTES 24
#define MBXL_COEF_DOUBLES 10   /* per item: b0 b1 b2 a1 a2 of the first biquad, then of the second */
#define MBXL_MAX_TAPS 8192     /* the 4x filter is staged in LDS */

/*
 * Measure every item of a batch.
 *
 *   audio         (batch, stride) float32: item b is audio[b * stride .. b * stride + n_samples[b]); nothing behind an
 *                 item's end is read
 *   n_samples     HOST array of `batch` counts, each in [0, stride]
 *   hops          HOST array of `batch` hop lengths in samples, each in [1, 2^28] (a batch may mix rates)
 *   coefs         HOST array double (batch, MBXL_COEF_DOUBLES): the item's filter coefficients
 *   abs_gate      HOST pointer to the absolute gate as a power
 *   taps          NULL (no true peak), or float32 (n_taps): the taps of the 4x resampler, already scaled by 4 (what
 *                 mbxa_resample_poly takes); 1 <= n_taps <= MBXL_MAX_TAPS.  The design depends on the ratio alone, so one
 *                 set serves every rate of the batch.
 *   workspace     double (batch, 2, hops_cap): receives e of item b at [b][0][0 .. H) and z at [b][1][0 .. H - 3); the
 *                 rest is not written
 *   hops_cap      row length of the workspace, >= 1; an item with more hops is refused (the workspace is too small)
 *   records       batch records (above)
 *
 * Three kernels: the hop energies, one thread per hop (a dependent chain of 3 * hop steps); the peaks, one block per tile of
 * 4096 samples, reduced as a maximum of non-negative bit patterns so that the launch geometry cannot change the result; per
 * item the block powers and the two gates.
 *
 * Refused before any launch with MBX_ERR_INVALID_ARGUMENT: batch < 0, a NULL pointer (taps excepted), stride < 0, a count
 * outside [0, stride], a hop outside [1, 2^28], hops_cap < 1 or smaller than an item's hops, n_taps outside its range when taps is given.
 * batch == 0 is nothing to do.
 */
mbx_status mbxl_measure(const float *audio, int64_t stride, int32_t batch, const int64_t *n_samples, const int32_t *hops,
                        const double *coefs, const double *abs_gate, const float *taps, int32_t n_taps, double *workspace,
                        int32_t hops_cap, void *records, void *hip_stream);

/*
 * One gain per item from its record, on the device.
 *
 *   records         batch records of mbxl_measure
 *   targets         HOST array double (batch): the target power of item b; a value that is not > 0: no target
 *   target_records  NULL, or batch records of another measurement: item b then takes the P of record b as its target where
 *                   that record has count > 0, and no target where it has not, whatever targets[b] says
 *   ceiling         HOST pointer to the linear ceiling, or NULL for none
 *   true_peak       0: the gain is limited by the sample peak; else by the true peak
 *   gains           float32 (batch): receives the gains
 *
 * One launch per 32 items.  Refused before any launch: batch < 0, a NULL records, targets or gains, a ceiling that is not > 0.  batch == 0 is nothing to do.
 */
mbx_status mbxl_gains(const void *records, int32_t batch, const double *targets, const void *target_records,
                      const double *ceiling, int32_t true_peak, float *gains, void *hip_stream);

/*
 * out[b * out_stride + i] = audio[b * stride + i] * gains[b] for 0 <= i < n_samples[b].  `out` may be `audio` (with
 * out_stride == stride): in place.  Nothing behind an item's end is read or written.
 *
 * Refused before the launch: batch < 0, a NULL pointer, a negative stride, a count outside [0, min(stride, out_stride)], an
 * `out` that is `audio` with another stride.  batch == 0 is nothing to do.
 */
mbx_status mbxl_apply(const float *audio, int64_t stride, int32_t batch, const int64_t *n_samples, const float *gains,
                      float *out, int64_t out_stride, void *hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* MBEXWN_LEVEL_H */
