/*
 * mbexwn_flac.h -- the compressing FLAC encoder of libmbexwn_hip.so (prefix mbxf_): fixed predictors of orders 0-4 with
 * partitioned Rice codes, on the device (csrc/flac_fixed.hip).
 *
 * It lives in the same shared library as include/mbexwn.h, include/mbexwn_audio.h, include/mbexwn_live.h and
 * include/mbexwn_live_resample.h, returns the same mbx_status codes and leaves its message in the same thread-local
 * mbx_last_error().  It is declared in a header of its own because the export lists of the other headers (and
 * MBX_ABI_VERSION) are pinned by the suite's contract tests; this header adds to the library without changing those lists.
 * mbx_encode_flac16 (mbexwn.h), the uncompressed encoder, is unchanged.
 *
 * Conventions as in mbexwn_audio.h: no handle; the caller owns all buffers, every pointer but `n_samples` is a device
 * pointer; a call only enqueues work on `hip_stream` (NULL: the default stream) of the CURRENT device, never allocates,
 * never synchronises and reads no environment variable.
 *
 * THE STREAM.  Mono, 16 bits, 4096-sample blocks, the last block shorter: frame headers, frame numbers, CRC-8 and CRC-16 as
 * mbx_encode_flac16 writes them.  Only the sub-frame behind the frame header differs, and with it the frame's length.  With
 * x[0..size) the int16 samples of a frame (clip(rint(double(audio) * 32767)), ties to even):
 *
 *   residual of order o at n >= o: the o-th finite difference of x; zigzag u = 2r for r >= 0, else -2r - 1
 *   partition order p = min(4, trailing zero bits of size), lowered while p > 0 and (size >> p) <= 4; partition 0 holds
 *     (size >> p) - o residuals, the others size >> p
 *   cost of a partition at Rice parameter k, 0 <= k <= 14: B(k) = sum (u >> k) + (k + 1) * count; the smallest B, ties to the
 *     smaller k
 *   cost of an order: T(o) = 16 o + 6 + sum over partitions (4 + min_k B), o = 0 .. min(4, size - 1); the smallest T, ties to
 *     the smaller o
 *   sub-frame: CONSTANT (byte 0x00, the 16-bit value) if all samples are equal; FIXED if T(o) < 16 size; else VERBATIM
 *     (byte 0x02, the samples in 16 bits each)
 *   FIXED, most significant bit first: the byte 0x10 + 2 o; o warm-up samples of 16 bits; 00; p in 4 bits; per partition k
 *     in 4 bits, then per residual u >> k zero bits, a one bit and the k low bits of u; zero bits up to the byte boundary
 *
 * then the CRC-16 of the frame.  No escape partition, no wasted bits and no 5-bit Rice parameter is ever written.  The bytes
 * are those of the host writer, mbexwn_vocoder_amd/flac.py::encode(..., compression="fixed"), behind its 42-byte header.
 */
#ifndef MBEXWN_FLAC_H
#define MBEXWN_FLAC_H

#include "mbexwn.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Encode the frames of a batch of mono items and pack them densely.
 *
 *   audio         (batch, stride) float32: item b is audio[b * stride .. b * stride + n_samples[b])
 *   n_samples     HOST array of `batch` counts, each in [0, min(stride, 2^28)]
 *   sample_rate   in (0, 2^20) Hz
 *   crc_tables    uint16 (256 + 16 * 16): the byte table of the CRC-16, then the columns of its shift operators
 *                 M_1, M_2, M_4, ... (what mbx_encode_flac16 takes; flac.py::crc16_device_tables)
 *   out           receives the frames of the whole batch back to back in (item, frame) order from out[0]: frame j of the
 *                 batch (items in order, every item's frames in order; item b has ceil(n_samples[b] / 4096) of them) spans
 *                 out[workspace[j] .. workspace[j] + frame_bytes[j])
 *   out_bytes     capacity of `out`.  It must cover the case that nothing compresses, the bytes mbx_encode_flac16 needs for
 *                 the same counts; a smaller value is refused.  Nothing behind the packed total is written.
 *   frame_bytes   int32, one entry per frame of the batch: receives every frame's length
 *   workspace     int64, 3 * frames + 1 entries, frames the number of frames of the batch: entries [0, frames] receive the
 *                 byte offset of every frame in `out` and, at [frames], the packed total; the rest carries the choices made
 *                 for every frame from the first pass to the second and holds nothing of use afterwards
 *   pcm_out       NULL, or int16 (batch, stride): receives the samples the frames hold, item b at pcm_out + b * stride,
 *                 n_samples[b] of them, little-endian as the device stores them (the MD5 of STREAMINFO is taken over them)
 *   max_abs       float32 (batch): max |x| of every item as mbx_encode_flac16 reports it (the maximum of the bit patterns of
 *                 |x|, so that a NaN item shows as NaN; such an item's frames hold nothing of use)
 *
 * Three passes, all enqueued by the one call: per frame the choices and the frame's length; an exclusive scan of the
 * lengths; per frame the bits, the CRC-16 and the write-out to the frame's (unaligned) place.
 *
 * Refused before any launch with MBX_ERR_INVALID_ARGUMENT: what mbx_encode_flac16 refuses, and a NULL frame_bytes or
 * workspace.  batch == 0 is nothing to do.
 */
mbx_status mbxf_encode_flac16_fixed(const float *audio, int64_t stride, int32_t batch, const int64_t *n_samples,
                                    int32_t sample_rate, const uint16_t *crc_tables, uint8_t *out, int64_t out_bytes,
                                    int32_t *frame_bytes, int64_t *workspace, int16_t *pcm_out, float *max_abs, void *hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* MBEXWN_FLAC_H */
