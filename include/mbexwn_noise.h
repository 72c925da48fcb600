/*
 * mbexwn_noise.h -- keyed normal noise of libmbexwn_hip.so (prefix mbxn_): the N(0,1) draw of the model's noise channel as
 * a pure function of (seed, item key, absolute WaveNet step), on the device (csrc/noise_keyed.hip).
 *
 * It lives in the same shared library as include/mbexwn.h and the other mbexwn_*.h headers, returns the same mbx_status
 * codes and leaves its message in the same thread-local mbx_last_error().  It is declared in a header of its own because the
 * export lists of the other headers (and MBX_ABI_VERSION) are pinned by the suite's contract tests; this header adds to the
 * library without changing those lists.  mbexwn.h does not change: the noise stays an input of the forward.
 *
 * Conventions as in mbexwn_audio.h: no handle; the caller owns all buffers, every pointer is a device pointer; a call only
 * enqueues work on `hip_stream` (NULL: the default stream) of the CURRENT device, never allocates, never synchronises and
 * reads no environment variable.
 *
 * THE DEFINITION.  Value s of an item (s >= 0, the absolute step: the index of the value in the item's whole draw) belongs to
 * quad q = s >> 2, lane j = s & 3.
 *
 *   1. (x0, x1, x2, x3) = Philox4x32-10 of the counter (q & 0xFFFFFFFF, q >> 32, 0, 0) under the key (k0, k1), with
 *      k = seed ^ (item_key * 0x9E3779B97F4A7C15 mod 2^64), k0 its low and k1 its high 32 bits.  Philox4x32-10 is the
 *      published function (Salmon et al., SC'11; Random123): ten rounds of
 *          (c0, c1, c2, c3) <- (hi(M1 * c2) ^ c1 ^ k0, lo(M1 * c2), hi(M0 * c0) ^ c3 ^ k1, lo(M0 * c0))
 *      with M0 = 0xD2511F53, M1 = 0xCD9E8D57 and, between rounds, k0 += 0x9E3779B9, k1 += 0xBB67AE85 (mod 2^32).
 *   2. u(x) = (float(x >> 9) + 0.5f) * 2^-23.  The sum has at most 24 significant bits, so u is exact in float32 and lies in
 *      [2^-24, 1 - 2^-24], strictly inside (0, 1).
 *   3. Two Box-Muller pairs in float32: r = sqrtf(-2 logf(u(x0))), t = 6.283185307179586f * u(x1) give lane 0 = r cosf(t) and
 *      lane 1 = r sinf(t); (x2, x3) give lanes 2 and 3 the same way.
 *
 * The integer part (1., and the numerator of 2.) is exact and mirrored on the host bit for bit
 * (mbexwn_vocoder_amd/noise.py).  The float part exists on the device only: its bits are what the device's logf, sqrtf, sinf
 * and cosf give, and they are the same wherever the value is asked for, because a thread always computes a whole quad and
 * stores the lanes that fall inside the window asked for.  A window [first, first + count) of an item therefore holds
 * exactly the bits of the same steps of the whole item's fill, in any batch, at any stride, in any row.
 */
#ifndef MBEXWN_NOISE_H
#define MBEXWN_NOISE_H

#include "mbexwn.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Fill a ragged batch of rows with keyed N(0,1) values: out[b * stride + i] = value (first_step[b] + i) of the item with
 * keys[b], for 0 <= i < counts[b].
 *
 *   out         (batch, stride) float32.  Nothing behind counts[b] of a row is written, nor anything outside the rows.
 *   keys        (batch, 2) uint64: seed, item key
 *   first_step  (batch) int64, or NULL = 0: the absolute step of out[b * stride].  A row with a negative entry is skipped:
 *               nothing of it is written.
 *   counts      (batch) int32: values to write, clamped in the kernel to [0, min(stride, max_count)]
 *   max_count   HOST bound of counts[]: it sizes the grid (one 256-thread block per item and MBXN_FILL_TILE values)
 *
 * Stores are float4 where the address of a whole quad inside the window is 16-byte aligned, scalar otherwise.
 *
 * Refused before any launch with MBX_ERR_INVALID_ARGUMENT and a message starting "fill normal:": a NULL out, keys or counts;
 * a negative batch, stride or max_count; max_count > stride; more tiles than one launch can hold (2^31 - 1).  batch == 0 and
 * max_count == 0 are nothing to do.
 */
mbx_status mbxn_fill_normal(float *out, int64_t stride, int32_t batch, const uint64_t *keys, const int64_t *first_step,
                            const int32_t *counts, int32_t max_count, void *hip_stream);

/* values per block of mbxn_fill_normal's launch (for tests that straddle a tile edge) */
#define MBXN_FILL_TILE 4096

#ifdef __cplusplus
}
#endif

#endif /* MBEXWN_NOISE_H */
