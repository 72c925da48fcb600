// The FLAC frame of 16-bit mono audio, once: what flac_frames.hip (VERBATIM sub-frames) and flac_fixed.hip (CONSTANT, FIXED
// and VERBATIM sub-frames) share, so that the two encoders cannot drift apart -- as mel_frame.h is the one body of the two mel
// analyses.  Both run one 256-thread block per (frame, item), which
//   1. loads the frame's samples (coalesced), quantises them as flac.to_pcm16 does -- clip(rint(double(x) * 32767)), ties
//      to even; the product is exact in float64 -- into LDS, and takes max |x| on the bit pattern of |x| (so that a NaN
//      stays a NaN and the host can see it): load_pcm;
//   2. assembles the frame in an LDS image shifted by the frame's address mod 16, the header with its CRC-8 by thread 0
//      (frame_header); what follows the header is the encoder's own;
//   3. computes the CRC-16 of the frame: every thread the CRC of its own run of bytes, joined by a log-depth combine
//      (crc16_join) -- with init 0 and no final XOR the CRC is linear over GF(2), crc(A || B) = M_|B| crc(A) ^ crc(B),
//      where M_n advances the register over n zero bytes; M_n is the product of the operators M_{2^k} of the set bits of n
//      (host-built, flac.py::crc16_device_tables);
//   4. writes the frame out (write_frame): aligned 16-byte stores inside it, byte stores for the partial 16-byte words at
//      its two ends, which it shares with the neighbouring frames (written by other blocks at the same time; frames are
//      not aligned, their lengths vary).
#pragma once
#include "mbx_kernels.h"

namespace mbx {

constexpr int FT = FLAC_THREADS;
constexpr int PER = FLAC_BLOCK / FT;                        // consecutive samples per thread
// longest frame: 4 sync/code bytes + 3-byte frame number + 16-bit block size + CRC-8 + sub-frame byte + 2 * 4096 + CRC-16
constexpr int MAX_FRAME_BYTES = 4 + 3 + 2 + 1 + 1 + 2 * FLAC_BLOCK + 2;
constexpr int FRAME_WORDS = (15 + MAX_FRAME_BYTES + 15) / 16;   // LDS frame image, shifted by the frame's address mod 16

static_assert(FLAC_BLOCK % FT == 0 && PER == 16, "16 consecutive samples (one 32-byte run) per thread");

__host__ __device__ inline int frame_number_bytes(long long f) { return f < 128 ? 1 : (f < 2048 ? 2 : 3); }

// bytes of the header of frame f (`size` samples), its CRC-8 included
__host__ __device__ inline int frame_header_bytes(long long f, int size) {
    return 4 + frame_number_bytes(f) + (size != FLAC_BLOCK ? 2 : 0) + 1;
}

__device__ inline int quantise(float v) {
    return (int)fmin(fmax(rint((double)v * 32767.0), -32768.0), 32767.0);
}

// the frame's `size` samples at x into LDS (and to `keep`, unless null); -> this thread's max |x|, as the bit pattern of |x|
__device__ inline uint32_t load_pcm(const float *x, int size, int16_t *pcm, int16_t *keep) {
    uint32_t mx = 0;
    for (int i = threadIdx.x; i < size; i += FT) {
        const float v = x[i];
        mx = max(mx, __float_as_uint(v) & 0x7FFFFFFFu);
        const int16_t q = (int16_t)quantise(v);
        pcm[i] = q;
        if (keep) keep[i] = q;
    }
    return mx;
}

// crc_tables (CRC-16 byte table, then FLAC_CRC_SHIFTS x 16 operator columns) into LDS
__device__ inline void stage_crc_tables(const uint16_t *crc_tables, uint16_t *table, uint16_t *ops) {
    for (int i = threadIdx.x; i < 256; i += FT) table[i] = crc_tables[i];
    for (int i = threadIdx.x; i < 16 * FLAC_CRC_SHIFTS; i += FT) ops[i] = crc_tables[256 + i];
}

__device__ inline uint32_t crc16_byte(uint32_t crc, uint32_t byte, const uint16_t *table) {
    return ((crc << 8) & 0xFFFFu) ^ table[(crc >> 8) ^ byte];
}

// M_n crc: the operators of the set bits of n (powers of one matrix: they commute)
__device__ inline uint32_t crc16_shift(uint32_t crc, uint32_t n, const uint16_t *ops) {
    for (int k = 0; n != 0u && k < FLAC_CRC_SHIFTS; ++k, n >>= 1) {
        if (!(n & 1u)) continue;
        const uint16_t *col = ops + 16 * k;
        uint32_t r = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) r ^= (0u - ((crc >> j) & 1u)) & col[j];
        crc = r;
    }
    return crc;
}

// The header of frame f (`size` samples) with its CRC-8 into h (up to 10 bytes); -> its byte count.
__device__ inline int frame_header(uint8_t *h, long long f, int size, int rate_code) {
    const bool short_block = size != FLAC_BLOCK;
    const int nb = frame_number_bytes(f);
    int k = 0;
    h[k++] = 0xFF;
    h[k++] = 0xF8;                                          // sync, fixed block size
    h[k++] = (uint8_t)(((short_block ? 7 : 12) << 4) | rate_code);
    h[k++] = 0x08;                                          // one channel, 16 bits per sample
    const int fi = (int)f;
    if (nb == 1) {
        h[k++] = (uint8_t)fi;
    } else if (nb == 2) {
        h[k++] = (uint8_t)(0xC0 | (fi >> 6));
        h[k++] = (uint8_t)(0x80 | (fi & 63));
    } else {
        h[k++] = (uint8_t)(0xE0 | (fi >> 12));
        h[k++] = (uint8_t)(0x80 | ((fi >> 6) & 63));
        h[k++] = (uint8_t)(0x80 | (fi & 63));
    }
    if (short_block) {
        h[k++] = (uint8_t)((size - 1) >> 8);
        h[k++] = (uint8_t)((size - 1) & 255);
    }
    uint32_t c8 = 0;                                        // CRC-8, poly 0x07, init 0
    for (int i = 0; i < k; ++i) {
        c8 ^= h[i];
        for (int b = 0; b < 8; ++b) c8 = (c8 & 0x80u) ? ((c8 << 1) ^ 0x07u) & 0xFFu : (c8 << 1) & 0xFFu;
    }
    h[k++] = (uint8_t)c8;
    return k;
}

// Joins the threads' runs -- thread t holds the CRC `crc` of its `len` bytes, the runs in thread order -- into the frame's
// CRC-16 and writes it, big-endian, at crc_at: a log-depth combine inside the wave (lane i joins lane i + off, the run to
// its right, at every level), then thread 0 folds the waves' parts onto `start`, the CRC of the bytes in front of the runs
// (read on thread 0 only).  One barrier, between the two; part_crc and part_len: FT / 64 words of LDS each.
__device__ inline void crc16_join(uint32_t crc, uint32_t len, uint32_t start, const uint16_t *ops, uint32_t *part_crc,
                                  uint32_t *part_len, uint8_t *crc_at) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t cr = __shfl_down(crc, off), lr = __shfl_down(len, off);
        if ((lane & (2 * off - 1)) == 0) {
            crc = crc16_shift(crc, lr, ops) ^ cr;
            len += lr;
        }
    }
    if (lane == 0) {
        part_crc[wave] = crc;
        part_len[wave] = len;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = start;
        for (int wv = 0; wv < FT / 64; ++wv) total = crc16_shift(total, part_len[wv], ops) ^ part_crc[wv];
        crc_at[0] = (uint8_t)(total >> 8);
        crc_at[1] = (uint8_t)(total & 255u);
    }
}

// The frame image (byte k of the frame at byte lead + k of frame_words, lead = dst & 15) to dst: the 16-byte words that lie
// inside the frame whole, the two edge words byte by byte.
__device__ inline void write_frame(uint8_t *dst, int lead, int flen, const uint4 *frame_words) {
    const uint8_t *img = reinterpret_cast<const uint8_t *>(frame_words);
    const int span = lead + flen, words = (span + 15) / 16;
    uint8_t *base = dst - lead;
    for (int wd = threadIdx.x; wd < words; wd += FT) {
        const int lo = 16 * wd, hi = lo + 16;
        if (lo >= lead && hi <= span) {
            reinterpret_cast<uint4 *>(base)[wd] = frame_words[wd];
        } else {
            for (int k = max(lo, lead); k < min(hi, span); ++k) base[k] = img[k];
        }
    }
}

}  // namespace mbx
