// FLAC frames of 16-bit mono audio on the device: everything behind the 42-byte "fLaC" + STREAMINFO header that the host
// writer mbexwn_vocoder_amd/flac.py::encode emits (4096-sample blocks, VERBATIM sub-frames), byte for byte.
//
// One 256-thread block per (frame, item).  The block
//   1. loads the frame's samples (coalesced), quantises them as flac.to_pcm16 does -- clip(rint(double(x) * 32767)),
//      ties to even; the product is exact in float64 -- into LDS, and reduces max |x| on the bit pattern of |x| (so that a
//      NaN stays a NaN and the host can see it);
//   2. assembles the frame in LDS: header + CRC-8 (thread 0), sub-frame byte 0x02, big-endian samples (16 per thread);
//   3. computes the CRC-16 of the frame: every thread the CRC of its own run of up to 32 bytes, joined by a log-depth
//      combine -- with init 0 and no final XOR the CRC is linear over GF(2), crc(A || B) = M_|B| crc(A) ^ crc(B), where
//      M_n advances the register over n zero bytes; M_n is the product of the operators M_{2^k} of the set bits of n
//      (host-built, flac.py::crc16_device_tables);
//   4. writes the frame out: aligned 16-byte stores inside it, byte stores for the partial 16-byte words at its two ends,
//      which it shares with the neighbouring frames (written by other blocks at the same time; frames are not aligned,
//      their header lengths vary).
// Bandwidth-type: reads 4 B and writes about 2 B per sample.
#include "mbx_kernels.h"

namespace mbx {

namespace {

constexpr int FT = FLAC_THREADS;
constexpr int PER = FLAC_BLOCK / FT;                        // samples per thread in the CRC / byte stage
// longest frame: 4 sync/code bytes + 3-byte frame number + 16-bit block size + CRC-8 + sub-frame byte + 2 * 4096 + CRC-16
constexpr int MAX_FRAME_BYTES = 4 + 3 + 2 + 1 + 1 + 2 * FLAC_BLOCK + 2;
constexpr int FRAME_WORDS = (15 + MAX_FRAME_BYTES + 15) / 16;   // LDS frame image, shifted by the frame's address mod 16

static_assert(FLAC_BLOCK % FT == 0 && PER == 16, "one 32-byte run per thread");

__host__ __device__ inline int frame_number_bytes(long long f) { return f < 128 ? 1 : (f < 2048 ? 2 : 3); }

// byte offset of frame f inside an item: every frame in front of it is a full one (8200 bytes + its frame number)
__host__ __device__ inline long long frame_offset(long long f) {
    return 8200LL * f + f + (f > 128 ? f - 128 : 0) + (f > 2048 ? f - 2048 : 0);
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

__global__ __launch_bounds__(FLAC_THREADS) void flac_frames_kernel(FlacFramesArgs p) {
    __shared__ uint16_t table[256];
    __shared__ uint16_t ops[16 * FLAC_CRC_SHIFTS];
    __shared__ uint4 pcm_words[FLAC_BLOCK / 8];             // int16 samples of the frame
    __shared__ uint4 frame_words[FRAME_WORDS];
    __shared__ uint32_t part_crc[FT / 64], part_len[FT / 64], part_max[FT / 64];

    const int item = blockIdx.y, tid = threadIdx.x;
    const long long f = blockIdx.x;
    const long long n = p.n_samples[item];
    if (f * FLAC_BLOCK >= n) return;                        // behind this item's last frame
    const long long rest = n - f * FLAC_BLOCK;
    const int size = rest < FLAC_BLOCK ? (int)rest : FLAC_BLOCK;
    const bool short_block = size != FLAC_BLOCK;
    const int nb = frame_number_bytes(f);
    const int head = 4 + nb + (short_block ? 2 : 0) + 1;   // frame header with its CRC-8
    const int flen = head + 1 + 2 * size + 2;
    uint8_t *dst = p.out + p.offset[item] + frame_offset(f);
    const int lead = (int)(reinterpret_cast<uintptr_t>(dst) & 15);
    uint8_t *img = reinterpret_cast<uint8_t *>(frame_words);      // img[lead + k] = byte k of the frame
    int16_t *pcm = reinterpret_cast<int16_t *>(pcm_words);

    for (int i = tid; i < 256; i += FT) table[i] = p.crc_tables[i];
    for (int i = tid; i < 16 * FLAC_CRC_SHIFTS; i += FT) ops[i] = p.crc_tables[256 + i];
    const float *x = p.audio + (long long)item * p.stride + f * FLAC_BLOCK;
    uint32_t mx = 0;
    for (int i = tid; i < size; i += FT) {
        const float v = x[i];
        mx = max(mx, __float_as_uint(v) & 0x7FFFFFFFu);
        const double q = fmin(fmax(rint((double)v * 32767.0), -32768.0), 32767.0);
        pcm[i] = (int16_t)(int)q;
    }
    __syncthreads();

    uint32_t crc = 0, len = 0, head_crc = 0;
    if (tid == 0) {
        uint8_t h[10];
        int k = 0;
        h[k++] = 0xFF;
        h[k++] = 0xF8;                                      // sync, fixed block size
        h[k++] = (uint8_t)(((short_block ? 7 : 12) << 4) | p.rate_code);
        h[k++] = 0x08;                                      // one channel, 16 bits per sample
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
        uint32_t c8 = 0;                                    // CRC-8, poly 0x07, init 0
        for (int i = 0; i < k; ++i) {
            c8 ^= h[i];
            for (int b = 0; b < 8; ++b) c8 = (c8 & 0x80u) ? ((c8 << 1) ^ 0x07u) & 0xFFu : (c8 << 1) & 0xFFu;
        }
        h[k++] = (uint8_t)c8;
        for (int i = 0; i < k; ++i) {
            img[lead + i] = h[i];
            head_crc = crc16_byte(head_crc, h[i], table);
        }
        img[lead + k] = 0x02;                               // VERBATIM sub-frame, no wasted bits
        head_crc = crc16_byte(head_crc, 0x02, table);
    }
    {
        const int b0 = PER * tid;
        const int cnt = max(0, min(PER, size - b0));
        uint8_t *body = img + lead + head + 1 + 2 * b0;
        const uint4 w0 = pcm_words[2 * tid], w1 = pcm_words[2 * tid + 1];
        const uint32_t w[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            if (i < cnt) {
                const uint32_t v = (w[i >> 1] >> (16 * (i & 1))) & 0xFFFFu;
                body[2 * i] = (uint8_t)(v >> 8);
                body[2 * i + 1] = (uint8_t)(v & 255u);
                crc = crc16_byte(crc, v >> 8, table);
                crc = crc16_byte(crc, v & 255u, table);
            }
        }
        len = 2 * cnt;
    }
    // log-depth combine inside the wave: lane i joins lane i + off (the run to its right) at every level
    const int lane = tid & 63, wave = tid >> 6;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t cr = __shfl_down(crc, off), lr = __shfl_down(len, off);
        if ((lane & (2 * off - 1)) == 0) {
            crc = crc16_shift(crc, lr, ops) ^ cr;
            len += lr;
        }
        mx = max(mx, (uint32_t)__shfl_xor((int)mx, off));
    }
    if (lane == 0) {
        part_crc[wave] = crc;
        part_len[wave] = len;
        part_max[wave] = mx;
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t total = head_crc, m = 0;
        for (int wv = 0; wv < FT / 64; ++wv) {
            total = crc16_shift(total, part_len[wv], ops) ^ part_crc[wv];
            m = max(m, part_max[wv]);
        }
        img[lead + flen - 2] = (uint8_t)(total >> 8);
        img[lead + flen - 1] = (uint8_t)(total & 255u);
        atomicMax(reinterpret_cast<unsigned int *>(p.max_abs) + item, m);
    }
    __syncthreads();
    // write-out: the 16-byte words that lie inside the frame whole, the two edge words byte by byte
    const int span = lead + flen, words = (span + 15) / 16;
    uint8_t *base = dst - lead;
    for (int wd = tid; wd < words; wd += FT) {
        const int lo = 16 * wd, hi = lo + 16;
        if (lo >= lead && hi <= span) {
            reinterpret_cast<uint4 *>(base)[wd] = frame_words[wd];
        } else {
            for (int k = max(lo, lead); k < min(hi, span); ++k) base[k] = img[k];
        }
    }
}

}  // namespace

long long flac_frames_bytes(long long n) {
    if (n <= 0) return 0;
    const long long last = (n - 1) / FLAC_BLOCK, size = n - last * FLAC_BLOCK;
    return frame_offset(last) + 8 + frame_number_bytes(last) + 2 * size + (size != FLAC_BLOCK ? 2 : 0);
}

int flac_rate_code(int rate) {
    switch (rate) {
        case 88200: return 1;
        case 176400: return 2;
        case 192000: return 3;
        case 8000: return 4;
        case 16000: return 5;
        case 22050: return 6;
        case 24000: return 7;
        case 32000: return 8;
        case 44100: return 9;
        case 48000: return 10;
        case 96000: return 11;
        default: return 0;                                  // 0000: the rate is taken from STREAMINFO
    }
}

const char *check_flac_frames(const float *audio, long long stride, int batch, const int64_t *n_samples, int sample_rate,
                              const uint16_t *crc_tables, const uint8_t *out, long long out_bytes, const float *max_abs) {
    if (batch < 0 || (batch > 0 && !n_samples)) return "need batch >= 0 and the host array of sample counts";
    if (sample_rate <= 0 || sample_rate >= (1 << 20)) return "the sample rate must lie in (0, 2^20) Hz";
    long long total = 0;
    for (int b = 0; b < batch; ++b) {
        if (n_samples[b] < 0 || n_samples[b] > stride) return "every item needs 0 <= n_samples <= stride";
        if (n_samples[b] > FLAC_MAX_SAMPLES) return "an item may have at most 2^28 samples (frame numbers of at most 3 bytes)";
        total += flac_frames_bytes(n_samples[b]);
    }
    if (total > out_bytes) return "the output buffer is smaller than the frames of the batch";
    if (batch > 0 && (!audio || !crc_tables || !out || !max_abs)) return "null device pointer";
    return nullptr;
}

void launch_flac_frames(const float *audio, long long stride, int batch, const int64_t *n_samples, int sample_rate,
                        const uint16_t *crc_tables, uint8_t *out, float *max_abs, hipStream_t stream) {
    long long offset = 0;
    for (int b0 = 0; b0 < batch; b0 += FLAC_ITEMS_PER_LAUNCH) {
        FlacFramesArgs a{};
        a.audio = audio + (long long)b0 * stride;
        a.stride = stride;
        a.crc_tables = crc_tables;
        a.out = out;
        a.max_abs = max_abs + b0;
        a.items = batch - b0 < FLAC_ITEMS_PER_LAUNCH ? batch - b0 : FLAC_ITEMS_PER_LAUNCH;
        a.rate_code = flac_rate_code(sample_rate);
        long long frames = 0;
        for (int i = 0; i < a.items; ++i) {
            a.n_samples[i] = n_samples[b0 + i];
            a.offset[i] = offset;
            offset += flac_frames_bytes(a.n_samples[i]);
            const long long fi = (a.n_samples[i] + FLAC_BLOCK - 1) / FLAC_BLOCK;
            frames = fi > frames ? fi : frames;
        }
        if (frames > 0)
            hipLaunchKernelGGL(flac_frames_kernel, dim3((unsigned)frames, (unsigned)a.items), dim3(FT), 0, stream, a);
    }
}

}  // namespace mbx
