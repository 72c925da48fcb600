// FLAC frames of 16-bit mono audio on the device: everything behind the 42-byte "fLaC" + STREAMINFO header that the host
// writer mbexwn_vocoder_amd/flac.py::encode emits (4096-sample blocks, VERBATIM sub-frames), byte for byte.
//
// One 256-thread block per (frame, item), in the four steps of flac_frame.h, which holds the frame format: the samples into
// LDS, the header, the CRC-16 join and the write-out.  This kernel's own is what lies between header and CRC-16: the
// sub-frame byte 0x02 and the big-endian samples, 16 per thread, with the CRC of every thread's 32-byte run taken as the
// bytes are placed.
// Bandwidth-type: reads 4 B and writes about 2 B per sample.
#include "flac_frame.h"

namespace mbx {

namespace {

// byte offset of frame f inside an item: every frame in front of it is a full one (8200 bytes + its frame number)
__host__ __device__ inline long long frame_offset(long long f) {
    return 8200LL * f + f + (f > 128 ? f - 128 : 0) + (f > 2048 ? f - 2048 : 0);
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
    const int head = frame_header_bytes(f, size);
    const int flen = head + 1 + 2 * size + 2;
    uint8_t *dst = p.out + p.offset[item] + frame_offset(f);
    const int lead = (int)(reinterpret_cast<uintptr_t>(dst) & 15);
    uint8_t *img = reinterpret_cast<uint8_t *>(frame_words);      // img[lead + k] = byte k of the frame

    stage_crc_tables(p.crc_tables, table, ops);
    uint32_t mx = load_pcm(p.audio + (long long)item * p.stride + f * FLAC_BLOCK, size,
                           reinterpret_cast<int16_t *>(pcm_words), nullptr);
    __syncthreads();

    uint32_t crc = 0, head_crc = 0;
    if (tid == 0) {
        uint8_t h[11];
        int k = frame_header(h, f, size, p.rate_code);
        h[k++] = 0x02;                                      // VERBATIM sub-frame, no wasted bits
        for (int i = 0; i < k; ++i) {
            img[lead + i] = h[i];
            head_crc = crc16_byte(head_crc, h[i], table);
        }
    }
    // this thread's samples, big-endian, and the CRC of their bytes
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
    for (int off = 1; off < 64; off <<= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, off));
    if ((tid & 63) == 0) part_max[tid >> 6] = mx;
    crc16_join(crc, 2 * cnt, head_crc, ops, part_crc, part_len, img + lead + flen - 2);
    if (tid == 0) {
        uint32_t m = 0;
        for (int wv = 0; wv < FT / 64; ++wv) m = max(m, part_max[wv]);
        atomicMax(reinterpret_cast<unsigned int *>(p.max_abs) + item, m);
    }
    __syncthreads();
    write_frame(dst, lead, flen, frame_words);
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
