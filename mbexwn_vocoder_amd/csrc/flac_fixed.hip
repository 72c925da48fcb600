// Compressed FLAC frames of 16-bit mono audio on the device (include/mbexwn_flac.h): the frames that the host writer
// mbexwn_vocoder_amd/flac.py::encode(..., compression="fixed") emits behind its 42-byte header, byte for byte -- CONSTANT,
// FIXED (orders 0-4, partitioned Rice codes) or VERBATIM sub-frames in 4096-sample blocks.
//
// A frame's place depends on the lengths of all frames in front of it, so the work is three passes:
//   plan    one 256-thread block per (frame, item): quantise as flac.to_pcm16 does, into LDS; every thread takes 16
//           consecutive samples and adds, per order o = 0..4 and Rice parameter k = 0..14, sum (u >> k) of its zigzag
//           residuals into the (order, partition) sums in LDS (64-bit: a short block is one partition of up to 4095 residuals
//           below 2^21); 80 threads take the cheapest k of their (order, partition), 5 threads add up T(o), one thread
//           chooses and writes the frame's length and its choices (kind, order, the partitions' parameters).
//   scan    one block: exclusive scan of the batch's frame lengths into 64-bit offsets.
//   encode  one block per (frame, item) again: quantise again (cheaper than staging the samples through memory), every
//           thread the lengths of the codes of its 16 samples, a block-wide prefix sum for their bit positions, the bits
//           OR-ed into a zeroed frame image in LDS (neighbouring threads share words: LDS atomics, one per 32-bit word a
//           thread touches), CRC-16 by flac_frame.h's log-depth combine over a now variable byte count, write-out to the
//           unaligned destination by flac_frame.h's write_frame.
// A VERBATIM or CONSTANT frame runs through the same encode path: its "codes" are the samples in 16 bits each.
// What a frame is -- quantisation, header, CRC-16, write-out -- is flac_frame.h's, shared with flac_frames.hip.
#include "flac_frame.h"

namespace mbx {

namespace {

constexpr int MAX_ORDER = 4, RICE_PARAMS = 15, MAX_PARTS = 16;
constexpr int CRC_RUN = 36;                                 // bytes per thread in the CRC stage
constexpr int SCAN_THREADS = 1024;
enum { KIND_CONSTANT = 0, KIND_VERBATIM = 1, KIND_FIXED = 2 };

static_assert(CRC_RUN * FT >= MAX_FRAME_BYTES - 2, "the CRC runs cover the longest frame");

struct FlacFixedArgs {
    const float *audio;          // item i of the launch at audio + i * stride
    long long stride;
    const uint16_t *crc_tables;  // CRC-16 byte table (256), then FLAC_CRC_SHIFTS x 16 operator columns
    uint8_t *out;                // frame j of the batch at out + offsets[j]
    int32_t *frame_bytes;        // (frames of the batch)
    long long *offsets;          // (frames + 1)
    unsigned long long *plan;    // (frames, 2): the partitions' Rice parameters, 4 bits each; kind | order << 8 | p << 16
    int16_t *pcm_out;            // null, or item i of the launch at pcm_out + i * stride
    float *max_abs;              // (items), zeroed before the launch
    int items, rate_code;
    long long n_samples[FLAC_ITEMS_PER_LAUNCH];
    long long frame_base[FLAC_ITEMS_PER_LAUNCH];    // index in the batch of the item's first frame
};

__device__ inline int partition_order(int size) {
    int p = min(4, __ffs(size) - 1);
    while (p > 0 && (size >> p) <= 4) --p;
    return p;
}

// zigzag of the o-th finite difference at n >= o
__device__ inline uint32_t zigzag_residual(const int16_t *x, int n, int o) {
    int r = x[n];
    switch (o) {
        case 1: r = r - x[n - 1]; break;
        case 2: r = r - 2 * x[n - 1] + x[n - 2]; break;
        case 3: r = r - 3 * x[n - 1] + 3 * x[n - 2] - x[n - 3]; break;
        case 4: r = r - 4 * x[n - 1] + 6 * x[n - 2] - 4 * x[n - 3] + x[n - 4]; break;
        default: break;
    }
    return r >= 0 ? 2u * (uint32_t)r : 2u * (uint32_t)(-r) - 1u;
}

__global__ __launch_bounds__(FLAC_THREADS) void flac_fixed_plan_kernel(FlacFixedArgs p) {
    __shared__ int16_t pcm[FLAC_BLOCK];
    __shared__ unsigned long long sums[MAX_ORDER + 1][MAX_PARTS][RICE_PARAMS];
    __shared__ unsigned long long best_cost[MAX_ORDER + 1][MAX_PARTS];
    __shared__ uint32_t best_k[MAX_ORDER + 1][MAX_PARTS];
    __shared__ unsigned long long order_cost[MAX_ORDER + 1];
    __shared__ uint32_t part_max[FT / 64];

    const int item = blockIdx.y, tid = threadIdx.x;
    const long long f = blockIdx.x;
    const long long n = p.n_samples[item];
    if (f * FLAC_BLOCK >= n) return;                        // behind this item's last frame
    const long long rest = n - f * FLAC_BLOCK;
    const int size = rest < FLAC_BLOCK ? (int)rest : FLAC_BLOCK;
    const int po = partition_order(size), parts = 1 << po, plen = size >> po;
    const int max_o = min(MAX_ORDER, size - 1);

    const long long at = (long long)item * p.stride + f * FLAC_BLOCK;
    uint32_t mx = load_pcm(p.audio + at, size, pcm, p.pcm_out ? p.pcm_out + at : nullptr);
    for (int i = tid; i < (MAX_ORDER + 1) * MAX_PARTS * RICE_PARAMS; i += FT) (&sums[0][0][0])[i] = 0ull;
    for (int off = 1; off < 64; off <<= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, off));
    if ((tid & 63) == 0) part_max[tid >> 6] = mx;
    __syncthreads();

    const int n0 = PER * tid;
    int differs = 0;
    for (int i = 0; i < PER; ++i)
        if (n0 + i < size) differs |= pcm[n0 + i] != pcm[0];
    const int part0 = n0 < size ? n0 / plen : 0;
    for (int o = 0; o <= max_o; ++o) {
        uint32_t acc[RICE_PARAMS];
#pragma unroll
        for (int k = 0; k < RICE_PARAMS; ++k) acc[k] = 0u;
        int part = part0, edge = (part0 + 1) * plen;
        bool any = false;
        for (int i = 0; i < PER; ++i) {
            const int s = n0 + i;
            if (s >= size) break;
            if (s >= edge) {                                // into the next partition: hand the sums over
                if (any) {
#pragma unroll
                    for (int k = 0; k < RICE_PARAMS; ++k) {
                        atomicAdd(&sums[o][part][k], (unsigned long long)acc[k]);
                        acc[k] = 0u;
                    }
                }
                any = false;
                ++part;
                edge += plen;
            }
            if (s < o) continue;                            // warm-up sample
            const uint32_t u = zigzag_residual(pcm, s, o);
#pragma unroll
            for (int k = 0; k < RICE_PARAMS; ++k) acc[k] += u >> k;     // at most 16 terms below 2^21
            any = true;
        }
        if (any) {
#pragma unroll
            for (int k = 0; k < RICE_PARAMS; ++k) atomicAdd(&sums[o][part][k], (unsigned long long)acc[k]);
        }
    }
    const int any_differs = __syncthreads_or(differs);

    if (tid < (MAX_ORDER + 1) * MAX_PARTS) {
        const int o = tid / MAX_PARTS, part = tid % MAX_PARTS;
        if (o <= max_o && part < parts) {
            const unsigned long long count = (unsigned long long)(plen - (part == 0 ? o : 0));
            unsigned long long best = sums[o][part][0] + count;
            uint32_t bk = 0;
            for (int k = 1; k < RICE_PARAMS; ++k) {
                const unsigned long long b = sums[o][part][k] + (unsigned long long)(k + 1) * count;
                if (b < best) {                             // ties go to the smaller parameter
                    best = b;
                    bk = (uint32_t)k;
                }
            }
            best_cost[o][part] = best;
            best_k[o][part] = bk;
        }
    }
    __syncthreads();
    if (tid <= max_o) {
        unsigned long long t = 16ull * tid + 6ull;
        for (int part = 0; part < parts; ++part) t += 4ull + best_cost[tid][part];
        order_cost[tid] = t;
    }
    __syncthreads();
    if (tid == 0) {
        int order = 0;
        for (int o = 1; o <= max_o; ++o)
            if (order_cost[o] < order_cost[order]) order = o;   // ties go to the smaller order
        const int head = frame_header_bytes(f, size);
        int kind, body;
        unsigned long long ks = 0ull;
        if (!any_differs) {
            kind = KIND_CONSTANT;
            body = 2;
            order = 0;
        } else if (order_cost[order] < 16ull * (unsigned long long)size) {
            kind = KIND_FIXED;
            body = (int)((order_cost[order] + 7ull) >> 3);
            for (int part = 0; part < parts; ++part) ks |= (unsigned long long)best_k[order][part] << (4 * part);
        } else {
            kind = KIND_VERBATIM;
            body = 2 * size;
            order = 0;
        }
        const long long fidx = p.frame_base[item] + f;
        p.frame_bytes[fidx] = head + 1 + body + 2;
        p.plan[2 * fidx] = ks;
        p.plan[2 * fidx + 1] = (unsigned long long)(kind | (order << 8) | (po << 16));
        uint32_t m = 0;
        for (int wv = 0; wv < FT / 64; ++wv) m = max(m, part_max[wv]);
        atomicMax(reinterpret_cast<unsigned int *>(p.max_abs) + item, m);
    }
}

// offsets[j] = sum of len[0..j), offsets[frames] the total
__global__ __launch_bounds__(SCAN_THREADS) void flac_fixed_scan_kernel(const int32_t *len, long long *offsets, long long frames) {
    __shared__ long long wave_sum[SCAN_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long carry = 0;
    for (long long base = 0; base < frames; base += SCAN_THREADS) {
        const long long j = base + tid;
        const long long v = j < frames ? (long long)len[j] : 0ll;
        long long inc = v;
        for (int off = 1; off < 64; off <<= 1) {
            const long long up = __shfl_up(inc, off);
            if (lane >= off) inc += up;
        }
        if (lane == 63) wave_sum[wave] = inc;
        __syncthreads();
        long long before = 0, total = 0;
        for (int wv = 0; wv < SCAN_THREADS / 64; ++wv) {
            const long long s = wave_sum[wv];
            if (wv < wave) before += s;
            total += s;
        }
        if (j < frames) offsets[j] = carry + before + inc - v;
        carry += total;
        __syncthreads();
    }
    if (tid == 0) offsets[frames] = carry;
}

// Bits into the frame image, most significant bit first: a thread's fields are consecutive, so it collects the 32-bit word
// it is in and ORs it into LDS once (other threads' fields share the words at its two ends).
struct BitWriter {
    uint32_t *words;
    int group;
    uint32_t acc;
    __device__ void flush() {
        if (acc != 0u && group >= 0 && group < 4 * FRAME_WORDS) atomicOr(&words[group], __builtin_bswap32(acc));
        acc = 0u;
    }
    // the `width` (1..16) low bits of value at bit `pos` of the image
    __device__ void put(int pos, uint32_t value, int width) {
        const int g = pos >> 5, s = pos & 31;
        const unsigned long long t = (unsigned long long)value << (64 - width - s);
        if (g != group) {
            flush();
            group = g;
        }
        acc |= (uint32_t)(t >> 32);
        if ((uint32_t)t != 0u) {
            flush();
            group = g + 1;
            acc = (uint32_t)t;
        }
    }
};

// what sample s of the frame puts into the stream: `pw` bits `pv` (the residual header / a partition's parameter), `zeros`
// zero bits, `cw` bits `cv`
struct Code {
    uint32_t pv, cv;
    int pw, zeros, cw;
};

__device__ inline Code sample_code(const int16_t *pcm, int s, int kind, int order, int po, int plen, unsigned long long ks) {
    Code c{0u, 0u, 0, 0, 0};
    if (kind != KIND_FIXED || s < order) {                  // the sample as it is
        if (kind != KIND_CONSTANT || s == 0) {
            c.cv = (uint32_t)(uint16_t)pcm[s];
            c.cw = 16;
        }
        return c;
    }
    const int part = s / plen;
    const uint32_t k = (uint32_t)(ks >> (4 * part)) & 15u;
    if (s == order) {                                       // 00: 4-bit parameters; the partition order; partition 0's
        c.pv = ((uint32_t)po << 4) | k;
        c.pw = 10;
    } else if (s == part * plen) {
        c.pv = k;
        c.pw = 4;
    }
    const uint32_t u = zigzag_residual(pcm, s, order);
    c.zeros = (int)(u >> k);
    c.cv = (1u << k) | (u & ((1u << k) - 1u));
    c.cw = (int)k + 1;
    return c;
}

__global__ __launch_bounds__(FLAC_THREADS) void flac_fixed_encode_kernel(FlacFixedArgs p) {
    __shared__ uint16_t table[256];
    __shared__ uint16_t ops[16 * FLAC_CRC_SHIFTS];
    __shared__ int16_t pcm[FLAC_BLOCK];
    __shared__ uint4 frame_words[FRAME_WORDS];
    __shared__ uint32_t part_crc[FT / 64], part_len[FT / 64], part_bits[FT / 64];

    const int item = blockIdx.y, tid = threadIdx.x;
    const long long f = blockIdx.x;
    const long long n = p.n_samples[item];
    if (f * FLAC_BLOCK >= n) return;                        // behind this item's last frame
    const long long rest = n - f * FLAC_BLOCK;
    const int size = rest < FLAC_BLOCK ? (int)rest : FLAC_BLOCK;
    const int head = frame_header_bytes(f, size);
    const long long fidx = p.frame_base[item] + f;
    const int flen = min(max(p.frame_bytes[fidx], head + 3), head + 1 + 2 * size + 2);   // what the plan pass wrote
    const unsigned long long ks = p.plan[2 * fidx];
    const uint32_t choice = (uint32_t)p.plan[2 * fidx + 1];
    const int kind = (int)(choice & 255u), order = min((int)((choice >> 8) & 255u), min(MAX_ORDER, size - 1));
    const int po = partition_order(size), plen = size >> po;
    uint8_t *dst = p.out + p.offsets[fidx];
    const int lead = (int)(reinterpret_cast<uintptr_t>(dst) & 15);
    uint8_t *img = reinterpret_cast<uint8_t *>(frame_words);      // img[lead + k] = byte k of the frame
    const int lane = tid & 63, wave = tid >> 6;

    stage_crc_tables(p.crc_tables, table, ops);
    for (int i = tid; i < FRAME_WORDS; i += FT) frame_words[i] = make_uint4(0u, 0u, 0u, 0u);
    load_pcm(p.audio + (long long)item * p.stride + f * FLAC_BLOCK, size, pcm, nullptr);
    __syncthreads();

    // the bits of this thread's samples, and where they start
    const int n0 = PER * tid;
    int bits = 0;
    for (int i = 0; i < PER; ++i) {
        if (n0 + i >= size) break;
        const Code c = sample_code(pcm, n0 + i, kind, order, po, plen, ks);
        bits += c.pw + c.zeros + c.cw;
    }
    int inc = bits;
    for (int off = 1; off < 64; off <<= 1) {
        const int up = __shfl_up(inc, off);
        if (lane >= off) inc += up;
    }
    if (lane == 63) part_bits[wave] = (uint32_t)inc;
    __syncthreads();
    int pos = 8 * (lead + head + 1) + inc - bits;
    for (int wv = 0; wv < wave; ++wv) pos += (int)part_bits[wv];
    const int limit = 8 * (lead + flen - 2);                // the CRC-16 follows the last code

    BitWriter bw{reinterpret_cast<uint32_t *>(frame_words), -1, 0u};
    if (tid == 0) {
        uint8_t h[11];
        int k = frame_header(h, f, size, p.rate_code);
        // sub-frame byte: CONSTANT 0x00, VERBATIM 0x02, FIXED 0x10 + 2 * order; no wasted bits
        h[k++] = kind == KIND_CONSTANT ? 0x00 : (kind == KIND_VERBATIM ? 0x02 : (uint8_t)(0x10 + 2 * order));
        for (int i = 0; i < k; ++i)
            if (h[i]) bw.put(8 * (lead + i), h[i], 8);
    }
    for (int i = 0; i < PER; ++i) {
        if (n0 + i >= size) break;
        const Code c = sample_code(pcm, n0 + i, kind, order, po, plen, ks);
        if (c.pw && pos + c.pw <= limit) bw.put(pos, c.pv, c.pw);
        pos += c.pw + c.zeros;
        if (c.cw && pos + c.cw <= limit) bw.put(pos, c.cv, c.cw);
        pos += c.cw;
    }
    bw.flush();
    __syncthreads();

    // CRC-16 of the frame in front of it: every thread its run of bytes, joined by the log-depth combine
    uint32_t crc = 0, len = 0;
    {
        const int b0 = CRC_RUN * tid, b1 = min(b0 + CRC_RUN, flen - 2);
        for (int b = b0; b < b1; ++b) crc = crc16_byte(crc, img[lead + b], table);
        len = (uint32_t)max(0, b1 - b0);
    }
    crc16_join(crc, len, 0u, ops, part_crc, part_len, img + lead + flen - 2);
    __syncthreads();
    write_frame(dst, lead, flen, frame_words);
}

}  // namespace

long long flac_fixed_frames(int batch, const int64_t *n_samples) {
    long long frames = 0;
    for (int b = 0; b < batch; ++b) frames += (n_samples[b] + FLAC_BLOCK - 1) / FLAC_BLOCK;
    return frames;
}

const char *check_flac_fixed(const float *audio, long long stride, int batch, const int64_t *n_samples, int sample_rate,
                             const uint16_t *crc_tables, const uint8_t *out, long long out_bytes, const int32_t *frame_bytes,
                             const int64_t *workspace, const float *max_abs) {
    if (const char *why = check_flac_frames(audio, stride, batch, n_samples, sample_rate, crc_tables, out, out_bytes, max_abs))
        return why;
    if (batch > 0 && (!frame_bytes || !workspace)) return "null device pointer";
    return nullptr;
}

void launch_flac_fixed(const float *audio, long long stride, int batch, const int64_t *n_samples, int sample_rate,
                       const uint16_t *crc_tables, uint8_t *out, int32_t *frame_bytes, int64_t *workspace, int16_t *pcm_out,
                       float *max_abs, hipStream_t stream) {
    const long long total_frames = flac_fixed_frames(batch, n_samples);
    long long *offsets = reinterpret_cast<long long *>(workspace);
    for (int pass = 0; pass < 2; ++pass) {
        long long frame_base = 0;
        for (int b0 = 0; b0 < batch; b0 += FLAC_ITEMS_PER_LAUNCH) {
            FlacFixedArgs a{};
            a.audio = audio + (long long)b0 * stride;
            a.stride = stride;
            a.crc_tables = crc_tables;
            a.out = out;
            a.frame_bytes = frame_bytes;
            a.offsets = offsets;
            a.plan = reinterpret_cast<unsigned long long *>(offsets + total_frames + 1);
            a.pcm_out = pcm_out ? pcm_out + (long long)b0 * stride : nullptr;
            a.max_abs = max_abs + b0;
            a.items = batch - b0 < FLAC_ITEMS_PER_LAUNCH ? batch - b0 : FLAC_ITEMS_PER_LAUNCH;
            a.rate_code = flac_rate_code(sample_rate);
            long long frames = 0;
            for (int i = 0; i < a.items; ++i) {
                a.n_samples[i] = n_samples[b0 + i];
                a.frame_base[i] = frame_base;
                const long long fi = (a.n_samples[i] + FLAC_BLOCK - 1) / FLAC_BLOCK;
                frame_base += fi;
                frames = fi > frames ? fi : frames;
            }
            if (frames == 0) continue;
            const dim3 grid((unsigned)frames, (unsigned)a.items);
            if (pass == 0)
                hipLaunchKernelGGL(flac_fixed_plan_kernel, grid, dim3(FT), 0, stream, a);
            else
                hipLaunchKernelGGL(flac_fixed_encode_kernel, grid, dim3(FT), 0, stream, a);
        }
        if (pass == 0)
            hipLaunchKernelGGL(flac_fixed_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, stream, frame_bytes, offsets, total_frames);
    }
}

}  // namespace mbx
