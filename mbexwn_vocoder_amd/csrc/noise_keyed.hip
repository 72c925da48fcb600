// Keyed N(0,1) noise of a ragged batch: the draw of the model's noise channel as a function of (seed, item key, absolute
// step) alone (include/mbexwn_noise.h states the definition; mbexwn_vocoder_amd/noise.py mirrors its integer part).
//
//   quad q = s >> 2 of an item: Philox4x32-10 of the counter (q lo, q hi, 0, 0) under the item's 64-bit key
//   u(x) = (float(x >> 9) + 0.5f) * 2^-23, exact in float32 and strictly inside (0, 1)
//   lanes 0, 1 = r cos t, r sin t with r = sqrtf(-2 logf(u(x0))), t = 2 pi u(x1); lanes 2, 3 from (x2, x3)
//
// One 256-thread block per (item, tile of NOISE_TILE values); a tile is 1024 whole quads counted from the quad the row's
// first step falls in, thread t takes quads t, t + 256, t + 512, t + 768 of it (coalesced stores).  A thread always computes
// a whole quad and stores the lanes inside [first, first + count): a window that starts or ends inside a quad holds the bits
// of the whole item's fill.  A quad that lies wholly inside the window and whose address is 16-byte aligned leaves as one
// float4; the others leave lane by lane.  Bandwidth and transcendental issue, no LDS, no MFMA.
#include "mbx_kernels.h"

namespace mbx {

constexpr int NZ_THREADS = 256;
constexpr int NZ_QUADS = NOISE_TILE / 4;             // quads per tile
constexpr unsigned PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;
constexpr unsigned PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;

__device__ __forceinline__ void philox4x32_10(unsigned long long q, unsigned k0, unsigned k1, unsigned (&x)[4]) {
    unsigned c0 = (unsigned)q, c1 = (unsigned)(q >> 32), c2 = 0u, c3 = 0u;
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const unsigned hi0 = __umulhi(PHILOX_M0, c0), lo0 = PHILOX_M0 * c0;
        const unsigned hi1 = __umulhi(PHILOX_M1, c2), lo1 = PHILOX_M1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += PHILOX_W0;
        k1 += PHILOX_W1;
    }
    x[0] = c0, x[1] = c1, x[2] = c2, x[3] = c3;
}

__device__ __forceinline__ float unit_open(unsigned x) { return ((float)(x >> 9) + 0.5f) * 0x1p-23f; }

__device__ __forceinline__ void box_muller(unsigned xa, unsigned xb, float &z0, float &z1) {
    const float r = sqrtf(-2.0f * logf(unit_open(xa)));
    const float t = 6.283185307179586f * unit_open(xb);
    z0 = r * cosf(t);
    z1 = r * sinf(t);
}

typedef float quad_t __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(NZ_THREADS) void fill_normal_kernel(NoiseArgs p) {
    const int b = (int)(blockIdx.x / (unsigned)p.tiles), tile = (int)(blockIdx.x % (unsigned)p.tiles);
    const long long first = p.first_step ? p.first_step[b] : 0;
    if (first < 0) return;                               // a skipped row
    // the row's count from the device array, clamped to the row and to what the grid covers
    const long long count = min((long long)max(p.counts[b], 0), min(p.stride, (long long)p.max_count));
    const long long quad0 = (long long)tile * NZ_QUADS;  // first quad of the tile, counted from the quad of `first`
    const int lead = (int)(first & 3);                   // lanes of the row's first quad in front of the window
    if (quad0 * 4 >= lead + count) return;               // the tile starts behind the window
    const unsigned long long key = p.keys[2 * b] ^ (p.keys[2 * b + 1] * 0x9E3779B97F4A7C15ull);
    const unsigned k0 = (unsigned)key, k1 = (unsigned)(key >> 32);
    const unsigned long long q_first = (unsigned long long)first >> 2;
    float *row = p.out + (long long)b * p.stride;
#pragma unroll
    for (int i = 0; i < NZ_QUADS / NZ_THREADS; ++i) {
        const long long qi = quad0 + i * NZ_THREADS + (int)threadIdx.x;
        const long long idx = qi * 4 - lead;             // index in the row of the quad's lane 0: may be -3 .. -1
        if (idx >= count) continue;
        unsigned x[4];
        philox4x32_10(q_first + (unsigned long long)qi, k0, k1, x);
        float z[4];
        box_muller(x[0], x[1], z[0], z[1]);
        box_muller(x[2], x[3], z[2], z[3]);
        float *dst = row + idx;
        if (idx >= 0 && idx + 4 <= count && ((uintptr_t)dst & 15u) == 0) {
            // volatile: keeps the quad one 16-byte store (the optimiser otherwise shares lane 0 with the branch below)
            *reinterpret_cast<volatile quad_t *>(dst) = quad_t{z[0], z[1], z[2], z[3]};
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (idx + j >= 0 && idx + j < count) dst[j] = z[j];
        }
    }
}

const char *check_fill_normal(const NoiseArgs &a) {
    if (!a.out || !a.keys || !a.counts) return "null pointer";
    if (a.batch < 0 || a.stride < 0 || a.max_count < 0) return "batch, stride and max_count must not be negative";
    if ((long long)a.max_count > a.stride) return "max_count is larger than stride";
    const long long tiles = ((long long)a.max_count + 3 + NOISE_TILE - 1) / NOISE_TILE;
    if (tiles * a.batch > 0x7FFFFFFFLL) return "more tiles than one launch holds";
    return nullptr;
}

void launch_fill_normal(const NoiseArgs &a, hipStream_t stream) {
    if (a.batch == 0 || a.max_count == 0) return;
    NoiseArgs k = a;
    // a window of max_count values that starts at lane 3 of a quad reaches max_count + 3 lanes from that quad's start
    k.tiles = (int)(((long long)a.max_count + 3 + NOISE_TILE - 1) / NOISE_TILE);
    const dim3 grid((unsigned)((long long)k.tiles * a.batch)), block(NZ_THREADS);
    hipLaunchKernelGGL(fill_normal_kernel, grid, block, 0, stream, k);
}

}  // namespace mbx
