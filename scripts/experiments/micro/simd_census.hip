// Where do the waves of a block land?  One resident round of 6-wave blocks (384 threads, 79 104 bytes of LDS: 2 blocks per CU),
// of 4-wave blocks (53 760 bytes: 3 per CU) and of 8-wave blocks; every wave records HW_ID, the census counts waves per SIMD of
// every CU.  Round 7: 6-wave blocks leave every CU with 4 / 3 / 3 / 2 waves per SIMD (NOTEBOOK, profiles/r07_gate_shapes_ab.txt).
//   hipcc --offload-arch=gfx950 -O3 -o simd_census simd_census.hip && ./simd_census
#include <hip/hip_runtime.h>
#include <cstdio>
#include <map>
#include <vector>
#include <algorithm>
struct Rec { unsigned xcc, hwid; unsigned long long t0; };
__global__ __launch_bounds__(512) void census(Rec *out, int spin_ticks, int waves) {
    extern __shared__ float lds[];
    lds[threadIdx.x] = threadIdx.x;
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (__builtin_amdgcn_s_memrealtime() - t0 < (unsigned long long)spin_ticks) __builtin_amdgcn_s_sleep(16);
    if ((threadIdx.x & 63) == 0) {
        Rec r;
        r.xcc = __builtin_amdgcn_s_getreg((20) | (0 << 6) | (31 << 11));
        r.hwid = __builtin_amdgcn_s_getreg((4) | (0 << 6) | (31 << 11));
        r.t0 = t0;
        out[blockIdx.x * waves + (threadIdx.x >> 6)] = r;
    }
    if (lds[(threadIdx.x * 7) & 255] == -1.f) out[0].xcc = 0;
}
int main() {
    for (int waves : {6, 4, 8}) {
        const int lds_bytes = waves == 4 ? 53760 : 79104;
        const int per_cu = waves == 4 ? 3 : 2;
        const int blocks = 256 * per_cu;            // exactly one resident round
        if (hipFuncSetAttribute((const void *)census, hipFuncAttributeMaxDynamicSharedMemorySize, 79104) != hipSuccess) { printf("attr failed\n"); return 1; }
        Rec *d; hipMalloc(&d, blocks * waves * sizeof(Rec));
        std::vector<Rec> h(blocks * waves);
        for (int rep = 0; rep < 2; ++rep) {
            hipLaunchKernelGGL(census, dim3(blocks), dim3(64 * waves), lds_bytes, 0, d, 3000, waves);
            if (hipDeviceSynchronize() != hipSuccess) { printf("sync failed\n"); return 1; }
        }
        hipMemcpy(h.data(), d, h.size() * sizeof(Rec), hipMemcpyDeviceToHost);
        std::map<unsigned, std::vector<int>> by_cu;      // (xcc, se, sh, cu) -> simd ids of its waves
        std::map<unsigned, std::vector<int>> blk_cu;
        for (int i = 0; i < blocks * waves; ++i) {
            const unsigned cu = (h[i].hwid >> 8) & 15, sh = (h[i].hwid >> 12) & 1, se = (h[i].hwid >> 13) & 7, simd = (h[i].hwid >> 4) & 3;
            by_cu[((h[i].xcc & 15) << 12) | (se << 8) | (sh << 4) | cu].push_back(simd);
        }
        std::map<std::vector<int>, int> hist;
        for (auto &kv : by_cu) {
            std::vector<int> c(4, 0);
            for (int s : kv.second) c[s]++;
            hist[c]++;
        }
        printf("%d-wave blocks, %d per CU, %zu CUs: waves per SIMD (simd0 simd1 simd2 simd3) -> number of CUs\n", waves, per_cu, by_cu.size());
        for (auto &kv : hist) printf("   %d %d %d %d : %d\n", kv.first[0], kv.first[1], kv.first[2], kv.first[3], kv.second);
        printf("   first block's waves -> simd:");
        for (int w = 0; w < waves; ++w) printf(" %u", (h[w].hwid >> 4) & 3);
        printf("\n");
        hipFree(d);
    }
    return 0;
}
