// Device helpers shared by the two convolution sources: the generic implicit GEMM (conv_mfma.hip) and the mel-rate
// family (conv_mel.hip).
//
// C/D layout of a 32 x 32 tile of v_mfma_f32_32x32x2_f32 (16 registers per lane):
//   column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
#pragma once
#include <hip/hip_runtime.h>

namespace mbx {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// source row of the padded input: -1 = zero sample.  Branch free (selects only) so that the K loop stays one
// scheduling region.  mode: 0 zero, 1 symmetric (edge sample repeated), 2 edge.
__device__ __forceinline__ int map_row(int s, int n, int mode) {
    const bool inside = (s >= 0) & (s < n);
    const int refl = min(max(s < 0 ? -s - 1 : 2 * n - s - 1, 0), n - 1);
    const int edge = min(max(s, 0), n - 1);
    const int outside = mode == 0 ? -1 : (mode == 1 ? refl : edge);
    return inside ? s : outside;
}

// One LDS-DMA wave-instruction: 64 lanes x 16 bytes, global (per-lane address) -> LDS (M0 = wave-uniform byte
// address, lane l lands at M0 + 16*l).  Issued through inline asm on purpose: with the builtin hipcc waits
// vmcnt(0) in front of the next ds_read of the same __shared__ array (it cannot tell the two LDS buffers
// apart), which would serialise the prefetch of slice k+1 with the MFMAs of slice k.  The kernel orders DMA and
// reads itself: s_waitcnt vmcnt(0) + barrier before a buffer is read, barrier before it is overwritten.
__device__ __forceinline__ void lds_dma16(const float *src, unsigned lds_byte_addr) {
    asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, off" ::"s"(lds_byte_addr), "v"(src) : "memory", "m0");
}

}  // namespace mbx
