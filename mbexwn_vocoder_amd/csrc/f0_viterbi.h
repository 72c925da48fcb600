// What the two Viterbi kernels over YIN candidates share -- f0_decode_kernel (f0_decode.hip: a whole item) and
// f0_lag_decode_kernel (f0_lag.hip: a stream, decided with a fixed lag): the lane layout, the DPP minimum over a group of 8
// lanes, the availability tests and ONE forward step.  The host definition is mbexwn_vocoder_amd/f0decode.py (viterbi_host,
// viterbi_lag_host); DESIGN.md sections 6i and 6l.
//
// One 64-lane wave per item.  Lane 8 j + i owns the transition i -> j.  The chain of a step is: v = delta[i] + tr(i, j); the
// minimum over i inside the groups of 8 lanes by DPP (quad_perm twice, row_half_mirror); new[j] = best + loc[j]; one
// ds_bpermute (the crossbar, no LDS memory) hands lane 8 j + i the new[i] of group i; the minimum over that group is the
// frame's m, and delta[i] = new[i] - m.  Selects only: the wave never splits.  Off the chain: the arg-minimum is the first
// set bit of the group's byte in the wave's mask of v == best (the smallest i wins a tie), and the back pointers of a frame
// are 8 x 3 bits gathered by lane swaps into one word.
//
// Host and device must give the same bits: plain operators, contraction off (set here, and it holds for the rest of a file
// that includes this header), no fused multiply-add, the correctly rounded division.
#pragma once

#include <cmath>

#include <hip/hip_runtime.h>

#include "mbx_kernels.h"

#pragma clang fp contract(off)

namespace mbx {

constexpr float F0_COST_LIMIT = 1e6f;                       // f0decode.LIMIT

// what lane 8 j + i holds of a frame: period and cost of its slots i and j
struct DecodeFrame {
    float pi, ci, pj, cj;
};

__device__ inline unsigned f0_dpp_quad_1032(unsigned v) { return __builtin_amdgcn_update_dpp(0u, v, 0xB1, 0xf, 0xf, true); }
__device__ inline unsigned f0_dpp_quad_2301(unsigned v) { return __builtin_amdgcn_update_dpp(0u, v, 0x4E, 0xf, 0xf, true); }
__device__ inline unsigned f0_dpp_half_mirror(unsigned v) { return __builtin_amdgcn_update_dpp(0u, v, 0x141, 0xf, 0xf, true); }

// the smaller of (v, arg) and a partner's pair, the smaller arg winning a tie: over lanes l ^ 1, l ^ 2 and 7 - l of a group
// of 8 lanes it leaves the group's minimum and the smallest index that has it on all eight.  Selects, no branches: the
// chain of a step is short only if the wave never splits.
#define F0_MIN_STEP(PERM)                                                  \
    {                                                                      \
        const float ov = __uint_as_float(PERM(__float_as_uint(v)));        \
        const int oa = (int)PERM((unsigned)arg);                           \
        const bool take = (ov < v) | ((ov == v) & (oa < arg));             \
        v = take ? ov : v;                                                 \
        arg = take ? oa : arg;                                             \
    }

__device__ inline void f0_group_min(float &v, int &arg) {
    F0_MIN_STEP(f0_dpp_quad_1032)
    F0_MIN_STEP(f0_dpp_quad_2301)
    F0_MIN_STEP(f0_dpp_half_mirror)
}

__device__ inline bool f0_cost_ok(float cst) { return (cst >= 0.f) & (cst <= F0_COST_LIMIT); }
__device__ inline bool f0_slot_available(bool unvoiced, float per, float cst) {
    return unvoiced | (f0_cost_ok(cst) & (per >= 1.f) & (per <= F0_COST_LIMIT));
}
// the minimum over a group of 8 lanes, on all eight.  No NaN comes here, so a compare and a select do (fminf would
// canonicalise its operands first)
__device__ inline float f0_group_smallest(float v) {
    float o = __uint_as_float(f0_dpp_quad_1032(__float_as_uint(v)));
    v = o < v ? o : v;
    o = __uint_as_float(f0_dpp_quad_2301(__float_as_uint(v)));
    v = o < v ? o : v;
    o = __uint_as_float(f0_dpp_half_mirror(__float_as_uint(v)));
    return o < v ? o : v;
}

// what a lane knows of its transition i -> j, fixed over the frames
struct ViterbiLane {
    int i, j;
    bool i_unvoiced, j_unvoiced, both_voiced;
    float w_jump, tr_fixed;                                 // tr_fixed: of the transitions that touch the unvoiced state
    __device__ ViterbiLane(int lane, float w_jump_, float w_switch)
        : i(lane & 7), j(lane >> 3), i_unvoiced(i == F0_SLOTS - 1), j_unvoiced(j == F0_SLOTS - 1),
          both_voiced(!i_unvoiced & !j_unvoiced), w_jump(w_jump_), tr_fixed(i == j ? 0.f : w_switch) {}
};

// One forward step, from frame t - 1 to frame t = `fr`.  In: delta[i], and period and availability of slot i of frame t - 1.
// Out: the same of frame t, and (on every lane) the frame's back pointers, 3 bits per available j.  The whole wave calls it.
// (The frame and the lane come by value and the step works on copies of the three carried values: with references for
// either, the compiler put the division of `jump` behind a branch on both_voiced -- sixteen splits of the wave per turn of
// f0_decode_kernel's loop, which the kernel had not before the step moved here.)
__device__ __forceinline__ unsigned f0_viterbi_step(const DecodeFrame fr, const ViterbiLane ln, float &delta_io, float &prev_p_io,
                                                    bool &prev_avail_io) {
    const int i = ln.i, j = ln.j;
    float delta = delta_io, prev_p = prev_p_io;
    bool prev_avail = prev_avail_io;
    const bool avail_j = f0_slot_available(ln.j_unvoiced, fr.pj, fr.cj);
    const float loc_j = f0_cost_ok(fr.cj) ? fr.cj : 0.f;
    const float jump = ln.w_jump * (fabsf(fr.pj - prev_p) / (fr.pj + prev_p));
    const float tr = ln.both_voiced ? jump : ln.tr_fixed;
    const float v = (prev_avail & avail_j) ? delta + tr : INFINITY;   // (an unavailable end: tr may be anything)
    const float best = f0_group_smallest(v);
    const float nw = avail_j ? best + loc_j : INFINITY;
    // this lane's new[i] comes from group i (one ds_bpermute: the crossbar, no LDS memory); the group then
    // holds new[0 .. 7], and their minimum is the frame's m
    const float ni = __int_as_float(__builtin_amdgcn_ds_bpermute(32 * i, __float_as_int(nw)));
    delta = ni - f0_group_smallest(ni);
    // off the chain: the smallest i that has the minimum, from the wave's equality mask
    const unsigned long long hit = __ballot(v == best);
    const int arg = __ffs((unsigned)(hit >> (8 * j)) & 0xffu) - 1;
    prev_avail = f0_slot_available(ln.i_unvoiced, fr.pi, fr.ci);
    prev_p = fr.pi;
    // the frame's back pointers, 3 bits per j, gathered over the eight groups
    typedef unsigned f0_pair __attribute__((ext_vector_type(2)));
    unsigned w = avail_j ? (unsigned)arg << (3 * j) : 0u;                                      // (arg is in 0 .. 7)
    w |= __builtin_amdgcn_update_dpp(0u, w, 0x128, 0xf, 0xf, true);                            // row_ror:8
    f0_pair r = __builtin_amdgcn_permlane16_swap(w, w, false, false);
    w = r[0] | r[1];
    r = __builtin_amdgcn_permlane32_swap(w, w, false, false);
    w = r[0] | r[1];
    delta_io = delta;
    prev_p_io = prev_p;
    prev_avail_io = prev_avail;
    return w;
}

// the smallest index of the minimum of delta over the available slots of the frame a step has left (on every lane)
__device__ inline int f0_best_state(float delta, bool avail, int i) {
    float v = avail ? delta : INFINITY;
    int arg = i;
    f0_group_min(v, arg);
    return arg;
}

}  // namespace mbx
