// The per-pick arg-max of the sequential list kernels (one 1024-thread workgroup per image: postprocess.hip's soft_nms_kernel and
// wbf.hip's wbf_kernel): every thread offers a (value, index) pair and every thread ends with the workgroup's best after ONE barrier --
// a wave butterfly, lane 0 writes red[parity][wave], the barrier, every thread re-reduces the 16 slots with `lane & 15`.
//
// Shared here: the order and the DPP wave step.  The shuffle wave step of soft_nms_kernel and the cross-wave half of both kernels
// stay written out in the kernels: as functions of this header they left the instructions of soft_nms_kernel and wbf_kernel the same
// but changed their order and register allocation, and these two kernels are held to identical assembly
// (profiles/box_lists_resource_usage.txt).  For the same reason op_point.hip's op_best_kernel writes the order out on its LDS slots.
// Two other kernels follow the pattern with payloads of their own: slices.hip's slice_merge_kernel (lowest index, plus a hull that is
// min / max combined) and track.hip's block_max_key (one 64-bit key, four waves, a linear read of the four slots).
#pragma once
#include "common.h"

namespace {

// THE (value, index) arg-max order: the larger value first, then the lower index; "none" is (-inf, INT_MAX) and a NaN never wins
__device__ __forceinline__ void best_take(float& s, int& q, float os, int oq) { if (os > s || (os == s && oq < q)) { s = os; q = oq; } }

// the wave's best in every lane: an xor butterfly whose four steps inside a row of 16 lanes are DPP moves (no LDS crossbar round
// trip: the step sits on the critical path of every pick), the two across rows shuffles.  All 64 lanes must be active.
// (The other wave step in use is the plain butterfly: best_take over __shfl_xor for o = 32 .. 1, soft_nms_kernel's.)
template <int CTRL> __device__ __forceinline__ void best_dpp_step(float& s, int& q) {
  const float os = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(s), CTRL, 0xf, 0xf, false));
  const int oq = __builtin_amdgcn_update_dpp(0, q, CTRL, 0xf, 0xf, false);
  best_take(s, q, os, oq);
}
__device__ __forceinline__ void wave_best_dpp(float& s, int& q) {
  best_dpp_step<0xB1>(s, q);                                           // quad_perm [1,0,3,2]: lane ^ 1
  best_dpp_step<0x4E>(s, q);                                           // quad_perm [2,3,0,1]: lane ^ 2
  best_dpp_step<0x141>(s, q);                                          // row_half_mirror: 7 - lane of 8, a lane of the other quad
  best_dpp_step<0x140>(s, q);                                          // row_mirror: 15 - lane of 16, a lane of the other half row
  best_take(s, q, __shfl_xor(s, 16, 64), __shfl_xor(q, 16, 64));
  best_take(s, q, __shfl_xor(s, 32, 64), __shfl_xor(q, 32, 64));
}

}  // namespace
