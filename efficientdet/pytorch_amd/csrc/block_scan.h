// Block-wide inclusive scans over threadIdx order for a 256-thread workgroup (4 waves): shuffles inside the wave, then the wave
// totals through wtot[4] in LDS, combined in wave order -- a fixed order, so the integer sums are exact and the result does not
// depend on timing.  *total = the whole block's result.  Every thread of the block must call (two barriers inside).  Used by the
// sweeps of voc_ap_kernel (voc_map.hip) and coco_accumulate_kernel (coco_map.hip).
#pragma once
#include "common.h"

template <typename T> __device__ __forceinline__ T block_scan_sum(T x, T* wtot, T* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const T t = __shfl_up(x, o, 64); if (lane >= o) x += t; }
  if (lane == 63) wtot[wave] = x;
  __syncthreads();
  T pre = 0;
  for (int w = 0; w < wave; ++w) pre += wtot[w];
  *total = wtot[0] + wtot[1] + wtot[2] + wtot[3];
  __syncthreads();
  return x + pre;
}

__device__ __forceinline__ double block_scan_max(double x, double* wtot, double* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const double t = __shfl_up(x, o, 64); if (lane >= o) x = fmax(x, t); }
  if (lane == 63) wtot[wave] = x;
  __syncthreads();
  double pre = 0.0;                                  // (every value is >= 0)
  for (int w = 0; w < wave; ++w) pre = fmax(pre, wtot[w]);
  *total = fmax(fmax(wtot[0], wtot[1]), fmax(wtot[2], wtot[3]));
  __syncthreads();
  return fmax(x, pre);
}
