// Box geometry of the detection-list kernels, once: postprocess.hip (greedy and rescoring NMS), wbf.hip, slices.hip, track.hip (fp32
// corner boxes), voc_map.hip, op_point.hip (the reference's fp64 overlap) and coco_map.hip (the label test only; its IoU follows
// maskApi.c on xywh boxes and stays there).  Every file that includes this is built with -ffp-contract=off: each operation rounds once,
// which is what the restated-semantics tests compare bit for bit.  loss.hip's IoU family and assign.h are not users.
#pragma once
#include "common.h"
#include <float.h>

namespace {

// fp32 area of a corner box (x1, y1, x2, y2)
__device__ __forceinline__ float box_area(const float4& b) { return (b.z - b.x) * (b.w - b.y); }

// positive and finite (false for NaN): an area, a confidence or a weight that may take part
__host__ __device__ __forceinline__ bool pos_finite(float a) { return a > 0.f && a < __builtin_huge_valf(); }

// fp32 intersection of two corner boxes -> do they overlap?  `iw <= 0.f || ih <= 0.f` refuses, so a NaN extent PASSES and the NaN
// reaches the caller's IoU.  (track.hip's tr_iou refuses with !(iw > 0.f) instead, which sends a NaN extent to 0: it keeps its own
// test over box_area and does not call this.)
__device__ __forceinline__ bool box_inter(const float4& a, const float4& b, float& inter) {
  const float iw = fminf(a.z, b.z) - fmaxf(a.x, b.x);
  const float ih = fminf(a.w, b.w) - fmaxf(a.y, b.y);
  if (iw <= 0.f || ih <= 0.f) return false;
  inter = iw * ih;
  return true;
}

// fp32 IoU from the two stored areas: inter / (aa + ab - inter), 0 for boxes that do not overlap
// (division-free forms -- bracketing products, or the exact f64 midpoint compare -- measured no faster: the phases that call this
//  are LDS/latency-bound, not VALU-bound)
__device__ __forceinline__ float box_iou(const float4& a, float aa, const float4& b, float ab) {
  float inter;
  if (!box_inter(a, b, inter)) return 0.f;
  return inter / (aa + ab - inter);
}

// the reference's compute_overlap for one (detection a, ground truth b) pair in its fp64 operation order: iw and ih clamped at 0,
// ua = max(aarea + area - iw * ih, DBL_EPSILON)
__device__ __forceinline__ double box_overlap_f64(double a0, double a1, double a2, double a3, double aarea, const double* b) {
  const double b0 = b[0], b1 = b[1], b2 = b[2], b3 = b[3];
  const double area = (b2 - b0) * (b3 - b1);
  double iw = fmin(a2, b2) - fmax(a0, b0);
  double ih = fmin(a3, b3) - fmax(a1, b1);
  iw = fmax(iw, 0.0);
  ih = fmax(ih, 0.0);
  double ua = aarea + area - iw * ih;
  ua = fmax(ua, DBL_EPSILON);
  return iw * ih / ua;
}

// a float label that is an integer in [0, C) -> its class in c
__device__ __forceinline__ bool label_class(float lf, int C, int& c) {
  c = (int)lf;
  return lf >= 0.f && lf < (float)C && (float)c == lf;
}

}  // namespace
