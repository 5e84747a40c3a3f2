// The random affine / perspective warp between the mosaic stage and the 'train' augmentation chain (include/effdet_affine.h holds the
// semantics; tests/affine_restated.py restates them): B uint8 source images (dataset images or mosaic canvases) -> B images of
// S x S uint8 RGB and their boxes, which augment.hip then takes as if they were dataset images.  Every random decision is in the
// per-image fp64 table drawn on the host: the forward matrix F for the boxes, its inverse G for the pixels.  Two launches:
//   affine_warp_kernel    a thread writes a run of 4 consecutive pixels of one output row (12 bytes, three dword stores; bytes where
//                         S is no multiple of 4).  Each pixel goes through G in fp64 and reads its four taps as bytes straight from
//                         the source.  A pixel that the rule calls outside the source gets coordinates (0, 0) before any index is
//                         formed, and a tap index is clamped into the source before it becomes an address, so the 48 byte loads of
//                         a run are always in bounds and independent of each other; `fill` is selected afterwards.  The image's row
//                         of the table is the same for the whole workgroup, so the three paths (a source without pixels,
//                         pass-through, warp) are uniform branches.
//   affine_boxes_kernel   one 64-lane workgroup per image: the four corners of each box through F in fp64, min / max, the clip to
//                         the output, YOLOv5's box_candidates filter, and a compaction in input order with block_scan.h.
// Built with -ffp-contract=off: the fp64 coordinates, the fp32 blends and the fp64 box steps round as the restatement's.
#include "block_scan.h"
#include "resize_u8.h"
#include "../../../include/effdet_affine.h"

namespace {

__device__ __forceinline__ bool finite64(double v) { return fabs(v) <= 1.7976931348623157e308; }      // false for NaN and +-Inf

// LongestMaxSize(S) + the central pad of an (h, w) source: the pass-through geometry, shared by the pixels and the boxes
struct Pad { int rh, rw, ox, oy; };
__device__ __forceinline__ Pad pad_of(int h, int w, int S) {
  Pad g;
  lms_dims(h, w, S, g.rh, g.rw);
  g.ox = (S - g.rw) / 2; g.oy = (S - g.rh) / 2;
  return g;
}

// grid (ceil(S * ceil(S / 4) / 256), B): out [B][S][S][3].  vec: S % 4 == 0 and out is 4-byte aligned, so a run is three dwords
__global__ __launch_bounds__(256) void affine_warp_kernel(const unsigned char* __restrict__ src, const long long* __restrict__ src_off,
                                                          const int* __restrict__ src_hw, const double* __restrict__ table, int B, int S,
                                                          int fill, int vec, unsigned char* __restrict__ out) {
  const int b = (int)blockIdx.y < B ? (int)blockIdx.y : B - 1;
  const double* p = table + (long long)b * EFFDET_AFFINE_P;
  const int R = (S + 3) >> 2;      // runs per row
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= R * S) return;
  const int y = r / R, x0 = (r - y * R) * 4;
  const int h = src_hw[2 * b], w = src_hw[2 * b + 1];
  const bool on = p[EFFDET_AFFINE_ON] != 0.0;
  unsigned char o[12];
  if (h < 1 || w < 1) {            // outside the domain: the source has no pixel, and none is read
#pragma unroll
    for (int j = 0; j < 12; ++j) o[j] = on ? (unsigned char)fill : (unsigned char)0;
  } else if (!on) {                // LongestMaxSize(S) + the central pad with zeros, as the chain's stage 'a'
    const unsigned char* base = src + src_off[b];
    const Pad g = pad_of(h, w, S);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = x0 + j < S ? x0 + j : S - 1;
      o[3 * j] = o[3 * j + 1] = o[3 * j + 2] = 0;
      if ((unsigned)(y - g.oy) < (unsigned)g.rh && (unsigned)(x - g.ox) < (unsigned)g.rw)
        bilinear_u8(base, 3, w, 0, 0, h, w, g.rh, g.rw, y - g.oy, x - g.ox, o + 3 * j);
    }
  } else {
    const unsigned char* base = src + src_off[b];
    const double g0 = p[EFFDET_AFFINE_G0], g1 = p[EFFDET_AFFINE_G1], g2 = p[EFFDET_AFFINE_G2], g3 = p[EFFDET_AFFINE_G3],
                 g4 = p[EFFDET_AFFINE_G4], g5 = p[EFFDET_AFFINE_G5], g6 = p[EFFDET_AFFINE_G6], g7 = p[EFFDET_AFFINE_G7],
                 g8 = p[EFFDET_AFFINE_G8];
    const double yd = (double)y, uy = g1 * yd, vy = g4 * yd, dy = g7 * yd;
    const float bg = (float)fill;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = x0 + j < S ? x0 + j : S - 1;
      const double xd = (double)x;
      const double d = (g6 * xd + dy) + g8;
      const double u = ((g0 * xd + uy) + g2) / d, v = ((g3 * xd + vy) + g5) / d;
      const bool in = finite64(d) && d > 0.0 && finite64(u) && finite64(v) && u > -1.0 && u < (double)w && v > -1.0 && v < (double)h;
      const double us = in ? u : 0.0, vs = in ? v : 0.0;             // from here on -1 < us < w and -1 < vs < h
      const double fu = floor(us), fv = floor(vs);
      const int ix = (int)fu, iy = (int)fv;                         // -1 .. w - 1, -1 .. h - 1
      const float fx = (float)(us - fu), fy = (float)(vs - fv);
      const bool xa = ix >= 0, xb = ix + 1 < w, ya = iy >= 0, yb = iy + 1 < h;     // which taps lie inside the source
      const int cxa = xa ? ix : 0, cxb = xb ? ix + 1 : w - 1, cya = ya ? iy : 0, cyb = yb ? iy + 1 : h - 1;   // clamped: always inside
      const unsigned char* ra = base + (long long)cya * w * 3;
      const unsigned char* rb = base + (long long)cyb * w * 3;
      const unsigned char *p00 = ra + (long long)cxa * 3, *p01 = ra + (long long)cxb * 3;
      const unsigned char *p10 = rb + (long long)cxa * 3, *p11 = rb + (long long)cxb * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float t00 = ya && xa ? (float)p00[c] : bg, t01 = ya && xb ? (float)p01[c] : bg;
        const float t10 = yb && xa ? (float)p10[c] : bg, t11 = yb && xb ? (float)p11[c] : bg;
        const unsigned char val = blend_u8(t00, t01, t10, t11, fx, fy);
        o[3 * j + c] = in ? val : (unsigned char)fill;
      }
    }
  }
  unsigned char* dst = out + ((long long)b * S * S + (long long)y * S + x0) * 3;
  if (vec) {
    uint3 q;
    q.x = (unsigned)o[0] | (unsigned)o[1] << 8 | (unsigned)o[2] << 16 | (unsigned)o[3] << 24;
    q.y = (unsigned)o[4] | (unsigned)o[5] << 8 | (unsigned)o[6] << 16 | (unsigned)o[7] << 24;
    q.z = (unsigned)o[8] | (unsigned)o[9] << 8 | (unsigned)o[10] << 16 | (unsigned)o[11] << 24;
    *(uint3*)dst = q;
  } else {
    const int n = S - x0 < 4 ? S - x0 : 4;
#pragma unroll
    for (int j = 0; j < 12; ++j)
      if (j < 3 * n) dst[j] = o[j];
  }
}

// grid (B), 64 lanes: lane l takes rows l, l + 64, ...; the kept rows go out in input order
__global__ __launch_bounds__(64) void affine_boxes_kernel(const int* __restrict__ src_hw, const double* __restrict__ table, int B, int S,
                                                          const float* __restrict__ ann, int M, double wh_thr, double ar_thr,
                                                          double area_thr, float* __restrict__ out, int* __restrict__ counts) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const double* p = table + (long long)b * EFFDET_AFFINE_P;
  __shared__ int wtot[4];          // block_scan_sum adds four wave totals; this workgroup is one wave, the other three stay 0
  if (lane < 4) wtot[lane] = 0;
  __syncthreads();
  const bool on = p[EFFDET_AFFINE_ON] != 0.0;
  const int h = src_hw[2 * b], w = src_hw[2 * b + 1];
  const Pad g = pad_of(h, w, S);
  const double sx = (double)g.rw / (double)w, sy = (double)g.rh / (double)h;
  const double f0 = p[EFFDET_AFFINE_F0], f1 = p[EFFDET_AFFINE_F1], f2 = p[EFFDET_AFFINE_F2], f3 = p[EFFDET_AFFINE_F3],
               f4 = p[EFFDET_AFFINE_F4], f5 = p[EFFDET_AFFINE_F5], f6 = p[EFFDET_AFFINE_F6], f7 = p[EFFDET_AFFINE_F7],
               f8 = p[EFFDET_AFFINE_F8], scale = p[EFFDET_AFFINE_SCALE];
  int kept = 0;
  for (int m0 = 0; m0 < M; m0 += 64) {
    const int m = m0 + lane;
    bool keep = false;
    double x1 = 0.0, y1 = 0.0, x2 = 0.0, y2 = 0.0;
    float label = -1.0f;
    if (m < M) {
      const float* a = ann + ((long long)b * M + m) * 5;
      label = a[4];
      if (label != -1.0f) {                                            // collater padding
        const double ax1 = (double)a[0], ay1 = (double)a[1], ax2 = (double)a[2], ay2 = (double)a[3];
        if (!on) {
          x1 = ax1 * sx + (double)g.ox; x2 = ax2 * sx + (double)g.ox;
          y1 = ay1 * sy + (double)g.oy; y2 = ay2 * sy + (double)g.oy;
          keep = true;
        } else {
          bool ok = true;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const double cx = k & 1 ? ax2 : ax1, cy = k & 2 ? ay2 : ay1;
            const double d = (f6 * cx + f7 * cy) + f8;
            const double X = ((f0 * cx + f1 * cy) + f2) / d, Y = ((f3 * cx + f4 * cy) + f5) / d;
            ok = ok && finite64(d) && d > 0.0;
            x1 = k ? fmin(x1, X) : X; x2 = k ? fmax(x2, X) : X;
            y1 = k ? fmin(y1, Y) : Y; y2 = k ? fmax(y2, Y) : Y;
          }
          const double lim = (double)S;
          x1 = fmin(fmax(x1, 0.0), lim); x2 = fmin(fmax(x2, 0.0), lim);
          y1 = fmin(fmax(y1, 0.0), lim); y2 = fmin(fmax(y2, 0.0), lim);
          const double w2 = x2 - x1, h2 = y2 - y1, w1 = ax2 - ax1, h1 = ay2 - ay1;
          const double ar = fmax(w2 / (h2 + 1e-16), h2 / (w2 + 1e-16));
          keep = ok && w2 > wh_thr && h2 > wh_thr && ar < ar_thr && w2 * h2 / (w1 * h1 * scale * scale + 1e-16) > area_thr;
        }
      }
    }
    int total;
    const int incl = block_scan_sum<int>(keep ? 1 : 0, wtot, &total);
    if (keep) {
      float* o = out + ((long long)b * M + kept + incl - 1) * 5;
      o[0] = (float)x1; o[1] = (float)y1; o[2] = (float)x2; o[3] = (float)y2; o[4] = label;
    }
    kept += total;
  }
  for (int m = kept + lane; m < M; m += 64) {
    float* o = out + ((long long)b * M + m) * 5;
    o[0] = o[1] = o[2] = o[3] = o[4] = -1.0f;
  }
  if (lane == 0) counts[b] = kept;
}

bool bad_dims(int B, int S) { return B < 1 || B > 65535 || S < 8 || (long long)S * S > (1LL << 30); }

}  // namespace

extern "C" int effdet_affine_warp(const unsigned char* src, const long long* src_off, const int* src_hw, const double* table, int B,
                                  int S, int fill, unsigned char* out, effdet_stream_t stream) {
  if (!src || !src_off || !src_hw || !table || !out) return EFFDET_EINVAL;
  if (bad_dims(B, S) || fill < 0 || fill > 255) return EFFDET_EINVAL;
  const long long runs = (long long)S * ((S + 3) >> 2);
  const int vec = (S & 3) == 0 && ((uintptr_t)out & 3) == 0;
  hipLaunchKernelGGL(affine_warp_kernel, dim3((unsigned)((runs + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, src,
                     src_off, src_hw, table, B, S, fill, vec, out);
  EFFDET_CHECK_LAUNCH();
  return EFFDET_OK;
}

extern "C" int effdet_affine_boxes(const int* src_hw, const double* table, int B, int S, const float* annots, int M, double wh_thr,
                                   double ar_thr, double area_thr, float* out, int* counts, effdet_stream_t stream) {
  if (!src_hw || !table || !annots || !out || !counts) return EFFDET_EINVAL;
  if (bad_dims(B, S) || M < 1) return EFFDET_EINVAL;
  hipLaunchKernelGGL(affine_boxes_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, src_hw, table, B, S, annots, M, wh_thr,
                     ar_thr, area_thr, out, counts);
  EFFDET_CHECK_LAUNCH();
  return EFFDET_OK;
}
