// Mosaic and MixUp in front of the 'train' augmentation chain (include/effdet_mosaic.h holds the semantics; tests/mosaic_restated.py
// restates them): B uint8 source images of the batch -> B canvases of S x S uint8 RGB and their boxes, which augment.hip then takes as
// if they were dataset images.  Every random decision is a column of the per-image fp32 table drawn on the host.  Two launches:
//   mosaic_compose_kernel   a thread writes a run of 4 consecutive pixels of one canvas row (12 bytes, three dword stores).  The
//                           geometry of the image's five sources (four quadrants and the MixUp partner) is worked out once per
//                           workgroup into LDS; a pixel picks its quadrant with two compares and samples its source by the chain's
//                           resize rule (resize_u8.h).  The taps are loaded whether or not the pixel lies inside the resized image
//                           (their indices are clamped into the source, so they are always in bounds) and `fill` is selected
//                           afterwards, which leaves the 48 byte loads of a run independent of each other.
//   mosaic_boxes_kernel     one 64-lane workgroup per output image: the boxes of TL, TR, BL, BR and the partner in fp64, clipped to
//                           their window, filtered by filter_bboxes' rule and compacted in order with block_scan.h.
// Built with -ffp-contract=off: the fp32 blends and the fp64 box steps round as the restatement's.
#include "block_scan.h"
#include "resize_u8.h"
#include "../../../include/effdet_mosaic.h"

namespace {

// one source of an output image: slot 0..3 = the quadrants TL, TR, BL, BR (slot 0 alone, over the whole canvas, for a pass-through
// row), slot 4 = the MixUp partner
struct Slot {
  int s, h, w, rh, rw, ox, oy;     // source index (clamped into the batch), its size, its resized size and origin on the canvas
  int wx0, wx1, wy0, wy1;          // the window its pixels and boxes are clipped to
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ Slot mosaic_slot(const float* __restrict__ p, const int* __restrict__ src_hw, int b, int B, int S, int q) {
  const bool on = p[EFFDET_MOSAIC_ON] != 0.f;
  const bool quadrant = on && q < 4;
  Slot g;
  g.s = clampi(quadrant ? (int)p[EFFDET_MOSAIC_SRC0 + q] : (q == 4 ? (int)p[EFFDET_MOSAIC_MIX_SRC] : b), 0, B - 1);
  const int side = quadrant ? clampi((int)p[EFFDET_MOSAIC_SIDE0 + q], 1, S) : S;
  g.h = src_hw[2 * g.s]; g.w = src_hw[2 * g.s + 1];
  lms_dims(g.h, g.w, side, g.rh, g.rw);
  if (quadrant) {
    const int cx = clampi((int)p[EFFDET_MOSAIC_CX], 0, S), cy = clampi((int)p[EFFDET_MOSAIC_CY], 0, S);
    const bool right = q & 1, bottom = q & 2;
    g.ox = right ? cx : cx - g.rw; g.oy = bottom ? cy : cy - g.rh;
    g.wx0 = right ? cx : 0; g.wx1 = right ? S : cx;
    g.wy0 = bottom ? cy : 0; g.wy1 = bottom ? S : cy;
  } else {                         // LongestMaxSize(S) + the central pad
    g.ox = (S - g.rw) / 2; g.oy = (S - g.rh) / 2;
    g.wx0 = 0; g.wx1 = S; g.wy0 = 0; g.wy1 = S;
  }
  return g;
}

// what a pixel needs of a slot: LDS copy, with the two resize ratios formed once
struct Geo {
  long long off;                   // byte offset of the source in src
  double ry, rx;                   // h / rh, w / rw: lin_axis' ratio
  int h, w, rh, rw, ox, oy;
};

struct AxisY { int a, b; float f; bool in; };

__device__ __forceinline__ AxisY axis_y(const Geo& g, int y) {
  AxisY r;
  lin_axis_ratio(y - g.oy, g.h, g.ry, r.a, r.b, r.f);
  r.in = (unsigned)(y - g.oy) < (unsigned)g.rh;
  return r;
}

__device__ __forceinline__ Geo pick(const Geo& l, const Geo& r, bool right) {
  Geo g;
  g.off = right ? r.off : l.off; g.ry = right ? r.ry : l.ry; g.rx = right ? r.rx : l.rx;
  g.h = right ? r.h : l.h; g.w = right ? r.w : l.w; g.rh = right ? r.rh : l.rh; g.rw = right ? r.rw : l.rw;
  g.ox = right ? r.ox : l.ox; g.oy = right ? r.oy : l.oy;
  return g;
}
__device__ __forceinline__ AxisY pick(const AxisY& l, const AxisY& r, bool right) {
  AxisY a;
  a.a = right ? r.a : l.a; a.b = right ? r.b : l.b; a.f = right ? r.f : l.f; a.in = right ? r.in : l.in;
  return a;
}

// canvas pixel x of the row whose y geometry is `ay`: the bilinear sample of the source, or bg outside the resized image
__device__ __forceinline__ void sample(const unsigned char* __restrict__ src, const Geo& g, const AxisY& ay, int x, unsigned char bg,
                                       unsigned char out[3]) {
  int xa, xb; float fx;
  lin_axis_ratio(x - g.ox, g.w, g.rx, xa, xb, fx);
  const bool in = ay.in && (unsigned)(x - g.ox) < (unsigned)g.rw;
  const unsigned char* ra = src + g.off + (long long)ay.a * g.w * 3;
  const unsigned char* rb = src + g.off + (long long)ay.b * g.w * 3;
  const unsigned char *p00 = ra + (long long)xa * 3, *p01 = ra + (long long)xb * 3;
  const unsigned char *p10 = rb + (long long)xa * 3, *p11 = rb + (long long)xb * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float top = (float)p00[c] + fx * ((float)p01[c] - (float)p00[c]);
    const float bot = (float)p10[c] + fx * ((float)p11[c] - (float)p10[c]);
    const unsigned char v = round_u8(top + ay.f * (bot - top));
    out[c] = in ? v : bg;
  }
}

// grid (ceil(S * ceil(S / 4) / 256), B): out [B][S][S][3].  vec: S % 4 == 0 and out is 4-byte aligned, so a run is three dwords
__global__ __launch_bounds__(256) void mosaic_compose_kernel(const unsigned char* __restrict__ src, const long long* __restrict__ src_off,
                                                             const int* __restrict__ src_hw, const float* __restrict__ table, int B, int S,
                                                             int fill, int vec, unsigned char* __restrict__ out) {
  const int b = blockIdx.y;
  const float* p = table + (long long)b * EFFDET_MOSAIC_P;
  __shared__ Geo geo[5];
  if (threadIdx.x < 5) {
    const Slot s = mosaic_slot(p, src_hw, b, B, S, threadIdx.x);
    Geo g;
    g.off = src_off[s.s];
    g.h = s.h; g.w = s.w; g.rh = s.rh; g.rw = s.rw; g.ox = s.ox; g.oy = s.oy;
    g.ry = (double)s.h / (double)(s.rh > 1 ? s.rh : 1); g.rx = (double)s.w / (double)(s.rw > 1 ? s.rw : 1);
    geo[threadIdx.x] = g;
  }
  __syncthreads();
  const bool on = p[EFFDET_MOSAIC_ON] != 0.f;
  const bool mix = on && p[EFFDET_MOSAIC_MIX] != 0.f;
  // a pass-through row is slot 0 over the whole canvas on a zero background
  const int cx = on ? clampi((int)p[EFFDET_MOSAIC_CX], 0, S) : S, cy = on ? clampi((int)p[EFFDET_MOSAIC_CY], 0, S) : S;
  const unsigned char bg = on ? (unsigned char)fill : (unsigned char)0;
  const int R = (S + 3) >> 2;      // runs per row
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= R * S) return;
  const int y = r / R, x0 = (r - y * R) * 4;
  const int qy = y >= cy ? 2 : 0;
  const Geo gl = geo[qy], gr = geo[qy + 1];
  const AxisY yl = axis_y(gl, y), yr = axis_y(gr, y);
  unsigned char o[12];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int x = x0 + j < S ? x0 + j : S - 1;
    const bool right = x >= cx;  // selects, not a branch: the loads of the four pixels stay independent
    sample(src, pick(gl, gr, right), pick(yl, yr, right), x, bg, o + 3 * j);
  }
  if (mix) {
    const float lam = p[EFFDET_MOSAIC_LAM], mal = 1.f - lam;
    const Geo gp = geo[4];
    const AxisY yp = axis_y(gp, y);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = x0 + j < S ? x0 + j : S - 1;
      unsigned char pb[3];
      sample(src, gp, yp, x, (unsigned char)fill, pb);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float a = (float)o[3 * j + c] * lam, bpart = (float)pb[c] * mal;
        o[3 * j + c] = round_u8(a + bpart);
      }
    }
  }
  unsigned char* dst = out + ((long long)b * S * S + (long long)y * S + x0) * 3;
  if (vec) {
    uint3 v;
    v.x = (unsigned)o[0] | (unsigned)o[1] << 8 | (unsigned)o[2] << 16 | (unsigned)o[3] << 24;
    v.y = (unsigned)o[4] | (unsigned)o[5] << 8 | (unsigned)o[6] << 16 | (unsigned)o[7] << 24;
    v.z = (unsigned)o[8] | (unsigned)o[9] << 8 | (unsigned)o[10] << 16 | (unsigned)o[11] << 24;
    *(uint3*)dst = v;
  } else {
    const int n = S - x0 < 4 ? S - x0 : 4;
#pragma unroll
    for (int j = 0; j < 12; ++j)
      if (j < 3 * n) dst[j] = o[j];
  }
}

// grid (B), 64 lanes: lane l takes rows l, l + 64, ... of one source at a time; the kept rows go out in slot order, then row order
__global__ __launch_bounds__(64) void mosaic_boxes_kernel(const int* __restrict__ src_hw, const float* __restrict__ table, int B, int S,
                                                          const float* __restrict__ ann, int M, double min_area, double min_vis,
                                                          float* __restrict__ out, int M_out, int* __restrict__ counts) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const float* p = table + (long long)b * EFFDET_MOSAIC_P;
  __shared__ int wtot[4];          // block_scan_sum adds four wave totals; this workgroup is one wave, the other three stay 0
  if (lane < 4) wtot[lane] = 0;
  __syncthreads();
  const bool on = p[EFFDET_MOSAIC_ON] != 0.f;
  const int nslot = on ? (p[EFFDET_MOSAIC_MIX] != 0.f ? 5 : 4) : 1;
  int kept = 0;
  for (int q = 0; q < nslot; ++q) {
    const Slot g = mosaic_slot(p, src_hw, b, B, S, q);
    const double fx = (double)g.rw / (double)g.w, fy = (double)g.rh / (double)g.h;
    for (int m0 = 0; m0 < M; m0 += 64) {
      const int m = m0 + lane;
      bool keep = false;
      double x1 = 0.0, y1 = 0.0, x2 = 0.0, y2 = 0.0;
      float label = -1.0f;
      if (m < M) {
        const float* a = ann + ((long long)g.s * M + m) * 5;
        label = a[4];
        if (label != -1.0f) {                                          // collater padding
          x1 = (double)a[0] * fx + (double)g.ox; x2 = (double)a[2] * fx + (double)g.ox;
          y1 = (double)a[1] * fy + (double)g.oy; y2 = (double)a[3] * fy + (double)g.oy;
          const double area = (x2 - x1) * (y2 - y1);
          x1 = fmin(fmax(x1, (double)g.wx0), (double)g.wx1); x2 = fmin(fmax(x2, (double)g.wx0), (double)g.wx1);
          y1 = fmin(fmax(y1, (double)g.wy0), (double)g.wy1); y2 = fmin(fmax(y2, (double)g.wy0), (double)g.wy1);
          const double clipped = (x2 - x1) * (y2 - y1);
          keep = !(area == 0.0 || clipped / area < min_vis || clipped <= min_area);
        }
      }
      int total;
      const int incl = block_scan_sum<int>(keep ? 1 : 0, wtot, &total);
      if (keep) {
        float* o = out + ((long long)b * M_out + kept + incl - 1) * 5;
        o[0] = (float)x1; o[1] = (float)y1; o[2] = (float)x2; o[3] = (float)y2; o[4] = label;
      }
      kept += total;
    }
  }
  for (int m = kept + lane; m < M_out; m += 64) {
    float* o = out + ((long long)b * M_out + m) * 5;
    o[0] = o[1] = o[2] = o[3] = o[4] = -1.0f;
  }
  if (lane == 0) counts[b] = kept;
}

}  // namespace

extern "C" int effdet_mosaic_compose(const unsigned char* src, const long long* src_off, const int* src_hw, const float* table, int B,
                                     int S, int fill, unsigned char* out, effdet_stream_t stream) {
  if (!src || !src_off || !src_hw || !table || !out) return EFFDET_EINVAL;
  if (B < 1 || B > 65535 || S < 8 || (long long)S * S > (1LL << 30) || fill < 0 || fill > 255) return EFFDET_EINVAL;
  const long long runs = (long long)S * ((S + 3) >> 2);
  const int vec = (S & 3) == 0 && ((uintptr_t)out & 3) == 0;
  hipLaunchKernelGGL(mosaic_compose_kernel, dim3((unsigned)((runs + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, src,
                     src_off, src_hw, table, B, S, fill, vec, out);
  EFFDET_CHECK_LAUNCH();
  return EFFDET_OK;
}

extern "C" int effdet_mosaic_boxes(const int* src_hw, const float* table, int B, int S, const float* annots, int M, float min_area,
                                   float min_visibility, float* out, int M_out, int* counts, effdet_stream_t stream) {
  if (!src_hw || !table || !annots || !out || !counts) return EFFDET_EINVAL;
  if (B < 1 || S < 8 || M < 1 || (long long)M_out < 5LL * M) return EFFDET_EINVAL;
  hipLaunchKernelGGL(mosaic_boxes_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, src_hw, table, B, S, annots, M,
                     (double)min_area, (double)min_visibility, out, M_out, counts);
  EFFDET_CHECK_LAUNCH();
  return EFFDET_OK;
}
