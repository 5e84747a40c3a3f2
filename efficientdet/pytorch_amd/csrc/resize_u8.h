// The uint8 resize rule shared by the augmentation chain (augment.hip) and the mosaic stage (mosaic.hip): cv2.resize INTER_LINEAR as
// tests/augment_restated.py restates it (half-pixel centres, edge clamp, fp32 blend, round half up) and LongestMaxSize's dimensions.
// Both files are built with -ffp-contract=off, so every float step rounds as the restatement's.  The warp (affine.hip) has its own
// geometry and takes the pass-through resize and the blend of four taps (blend_u8) from here.
#pragma once
#include "common.h"

// cv2.resize INTER_LINEAR geometry along one axis (half-pixel centres, edge clamp), as oracle.pipeline_oracle.resize_bilinear
__device__ __forceinline__ void lin_axis(int o, int n_src, int n_dst, int& i0, int& i1, float& f) {
  const float s = (float)(((double)o + 0.5) * ((double)n_src / (double)n_dst) - 0.5);
  i0 = (int)floorf(s); f = s - (float)i0;
  if (i0 < 0) { i0 = 0; f = 0.f; }
  if (i0 >= n_src - 1) { i0 = n_src - 1; f = 0.f; }
  i1 = i0 + 1 < n_src ? i0 + 1 : n_src - 1;
}
// the same with ratio = (double)n_src / (double)n_dst formed by the caller, once for many output coordinates (the same double, so
// the same result)
__device__ __forceinline__ void lin_axis_ratio(int o, int n_src, double ratio, int& i0, int& i1, float& f) {
  const float s = (float)(((double)o + 0.5) * ratio - 0.5);
  i0 = (int)floorf(s); f = s - (float)i0;
  if (i0 < 0) { i0 = 0; f = 0.f; }
  if (i0 >= n_src - 1) { i0 = n_src - 1; f = 0.f; }
  i1 = i0 + 1 < n_src ? i0 + 1 : n_src - 1;
}

__device__ __forceinline__ unsigned char round_u8(float v) {      // the uint8 result of a resample: round half up, saturate
  v = floorf(v + 0.5f);
  return (unsigned char)(v < 0.f ? 0.f : (v > 255.f ? 255.f : v));
}

// bilinear sample of channels 0..2 of a pixel grid with `bpp` bytes per pixel and `pitch` pixels per row; (y, x) are output
// coordinates of an (n_h x n_w) -> (rh x rw) resize of the window whose top-left pixel is (y0w, x0w)
__device__ __forceinline__ void bilinear_u8(const unsigned char* base, int bpp, int pitch, int y0w, int x0w, int n_h, int n_w, int rh,
                                            int rw, int y, int x, unsigned char out[3]) {
  int ya, yb, xa, xb; float fy, fx;
  lin_axis(y, n_h, rh, ya, yb, fy);
  lin_axis(x, n_w, rw, xa, xb, fx);
  const unsigned char* p00 = base + ((long long)(y0w + ya) * pitch + x0w + xa) * bpp;
  const unsigned char* p01 = base + ((long long)(y0w + ya) * pitch + x0w + xb) * bpp;
  const unsigned char* p10 = base + ((long long)(y0w + yb) * pitch + x0w + xa) * bpp;
  const unsigned char* p11 = base + ((long long)(y0w + yb) * pitch + x0w + xb) * bpp;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float top = (float)p00[c] + fx * ((float)p01[c] - (float)p00[c]);
    const float bot = (float)p10[c] + fx * ((float)p11[c] - (float)p10[c]);
    out[c] = round_u8(top + fy * (bot - top));
  }
}

// bilinear_u8's blend of one channel for a caller that has its four taps as values (the warp of affine.hip, whose taps outside the
// source are the border byte): top, bot and the result in fp32, then round_u8.  bilinear_u8 keeps the same three lines written out:
// routed through this function its loads come out in another order, and augment.hip and mosaic.hip are to compile as they did.
__device__ __forceinline__ unsigned char blend_u8(float p00, float p01, float p10, float p11, float fx, float fy) {
  const float top = p00 + fx * (p01 - p00);
  const float bot = p10 + fx * (p11 - p10);
  return round_u8(top + fy * (bot - top));
}

// LongestMaxSize(S): scale = S / max(h, w), new dims rounded half to even (Python's round)
__device__ __forceinline__ void lms_dims(int h, int w, int S, int& rh, int& rw) {
  const double scale = (double)S / (double)(h > w ? h : w);
  rh = (int)rint((double)h * scale); rw = (int)rint((double)w * scale);
}
