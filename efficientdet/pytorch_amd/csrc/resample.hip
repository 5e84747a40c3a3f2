// The model-input resampler (include/effdet_resample.h holds the semantics; tests/resample_restated.py restates them): a normalised
// batch -- NCHW fp32, or the stem conv's NHWC layout in fp32 / bf16, strided or dense -- resized bilinearly to (Ho, Wo), optionally
// mirrored left-right, written as the stem conv's dense input [B][Ho][Wo][one 16-byte chunk].  A pure stream: 4 taps x 3 channels in,
// one 16-byte store out per pixel.
//   resample_kernel   grid (ceil(Ho * Wo / 256), B), one thread per output pixel, adjacent threads along x: the NCHW plane reads, the
//                     NHWC pixel reads and the stores of a wave are runs of neighbouring addresses (a mirrored view stores them in
//                     descending order, still one run).  The axis rule is resize_u8.h's lin_axis_ratio, so both tap indices are
//                     clamped into the source before they become addresses.  Batch and row terms of every offset are 64-bit.
//                     SRC selects the loads: the three fp32 planes; one 16-byte (fp32) or 8-byte (bf16) load per tap where the
//                     map's base and strides are aligned for it; three element loads per tap for any other map.
// Built with -ffp-contract=off: the fp64 coordinate and the three fp32 blend steps round as the restatement's.
#include "resize_u8.h"
#include "../../../include/effdet_resample.h"

namespace {

enum { SRC_NCHW = 0, SRC_NHWC_VEC = 1, SRC_NHWC_ELEM = 2 };

struct Px { float c[3]; };

// channels 0..2 of the NHWC pixel at p
template <typename T, int SRC> __device__ __forceinline__ Px load_px(const T* p) {
  Px v;
  if (SRC == SRC_NHWC_VEC) {
    const f32x4 q = load4(p);
    v.c[0] = q[0]; v.c[1] = q[1]; v.c[2] = q[2];
  } else {
    v.c[0] = Elem<T>::ld(p); v.c[1] = Elem<T>::ld(p + 1); v.c[2] = Elem<T>::ld(p + 2);
  }
  return v;
}

__device__ __forceinline__ float blend(float p00, float p01, float p10, float p11, float fx, float fy) {
  const float top = p00 + fx * (p01 - p00);
  const float bot = p10 + fx * (p11 - p10);
  return top + fy * (bot - top);
}

__device__ __forceinline__ void store_px(float* dst, float r0, float r1, float r2) { *(f32x4*)dst = f32x4{r0, r1, r2, 0.f}; }
__device__ __forceinline__ void store_px(bf16_t* dst, float r0, float r1, float r2) {
  *(uint4*)dst = uint4{pack2bf(r0, r1), pack2bf(r2, 0.f), 0u, 0u};
}

template <typename T, int SRC>
__global__ __launch_bounds__(256) void resample_kernel(const T* __restrict__ src, T* __restrict__ dst, int B, int H, int W, int Ho, int Wo,
                                                       int flip, long long ld, long long bstride, double ry, double rx) {
  const int b = (int)blockIdx.y < B ? (int)blockIdx.y : B - 1;
  const int r = blockIdx.x * 256 + threadIdx.x;          // Ho * Wo <= 2^30
  if (r >= Ho * Wo) return;
  const int oy = r / Wo, ox = r - oy * Wo;
  const int cx = flip ? Wo - 1 - ox : ox;                // the unmirrored result's column that lands here
  int y0, y1, x0, x1; float fy, fx;
  lin_axis_ratio(oy, H, ry, y0, y1, fy);
  lin_axis_ratio(cx, W, rx, x0, x1, fx);
  float out[3];
  if (SRC == SRC_NCHW) {
    const T* plane = src + (long long)b * 3 * H * W;
    const long long ra = (long long)y0 * W, rb = (long long)y1 * W, hw = (long long)H * W;
#pragma unroll
    for (int c = 0; c < 3; ++c, plane += hw)
      out[c] = blend(Elem<T>::ld(plane + ra + x0), Elem<T>::ld(plane + ra + x1), Elem<T>::ld(plane + rb + x0),
                     Elem<T>::ld(plane + rb + x1), fx, fy);
  } else {
    const T* img = src + (long long)b * bstride;
    const T* ra = img + (long long)y0 * W * ld;
    const T* rb = img + (long long)y1 * W * ld;
    const Px p00 = load_px<T, SRC>(ra + (long long)x0 * ld), p01 = load_px<T, SRC>(ra + (long long)x1 * ld);
    const Px p10 = load_px<T, SRC>(rb + (long long)x0 * ld), p11 = load_px<T, SRC>(rb + (long long)x1 * ld);
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = blend(p00.c[c], p01.c[c], p10.c[c], p11.c[c], fx, fy);
  }
  store_px(dst + ((long long)b * Ho * Wo + r) * Elem<T>::CE, out[0], out[1], out[2]);
}

template <typename T, int SRC> void launch(const effdet_resample_t* p, hipStream_t stream) {
  const long long n = (long long)p->Ho * p->Wo;
  hipLaunchKernelGGL((resample_kernel<T, SRC>), dim3((unsigned)((n + 255) / 256), (unsigned)p->B), dim3(256), 0, stream, (const T*)p->src,
                     (T*)p->dst, p->B, p->H, p->W, p->Ho, p->Wo, p->flip, p->src_ld, p->src_bstride, (double)p->H / (double)p->Ho,
                     (double)p->W / (double)p->Wo);
}

bool bad_side(int n) { return n < 1 || n > 32768; }

}  // namespace

extern "C" int effdet_resample_images(const effdet_resample_t* p, effdet_stream_t stream) {
  if (!p || !p->src || !p->dst || ((uintptr_t)p->dst & 15)) return EFFDET_EINVAL;
  if ((p->src_layout != EFFDET_RESAMPLE_NCHW && p->src_layout != EFFDET_RESAMPLE_NHWC) || (p->dtype != EFFDET_F32 && p->dtype != EFFDET_BF16) ||
      (p->src_layout == EFFDET_RESAMPLE_NCHW && p->dtype != EFFDET_F32) || (p->flip != 0 && p->flip != 1) || p->B < 1 || p->B > 65535 ||
      bad_side(p->H) || bad_side(p->W) || bad_side(p->Ho) || bad_side(p->Wo))
    return EFFDET_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (p->src_layout == EFFDET_RESAMPLE_NCHW) {
    launch<float, SRC_NCHW>(p, s);
  } else {
    if (p->C < 3 || p->src_ld < p->C || p->src_bstride < 0) return EFFDET_EUNSUPPORTED;
    // one load4 per tap reads 4 elements (16 bytes of fp32, 8 of bf16): it needs a fourth channel in memory and that alignment of every pixel
    const long long isz = p->dtype == EFFDET_F32 ? 4 : 2, al = 4 * isz;
    const bool vec = p->C >= 4 && ((uintptr_t)p->src % al) == 0 && (p->src_ld * isz) % al == 0 && (p->src_bstride * isz) % al == 0;
    if (p->dtype == EFFDET_F32) {
      if (vec) launch<float, SRC_NHWC_VEC>(p, s); else launch<float, SRC_NHWC_ELEM>(p, s);
    } else {
      if (vec) launch<bf16_t, SRC_NHWC_VEC>(p, s); else launch<bf16_t, SRC_NHWC_ELEM>(p, s);
    }
  }
  EFFDET_CHECK_LAUNCH();
  return EFFDET_OK;
}
