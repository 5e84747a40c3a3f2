// Device-side get_augumentation (datasets/augmentation.py:8-50): the reference's albumentations chains on uint8 images.
//   'train':  LongestMaxSize -> PadIfNeeded -> RandomResizedCrop -> Flip -> Transpose -> OneOf[brightness/contrast, gamma,
//             NoOp] -> OneOf[RGB shift, HSV shift, NoOp] -> CLAHE on the L of uint8 LAB -> HorizontalFlip -> VerticalFlip ->
//             Normalize, packed into the stem conv's NHWC input;
//   'valid' / 'test':  Resize (stretch) -> Normalize.
// Every random decision is a column of a per-image fp32 table drawn on the host (include/effdet_hip.h, EFFDET_AUG_*), so the
// kernels are deterministic functions of the images and the table.  Launches of the train chain:
//   1. resize_pad_kernel    LongestMaxSize + centred PadIfNeeded into an S x S uint8 canvas (stage A, 4 bytes per pixel);
//   2. geo_color_kernel     crop resample, flips / transpose as index maps, the pointwise LUTs / HSV shift, and the L byte of
//                           the CLAHE input (stage B = R, G, B, L);
//   3. clahe_lut_kernel     one workgroup per (tile, image): the 256-bin histogram in LDS (integer atomics), clip, redistribute,
//                           cdf -> the tile's LUT;
//   4. finish_kernel        the final flips as index maps, CLAHE's bilinear LUT blend, LAB -> RGB, Normalize, pack.
// Built with -ffp-contract=off: the float steps round exactly as tests/augment_restated.py restates them.  The colour-space
// steps use the documented float formulas of OpenCV's conversions in fp64 (its 8-bit fixed-point LAB tables are not restated).
#include "common.h"
#include "resize_u8.h"   // lin_axis, round_u8, bilinear_u8, lms_dims

namespace {

enum {
  A_RRC = 0, A_CY, A_CX, A_CH, A_CW, A_FLIP, A_FLIP_CODE, A_TRANSPOSE, A_COLOR, A_ALPHA, A_BETA, A_GAMMA,
  A_SHIFT, A_R, A_G, A_B, A_HUE, A_SAT, A_VAL, A_CLAHE, A_CLIP, A_HFLIP, A_VFLIP, A_P
};
static_assert(A_P == EFFDET_AUG_P, "table layout");

struct AugK {
  const unsigned char* src; const long long* src_off; const int* src_hw; const float* table;
  unsigned char* stage_a; unsigned char* stage_b; unsigned char* lut; void* out;
  int B, H, W, Cpad;
  float mean255[3], inv_std255[3];
};

// ------------------------------------------------------------------------------------------------ colour spaces
// sRGB -> linear for the 256 uint8 values (each workgroup fills an LDS copy)
__device__ __forceinline__ double srgb_to_linear(int v) {
  const double x = (double)v / 255.0;
  return x <= 0.04045 ? x / 12.92 : pow((x + 0.055) / 1.055, 2.4);
}
__device__ __forceinline__ double lab_f(double t) { return t > 0.008856 ? cbrt(t) : 7.787 * t + 16.0 / 116.0; }
__device__ __forceinline__ unsigned char sat_rint_u8(double v) {   // saturate_cast<uchar>: round half to even, saturate
  v = rint(v);
  return (unsigned char)(v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v));
}
__device__ __forceinline__ double lin_Y(const double* lin, int r, int g, int b) {
  return 0.212671 * lin[r] + 0.715160 * lin[g] + 0.072169 * lin[b];
}
__device__ __forceinline__ unsigned char lab_L8(double Y) {
  const double L = Y > 0.008856 ? 116.0 * cbrt(Y) - 16.0 : 903.3 * Y;
  return sat_rint_u8(L * (255.0 / 100.0));
}
__device__ __forceinline__ void lab_ab8(const double* lin, int r, int g, int b, double Y, unsigned char& a8, unsigned char& b8) {
  const double X = (0.412453 * lin[r] + 0.357580 * lin[g] + 0.180423 * lin[b]) / 0.950456;
  const double Z = (0.019334 * lin[r] + 0.119193 * lin[g] + 0.950227 * lin[b]) / 1.088754;
  const double fx = lab_f(X), fy = lab_f(Y), fz = lab_f(Z);
  a8 = sat_rint_u8(500.0 * (fx - fy) + 128.0);
  b8 = sat_rint_u8(200.0 * (fy - fz) + 128.0);
}
__device__ __forceinline__ unsigned char linear_to_srgb8(double x) {
  x = x < 0.0 ? 0.0 : (x > 1.0 ? 1.0 : x);
  x = x <= 0.0031308 ? 12.92 * x : 1.055 * pow(x, 1.0 / 2.4) - 0.055;
  return sat_rint_u8(x * 255.0);
}
__device__ __forceinline__ void lab8_to_rgb8(int L8, int a8, int b8, unsigned char out[3]) {
  const double L = (double)L8 * (100.0 / 255.0), a = (double)(a8 - 128), b = (double)(b8 - 128);
  double Y, fy;
  if (L <= 0.008856 * 903.3) { Y = L / 903.3; fy = 7.787 * Y + 16.0 / 116.0; }
  else { fy = (L + 16.0) / 116.0; Y = fy * fy * fy; }
  double fx = fy + a / 500.0, fz = fy - b / 200.0;
  const double th = 7.787 * 0.008856 + 16.0 / 116.0;
  fx = fx > th ? fx * fx * fx : (fx - 16.0 / 116.0) / 7.787;
  fz = fz > th ? fz * fz * fz : (fz - 16.0 / 116.0) / 7.787;
  const double X = fx * 0.950456, Z = fz * 1.088754;
  out[0] = linear_to_srgb8(3.240479 * X - 1.53715 * Y - 0.498535 * Z);
  out[1] = linear_to_srgb8(-0.969256 * X + 1.875991 * Y + 0.041556 * Z);
  out[2] = linear_to_srgb8(0.055648 * X - 0.204043 * Y + 1.057311 * Z);
}

// cv2 COLOR_RGB2HSV on uint8 (H in [0, 180)): its 12-bit fixed-point reciprocal tables, computed per call
__device__ __forceinline__ void rgb_to_hsv8(int r, int g, int b, int& h, int& s, int& v) {
  v = max(max(r, g), b);
  const int vmin = min(min(r, g), b), diff = v - vmin;
  const int sdiv = v ? (int)rint((double)(255 << 12) / (double)v) : 0;
  const int hdiv = diff ? (int)rint((double)(180 << 12) / (6.0 * (double)diff)) : 0;
  s = (diff * sdiv + (1 << 11)) >> 12;
  const int hh = v == r ? g - b : (v == g ? b - r + 2 * diff : r - g + 4 * diff);
  h = (hh * hdiv + (1 << 11)) >> 12;
  if (h < 0) h += 180;
}

// cv2 COLOR_HSV2RGB on uint8: the float conversion of (h, s / 255, v / 255), outputs saturate_cast<uchar>(x * 255)
__device__ __forceinline__ void hsv8_to_rgb8(int h8, int s8, int v8, unsigned char out[3]) {
  float h = (float)h8;
  const float s = (float)s8 * (1.f / 255.f), v = (float)v8 * (1.f / 255.f);
  float r, g, b;
  if (s == 0.f) { r = g = b = v; }
  else {
    h = h * (6.f / 180.f);
    h = fmodf(h, 6.f);
    int sector = (int)floorf(h);
    h -= (float)sector;
    if ((unsigned)sector >= 6u) { sector = 0; h = 0.f; }
    float tab[4];
    tab[0] = v; tab[1] = v * (1.f - s); tab[2] = v * (1.f - s * h); tab[3] = v * (1.f - s * (1.f - h));
    const int sd[6][3] = {{1, 3, 0}, {1, 0, 2}, {3, 0, 1}, {0, 2, 1}, {0, 1, 3}, {2, 1, 0}};   // (b, g, r) per sector
    b = tab[sd[sector][0]]; g = tab[sd[sector][1]]; r = tab[sd[sector][2]];
  }
  out[0] = sat_rint_u8((double)(r * 255.f)); out[1] = sat_rint_u8((double)(g * 255.f)); out[2] = sat_rint_u8((double)(b * 255.f));
}

// ------------------------------------------------------------------------------------------------ 1. LongestMaxSize + pad
// grid (ceil(S*S / 256), B): stage A [B][S][S][4] = (r, g, b, 0), zero outside the centred resized image
__global__ __launch_bounds__(256) void resize_pad_kernel(const AugK k) {
  const int b = blockIdx.y, S = k.H;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= S * S) return;
  const int y = i / S, x = i - y * S;
  const int h = k.src_hw[2 * b], w = k.src_hw[2 * b + 1];
  int rh, rw;
  lms_dims(h, w, S, rh, rw);
  const int top = (S - rh) / 2, left = (S - rw) / 2;
  uchar4 o = make_uchar4(0, 0, 0, 0);
  if (y >= top && y < top + rh && x >= left && x < left + rw) {
    unsigned char v[3];
    bilinear_u8(k.src + k.src_off[b], 3, w, 0, 0, h, w, rh, rw, y - top, x - left, v);
    o = make_uchar4(v[0], v[1], v[2], 0);
  }
  ((uchar4*)k.stage_a)[(long long)b * S * S + i] = o;
}

// ------------------------------------------------------------------------------------------------ 2. crop / permute / colour
__global__ __launch_bounds__(256) void geo_color_kernel(const AugK k) {
  const int b = blockIdx.y, S = k.H;
  const float* p = k.table + (long long)b * EFFDET_AUG_P;
  __shared__ unsigned char lut1[3][256], lut2[3][256];
  __shared__ double lin[256];
  const int color = (int)p[A_COLOR], shift = (int)p[A_SHIFT];
  const bool clahe = p[A_CLAHE] != 0.f;
  {
    const int t = threadIdx.x;
    unsigned char c1 = (unsigned char)t;
    if (color == 1) {              // RandomBrightnessContrast: float32 LUT i * alpha + beta * 255, clipped, truncated
      float v = (float)t * p[A_ALPHA];
      v = v + (float)((double)p[A_BETA] * 255.0);
      v = v < 0.f ? 0.f : (v > 255.f ? 255.f : v);
      c1 = (unsigned char)v;
    } else if (color == 2) {       // RandomGamma: (i / 255) ** gamma * 255, truncated
      c1 = (unsigned char)(pow((double)t * (1.0 / 255.0), (double)p[A_GAMMA]) * 255.0);
    }
    lut1[0][t] = lut1[1][t] = lut1[2][t] = c1;
    if (shift == 1) {              // RGBShift: float32 LUT i + shift, clipped, truncated
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float v = (float)t + p[A_R + c];
        v = v < 0.f ? 0.f : (v > 255.f ? 255.f : v);
        lut2[c][t] = (unsigned char)v;
      }
    } else if (shift == 2) {       // HueSaturationValue: hue LUT mod 180, sat / val clipped, all truncated
      double hv = fmod((double)t + (double)p[A_HUE], 180.0);
      if (hv < 0.0) hv += 180.0;
      lut2[0][t] = (unsigned char)hv;
#pragma unroll
      for (int c = 1; c < 3; ++c) {
        double v = (double)t + (double)p[A_HUE + c];
        v = v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v);
        lut2[c][t] = (unsigned char)v;
      }
    }
    if (clahe) lin[t] = srgb_to_linear(t);
  }
  __syncthreads();
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= S * S) return;
  int y = i / S, x = i - y * S;
  if (p[A_TRANSPOSE] != 0.f) { const int t = y; y = x; x = t; }           // out[y][x] = in[x][y]
  if (p[A_FLIP] != 0.f) {                                                   // cv2.flip code: 1 horizontal, 0 vertical, -1 both
    const int code = (int)p[A_FLIP_CODE];
    if (code != 0) x = S - 1 - x;
    if (code != 1) y = S - 1 - y;
  }
  const unsigned char* A = k.stage_a + (long long)b * S * S * 4;
  unsigned char v[3];
  if (p[A_RRC] != 0.f) {          // RandomResizedCrop: the (ch x cw) window at (cy, cx) resampled to S x S (clamped into the canvas)
    const int ch = min(max((int)p[A_CH], 1), S), cw = min(max((int)p[A_CW], 1), S);
    const int cy = min(max((int)p[A_CY], 0), S - ch), cx = min(max((int)p[A_CX], 0), S - cw);
    bilinear_u8(A, 4, S, cy, cx, ch, cw, S, S, y, x, v);
  } else {
    const uchar4 q = ((const uchar4*)A)[(long long)y * S + x];
    v[0] = q.x; v[1] = q.y; v[2] = q.z;
  }
  if (color == 1 || color == 2) { v[0] = lut1[0][v[0]]; v[1] = lut1[1][v[1]]; v[2] = lut1[2][v[2]]; }
  if (shift == 1) { v[0] = lut2[0][v[0]]; v[1] = lut2[1][v[1]]; v[2] = lut2[2][v[2]]; }
  else if (shift == 2) {
    int hh, ss, vv;
    rgb_to_hsv8(v[0], v[1], v[2], hh, ss, vv);
    hsv8_to_rgb8(lut2[0][hh], lut2[1][ss], lut2[2][vv], v);
  }
  const unsigned char L = clahe ? lab_L8(lin_Y(lin, v[0], v[1], v[2])) : 0;
  ((uchar4*)k.stage_b)[(long long)b * S * S + i] = make_uchar4(v[0], v[1], v[2], L);
}

// ------------------------------------------------------------------------------------------------ 3. CLAHE tile LUTs
// cv2 CLAHE (tile grid 8 x 8) on the L bytes of stage B.  An S not divisible by 8 is first extended by 8 - S % 8 rows and
// columns at the bottom / right with BORDER_REFLECT_101.  grid (64, B), 256 threads: thread t owns bin t.
__global__ __launch_bounds__(256) void clahe_lut_kernel(const AugK k) {
  const int b = blockIdx.y, tile = blockIdx.x, S = k.H;
  const float* p = k.table + (long long)b * EFFDET_AUG_P;
  if (p[A_CLAHE] == 0.f) return;
  const int Sp = S % 8 ? S + 8 - S % 8 : S, ts = Sp / 8, area = ts * ts;
  const int ty = tile / 8, tx = tile - ty * 8;
  __shared__ int hist[256];
  __shared__ int cnt;
  const int t = threadIdx.x;
  hist[t] = 0;
  if (t == 0) cnt = 0;
  __syncthreads();
  const uchar4* Bs = (const uchar4*)k.stage_b + (long long)b * S * S;
  for (int j = t; j < area; j += 256) {
    int r = ty * ts + j / ts, c = tx * ts + j % ts;
    if (r >= S) r = 2 * (S - 1) - r;           // reflect-101 (the extension is < 8 <= S)
    if (c >= S) c = 2 * (S - 1) - c;
    atomicAdd((int*)&hist[Bs[(long long)r * S + c].w], 1);
  }
  __syncthreads();
  int limit = (int)((double)p[A_CLIP] * (double)area / 256.0);
  limit = limit < 1 ? 1 : limit;
  int hv = hist[t];
  const int excess = hv > limit ? hv - limit : 0;
  hv -= excess;
  if (excess) atomicAdd(&cnt, excess);
  __syncthreads();
  const int clipped = cnt, batch = clipped / 256, residual = clipped - batch * 256;
  hv += batch;
  if (residual) {
    const int step = max(256 / residual, 1);
    if (t % step == 0 && t / step < residual) hv += 1;
  }
  hist[t] = hv;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {          // inclusive prefix sum
    const int add = t >= o ? hist[t - o] : 0;
    __syncthreads();
    hist[t] += add;
    __syncthreads();
  }
  const float scale = 255.0f / (float)area;
  float v = rintf((float)hist[t] * scale);
  v = v < 0.f ? 0.f : (v > 255.f ? 255.f : v);
  k.lut[((long long)b * 64 + tile) * 256 + t] = (unsigned char)v;
}

// ------------------------------------------------------------------------------------------------ 4. CLAHE apply + flips + pack
template <typename T>
__global__ __launch_bounds__(256) void finish_kernel(const AugK k) {
  const int b = blockIdx.y, S = k.H;
  const float* p = k.table + (long long)b * EFFDET_AUG_P;
  const bool clahe = p[A_CLAHE] != 0.f;
  __shared__ double lin[256];
  if (clahe) lin[threadIdx.x] = srgb_to_linear(threadIdx.x);
  __syncthreads();
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= S * S) return;
  const int y = i / S, x = i - y * S;
  const int sy = p[A_VFLIP] != 0.f ? S - 1 - y : y, sx = p[A_HFLIP] != 0.f ? S - 1 - x : x;   // HorizontalFlip / VerticalFlip
  const uchar4 q = ((const uchar4*)k.stage_b)[(long long)b * S * S + (long long)sy * S + sx];
  unsigned char rgb[3] = {q.x, q.y, q.z};
  if (clahe) {
    const int Sp = S % 8 ? S + 8 - S % 8 : S, ts = Sp / 8;
    const float inv_t = 1.0f / (float)ts;
    const float tyf = (float)sy * inv_t - 0.5f, txf = (float)sx * inv_t - 0.5f;
    int ty1 = (int)floorf(tyf), tx1 = (int)floorf(txf);
    int ty2 = ty1 + 1, tx2 = tx1 + 1;
    const float ya = tyf - (float)ty1, ya1 = 1.0f - ya, xa = txf - (float)tx1, xa1 = 1.0f - xa;
    ty1 = max(ty1, 0); tx1 = max(tx1, 0); ty2 = min(ty2, 7); tx2 = min(tx2, 7);
    const unsigned char* lut = k.lut + (long long)b * 64 * 256 + q.w;
    const float res = ((float)lut[(ty1 * 8 + tx1) * 256] * xa1 + (float)lut[(ty1 * 8 + tx2) * 256] * xa) * ya1 +
                      ((float)lut[(ty2 * 8 + tx1) * 256] * xa1 + (float)lut[(ty2 * 8 + tx2) * 256] * xa) * ya;
    unsigned char a8, b8;
    lab_ab8(lin, q.x, q.y, q.z, lin_Y(lin, q.x, q.y, q.z), a8, b8);
    lab8_to_rgb8(sat_rint_u8((double)res), a8, b8, rgb);
  }
  float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = ((float)rgb[c] - k.mean255[c]) * k.inv_std255[c];
  T* o = (T*)k.out + ((long long)b * S * S + i) * k.Cpad;
  if (k.Cpad == Elem<T>::CE) *(uint4*)o = Chunk<T>::pack(v);
  else for (int c = 0; c < k.Cpad; ++c) Elem<T>::st(o + c, c < 3 ? v[c] : 0.f);
}

// ------------------------------------------------------------------------------------------------ 'valid' / 'test'
// Resize(H, W) (stretch, uint8) + Normalize + pack; optional stage A copy [B][H][W][4] of the resized uint8 image
template <typename T>
__global__ __launch_bounds__(256) void resize_norm_kernel(const AugK k) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= k.H * k.W) return;
  const int y = i / k.W, x = i - y * k.W;
  const int h = k.src_hw[2 * b], w = k.src_hw[2 * b + 1];
  unsigned char u[3];
  bilinear_u8(k.src + k.src_off[b], 3, w, 0, 0, h, w, k.H, k.W, y, x, u);
  const long long pix = (long long)b * k.H * k.W + i;
  if (k.stage_a) ((uchar4*)k.stage_a)[pix] = make_uchar4(u[0], u[1], u[2], 0);
  float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = ((float)u[c] - k.mean255[c]) * k.inv_std255[c];
  T* o = (T*)k.out + pix * k.Cpad;
  if (k.Cpad == Elem<T>::CE) *(uint4*)o = Chunk<T>::pack(v);
  else for (int c = 0; c < k.Cpad; ++c) Elem<T>::st(o + c, c < 3 ? v[c] : 0.f);
}

// ------------------------------------------------------------------------------------------------ boxes
// one thread per image, rows in order: pascal_voc boxes through the geometric steps in fp64, clipped to the image, filtered
// (albumentations filter_bboxes), kept rows compacted to the front, the rest -1.  table == nullptr: the stretch resize.
__global__ __launch_bounds__(64) void boxes_kernel(const int* __restrict__ src_hw, const float* __restrict__ table, int B, int H, int W,
                                                   const float* __restrict__ ann, int M, double min_area, double min_vis,
                                                   float* __restrict__ out, int* __restrict__ counts) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const int h = src_hw[2 * b], w = src_hw[2 * b + 1];
  const float* p = table ? table + (long long)b * EFFDET_AUG_P : nullptr;
  int kept = 0;
  for (int m = 0; m < M; ++m) {
    const float* a = ann + ((long long)b * M + m) * 5;
    if (a[4] == -1.0f) continue;                                   // collater padding
    double x1 = a[0], y1 = a[1], x2 = a[2], y2 = a[3];
    if (!p) {
      const double fx = (double)W / (double)w, fy = (double)H / (double)h;
      x1 *= fx; x2 *= fx; y1 *= fy; y2 *= fy;
    } else {
      const int S = H;
      int rh, rw;
      lms_dims(h, w, S, rh, rw);
      const double fx = (double)rw / (double)w, fy = (double)rh / (double)h;
      const double top = (double)((S - rh) / 2), left = (double)((S - rw) / 2);
      x1 = x1 * fx + left; x2 = x2 * fx + left; y1 = y1 * fy + top; y2 = y2 * fy + top;
      if (p[A_RRC] != 0.f) {
        const int ch = min(max((int)p[A_CH], 1), S), cw = min(max((int)p[A_CW], 1), S);
        const int cy = min(max((int)p[A_CY], 0), S - ch), cx = min(max((int)p[A_CX], 0), S - cw);
        const double sx = (double)S / (double)cw, sy = (double)S / (double)ch;
        x1 = (x1 - cx) * sx; x2 = (x2 - cx) * sx; y1 = (y1 - cy) * sy; y2 = (y2 - cy) * sy;
      }
      if (p[A_FLIP] != 0.f) {
        const int code = (int)p[A_FLIP_CODE];
        if (code != 0) { const double t = x1; x1 = S - x2; x2 = S - t; }
        if (code != 1) { const double t = y1; y1 = S - y2; y2 = S - t; }
      }
      if (p[A_TRANSPOSE] != 0.f) { double t = x1; x1 = y1; y1 = t; t = x2; x2 = y2; y2 = t; }
      if (p[A_HFLIP] != 0.f) { const double t = x1; x1 = S - x2; x2 = S - t; }
      if (p[A_VFLIP] != 0.f) { const double t = y1; y1 = S - y2; y2 = S - t; }
    }
    const double area = (x2 - x1) * (y2 - y1);
    x1 = fmin(fmax(x1, 0.0), (double)W); x2 = fmin(fmax(x2, 0.0), (double)W);
    y1 = fmin(fmax(y1, 0.0), (double)H); y2 = fmin(fmax(y2, 0.0), (double)H);
    const double clipped = (x2 - x1) * (y2 - y1);
    if (area == 0.0 || clipped / area < min_vis || clipped <= min_area) continue;
    float* o = out + ((long long)b * M + kept) * 5;
    o[0] = (float)x1; o[1] = (float)y1; o[2] = (float)x2; o[3] = (float)y2; o[4] = a[4];
    ++kept;
  }
  for (int m = kept; m < M; ++m) {
    float* o = out + ((long long)b * M + m) * 5;
    o[0] = o[1] = o[2] = o[3] = o[4] = -1.0f;
  }
  counts[b] = kept;
}

AugK make_k(const unsigned char* src, const long long* src_off, const int* src_hw, const float* table, int B, int H, int W,
            void* out, int Cpad, const float mean255[3], const float inv_std255[3]) {
  AugK k{};
  k.src = src; k.src_off = src_off; k.src_hw = src_hw; k.table = table; k.out = out;
  k.B = B; k.H = H; k.W = W; k.Cpad = Cpad;
  for (int c = 0; c < 3; ++c) { k.mean255[c] = mean255[c]; k.inv_std255[c] = inv_std255[c]; }
  return k;
}

}  // namespace

extern "C" int effdet_augment_train(const unsigned char* src, const long long* src_off, const int* src_hw, const float* table, int B,
                                    int S, unsigned char* stage_a, unsigned char* stage_b, unsigned char* clahe_lut, void* out_nhwc,
                                    int dtype, int Cpad, const float mean255[3], const float inv_std255[3], effdet_stream_t stream) {
  if (!src || !src_off || !src_hw || !table || !stage_a || !stage_b || !clahe_lut || !out_nhwc || !mean255 || !inv_std255) return EFFDET_EINVAL;
  if (B < 1 || S < 8 || (long long)S * S > (1LL << 30) || B > 65535) return EFFDET_EINVAL;
  if (dtype != EFFDET_F32 && dtype != EFFDET_BF16) return EFFDET_EINVAL;
  if (Cpad < 3 || Cpad > 8) return EFFDET_EUNSUPPORTED;
  AugK k = make_k(src, src_off, src_hw, table, B, S, S, out_nhwc, Cpad, mean255, inv_std255);
  k.stage_a = stage_a; k.stage_b = stage_b; k.lut = clahe_lut;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(((long long)S * S + 255) / 256), (unsigned)B);
  hipLaunchKernelGGL(resize_pad_kernel, grid, dim3(256), 0, st, k);
  EFFDET_CHECK_LAUNCH();
  hipLaunchKernelGGL(geo_color_kernel, grid, dim3(256), 0, st, k);
  EFFDET_CHECK_LAUNCH();
  hipLaunchKernelGGL(clahe_lut_kernel, dim3(64, (unsigned)B), dim3(256), 0, st, k);
  EFFDET_CHECK_LAUNCH();
  if (dtype == EFFDET_F32) hipLaunchKernelGGL(finish_kernel<float>, grid, dim3(256), 0, st, k);
  else hipLaunchKernelGGL(finish_kernel<bf16_t>, grid, dim3(256), 0, st, k);
  EFFDET_CHECK_LAUNCH();
  return EFFDET_OK;
}

extern "C" int effdet_augment_resize(const unsigned char* src, const long long* src_off, const int* src_hw, int B, int H, int W,
                                     unsigned char* stage_a, void* out_nhwc, int dtype, int Cpad, const float mean255[3],
                                     const float inv_std255[3], effdet_stream_t stream) {
  if (!src || !src_off || !src_hw || !out_nhwc || !mean255 || !inv_std255) return EFFDET_EINVAL;
  if (B < 1 || H < 1 || W < 1 || (long long)H * W > (1LL << 30) || B > 65535) return EFFDET_EINVAL;
  if (dtype != EFFDET_F32 && dtype != EFFDET_BF16) return EFFDET_EINVAL;
  if (Cpad < 3 || Cpad > 8) return EFFDET_EUNSUPPORTED;
  AugK k = make_k(src, src_off, src_hw, nullptr, B, H, W, out_nhwc, Cpad, mean255, inv_std255);
  k.stage_a = stage_a;
  const dim3 grid((unsigned)(((long long)H * W + 255) / 256), (unsigned)B);
  if (dtype == EFFDET_F32) hipLaunchKernelGGL(resize_norm_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, k);
  else hipLaunchKernelGGL(resize_norm_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, k);
  EFFDET_CHECK_LAUNCH();
  return EFFDET_OK;
}

extern "C" int effdet_augment_boxes(const int* src_hw, const float* table, int B, int H, int W, const float* annots, int M,
                                    double min_area, double min_visibility, float* annots_out, int* counts, effdet_stream_t stream) {
  if (!src_hw || !annots || !annots_out || !counts || B < 1 || M < 1 || H < 1 || W < 1) return EFFDET_EINVAL;
  if (table && H != W) return EFFDET_EINVAL;
  hipLaunchKernelGGL(boxes_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, src_hw, table, B, H, W, annots,
                     M, min_area, min_visibility, annots_out, counts);
  EFFDET_CHECK_LAUNCH();
  return EFFDET_OK;
}
