// Liveness flags for the sparse backward pass of the RetinaHead's regression tower (include/effdet_live_tiles.h).
//
// d(reg) -- the smooth-L1 gradient, pixel-major rows of reg_ld channels -- is an exact zero everywhere but at the positive anchors.
// Three small kernels per step turn it into byte flags for the gradient kernels' units of work:
//   live_nz_kernel     one pass over the rows (B = 32 @512: 174 592 pixels x 256 B = 45 MB, just written, bandwidth-bound):
//                      nz[pixel] = any word of the row with a bit outside the sign bit(s); 16 lanes x 16 B per pixel.
//   live_hdist_kernel  thread = pixel: hd = distance to the nearest non-zero pixel of its image ROW (11 bytes of the map).
//   live_flags_kernel  one workgroup of 128 threads per 128-pixel tile of a level: thread = pixel, Chebyshev distance to the nearest
//                      non-zero pixel of its image d = min over the 11 rows around it of max(|dy|, hd) (the separable form of the
//                      11 x 11 window: 11 + 11 byte loads per pixel instead of 121), the minimum over each 32-pixel step (wave
//                      shuffles) and over the tile (LDS), then for r = 0..5 the flags live32[r][step] = (min d <= r),
//                      live128[r][tile] likewise -- each flag one plain store of one workgroup, no atomics, nothing assumed about
//                      the buffers' previous content.
//   unit_lists_kernel  (include/effdet_unit_lists.h; one workgroup per radius) live32[r] -> the ascending list of its set flags and the
//                      counts the gathered conv launches read on the device.
// All are plain kernel launches: capturable, no memset, no host sync.
#include "common.h"
#include "../../../include/effdet_live_tiles.h"
#include "../../../include/effdet_needed_tiles.h"
#include "../../../include/effdet_unit_lists.h"
#include "block_scan.h"

namespace {

struct LiveK {
  const void* dreg; unsigned char* nz; unsigned char* hd; unsigned char* l32; unsigned char* l128;
  int nlev, reg_ld, apix, ntiles;
  unsigned mask;                 // bits of a word that make it non-zero
  long long S32, S128, P;        // steps / tiles / pixels over all levels
  int H[EFFDET_MAX_SEG], W[EFFDET_MAX_SEG], M[EFFDET_MAX_SEG];
  int pix0[EFFDET_MAX_SEG];      // first pixel of the level in the level-major byte map
  int poff[EFFDET_MAX_SEG];      // first pixel of the level inside an image's rows of dreg
  int step0[EFFDET_MAX_SEG], tile0[EFFDET_MAX_SEG];
};

__global__ __launch_bounds__(256) void live_nz_kernel(const LiveK p) {
  const int sub = threadIdx.x & 15;
  const int q4 = p.reg_ld >> 2;                                   // 16-byte chunks per row
  for (long long g = (long long)blockIdx.x * 16 + (threadIdx.x >> 4); g < p.P; g += (long long)gridDim.x * 16) {
    int l = 0;
#pragma unroll
    for (int s = 1; s < EFFDET_MAX_SEG; ++s)
      if (s < p.nlev && g >= p.pix0[s]) l = s;
    const int m = (int)(g - p.pix0[l]);
    const int hw = p.H[l] * p.W[l];
    const int b = m / hw, q = m - b * hw;
    const uint4* row = (const uint4*)p.dreg + ((long long)b * p.apix + p.poff[l] + q) * q4;
    unsigned any = 0u;
    for (int c = sub; c < q4; c += 16) {
      const uint4 v = row[c];
      any |= (v.x | v.y | v.z | v.w) & p.mask;
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) any |= (unsigned)__shfl_xor((int)any, o, 64);
    if (sub == 0) p.nz[g] = any ? 1 : 0;
  }
}

__global__ __launch_bounds__(256) void live_hdist_kernel(const LiveK p) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= p.P) return;
  int l = 0;
#pragma unroll
  for (int s = 1; s < EFFDET_MAX_SEG; ++s)
    if (s < p.nlev && g >= p.pix0[s]) l = s;
  const int W = p.W[l];
  const int m = (int)(g - p.pix0[l]);
  const int w = m % W;                                            // (rows of W pixels are contiguous across images and image rows)
  const unsigned char* rowp = p.nz + (g - w);
  const int R = EFFDET_LIVE_RADII - 1;
  const int x0 = max(w - R, 0), x1 = min(w + R, W - 1);
  int d = EFFDET_LIVE_RADII;
  for (int x = x0; x <= x1; ++x)
    if (rowp[x]) d = min(d, abs(x - w));
  p.hd[g] = (unsigned char)d;
}

__global__ __launch_bounds__(128) void live_flags_kernel(const LiveK p) {
  __shared__ int smin[4];
  const int t = threadIdx.x;
  const int tile = blockIdx.x;
  int l = 0;
#pragma unroll
  for (int s = 1; s < EFFDET_MAX_SEG; ++s)
    if (s < p.nlev && tile >= p.tile0[s]) l = s;
  const int tl = tile - p.tile0[l];
  const int H = p.H[l], W = p.W[l], hw = H * W, M = p.M[l];
  const int m = tl * 128 + t;
  int d = EFFDET_LIVE_RADII;                                      // "farther than every radius"
  if (m < M) {
    const int b = m / hw, rem = m - b * hw;
    const int h = rem / W, w = rem - h * W;
    const unsigned char* col = p.hd + p.pix0[l] + (long long)b * hw + w;
    const int R = EFFDET_LIVE_RADII - 1;
    const int y0 = max(h - R, 0), y1 = min(h + R, H - 1);
    for (int y = y0; y <= y1; ++y) d = min(d, max(abs(y - h), (int)col[y * W]));
  }
  // minimum over each 32-pixel step (the two halves of a wave), then over the tile
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) d = min(d, __shfl_xor(d, o, 64));
  if ((t & 31) == 0) smin[t >> 5] = d;
  __syncthreads();
  if (t < 4 * EFFDET_LIVE_RADII) {
    const int r = t >> 2, s = t & 3;
    const int step = tl * 4 + s;
    if (step * 32 < M) p.l32[(long long)r * p.S32 + p.step0[l] + step] = smin[s] <= r ? 1 : 0;
  } else if (t >= 32 && t < 32 + EFFDET_LIVE_RADII) {
    const int r = t - 32;
    const int dm = min(min(smin[0], smin[1]), min(smin[2], smin[3]));
    p.l128[(long long)r * p.S128 + tile] = dm <= r ? 1 : 0;
  }
}

// Compacted unit lists (include/effdet_unit_lists.h): workgroup r walks live32[r] in runs of 256 x 8 flags -- thread t counts its 8
// consecutive flags, a block scan in thread order places them behind the runs before -- and writes the set flags' indices in ascending
// order; then the set flags of live128[r] are counted the same way.  Plain stores, one writer per word.
__global__ __launch_bounds__(256) void unit_lists_kernel(const unsigned char* l32, const unsigned char* l128, long long S32, long long S128,
                                                         int* units, int* counts) {
  __shared__ int wtot[4];
  const int r = blockIdx.x, t = threadIdx.x;
  const unsigned char* f = l32 + (long long)r * S32;
  int* out = units + (long long)r * S32;
  int base = 0;
  for (long long run = 0; run < S32; run += 2048) {
    const long long i0 = run + 8 * t;
    int c = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) c += (i0 + e < S32 && f[i0 + e]) ? 1 : 0;
    int total;
    int o = base + block_scan_sum(c, wtot, &total) - c;
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (i0 + e < S32 && f[i0 + e]) out[o++] = (int)(i0 + e);
    base += total;
  }
  const unsigned char* g = l128 + (long long)r * S128;
  int n128 = 0;
  for (long long run = 0; run < S128; run += 2048) {
    const long long i0 = run + 8 * t;
    int c = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) c += (i0 + e < S128 && g[i0 + e]) ? 1 : 0;
    int total;
    (void)block_scan_sum(c, wtot, &total);
    n128 += total;
  }
  if (t < EFFDET_UNIT_COUNTS) {
    const int gt = (base + 3) >> 2;
    counts[r * EFFDET_UNIT_COUNTS + t] = t == 0 ? base : t == 1 ? n128 : t == 2 ? (16 * gt <= 15 * n128 ? 1 : 0) : 0;
  }
}

// geometry of the flag arrays; -> EFFDET_OK or an error
int live_geometry(int B, int nlev, const int* H, const int* W, LiveK& k) {
  if (B < 1 || nlev < 1 || nlev > EFFDET_MAX_SEG || !H || !W) return EFFDET_EINVAL;
  long long P = 0, S32 = 0, S128 = 0, apix = 0;
  for (int l = 0; l < nlev; ++l) {
    if (H[l] < 1 || W[l] < 1) return EFFDET_EINVAL;
    const long long M = (long long)B * H[l] * W[l];
    if (M >= 0x40000000LL) return EFFDET_EUNSUPPORTED;
    k.H[l] = H[l]; k.W[l] = W[l]; k.M[l] = (int)M;
    k.pix0[l] = (int)P; k.poff[l] = (int)apix; k.step0[l] = (int)S32; k.tile0[l] = (int)S128;
    P += M; apix += (long long)H[l] * W[l]; S32 += (M + 31) / 32; S128 += (M + 127) / 128;
    if (P >= 0x40000000LL) return EFFDET_EUNSUPPORTED;
  }
  for (int l = nlev; l < EFFDET_MAX_SEG; ++l) { k.H[l] = k.W[l] = 1; k.M[l] = 0; k.pix0[l] = k.poff[l] = k.step0[l] = k.tile0[l] = 0x7fffffff; }
  k.nlev = nlev; k.apix = (int)apix; k.P = P; k.S32 = S32; k.S128 = S128; k.ntiles = (int)S128;
  return EFFDET_OK;
}

}  // namespace

extern "C" long long effdet_live_tiles_counts(int B, int nlev, const int* H, const int* W, long long* steps, long long* tiles) {
  LiveK k;
  const int rc = live_geometry(B, nlev, H, W, k);
  if (rc != EFFDET_OK) return rc;
  if (steps) *steps = k.S32;
  if (tiles) *tiles = k.S128;
  return k.P;
}

extern "C" int effdet_live_tiles(const void* dreg, int dtype, int reg_ld, int B, int nlev, const int* H, const int* W,
                                 unsigned char* scratch, unsigned char* live32, unsigned char* live128, effdet_stream_t stream) {
  if (!dreg || !scratch || !live32 || !live128) return EFFDET_EINVAL;
  if (dtype != EFFDET_F32 && dtype != EFFDET_F32_SPLIT) return EFFDET_EUNSUPPORTED;
  if (reg_ld < 4 || reg_ld % 4 || (dtype == EFFDET_F32_SPLIT && reg_ld % 32) || ((unsigned long long)dreg & 15ull)) return EFFDET_EINVAL;
  LiveK k;
  const int rc = live_geometry(B, nlev, H, W, k);
  if (rc != EFFDET_OK) return rc;
  k.dreg = dreg; k.nz = scratch; k.hd = scratch + k.P; k.l32 = live32; k.l128 = live128; k.reg_ld = reg_ld;
  k.mask = dtype == EFFDET_F32 ? 0x7fffffffu : 0x7fff7fffu;
  hipStream_t st = (hipStream_t)stream;
  long long g = (k.P + 63) / 64;                  // 16 pixels per pass, four passes per workgroup
  if (g > 8192) g = 8192;
  hipLaunchKernelGGL(live_nz_kernel, dim3((unsigned)g), dim3(256), 0, st, k);
  EFFDET_CHECK_LAUNCH();
  hipLaunchKernelGGL(live_hdist_kernel, dim3((unsigned)((k.P + 255) / 256)), dim3(256), 0, st, k);
  EFFDET_CHECK_LAUNCH();
  hipLaunchKernelGGL(live_flags_kernel, dim3((unsigned)k.ntiles), dim3(128), 0, st, k);
  EFFDET_CHECK_LAUNCH();
  return EFFDET_OK;
}

// The same flags from a per-pixel map the caller brings (include/effdet_needed_tiles.h: the positive-pixel map of the forward pass):
// the row-distance and flag kernels above read it where they read live_nz_kernel's.
extern "C" int effdet_live_tiles_from_map(const unsigned char* map, int B, int nlev, const int* H, const int* W, unsigned char* scratch,
                                          unsigned char* live32, unsigned char* live128, effdet_stream_t stream) {
  if (!map || !scratch || !live32 || !live128) return EFFDET_EINVAL;
  LiveK k;
  const int rc = live_geometry(B, nlev, H, W, k);
  if (rc != EFFDET_OK) return rc;
  k.dreg = nullptr; k.nz = const_cast<unsigned char*>(map); k.hd = scratch + k.P; k.l32 = live32; k.l128 = live128; k.reg_ld = 0; k.mask = 0u;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(live_hdist_kernel, dim3((unsigned)((k.P + 255) / 256)), dim3(256), 0, st, k);
  EFFDET_CHECK_LAUNCH();
  hipLaunchKernelGGL(live_flags_kernel, dim3((unsigned)k.ntiles), dim3(128), 0, st, k);
  EFFDET_CHECK_LAUNCH();
  return EFFDET_OK;
}

// The compacted lists of the set live32 flags, per radius (include/effdet_unit_lists.h)
extern "C" int effdet_unit_lists(const unsigned char* live32, const unsigned char* live128, long long steps, long long tiles, int* units,
                                 int* counts, effdet_stream_t stream) {
  if (!live32 || !live128 || !units || !counts) return EFFDET_EINVAL;
  if (steps < 1 || tiles < 1 || tiles > steps) return EFFDET_EINVAL;
  if (steps >= 0x40000000LL) return EFFDET_EUNSUPPORTED;
  hipLaunchKernelGGL(unit_lists_kernel, dim3(EFFDET_LIVE_RADII), dim3(256), 0, (hipStream_t)stream, live32, live128, steps, tiles, units, counts);
  EFFDET_CHECK_LAUNCH();
  return EFFDET_OK;
}
