// Sliced inference (include/effdet_slices.h holds the semantics; tests/slices_restated.py restates them in NumPy fp32 and the merge
// must equal it BIT FOR BIT, so this file is built with -ffp-contract=off like wbf.hip).
//   slice_kernel        the tile extractor: grid (ceil(h * w / 256), tiles of the range), one thread per output pixel, adjacent threads
//                       along x, so the NCHW plane reads, the NHWC pixel reads and the 16-byte stores of a wave are runs of neighbouring
//                       addresses.  Row and column are clamped into the source before they become addresses, whatever the table holds.
//                       The elements travel as raw bits (no float ever exists): NaN payloads survive.  SRC selects the loads as in
//                       resample.hip: three planes; one 16-byte (fp32) or 8-byte (bf16) load where the map is aligned for it; three
//                       element loads for any other map.
//   slice_key_kernel    one thread per (tile, row) slot j = tile * R + row: the 32-bit rs_score_key of a row that takes part, all ones
//                       for one that does not (no finite score has that key), value j.  rs_sort orders them per image: stable, so
//                       score descending, then tile, then row, the rows that do not take part last.
//   slice_merge_kernel  ONE 1024-thread workgroup per image.  The survivors' transformed boxes (16 B) and labels (2 B) are loaded into
//                       LDS in sorted order: 144 KiB at the 8192 cap.  Candidate q belongs to thread q % 1024, which keeps "alive" as a
//                       bit of a register (at most eight) and their scores in registers too.  A round: every thread offers its lowest
//                       alive candidate and -- NMM -- the hull of what it killed in the round before; a wave + cross-wave reduction
//                       through ping-ponged slots (ONE barrier) gives every thread the next keeper and the previous keeper's finished
//                       hull; that keeper's owner writes its row (stores only: a round loads nothing from global memory); every
//                       thread tests its alive candidates against the keeper's own box (an LDS broadcast).  Rounds are bounded
//                       by max_det, not by the candidates.  min / fminf / fmaxf are order-independent: the result does not depend on
//                       how the candidates are dealt.
#include "box_geom.h"
#include "radix_sort.h"
#include "../../../include/effdet_slices.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------ tile extractor
enum { SRC_NCHW = 0, SRC_NHWC_VEC = 1, SRC_NHWC_ELEM = 2 };

__device__ __forceinline__ int clamp_at(int origin, int o, int n) {
  const long long v = (long long)origin + o;
  return v < 0 ? 0 : (v > n - 1 ? n - 1 : (int)v);
}

__device__ __forceinline__ void store_bits(unsigned* dst, unsigned c0, unsigned c1, unsigned c2) { *(uint4*)dst = make_uint4(c0, c1, c2, 0u); }
__device__ __forceinline__ void store_bits(unsigned short* dst, unsigned c0, unsigned c1, unsigned c2) {
  *(uint4*)dst = make_uint4(c0 | (c1 << 16), c2, 0u, 0u);
}

// U: the element's bits (unsigned: fp32, unsigned short: bf16)
template <typename U, int SRC>
__global__ __launch_bounds__(256) void slice_kernel(const U* __restrict__ src, U* __restrict__ dst, const effdet_slice_tile_t* __restrict__ tiles,
                                                    int H, int W, int T, int t0, int nt, int h, int w, long long ld, long long bstride) {
  constexpr int CE = 16 / sizeof(U);
  const int ty = (int)blockIdx.y < nt ? (int)blockIdx.y : nt - 1;
  const int r = blockIdx.x * 256 + threadIdx.x;            // h * w <= 2^30
  if (r >= h * w) return;
  const int t = t0 + ty, b = t / T, j = t - b * T;         // t < B * T: b < B
  const int4 rec = ((const int4*)tiles)[j];                // x0, y0, (mx, my)
  const int oy = r / w, ox = r - oy * w;
  const int sy = clamp_at(rec.y, oy, H), sx = clamp_at(rec.x, ox, W);
  unsigned c0, c1, c2;
  if (SRC == SRC_NCHW) {
    const long long hw = (long long)H * W;
    const U* px = src + (long long)b * 3 * hw + (long long)sy * W + sx;
    c0 = px[0]; c1 = px[hw]; c2 = px[2 * hw];
  } else {
    const U* px = src + (long long)b * bstride + ((long long)sy * W + sx) * ld;
    if (SRC == SRC_NHWC_VEC && sizeof(U) == 4) {
      const uint4 q = *(const uint4*)px;
      c0 = q.x; c1 = q.y; c2 = q.z;
    } else if (SRC == SRC_NHWC_VEC) {
      const uint2 q = *(const uint2*)px;
      c0 = q.x & 0xffffu; c1 = q.x >> 16; c2 = q.y & 0xffffu;
    } else {
      c0 = px[0]; c1 = px[1]; c2 = px[2];
    }
  }
  store_bits(dst + ((long long)ty * h * w + r) * CE, c0, c1, c2);
}

template <typename U, int SRC> void launch_slice(const effdet_slice_images_t* p, hipStream_t stream) {
  const long long n = (long long)p->h * p->w;
  const int nt = p->t1 - p->t0;
  hipLaunchKernelGGL((slice_kernel<U, SRC>), dim3((unsigned)((n + 255) / 256), (unsigned)nt), dim3(256), 0, stream, (const U*)p->src, (U*)p->dst,
                     p->tiles, p->H, p->W, p->T, p->t0, nt, p->h, p->w, p->src_ld, p->src_bstride);
}

bool bad_side(int n) { return n < 1 || n > 32768; }

// --------------------------------------------------------------------------------------------------------------------------- merge
constexpr int SM_T = 1024, SM_MAX = EFFDET_SLICE_MAX_IN, SM_OWN = SM_MAX / SM_T;
constexpr unsigned SM_NO_KEY = 0xffffffffu;      // rs_score_key of no finite score (it is the key of the NaN with all bits set)
constexpr int SM_NONE = 0x7fffffff;

struct Merge {
  const float* score; const long long* label; const float* boxes; const int* count; const effdet_slice_tile_t* tiles;
  unsigned *key, *val;                           // the key kernel's outputs / the sorted pairs
  float* out_score; long long* out_label; float* out_boxes; int* out_count;
  int TPI, R, N, metric, class_aware, max_det; float W, H, thr, skip_thr;
};

// slot j of image b in the image's frame, clipped (step 1 of the header)
__device__ __forceinline__ float4 sm_box(const Merge& p, int b, int j) {
  const int t = j / p.R;
  const effdet_slice_tile_t rec = p.tiles[t];
  float4 bx = ((const float4*)p.boxes)[(long long)b * p.N + j];
  const float fx = (float)rec.x0, fy = (float)rec.y0;
  bx.x = bx.x * rec.mx + fx; bx.z = bx.z * rec.mx + fx;
  bx.y = bx.y * rec.my + fy; bx.w = bx.w * rec.my + fy;
  bx.x = fmaxf(fminf(bx.x, p.W), 0.f); bx.z = fmaxf(fminf(bx.z, p.W), 0.f);
  bx.y = fmaxf(fminf(bx.y, p.H), 0.f); bx.w = fmaxf(fminf(bx.w, p.H), 0.f);
  return bx;
}

__global__ __launch_bounds__(256) void slice_key_kernel(const Merge p) {
  const int b = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
  if (j >= p.N) return;
  const int t = j / p.R, r = j - t * p.R;
  const long long at = (long long)b * p.N + j;
  unsigned k = SM_NO_KEY;
  if (r < min(max(p.count[(long long)b * p.TPI + t], 0), p.R)) {
    const float s = p.score[at];
    const long long l = p.label[at];
    if (s >= p.skip_thr && fabsf(s) < __builtin_huge_valf() && l >= 0 && l < 65536 && pos_finite(box_area(sm_box(p, b, j)))) k = rs_score_key(s);
  }
  p.key[at] = k; p.val[at] = (unsigned)j;
}

__device__ __forceinline__ bool sm_match(const Merge& p, const float4& a, float aa, const float4& c) {
  float inter;
  if (!box_inter(a, c, inter)) return false;                            // (inter = 0: 0 > thr never holds)
  const float ca = box_area(c);
  const float m = p.metric == EFFDET_SLICE_IOS ? inter / fminf(aa, ca) : inter / (aa + ca - inter);
  return m > p.thr;
}

template <int NMM>
__global__ __launch_bounds__(SM_T) void slice_merge_kernel(const Merge p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  float4* tb = (float4*)smem_raw;                                       // [N] transformed boxes in sorted order
  unsigned short* tl = (unsigned short*)(tb + p.N);                     // [N] labels
  __shared__ int red_i[2][SM_T / 64];
  __shared__ float4 red_h[2][SM_T / 64];
  __shared__ int s_m;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long base = (long long)b * p.N;
  const unsigned* sk = p.key + base;
  const unsigned* sv = p.val + base;
  const float inf = __builtin_huge_valf();

  if (tid == 0) s_m = 0;
  __syncthreads();
  float own_score[SM_OWN];                                              // scores of this thread's candidates: no global load in a round
#pragma unroll
  for (int u = 0; u < SM_OWN; ++u) {
    const int q = tid + u * SM_T;
    own_score[u] = 0.f;
    if (q >= p.N || sk[q] == SM_NO_KEY) continue;
    if (q + 1 == p.N || sk[q + 1] == SM_NO_KEY) s_m = q + 1;            // (the survivors are a prefix: one thread sees its end)
    const int j = (int)sv[q];
    tb[q] = sm_box(p, b, j); tl[q] = (unsigned short)p.label[base + j]; own_score[u] = p.score[base + j];
  }
  __syncthreads();
  const int M = s_m;

  unsigned alive = 0u;                                                  // bit u: candidate tid + u * 1024 is neither keeper nor dead
#pragma unroll
  for (int u = 0; u < SM_OWN; ++u) if (tid + u * SM_T < M) alive |= 1u << u;
  int kept = 0, ki = 0;
  float4 kb = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 hull = make_float4(inf, inf, -inf, -inf);                      // of what this thread killed for keeper ki
  for (int round = 0;; ++round) {
    int mi = alive ? tid + (__ffs((int)alive) - 1) * SM_T : SM_NONE;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      mi = min(mi, __shfl_xor(mi, o, 64));
      if (NMM) {
        hull.x = fminf(hull.x, __shfl_xor(hull.x, o, 64)); hull.y = fminf(hull.y, __shfl_xor(hull.y, o, 64));
        hull.z = fmaxf(hull.z, __shfl_xor(hull.z, o, 64)); hull.w = fmaxf(hull.w, __shfl_xor(hull.w, o, 64));
      }
    }
    if (lane == 0) { red_i[round & 1][wave] = mi; if (NMM) red_h[round & 1][wave] = hull; }
    __syncthreads();
    mi = red_i[round & 1][lane & 15];
    if (NMM) hull = red_h[round & 1][lane & 15];
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
      mi = min(mi, __shfl_xor(mi, o, 64));
      if (NMM) {
        hull.x = fminf(hull.x, __shfl_xor(hull.x, o, 64)); hull.y = fminf(hull.y, __shfl_xor(hull.y, o, 64));
        hull.z = fmaxf(hull.z, __shfl_xor(hull.z, o, 64)); hull.w = fmaxf(hull.w, __shfl_xor(hull.w, o, 64));
      }
    }
    // (block-uniform from here: every thread reduced the same 16 slots)
    if (kept > 0 && (ki & (SM_T - 1)) == tid) {                         // the previous keeper's row, by its owner: the hull is complete now
      const long long at = (long long)b * p.max_det + (kept - 1);
      float4 ob = kb;
      if (NMM) ob = make_float4(fminf(kb.x, hull.x), fminf(kb.y, hull.y), fmaxf(kb.z, hull.z), fmaxf(kb.w, hull.w));
      float s = own_score[0];
#pragma unroll
      for (int u = 1; u < SM_OWN; ++u) if (u == (ki >> 10)) s = own_score[u];
      p.out_score[at] = s; p.out_label[at] = (long long)tl[ki]; ((float4*)p.out_boxes)[at] = ob;
    }
    if (mi == SM_NONE || kept == p.max_det) break;
    ki = mi; kb = tb[ki];
    const int kl = tl[ki];
    const float ka = box_area(kb);
    if ((ki & (SM_T - 1)) == tid) alive &= ~(1u << (ki >> 10));
    hull = make_float4(inf, inf, -inf, -inf);
#pragma unroll
    for (int u = 0; u < SM_OWN; ++u)
      if ((alive >> u) & 1u) {
        const int q = tid + u * SM_T;
        const float4 c = tb[q];
        if ((!p.class_aware || tl[q] == kl) && sm_match(p, kb, ka, c)) {
          alive &= ~(1u << u);
          if (NMM) { hull.x = fminf(hull.x, c.x); hull.y = fminf(hull.y, c.y); hull.z = fmaxf(hull.z, c.z); hull.w = fmaxf(hull.w, c.w); }
        }
      }
    ++kept;
  }
  for (int k = kept + tid; k < p.max_det; k += SM_T) {
    const long long at = (long long)b * p.max_det + k;
    p.out_score[at] = 0.f; p.out_label[at] = 0; ((float4*)p.out_boxes)[at] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if (tid == 0) p.out_count[b] = kept;
}

bool merge_shape_ok(int TPI, int R) {
  return TPI >= 1 && TPI <= EFFDET_SLICE_MAX_TILES && R >= 1 && (long long)TPI * R <= SM_MAX;
}

size_t carve(RsBufs<unsigned>& rs, void* base, int B, int N) {
  Carver c(base);
  rs_carve(rs, c, (size_t)B, (size_t)N);
  return c.off;
}

}  // namespace

extern "C" int effdet_slice_images(const effdet_slice_images_t* p, effdet_stream_t stream) {
  if (!p || !p->src || !p->dst || !p->tiles || ((uintptr_t)p->dst & 15) || ((uintptr_t)p->tiles & 15)) return EFFDET_EINVAL;
  if ((p->src_layout != EFFDET_RESAMPLE_NCHW && p->src_layout != EFFDET_RESAMPLE_NHWC) || (p->dtype != EFFDET_F32 && p->dtype != EFFDET_BF16) ||
      (p->src_layout == EFFDET_RESAMPLE_NCHW && p->dtype != EFFDET_F32) || p->B < 1 || p->B > 65535 || bad_side(p->H) || bad_side(p->W) ||
      bad_side(p->h) || bad_side(p->w) || p->T < 1 || (long long)p->B * p->T > 0x7fffffffLL || p->t0 < 0 || p->t1 <= p->t0 ||
      (long long)p->t1 > (long long)p->B * p->T || p->t1 - p->t0 > 65535)
    return EFFDET_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (p->src_layout == EFFDET_RESAMPLE_NCHW) {
    launch_slice<unsigned, SRC_NCHW>(p, s);
  } else {
    if (p->C < 3 || p->src_ld < p->C || p->src_bstride < 0) return EFFDET_EUNSUPPORTED;
    // one vector load per pixel reads 4 elements (16 bytes of fp32, 8 of bf16): it needs a fourth channel in memory and that alignment of every pixel
    const long long isz = p->dtype == EFFDET_F32 ? 4 : 2, al = 4 * isz;
    const bool vec = p->C >= 4 && ((uintptr_t)p->src % al) == 0 && (p->src_ld * isz) % al == 0 && (p->src_bstride * isz) % al == 0;
    if (p->dtype == EFFDET_F32) {
      if (vec) launch_slice<unsigned, SRC_NHWC_VEC>(p, s); else launch_slice<unsigned, SRC_NHWC_ELEM>(p, s);
    } else {
      if (vec) launch_slice<unsigned short, SRC_NHWC_VEC>(p, s); else launch_slice<unsigned short, SRC_NHWC_ELEM>(p, s);
    }
  }
  EFFDET_CHECK_LAUNCH();
  return EFFDET_OK;
}

extern "C" long long effdet_slice_merge_workspace_bytes(int B, int TPI, int R) {
  if (B < 1 || !merge_shape_ok(TPI, R)) return 0;
  RsBufs<unsigned> rs;
  return (long long)carve(rs, nullptr, B, TPI * R);
}

extern "C" int effdet_slice_merge(const effdet_slice_merge_t* d, void* workspace, long long workspace_bytes, effdet_stream_t stream) {
  if (!d || d->B < 1 || !d->score || !d->label || !d->boxes || !d->count || !d->tiles || !d->out_score || !d->out_label || !d->out_boxes ||
      !d->out_count || !workspace)
    return EFFDET_EINVAL;
  if (((uintptr_t)d->boxes & 15) || ((uintptr_t)d->out_boxes & 15) || ((uintptr_t)d->tiles & 15) || ((uintptr_t)d->score & 3) ||
      ((uintptr_t)d->label & 7) || ((uintptr_t)d->count & 3) || ((uintptr_t)d->out_score & 3) || ((uintptr_t)d->out_label & 7) ||
      ((uintptr_t)d->out_count & 3) || ((uintptr_t)workspace & 15))
    return EFFDET_EINVAL;
  if (!merge_shape_ok(d->TPI, d->R) || d->max_det < 1 || d->max_det > d->TPI * d->R || d->method < 0 || d->method > 1 || d->metric < 0 ||
      d->metric > 1 || !(d->thr >= 0.f && d->thr <= 1.f) || d->skip_thr != d->skip_thr || !pos_finite(d->W) || !pos_finite(d->H))
    return EFFDET_EUNSUPPORTED;
  const int N = d->TPI * d->R;
  RsBufs<unsigned> rs;
  if ((long long)carve(rs, workspace, d->B, N) > workspace_bytes) return EFFDET_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  Merge p;
  p.score = d->score; p.label = d->label; p.boxes = d->boxes; p.count = d->count; p.tiles = d->tiles;
  p.key = rs.ka; p.val = rs.va;
  p.out_score = d->out_score; p.out_label = d->out_label; p.out_boxes = d->out_boxes; p.out_count = d->out_count;
  p.TPI = d->TPI; p.R = d->R; p.N = N; p.metric = d->metric; p.class_aware = d->class_aware != 0; p.max_det = d->max_det;
  p.W = d->W; p.H = d->H; p.thr = d->thr; p.skip_thr = d->skip_thr;
  hipLaunchKernelGGL(slice_key_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)d->B), dim3(256), 0, st, p);
  EFFDET_CHECK_LAUNCH();
  unsigned *ki = rs.ka, *vi = rs.va, *ko = rs.kb, *vo = rs.vb;
  if (const int rc = rs_sort(ki, vi, ko, vo, rs.hist, d->B, (long long)N, rs.T, 0, 4, st)) return rc;
  p.key = ki; p.val = vi;
  const size_t lds = (size_t)N * 18;
  if (d->method == EFFDET_SLICE_NMM) {
    EFFDET_SET_MAX_LDS(slice_merge_kernel<1>, (size_t)SM_MAX * 18);     // (the cap: the attribute is set once per device)
    hipLaunchKernelGGL(slice_merge_kernel<1>, dim3(d->B), dim3(SM_T), lds, st, p);
  } else {
    EFFDET_SET_MAX_LDS(slice_merge_kernel<0>, (size_t)SM_MAX * 18);
    hipLaunchKernelGGL(slice_merge_kernel<0>, dim3(d->B), dim3(SM_T), lds, st, p);
  }
  EFFDET_CHECK_LAUNCH();
  return EFFDET_OK;
}
