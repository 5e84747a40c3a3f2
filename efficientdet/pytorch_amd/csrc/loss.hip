// Focal + box-regression detection loss on device (reference models/losses.py:32-152), batched over the images with no host loop
// and no device->host sync.  ONE family of kernels serves the reference's constants, the IoU-family box terms
// (include/effdet_box_loss.h) and the loss options (include/effdet_loss_opts.h); what differs is a compile-time policy:
//
//   focal policy  FocalDefault: alpha 0.25, gamma 2 as q * q, __logf, contraction left to the compiler (the reference's constants)
//                 FocalP:       alpha / gamma / label smoothing as launch arguments, exp2f(gamma log2f(u)), no contraction
//                 FocalQfl / FocalVfl: the quality focal / varifocal loss on a SOFT target (include/effdet_quality_loss.h): the
//                               per-anchor quality q[b][a] that loss_quality_kernel leaves after the assign pass, read where code >= 0
//   knee policy   KneeDefault:  the smooth-L1 knee 1/9 with the literals 0.5f * 9.0f, 0.5f / 9.0f, 9.0f spelled out
//                 KneeBeta:     the knee beta as a launch argument (0.5 d^2 / beta, d - 0.5 beta, diff / beta)
//   The default path is NOT the option kernels with default values: its arithmetic (and its single assign pass) stays as it was.
//
//   assign   one thread per (image, anchor): IoU against the image's valid annotations (pad rows label == -1 skipped), max /
//            first-argmax, state = positive / negative / ignored, smooth-L1 on the positives; stat[b] = {cls_sum, reg_sum, num_pos,
//            num_valid_annotations} (one 128-byte line per image).  num_pos is an INTEGER count (int atomics: exact whatever the
//            order); the smooth-L1 partial of every workgroup goes to its own slot part_reg[b][block].
//              loss_assign_kernel                    bands 0.5 / 0.4 as constants, IoU loop and tail in one pass
//              opts_iou_kernel, opts_assign_kernel   the IoU loop -> best[b][a], barg[b][a]; with low_quality also gtmax[b][n] = max
//                       over the anchors, as an INTEGER atomicMax on the bit pattern of the non-negative IoU (order-independent,
//                       exact), first per workgroup in LDS, then one global atomic per (workgroup, row).  Then the same grid: bands
//                       on best; with low_quality the IoU loop once more, promoting an anchor whose IoU with any row equals that
//                       row's gtmax (> 0); then the same tail (assign_tail)
//              atss_select_kernel, atss_assign_kernel   the ATSS matcher (include/effdet_atss.h): one workgroup per (valid row, image)
//                       selects the row's topk nearest anchors of every level (64-bit keys (bits of d2) << 32 | index within the level:
//                       per-thread sorted lists in registers, then topk rounds of a workgroup arg-min) -> kth[b][n][level], the
//                       topk-th key, and thr[b][n] = mean + std of the candidates' IoUs; then loss_assign_kernel's grid: an anchor is
//                       a candidate of row n iff its own key <= kth[b][n][its level] (the same device function forms both keys), positive
//                       iff its IoU >= thr and its centre is inside the box; the same tail
//              loss_pos_map_kernel                   the default pass's decision alone, per pixel and ahead of the head: one byte per
//                       pixel = one of its 9 anchors is positive (include/effdet_needed_tiles.h: the sparse regression-tower forward)
//              tal_select_kernel, tal_assign_kernel     the task-aligned matcher (include/effdet_tal.h): one workgroup per (valid row,
//                       image) scans ALL anchors, centre test first, and keeps the topk largest metrics m = s^alpha u^beta of the
//                       PREDICTIONS (64-bit keys ~bits(m) << 32 | anchor, the same register lists and arg-min rounds) -> keys[b][n][16];
//                       every winner then claims its anchor with a 64-bit integer atomicMax of bits(u) << 32 | ~n into slot[b][a]
//                       (zeroed by tal_zero_kernel; max is order-independent, so two runs agree bit for bit); then
//                       loss_assign_kernel's grid reads the slot -> the row with the largest u, the first on a tie; the same tail.
//                       tal_target_kernel (after the quality pass): per row the normalised metric over its final anchors -> q
//   quality  loss_quality_kernel: with a quality loss, after whichever assign pass ran: one thread per (image, anchor), q = the IoU
//            between the decoded prediction and the assigned annotation (box_overlap, the box terms' expression) at a positive, else 0
//   cls      loss_cls_kernel<F>: one thread per 4 class probabilities (16-byte loads): focal BCE with the reference's clamp to
//            [1e-4, 1-1e-4], one partial per workgroup in part_cls[b][block].  loss_cls_pix_kernel<T, F, GRAD_ONLY, IT>: the same
//            sum AND d/d(logit) in one pass, or the gradient alone, written pixel-major (see there)
//   final    loss_final_kernel: adds every image's partials in a fixed pattern (one wave per image), then
//            losses[0] = mean_b cls_sum/max(npos,1), losses[1] = reg_weight * mean_b reg_sum/(4*npos)
//   backward loss_bwd_cls_kernel<T, F> / loss_cls_pix_kernel<T, F, true, 1>: d/d(logit) of the class term (through clamp and
//            sigmoid); loss_bwd_reg_kernel<T, Knee>: d/d(reg); scaled by the upstream scalar grads, written in the activation
//            dtype that the head's data-gradient convs consume
//   box_*    an IoU-family box term over the same assignment, in place of smooth-L1 (second half of the file)
//   No float atomics on anything but exact integer counts: two runs give bitwise-equal losses.
// HBM-bound: reads cls once per pass (15.7 MB / image fp32 at 80 classes).
#include "common.h"
#include "../../../include/effdet_box_loss.h"
#include "../../../include/effdet_loss_opts.h"
#include "../../../include/effdet_atss.h"
#include "../../../include/effdet_quality_loss.h"
#include "../../../include/effdet_tal.h"
#include "../../../include/effdet_needed_tiles.h"

namespace {

constexpr int SS = 32;        // floats per image in stat[] (one cache line)
constexpr int CLS_IT = 8;     // 4-element groups per thread in the class pass (fewer blocks -> fewer atomics)
constexpr int FG_IT = 4;      // ... in the forward+gradient pass: keeps the per-workgroup partials (summed by loss_final_kernel) few

struct LossK {
  const float* cls; const float* reg; const float* anchors; const float* annots; const float* gscale;
  float* losses; int* assign; float* stat;           // stat[b][SS]
  float* part_reg; float* part_cls; int na, ncb;     // per-workgroup partial sums [B][na] / [B][ncb] (na, ncb: workgroups per image)
  void* dcls; void* dreg;
  int B, nc, N; long long A;
  int dld;           // channel pitch of the pixel-major dcls layout (0 = [B][A][nc])
  int reg_ld;        // channel pitch of a pixel-major dreg layout [B][A/9][reg_ld] (channel = anchor*4 + k, zeros beyond 36); 0 = [B][A][4]
};

// the matcher of the options path: bands, low-quality matches and the buffers between its two passes
struct OptsK {
  float pos_iou, neg_iou; int low_quality;
  int* gtmax; float* best; int* barg;         // [B][N] bit patterns, [B][A], [B][A]
};

// the ATSS matcher: topk, the levels of the anchor table, and the buffers between its two passes
struct AtssK {
  int topk, num_levels;
  long long ls[EFFDET_ATSS_MAX_LEVELS + 1];
  unsigned long long* kth; float* thr;        // [B][N][EFFDET_ATSS_MAX_LEVELS] keys, [B][N]
};

// stat[b][2] holds the number of positive anchors as an int32 bit pattern (integer atomics: exact, order-independent)
__device__ __forceinline__ float npos(const float* st) { return (float)__float_as_int(st[2]); }

// d(loss)/d(logit) where the class term does not reach p (ignored anchor, image without annotations): 0 -- but NaN for a NaN (or inf)
// p, because autograd's sigmoid backward still multiplies that zero by p (1 - p) (models/losses.py:53-57, :96)
__device__ __forceinline__ float nan_zero(float p) { return p - p; }

__device__ __forceinline__ int label_of(const LossK& p, int b, int code) {
  return code >= 0 ? (int)p.annots[((long long)b * p.N + code) * 5 + 4] : -1;
}

// ---- focal policies: f(praw, target_one, tq, dldp) -> the per-element class term; dldp its derivative wrt the (unclamped)
// probability.  tq = f.quality(b * A + a) is the soft target of a POSITIVE anchor (include/effdet_quality_loss.h), which the kernels
// ask for where code >= 0 only; the hard-target policies have none (no load, the argument is dead)
struct FocalDefault {
  __device__ __forceinline__ float quality(long long) const { return 0.f; }
  __device__ __forceinline__ float operator()(float praw, bool target_one, float, float& dldp) const {
    constexpr float ALPHA = 0.25f;
    const float pc = nan_min(nan_max(praw, 1e-4f), 1.0f - 1e-4f);         // (torch.clamp keeps a NaN: so does the loss)
    const bool pass = (praw >= 1e-4f) && (praw <= 1.0f - 1e-4f);   // clamp passes the gradient inside the range
    float l, d;
    if (target_one) {
      const float q = 1.f - pc, lg = __logf(pc);
      l = -ALPHA * q * q * lg;
      d = ALPHA * (2.f * q * lg - q * q / pc);
    } else {
      const float lg = __logf(1.f - pc);
      l = -(1.f - ALPHA) * pc * pc * lg;
      d = (1.f - ALPHA) * (pc * pc / (1.f - pc) - 2.f * pc * lg);
    }
    dldp = pass ? d : 0.f;
    return l;
  }
};

// (no contraction: every kernel and layout computes the same bits)
struct FocalP {
  float alpha, gamma, eps;
  __device__ __forceinline__ float quality(long long) const { return 0.f; }
  __device__ __forceinline__ float operator()(float praw, bool target_one, float, float& dldp) const {
#pragma clang fp contract(off)
    const float pc = nan_min(nan_max(praw, 1e-4f), 1.0f - 1e-4f);
    const bool pass = (praw >= 1e-4f) && (praw <= 1.0f - 1e-4f);
    const float h = target_one ? 1.f : 0.f;
    const float t = h * (1.f - eps) + 0.5f * eps;
    const float u = target_one ? 1.f - pc : pc, aw = target_one ? alpha : 1.f - alpha;
    const float pw = exp2f(gamma * log2f(u));
    const float ce = -(t * logf(pc) + (1.f - t) * logf(1.f - pc));
    const float dce = (1.f - t) / (1.f - pc) - t / pc;
    const float dpw = gamma * pw / u;                                 // d pw / d u; du / dp = -1 for a target of one
    dldp = pass ? aw * ((target_one ? -dpw : dpw) * ce + pw * dce) : 0.f;
    return aw * pw * ce;
  }
};

// The soft-target policies (include/effdet_quality_loss.h): t = q[b][a] on the assigned label of a positive anchor, 0 elsewhere; q is a
// constant of the gradient.  No contraction, as FocalP.
__device__ __forceinline__ float soft_bce(float pc, float t, float& dce) {
#pragma clang fp contract(off)
  dce = (1.f - t) / (1.f - pc) - t / pc;
  return -(t * logf(pc) + (1.f - t) * logf(1.f - pc));
}

// GFL's quality focal loss: |t - p|^beta BCE(p, t)
struct FocalQfl {
  float beta; const float* q;
  __device__ __forceinline__ float quality(long long i) const { return q[i]; }
  __device__ __forceinline__ float operator()(float praw, bool target_one, float tq, float& dldp) const {
#pragma clang fp contract(off)
    const float pc = nan_min(nan_max(praw, 1e-4f), 1.0f - 1e-4f);
    const bool pass = (praw >= 1e-4f) && (praw <= 1.0f - 1e-4f);
    const float t = target_one ? tq : 0.f;
    const float u = fabsf(t - pc);
    float dce;
    const float ce = soft_bce(pc, t, dce);
    // u == 0 (p == t exactly): the power and its derivative are 0, not exp2(beta * -inf) and 0 / 0.  (A NaN t leaves pw * ce = NaN.)
    const float pw = u == 0.f ? 0.f : exp2f(beta * log2f(u));
    const float dpw = u == 0.f ? 0.f : beta * pw / u;                 // d pw / d u; du / dp = sign(p - t)
    dldp = pass ? (pc > t ? dpw : -dpw) * ce + pw * dce : 0.f;
    return pw * ce;
  }
};

// VarifocalNet's varifocal loss: t BCE(p, t) where t > 0, alpha p^gamma BCE(p, 0) elsewhere
struct FocalVfl {
  float alpha, gamma; const float* q;
  __device__ __forceinline__ float quality(long long i) const { return q[i]; }
  __device__ __forceinline__ float operator()(float praw, bool target_one, float tq, float& dldp) const {
#pragma clang fp contract(off)
    const float pc = nan_min(nan_max(praw, 1e-4f), 1.0f - 1e-4f);
    const bool pass = (praw >= 1e-4f) && (praw <= 1.0f - 1e-4f);
    const float t = target_one ? tq : 0.f;
    float l, d;
    if (!(t <= 0.f)) {                                                // t > 0, or a NaN t (which the loss must keep)
      float dce;
      const float ce = soft_bce(pc, t, dce);
      l = t * ce; d = t * dce;
    } else {
      const float pw = exp2f(gamma * log2f(pc)), ce = -logf(1.f - pc);
      l = alpha * pw * ce;
      d = alpha * (gamma * pw / pc * ce + pw / (1.f - pc));
    }
    dldp = pass ? d : 0.f;
    return l;
  }
};

// ---- knee policies of smooth-L1 on d = |diff|: the term, and its derivative wrt diff (sgn = sign(diff)).
// (0 * d: autograd of the reference's where(d <= 1/9, 4.5 d^2, d - 1/18) sends 0 * 9d into the branch not taken -- NaN when d is
//  NaN or inf, and the gradient with it)
struct KneeDefault {
  __device__ __forceinline__ float term(float d) const { return (d <= 1.0f / 9.0f) ? 0.5f * 9.0f * d * d : d - 0.5f / 9.0f; }
  __device__ __forceinline__ float grad(float diff, float d, float sgn) const { return (d <= 1.0f / 9.0f) ? 9.0f * d * sgn : sgn + 0.f * d; }
};
struct KneeBeta {
  float beta;
  __device__ __forceinline__ float term(float d) const { return (d <= beta) ? 0.5f * d * d / beta : d - 0.5f * beta; }
  __device__ __forceinline__ float grad(float diff, float d, float sgn) const { return (d <= beta) ? diff / beta : sgn + 0.f * d; }
};

// ---- shared device functions
// the sum of s over the workgroup (4 waves) -> *out, by thread 0, in a fixed association order (part of the bitwise-determinism contract)
__device__ __forceinline__ void block_partial(float s, float* out) {
  __shared__ float red[4];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) *out = (red[0] + red[1]) + (red[2] + red[3]);
}

// IoU of anchor `an` (area aarea) with the box at r[0..3].  Every pass of either matcher evaluates THIS function, so the equality test
// of the promotion pass compares a value with a maximum over the same values (no contraction: whether a multiply-add is fused must not
// depend on the kernel the function is inlined into)
__device__ __forceinline__ float assign_iou(const float4 an, const float aarea, const float* r) {
#pragma clang fp contract(off)
  const float bx1 = r[0], by1 = r[1], bx2 = r[2], by2 = r[3];
  const float barea = (bx2 - bx1) * (by2 - by1);
  float iw = fminf(an.z, bx2) - fmaxf(an.x, bx1); float ih = fminf(an.w, by2) - fmaxf(an.y, by1);
  iw = fmaxf(iw, 0.f); ih = fmaxf(ih, 0.f);
  const float ua = fmaxf(aarea + barea - iw * ih, 1e-8f);
  const float iou = iw * ih / ua;
  return iou;
}

// thread 0 compacts the valid rows of chunk [n0, n0 + 64) of image b into ann[] (order preserved; ann[c][4] = the row index) -> their number
__device__ __forceinline__ int compact_chunk(const LossK& p, int b, int n0, float* ann) {
  int c = 0;
  for (int n = n0; n < min(p.N, n0 + 64); ++n) {
    const float* r = p.annots + ((long long)b * p.N + n) * 5;
    if (r[4] != -1.0f) { for (int q = 0; q < 5; ++q) ann[c * 5 + q] = r[q]; ann[c * 5 + 4] = (float)n; ++c; }
  }
  return c;
}

// ---- ATSS (include/effdet_atss.h)
// The selection key of anchor `an` (index i within its level) for the box at r[0..3]: (bits of d2) << 32 | i.  d2 >= 0, so its bit
// pattern orders as the float does, and the index breaks a distance tie towards the lower anchor.  BOTH ATSS kernels form the key with
// THIS function (no contraction, as assign_iou): the candidate test of the assign pass compares a key with a k-th smallest of the same keys
__device__ __forceinline__ unsigned long long atss_key(const float4 an, const float* r, unsigned i) {
#pragma clang fp contract(off)
  const float acx = 0.5f * (an.x + an.z), acy = 0.5f * (an.y + an.w);
  const float gcx = 0.5f * (r[0] + r[2]), gcy = 0.5f * (r[1] + r[3]);
  const float dx = acx - gcx, dy = acy - gcy;
  const float d2 = dx * dx + dy * dy;
  return ((unsigned long long)__float_as_uint(d2) << 32) | i;
}

// mmdet's centre test: the anchor's centre lies more than 0.01 inside every side of the box
__device__ __forceinline__ bool atss_inside(const float4 an, const float* r) {
#pragma clang fp contract(off)
  const float acx = 0.5f * (an.x + an.z), acy = 0.5f * (an.y + an.w);
  return fminf(fminf(acx - r[0], acy - r[1]), fminf(r[2] - acx, r[3] - acy)) > 0.01f;
}

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int o) {
  const unsigned lo = __shfl_xor((unsigned)v, o, 64), hi = __shfl_xor((unsigned)(v >> 32), o, 64);
  return ((unsigned long long)hi << 32) | lo;
}

constexpr unsigned long long ATSS_NO_KEY = ~0ull;     // above every key (d2's sign bit is clear)
constexpr int ATSS_MAX_CAND = EFFDET_ATSS_MAX_LEVELS * EFFDET_ATSS_MAX_TOPK;

// the regression target of anchor `an` for the annotation at g[0..3] (models/losses.py:119-137)
__device__ __forceinline__ void encode_target(const float4 an, const float* g, float* t) {
  const float aw = an.z - an.x, ah = an.w - an.y, acx = an.x + 0.5f * aw, acy = an.y + 0.5f * ah;
  float gw = g[2] - g[0], gh = g[3] - g[1];
  const float gcx = g[0] + 0.5f * gw, gcy = g[1] + 0.5f * gh;
  gw = fmaxf(gw, 1.f); gh = fmaxf(gh, 1.f);
  t[0] = (gcx - acx) / aw / 0.1f; t[1] = (gcy - acy) / ah / 0.1f; t[2] = logf(gw / aw) / 0.2f; t[3] = logf(gh / ah) / 0.2f;
}

// the end of an assign pass.  live: a valid anchor of an image with annotations; negative / positive: the band decisions on its best
// IoU (two ifs, not else-if: with neg_iou == pos_iou the second wins).  -> assign[], the workgroup's smooth-L1 partial, num_pos
template <typename Knee>
__device__ __forceinline__ void assign_tail(const LossK& p, int b, long long a, bool ok, bool live, bool negative, bool positive,
                                            int barg, const float4 an, const Knee knee) {
  __shared__ float red[2][4];
  float regl = 0.f, pos = 0.f;
  int code = -2;                       // -2 ignore, -1 negative, >= 0 positive (annotation row)
  if (live) {
    if (negative) code = -1;
    if (positive) {
      code = barg; pos = 1.f;
      float t[4];
      encode_target(an, p.annots + ((long long)b * p.N + barg) * 5, t);
      const float4 r = ((const float4*)p.reg)[(long long)b * p.A + a];
      const float rv[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
      for (int q = 0; q < 4; ++q) regl += knee.term(fabsf(t[q] - rv[q]));
    }
  }
  if (ok) p.assign[(long long)b * p.A + a] = code;
  regl = wave_sum(regl); pos = wave_sum(pos);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { red[0][wave] = regl; red[1][wave] = pos; }
  __syncthreads();
  if (threadIdx.x == 0) {
    p.part_reg[(long long)b * p.na + blockIdx.x] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    atomicAdd((int*)(p.stat + b * SS + 2), (int)(red[1][0] + red[1][1] + red[1][2] + red[1][3]));    // num_pos is kept as an INTEGER (npos())
  }
}

// d(reg) of anchor a of image b (i = b * A + a) -> [B][A][4], or with reg_ld the pixel-major rows with a padded pitch (the layout the
// head's data-gradient conv reads; pad channels zeroed here)
template <typename T>
__device__ __forceinline__ void store_dreg_row(const LossK& p, long long b, long long a, long long i, f32x4 g) {
  if (p.reg_ld) {
    const long long pix = a / 9; const int an = (int)(a - pix * 9);
    T* row = (T*)p.dreg + (b * (p.A / 9) + pix) * p.reg_ld;
    store4(row + an * 4, g);
    if (an == 8) for (int c = 36; c < p.reg_ld; c += 4) store4(row + c, f32x4{0.f, 0.f, 0.f, 0.f});
  } else {
    store4((T*)p.dreg + i * 4, g);
  }
}

// ---- kernels
// stat[] starts every pass at zero (num_pos is an integer atomic count).  A KERNEL, not hipMemsetAsync: captured into a hipGraph the
// memset node did not hold -- replays of the captured train step ran the assign pass on whatever the recycled workspace contained
// (num_pos ~ 1e9 from a float bit pattern: losses and every gradient scaled by ~1e-7; found in round 5 by comparing one replay with one
// eager step from the same state).  Kernel nodes only, like the NMS (postprocess.hip).
__global__ __launch_bounds__(256) void loss_zero_stat_kernel(float* __restrict__ stat, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) stat[i] = 0.f;
}

// ... and gtmax[] with it on the options path
__global__ __launch_bounds__(256) void opts_zero_kernel(float* __restrict__ stat, int n, int* __restrict__ gtmax, int m) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) stat[i] = 0.f;
  else if (i - n < m) gtmax[i - n] = 0;
}

__global__ __launch_bounds__(256) void loss_assign_kernel(const LossK p) {
  const int b = blockIdx.y;
  const long long a = blockIdx.x * 256LL + threadIdx.x;
  __shared__ float ann[64 * 5];
  __shared__ int nvalid_s;
  float best = -1.0f; int barg = -1;
  float4 an = make_float4(0, 0, 0, 0);
  const bool ok = a < p.A;
  if (ok) an = ((const float4*)p.anchors)[a];
  const float aarea = (an.z - an.x) * (an.w - an.y);
  int total_valid = 0;
  for (int n0 = 0; n0 < p.N; n0 += 64) {       // the image's valid annotations through LDS, in chunks of 64
    __syncthreads();
    if (threadIdx.x == 0) nvalid_s = compact_chunk(p, b, n0, ann);
    __syncthreads();
    const int c = nvalid_s;
    total_valid += c;
    if (ok) {
      for (int j = 0; j < c; ++j) {
        const float iou = assign_iou(an, aarea, ann + j * 5);
        if (iou > best) { best = iou; barg = (int)ann[j * 5 + 4]; }     // strict > keeps the FIRST max
      }
    }
  }
  assign_tail(p, b, a, ok, ok && total_valid > 0, best < 0.4f, best >= 0.5f, barg, an, KneeDefault{});
  if (blockIdx.x == 0 && threadIdx.x == 0) p.stat[b * SS + 3] = (float)total_valid;
}

// The positive-pixel map (include/effdet_needed_tiles.h): loss_assign_kernel's IoU loop and its decision (an image with a valid
// annotation, best >= 0.5f) ahead of the head, one thread per (image, pixel) over the pixel's 9 anchors -- the same device functions
// on the same operands, so map == (assign[] >= 0 OR-ed over the nine anchors) bit for bit.  No reg, no statistics, every byte stored.
struct PosMapK {
  unsigned char* map; int nlev, apix;
  int hw[EFFDET_MAX_SEG], poff[EFFDET_MAX_SEG], pix0[EFFDET_MAX_SEG];     // pixels per image, first pixel within an image, first byte of the level in the map
};

__global__ __launch_bounds__(256) void loss_pos_map_kernel(const LossK p, const PosMapK g) {
  const int b = blockIdx.y;
  const int q = blockIdx.x * 256 + threadIdx.x;
  __shared__ float ann[64 * 5];
  __shared__ int nvalid_s;
  const bool ok = q < g.apix;
  float4 an[9]; float aarea[9], best[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    an[k] = ok ? ((const float4*)p.anchors)[(long long)q * 9 + k] : make_float4(0, 0, 0, 0);
    aarea[k] = (an[k].z - an[k].x) * (an[k].w - an[k].y);
    best[k] = -1.0f;
  }
  int total_valid = 0;
  for (int n0 = 0; n0 < p.N; n0 += 64) {
    __syncthreads();
    if (threadIdx.x == 0) nvalid_s = compact_chunk(p, b, n0, ann);
    __syncthreads();
    const int c = nvalid_s;
    total_valid += c;
    if (ok) {
      for (int j = 0; j < c; ++j) {
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          const float iou = assign_iou(an[k], aarea[k], ann + j * 5);
          if (iou > best[k]) best[k] = iou;
        }
      }
    }
  }
  if (!ok) return;
  bool pos = false;
#pragma unroll
  for (int k = 0; k < 9; ++k) pos = pos || (best[k] >= 0.5f);
  int l = 0;
#pragma unroll
  for (int s = 1; s < EFFDET_MAX_SEG; ++s)
    if (s < g.nlev && q >= g.poff[s]) l = s;
  g.map[(long long)g.pix0[l] + (long long)b * g.hw[l] + (q - g.poff[l])] = (pos && total_valid > 0) ? 1 : 0;
}

__global__ __launch_bounds__(256) void opts_iou_kernel(const LossK p, const OptsK o) {
  const int b = blockIdx.y;
  const long long a = blockIdx.x * 256LL + threadIdx.x;
  __shared__ float ann[64 * 5];
  __shared__ int gm[64];
  __shared__ int nvalid_s;
  float best = -1.0f; int barg = -1;
  float4 an = make_float4(0, 0, 0, 0);
  const bool ok = a < p.A;
  if (ok) an = ((const float4*)p.anchors)[a];
  const float aarea = (an.z - an.x) * (an.w - an.y);
  int total_valid = 0;
  for (int n0 = 0; n0 < p.N; n0 += 64) {
    __syncthreads();
    if (threadIdx.x == 0) nvalid_s = compact_chunk(p, b, n0, ann);
    if (threadIdx.x < 64) gm[threadIdx.x] = 0;
    __syncthreads();
    const int c = nvalid_s;
    total_valid += c;
    if (ok) {
      for (int j = 0; j < c; ++j) {
        const float iou = assign_iou(an, aarea, ann + j * 5);
        if (iou > best) { best = iou; barg = (int)ann[j * 5 + 4]; }     // (the first max, as above)
        if (o.low_quality && iou > 0.f && __float_as_int(iou) > *(volatile int*)&gm[j]) atomicMax(&gm[j], __float_as_int(iou));
      }
    }
    if (o.low_quality) {
      __syncthreads();
      if ((int)threadIdx.x < c && gm[threadIdx.x] > 0) atomicMax(o.gtmax + (long long)b * p.N + (int)ann[threadIdx.x * 5 + 4], gm[threadIdx.x]);
    }
  }
  if (ok) { o.best[(long long)b * p.A + a] = best; o.barg[(long long)b * p.A + a] = barg; }
  if (blockIdx.x == 0 && threadIdx.x == 0) p.stat[b * SS + 3] = (float)total_valid;
}

__global__ __launch_bounds__(256) void opts_assign_kernel(const LossK p, const OptsK o, const KneeBeta knee) {
  const int b = blockIdx.y;
  const long long a = blockIdx.x * 256LL + threadIdx.x;
  __shared__ float ann[64 * 5];
  __shared__ float gmf[64];
  __shared__ int nvalid_s;
  const bool ok = a < p.A;
  float4 an = make_float4(0, 0, 0, 0);
  float best = -1.0f; int barg = -1;
  if (ok) { an = ((const float4*)p.anchors)[a]; best = o.best[(long long)b * p.A + a]; barg = o.barg[(long long)b * p.A + a]; }
  const bool any_valid = p.stat[b * SS + 3] > 0.f;
  bool promoted = false;
  if (o.low_quality && any_valid) {
    const float aarea = (an.z - an.x) * (an.w - an.y);
    for (int n0 = 0; n0 < p.N; n0 += 64) {
      __syncthreads();
      if (threadIdx.x == 0) {
        const int c = compact_chunk(p, b, n0, ann);
        for (int j = 0; j < c; ++j) gmf[j] = __int_as_float(o.gtmax[(long long)b * p.N + (int)ann[j * 5 + 4]]);
        nvalid_s = c;
      }
      __syncthreads();
      const int c = nvalid_s;
      if (ok) {
        for (int j = 0; j < c; ++j) {
          const float iou = assign_iou(an, aarea, ann + j * 5);
          promoted = promoted || (iou == gmf[j] && gmf[j] > 0.f);
        }
      }
    }
  }
  assign_tail(p, b, a, ok, ok && any_valid, best < o.neg_iou, (best >= o.pos_iou || promoted) && barg >= 0, barg, an, knee);
}

// ---- the ATSS matcher
// One workgroup per (row, image); a pad row exits at once.  Per level: every thread strides over the level's anchors and keeps its K
// smallest keys as a sorted list in registers (K >= topk is a compile-time bound: the insertion and the pop are fully unrolled, so the
// list never becomes a runtime-indexed array in scratch); then min(topk, level size) rounds, each the workgroup's arg-min over the
// heads of the lists (keys are distinct, so the minimum names its owner), which the owner pops.  The winners, in level then rank
// order, are the row's candidates; the last winner's key of a level is kth[b][n][level].  Then one IoU per candidate, and thread 0
// forms thr sequentially in that order.
template <int K>
__global__ __launch_bounds__(256) void atss_select_kernel(const LossK p, const AtssK t) {
  const int n = blockIdx.x, b = blockIdx.y;
  const float* rp = p.annots + ((long long)b * p.N + n) * 5;
  if (rp[4] == -1.0f) return;
  const float r[4] = {rp[0], rp[1], rp[2], rp[3]};
  __shared__ unsigned long long wmin[2][4];
  __shared__ long long cand[ATSS_MAX_CAND];
  __shared__ float ciou[ATSS_MAX_CAND];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float4* anc = (const float4*)p.anchors;
  int cnt = 0, round = 0;
  for (int l = 0; l < t.num_levels; ++l) {
    const long long base = t.ls[l], size = t.ls[l + 1] - base;
    unsigned long long keys[K];
#pragma unroll
    for (int j = 0; j < K; ++j) keys[j] = ATSS_NO_KEY;
    for (long long i = threadIdx.x; i < size; i += 256) {
      const unsigned long long key = atss_key(anc[base + i], r, (unsigned)i);
      if (key < keys[K - 1]) {
#pragma unroll
        for (int j = K - 1; j > 0; --j) {                    // new[j] = min(old[j], max(old[j - 1], key)), from the top down
          const unsigned long long m = keys[j - 1] > key ? keys[j - 1] : key;
          keys[j] = keys[j] < m ? keys[j] : m;
        }
        keys[0] = keys[0] < key ? keys[0] : key;
      }
    }
    const int k = (int)(size < (long long)t.topk ? size : (long long)t.topk);
    for (int q = 0; q < k; ++q, ++round) {
      unsigned long long m = keys[0];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) { const unsigned long long v = shfl_xor_u64(m, o); m = v < m ? v : m; }
      unsigned long long* w = wmin[round & 1];               // two slots: one barrier per round
      if (lane == 0) w[wave] = m;
      __syncthreads();
      const unsigned long long m01 = w[0] < w[1] ? w[0] : w[1], m23 = w[2] < w[3] ? w[2] : w[3];
      m = m01 < m23 ? m01 : m23;
      if (keys[0] == m) {                                    // the owner pops its head
#pragma unroll
        for (int j = 0; j + 1 < K; ++j) keys[j] = keys[j + 1];
        keys[K - 1] = ATSS_NO_KEY;
      }
      if (threadIdx.x == 0) {
        cand[cnt] = base + (long long)(unsigned)m;
        if (q == k - 1) t.kth[((long long)b * p.N + n) * EFFDET_ATSS_MAX_LEVELS + l] = m;
      }
      ++cnt;
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < cnt) {
    const float4 an = anc[cand[threadIdx.x]];
    ciou[threadIdx.x] = assign_iou(an, (an.z - an.x) * (an.w - an.y), r);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma clang fp contract(off)
    float sum = 0.f;
    for (int j = 0; j < cnt; ++j) sum += ciou[j];
    const float mean = sum / (float)cnt;
    float sq = 0.f;
    for (int j = 0; j < cnt; ++j) { const float d = ciou[j] - mean; sq += d * d; }
    const float var = cnt < 2 ? 0.f : sq / (float)(cnt - 1);
    t.thr[(long long)b * p.N + n] = mean + sqrtf(var);
  }
}

// loss_assign_kernel's grid and loop with the ATSS rule: per valid row (thr and the kth keys of every level ride along in LDS) the
// anchor's own key against the row's kth of the anchor's level, then the two tests of a positive; the best IoU among the rows it is
// positive for with strict > (the first row wins a tie)
__global__ __launch_bounds__(256) void atss_assign_kernel(const LossK p, const AtssK t, const KneeBeta knee) {
  const int b = blockIdx.y;
  const long long a = blockIdx.x * 256LL + threadIdx.x;
  __shared__ float ann[64 * 5];
  __shared__ float thr_s[64];
  __shared__ unsigned long long kth_s[64 * EFFDET_ATSS_MAX_LEVELS];
  __shared__ int nvalid_s;
  float best = -1.0f; int barg = -1;
  float4 an = make_float4(0, 0, 0, 0);
  const bool ok = a < p.A;
  int lev = 0; unsigned idx = 0;
  if (ok) {
    an = ((const float4*)p.anchors)[a];
    while (lev + 1 < t.num_levels && a >= t.ls[lev + 1]) ++lev;
    idx = (unsigned)(a - t.ls[lev]);
  }
  const float aarea = (an.z - an.x) * (an.w - an.y);
  int total_valid = 0;
  for (int n0 = 0; n0 < p.N; n0 += 64) {
    __syncthreads();
    if (threadIdx.x == 0) nvalid_s = compact_chunk(p, b, n0, ann);
    __syncthreads();
    const int c = nvalid_s;
    total_valid += c;
    for (int e = threadIdx.x; e < c * EFFDET_ATSS_MAX_LEVELS; e += 256) {
      const int j = e / EFFDET_ATSS_MAX_LEVELS, l = e - j * EFFDET_ATSS_MAX_LEVELS;
      const long long row = (long long)b * p.N + (int)ann[j * 5 + 4];
      kth_s[e] = l < t.num_levels ? t.kth[row * EFFDET_ATSS_MAX_LEVELS + l] : 0ull;
      if (l == 0) thr_s[j] = t.thr[row];
    }
    __syncthreads();
    if (ok) {
      for (int j = 0; j < c; ++j) {
        const float* r = ann + j * 5;
        if (atss_key(an, r, idx) > kth_s[j * EFFDET_ATSS_MAX_LEVELS + lev]) continue;
        const float iou = assign_iou(an, aarea, r);
        if (iou >= thr_s[j] && atss_inside(an, r) && iou > best) { best = iou; barg = (int)r[4]; }
      }
    }
  }
  assign_tail(p, b, a, ok, ok && total_valid > 0, barg < 0, barg >= 0, barg, an, knee);
  if (blockIdx.x == 0 && threadIdx.x == 0) p.stat[b * SS + 3] = (float)total_valid;
}

// 32-bit index arithmetic (A*nc < 2^31 is checked by the host): the 64-bit divisions per element of the first version made this HBM
// pass ALU-bound.  When nc % 4 == 0 a 4-element group never straddles two anchors.
template <typename F>
__global__ __launch_bounds__(256) void loss_cls_kernel(const LossK p, const F f) {
  const int b = blockIdx.y;
  const int per = (int)(p.A * p.nc);
  float s = 0.f;
  if (p.stat[b * SS + 3] > 0.f) {
    const float* c = p.cls + (long long)b * per;
    const int* asg = p.assign + (long long)b * p.A;
#pragma unroll
    for (int it = 0; it < CLS_IT; ++it) {
      const int e0 = ((blockIdx.x * CLS_IT + it) * 256 + threadIdx.x) * 4;
      if (e0 >= per) break;
      float v[4]; const int cnt = min(4, per - e0);
      const bool vec = cnt == 4 && ((per & 3) == 0);
      if (vec) { const f32x4 t = *(const f32x4*)(c + e0); v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3]; }
      else for (int q = 0; q < cnt; ++q) v[q] = c[e0 + q];
      int a = e0 / p.nc, k = e0 - a * p.nc;
      int code = asg[a];
      int lab = label_of(p, b, code);
      float tq = code >= 0 ? f.quality((long long)b * p.A + a) : 0.f;
      for (int q = 0; q < cnt; ++q) {
        if (code != -2) { float d; s += f(v[q], lab == k, tq, d); }
        if (++k == p.nc && q + 1 < cnt) {
          k = 0; ++a; code = asg[a]; lab = label_of(p, b, code);
          tq = code >= 0 ? f.quality((long long)b * p.A + a) : 0.f;
        }
      }
    }
  }
  block_partial(s, p.part_cls + (long long)b * p.ncb + blockIdx.x);
}

template <typename T, typename F>
__global__ __launch_bounds__(256) void loss_bwd_cls_kernel(const LossK p, const F f) {
  const int b = blockIdx.y;
  const int per = (int)(p.A * p.nc);
  const int e0 = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (e0 >= per) return;
  const float* st = p.stat + b * SS;
  const bool active = st[3] > 0.f;
  const float gs = active ? p.gscale[0] / ((float)p.B * fmaxf(npos(st), 1.0f)) : 0.f;
  const float* c = p.cls + (long long)b * per;
  const int* asg = p.assign + (long long)b * p.A;
  T* out = (T*)p.dcls + (long long)b * per;
  const int cnt = min(4, per - e0);
  const bool vec = cnt == 4 && ((per & 3) == 0);
  float v[4] = {0.f, 0.f, 0.f, 0.f}, g[4] = {0.f, 0.f, 0.f, 0.f};
  if (vec) { const f32x4 t = *(const f32x4*)(c + e0); v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3]; }
  else for (int q = 0; q < cnt; ++q) v[q] = c[e0 + q];
  int a = e0 / p.nc, k = e0 - a * p.nc;
  int code = asg[a];
  int lab = label_of(p, b, code);
  float tq = code >= 0 ? f.quality((long long)b * p.A + a) : 0.f;
  for (int q = 0; q < cnt; ++q) {
    if (active && code != -2) {
      float d; (void)f(v[q], lab == k, tq, d);
      g[q] = gs * d * v[q] * (1.f - v[q]);                 // through the sigmoid
    } else {
      g[q] = nan_zero(v[q]);
    }
    if (++k == p.nc && q + 1 < cnt) {
      k = 0; ++a; code = asg[a]; lab = label_of(p, b, code);
      tq = code >= 0 ? f.quality((long long)b * p.A + a) : 0.f;
    }
  }
  if (vec) store4(out + e0, f32x4{g[0], g[1], g[2], g[3]});
  else for (int q = 0; q < cnt; ++q) Elem<T>::st(out + e0 + q, g[q]);
}

// The class gradient written PIXEL-major with a padded channel pitch: dcls[b][pixel][dld], channel = anchor*nc + class,
// zeros in [9*nc, dld).  That is the layout the head's data-gradient conv reads as its input rows: with dld a multiple
// of 64 every 128-byte K-slice of a row is one aligned cache line (the natural 720-channel pitch = 1440 B straddles two
// lines for 3 pixels out of 4, and that conv is bound by its L2->LDS path).  Requires nc % 4 == 0.  IT 4-element groups per thread.
//   GRAD_ONLY:  backward -- the upstream gradient gscale[0] applied, no partial
//   otherwise:  forward AND gradient in ONE pass over cls (training): the focal sum goes to part_cls as in loss_cls_kernel, and the
//               gradient is written for an upstream gradient of 1.  The upstream scalar is applied downstream (it multiplies a LINEAR
//               chain: the head's data-gradient conv takes it as its per-image output scale, the retina_cls parameter gradients are
//               scaled after unpacking), so backward never re-reads the 15.7 MB/image of probabilities.
template <typename T, typename F, bool GRAD_ONLY, int IT>
__global__ __launch_bounds__(256) void loss_cls_pix_kernel(const LossK p, const F f) {
  const int b = blockIdx.y;
  const int apix = (int)(p.A / 9), perp = apix * p.dld, cmax = 9 * p.nc;
  const float* st = p.stat + b * SS;
  const bool active = st[3] > 0.f;
  const float gs = (GRAD_ONLY ? p.gscale[0] : 1.0f) / ((float)p.B * fmaxf(npos(st), 1.0f));
  float s = 0.f;
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    const int e0 = ((blockIdx.x * IT + it) * 256 + threadIdx.x) * 4;
    if (e0 >= perp) break;
    const int pix = e0 / p.dld, ch = e0 - pix * p.dld;
    f32x4 g = f32x4{0.f, 0.f, 0.f, 0.f};
    if (ch < cmax) {
      const int an = ch / p.nc, k = ch - an * p.nc, a = pix * 9 + an;
      const int code = active ? p.assign[(long long)b * p.A + a] : -2;
      const f32x4 v = *(const f32x4*)(p.cls + (long long)b * p.A * p.nc + (long long)pix * cmax + ch);
      if (code != -2) {
        const int lab = label_of(p, b, code);
        const float tq = code >= 0 ? f.quality((long long)b * p.A + a) : 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float d; s += f(v[q], lab == k + q, tq, d);
          g[q] = gs * d * v[q] * (1.f - v[q]);                 // through the sigmoid
        }
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) g[q] = nan_zero(v[q]);
      }
    }
    store4((T*)p.dcls + (long long)b * perp + e0, g);
  }
  if constexpr (!GRAD_ONLY) block_partial(s, p.part_cls + (long long)b * p.ncb + blockIdx.x);
}

// one workgroup: wave w adds the partials of images w, w + 16, ... (lane-strided, then the fixed shuffle tree), thread 0 the images
__global__ __launch_bounds__(1024) void loss_final_kernel(const LossK p, const float reg_weight) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // fixed summation pattern (lane-strided with four chains in flight -- the loop is pure L2 latency -- then the shuffle tree)
  auto lane_sum = [&](const float* q, int n) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int i = lane;
    for (; i + 192 < n; i += 256) { s0 += q[i]; s1 += q[i + 64]; s2 += q[i + 128]; s3 += q[i + 192]; }
    for (; i < n; i += 64) s0 += q[i];
    return wave_sum((s0 + s1) + (s2 + s3));
  };
  for (int b = wave; b < p.B; b += 16) {
    const float c = lane_sum(p.part_cls + (long long)b * p.ncb, p.ncb), r = lane_sum(p.part_reg + (long long)b * p.na, p.na);
    if (lane == 0) { p.stat[b * SS + 0] = c; p.stat[b * SS + 1] = r; }
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  float cl = 0.f, rl = 0.f;
  for (int b = 0; b < p.B; ++b) {
    const float* s = p.stat + b * SS;
    if (s[3] > 0.f) {
      cl += s[0] / fmaxf(npos(s), 1.0f);
      if (npos(s) > 0.f) rl += s[1] / (npos(s) * 4.0f);
    }
  }
  p.losses[0] = cl / (float)p.B; p.losses[1] = reg_weight * (rl / (float)p.B);
}

template <typename T, typename Knee>
__global__ void loss_bwd_reg_kernel(const LossK p, const Knee knee, const float reg_weight) {
  const long long total = (long long)p.B * p.A;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long b = i / p.A, a = i - b * p.A;
    const int code = p.assign[i];
    const float* st = p.stat + b * SS;
    f32x4 g = f32x4{0.f, 0.f, 0.f, 0.f};
    if (code >= 0 && st[3] > 0.f && npos(st) > 0.f) {
      const float gs = p.gscale[1] * reg_weight / ((float)p.B * npos(st) * 4.0f);
      float t[4];
      encode_target(((const float4*)p.anchors)[a], p.annots + (b * p.N + code) * 5, t);
      const float4 r = ((const float4*)p.reg)[i];
      const float rv[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float diff = rv[q] - t[q], d = fabsf(diff);
        const float sgn = diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f);
        g[q] = gs * knee.grad(diff, d, sgn);
      }
    }
    store_dreg_row<T>(p, b, a, i, g);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// IoU-family box regression losses (include/effdet_box_loss.h fixes the semantics): IoU / GIoU / DIoU / CIoU between the DECODED
// prediction and the assigned annotation, over the positives of the assign pass, in place of its smooth-L1 term.  The forward
// entry points run the smooth-L1 forward unchanged (assignment, focal term, losses[0]) and then two more kernels: one thread per
// anchor re-reads assign[] and puts the per-workgroup sum of the positives' losses into the same part_reg[b][block] slots, and a
// final kernel adds them per image in a fixed pattern and overwrites losses[1].  Kernel launches only, no float atomics.
constexpr float BOX_EPS = 1e-7f;
constexpr float BOX_4_PI2 = 0.40528473456935109f;    // 4 / pi^2

// d min(a, b) / d a (= d max(b, a) / d b) the way autograd splits it: 1 where a is selected, 0.5 on a tie
__device__ __forceinline__ float sel_lt(float a, float b) { return a < b ? 1.f : (a == b ? 0.5f : 0.f); }

// `decode` and `overlap` of include/effdet_box_loss.h for anchor an, annotation row g and regression row r: ONE expression for every
// IoU-family box term and for the quality target of include/effdet_quality_loss.h.  Contraction is left to the compiler, as it was
// when these lines stood in box_loss_elem: the box terms keep their bits.  (The quality target is computed by one kernel and read
// from memory by every class pass, so no two kernels have to agree on its bits.)
struct BoxOverlap {
  float aw, ah, pcx, pcy, dwr, dhr, pw, ph, px1, px2, py1, py2, gx1, gy1, gx2, gy2, gw, gh, iwr, ihr, iw, ih, I, U, D, iou;
};
#define EFFDET_BOX_OVERLAP_BODY \
  BoxOverlap o; \
  o.aw = an.z - an.x; o.ah = an.w - an.y; \
  const float acx = an.x + 0.5f * o.aw, acy = an.y + 0.5f * o.ah; \
  o.pcx = acx + 0.1f * r.x * o.aw; o.pcy = acy + 0.1f * r.y * o.ah; \
  o.dwr = 0.2f * r.z; o.dhr = 0.2f * r.w; \
  o.pw = expf(fminf(o.dwr, EFFDET_BOX_LOSS_DW_MAX)) * o.aw; o.ph = expf(fminf(o.dhr, EFFDET_BOX_LOSS_DW_MAX)) * o.ah; \
  o.px1 = o.pcx - 0.5f * o.pw; o.px2 = o.pcx + 0.5f * o.pw; o.py1 = o.pcy - 0.5f * o.ph; o.py2 = o.pcy + 0.5f * o.ph; \
  o.gx1 = g[0]; o.gy1 = g[1]; o.gx2 = g[2]; o.gy2 = g[3]; o.gw = o.gx2 - o.gx1; o.gh = o.gy2 - o.gy1; \
  o.iwr = fminf(o.px2, o.gx2) - fmaxf(o.px1, o.gx1); o.ihr = fminf(o.py2, o.gy2) - fmaxf(o.py1, o.gy1); \
  o.iw = fmaxf(o.iwr, 0.f); o.ih = fmaxf(o.ihr, 0.f); \
  o.I = o.iw * o.ih; o.U = o.pw * o.ph + o.gw * o.gh - o.I; o.D = o.U + BOX_EPS; o.iou = o.I / o.D; \
  return o;
__device__ __forceinline__ BoxOverlap box_overlap(float4 an, const float* __restrict__ g, float4 r) { EFFDET_BOX_OVERLAP_BODY }
// ... and the same lines with no multiply-add contracted, for the task-aligned matcher (include/effdet_tal.h): ITS kernels evaluate the
// IoU at several places (the select pass, its claim, the inspection call) and compare the bits, so whether a multiply-add is fused
// must not depend on the kernel the function is inlined into (as assign_iou)
__device__ __forceinline__ BoxOverlap box_overlap_strict(float4 an, const float* __restrict__ g, float4 r) {
#pragma clang fp contract(off)
  EFFDET_BOX_OVERLAP_BODY
}
#undef EFFDET_BOX_OVERLAP_BODY

// loss of one positive anchor; with GRAD its gradient wrt the regression row r (not yet scaled) in gr[4]
template <bool GRAD>
__device__ __forceinline__ float box_loss_elem(int kind, float4 an, const float* __restrict__ g, float4 r, float* gr) {
  const BoxOverlap o = box_overlap(an, g, r);
  const float aw = o.aw, ah = o.ah, pcx = o.pcx, pcy = o.pcy, dwr = o.dwr, dhr = o.dhr, pw = o.pw, ph = o.ph;
  const float px1 = o.px1, px2 = o.px2, py1 = o.py1, py2 = o.py2, gx1 = o.gx1, gy1 = o.gy1, gx2 = o.gx2, gy2 = o.gy2, gw = o.gw, gh = o.gh;
  const float iwr = o.iwr, ihr = o.ihr, iw = o.iw, ih = o.ih, I = o.I, U = o.U, D = o.D, iou = o.iou;
  const float cw = fmaxf(px2, gx2) - fminf(px1, gx1), ch = fmaxf(py2, gy2) - fminf(py1, gy1);
  float L = 1.f - iou;
  // gradients of L wrt the intermediate quantities, accumulated term by term
  float gI = -(D + I) / (D * D), gAp = I / (D * D);              // I and the predicted area pw * ph (U = pw ph + gw gh - I)
  float gcw = 0.f, gch = 0.f, gpcx = 0.f, gpcy = 0.f, gpw = 0.f, gph = 0.f;
  if (kind == EFFDET_BOX_LOSS_GIOU) {
    const float C = cw * ch, CE = C + BOX_EPS;
    L += (C - U) / CE;
    if (GRAD) { const float gC = D / (CE * CE); gcw = gC * ch; gch = gC * cw; gI += 1.f / CE; gAp -= 1.f / CE; }
  }
  if (kind >= EFFDET_BOX_LOSS_DIOU) {
    const float dx = pcx - (gx1 + gx2) * 0.5f, dy = pcy - (gy1 + gy2) * 0.5f;
    const float rho2 = dx * dx + dy * dy, K = cw * cw + ch * ch + BOX_EPS;
    L += rho2 / K;
    if (GRAD) { const float t = -2.f * rho2 / (K * K); gcw = t * cw; gch = t * ch; gpcx = 2.f * dx / K; gpcy = 2.f * dy / K; }
  }
  if (kind == EFFDET_BOX_LOSS_CIOU) {
    const float q = pw / ph, da = atanf(gw / gh) - atanf(q);
    const float v = BOX_4_PI2 * da * da, alpha = v / (1.f - iou + v + BOX_EPS);       // alpha: a constant of the gradient
    L += alpha * v;
    if (GRAD) { const float dvdq = -2.f * BOX_4_PI2 * da / (1.f + q * q); gpw = alpha * dvdq / ph; gph = -alpha * dvdq * q / ph; }
  }
  if (GRAD) {
    const float giw = iwr >= 0.f ? gI * ih : 0.f, gih = ihr >= 0.f ? gI * iw : 0.f;   // the clamp at 0 passes at exactly 0
    const float gpx2 = giw * sel_lt(px2, gx2) + gcw * sel_lt(gx2, px2), gpx1 = -giw * sel_lt(gx1, px1) - gcw * sel_lt(px1, gx1);
    const float gpy2 = gih * sel_lt(py2, gy2) + gch * sel_lt(gy2, py2), gpy1 = -gih * sel_lt(gy1, py1) - gch * sel_lt(py1, gy1);
    gpcx += gpx1 + gpx2; gpcy += gpy1 + gpy2;
    gpw += 0.5f * (gpx2 - gpx1) + gAp * ph; gph += 0.5f * (gpy2 - gpy1) + gAp * pw;
    gr[0] = gpcx * (0.1f * aw); gr[1] = gpcy * (0.1f * ah);
    gr[2] = dwr <= EFFDET_BOX_LOSS_DW_MAX ? gpw * pw * 0.2f : 0.f;                    // the cap passes at equality
    gr[3] = dhr <= EFFDET_BOX_LOSS_DW_MAX ? gph * ph * 0.2f : 0.f;
  }
  return L;
}

// the grid of the assign pass: one thread per (image, anchor), one partial per workgroup into part_reg[b][block]
__global__ __launch_bounds__(256) void box_loss_fwd_kernel(const LossK p, const int kind) {
  const int b = blockIdx.y;
  const long long a = blockIdx.x * 256LL + threadIdx.x;
  float l = 0.f;
  if (a < p.A) {
    const int code = p.assign[(long long)b * p.A + a];
    if (code >= 0)
      l = box_loss_elem<false>(kind, ((const float4*)p.anchors)[a], p.annots + ((long long)b * p.N + code) * 5,
                               ((const float4*)p.reg)[(long long)b * p.A + a], nullptr);
  }
  block_partial(l, p.part_reg + (long long)b * p.na + blockIdx.x);
}

// one workgroup: wave w adds part_reg of images w, w + 16, ... (lane-strided, then the fixed shuffle tree) into stat[b][1]; thread 0
// then losses[1] = weight * mean_b sum_b / num_pos_b (models/losses.py:148-152 with the per-anchor loss in place of the 4 deltas)
__global__ __launch_bounds__(1024) void box_loss_final_kernel(const LossK p, const float weight) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int b = wave; b < p.B; b += 16) {
    const float* q = p.part_reg + (long long)b * p.na;
    float s = 0.f;
    for (int i = lane; i < p.na; i += 64) s += q[i];
    s = wave_sum(s);
    if (lane == 0) p.stat[b * SS + 1] = s;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  float rl = 0.f;
  for (int b = 0; b < p.B; ++b) {
    const float* s = p.stat + b * SS;
    if (s[3] > 0.f && npos(s) > 0.f) rl += s[1] / npos(s);
  }
  p.losses[1] = weight * (rl / (float)p.B);
}

// loss_bwd_reg_kernel's grid and output layouts with the analytic gradient of box_loss_elem
template <typename T>
__global__ void box_loss_bwd_reg_kernel(const LossK p, const int kind, const float weight) {
  const long long total = (long long)p.B * p.A;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long b = i / p.A, a = i - b * p.A;
    const int code = p.assign[i];
    const float* st = p.stat + b * SS;
    f32x4 g = f32x4{0.f, 0.f, 0.f, 0.f};
    if (code >= 0 && st[3] > 0.f && npos(st) > 0.f) {
      const float gs = p.gscale[1] * weight / ((float)p.B * npos(st));
      float gr[4];
      (void)box_loss_elem<true>(kind, ((const float4*)p.anchors)[a], p.annots + (b * p.N + code) * 5, ((const float4*)p.reg)[i], gr);
#pragma unroll
      for (int q = 0; q < 4; ++q) g[q] = gs * gr[q];
    }
    store_dreg_row<T>(p, b, a, i, g);
  }
}

// The quality target of include/effdet_quality_loss.h, after whichever assign pass ran and ahead of the class pass: the assign
// pass's grid, one thread per (image, anchor); q = the IoU of box_overlap clamped to [0, 1] at a positive anchor (NaN for a
// non-finite r: r - r is 0 or NaN), 0 elsewhere.  Every element is stored, so the buffer needs no zeroing.
__global__ __launch_bounds__(256) void loss_quality_kernel(const LossK p, float* __restrict__ q) {
  const int b = blockIdx.y;
  const long long a = blockIdx.x * 256LL + threadIdx.x;
  if (a >= p.A) return;
  const long long i = (long long)b * p.A + a;
  const int code = p.assign[i];
  float v = 0.f;
  if (code >= 0) {
    const float4 r = ((const float4*)p.reg)[i];
    const BoxOverlap o = box_overlap(((const float4*)p.anchors)[a], p.annots + ((long long)b * p.N + code) * 5, r);
    v = nan_min(nan_max(o.iou, 0.f), 1.f) + (((r.x - r.x) + (r.y - r.y)) + ((r.z - r.z) + (r.w - r.w)));
  }
  q[i] = v;
}

// ---- the task-aligned matcher (include/effdet_tal.h)
// topk and the exponents, and the buffers between its passes
struct TalK {
  int topk; float alpha, beta;
  unsigned long long* keys; float* mm; unsigned long long* slot;      // [B][N][EFFDET_TAL_MAX_TOPK] keys, [B][N][2] (mmax, umax), [B][A] claims
};

constexpr unsigned long long TAL_NO_KEY = ~0ull;      // above every key: a candidate has m > 0, so the high half of its key is not all ones

// exp2(e log2(x)), 0 at x == 0 (a negative or NaN x gives NaN)
__device__ __forceinline__ float tal_pow(float x, float e) {
#pragma clang fp contract(off)
  return x == 0.f ? 0.f : exp2f(e * log2f(x));
}

// The pair quantities of anchor a (box an) of image b and the annotation row at g[0..3] with label lab: u = loss_quality_kernel's
// expression on box_overlap_strict, m = s^alpha u^beta.  EVERY kernel of the matcher evaluates THIS function (no contraction): the
// claim recomputes a winner's pair, and the inspection call's planes are compared with the keys bit for bit.
struct TalPair { float m, u; };
__device__ __forceinline__ TalPair tal_pair(const LossK& p, const TalK& t, int b, long long a, const float4 an, const float* g, int lab) {
#pragma clang fp contract(off)
  const long long i = (long long)b * p.A + a;
  const float4 r = ((const float4*)p.reg)[i];
  const BoxOverlap o = box_overlap_strict(an, g, r);
  TalPair v;
  v.u = nan_min(nan_max(o.iou, 0.f), 1.f) + (((r.x - r.x) + (r.y - r.y)) + ((r.z - r.z) + (r.w - r.w)));
  const float s = p.cls[i * p.nc + lab];
  v.m = tal_pow(s, t.alpha) * tal_pow(v.u, t.beta);
  return v;
}

// the label of the row at rp as a class index, or -1 for a pad row or a label outside [0, nc) (a NaN included): no candidates
__device__ __forceinline__ int tal_label(const float* rp, int nc) {
  return (rp[4] != -1.0f && rp[4] >= 0.f && rp[4] < (float)nc) ? (int)rp[4] : -1;
}

// every pass starts from stat = 0 (num_pos is an integer atomic count), no claim, no key and (mmax, umax) = 0: a kernel, as
// loss_zero_stat_kernel
__global__ __launch_bounds__(256) void tal_zero_kernel(float* __restrict__ stat, long long ns, const TalK t, long long nk, long long na) {
  const long long total = ns + nk + 2 * (nk / EFFDET_TAL_MAX_TOPK) + na;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += gridDim.x * 256LL) {
    long long j = i;
    if (j < ns) { stat[j] = 0.f; continue; }
    j -= ns;
    if (j < nk) { t.keys[j] = TAL_NO_KEY; continue; }
    j -= nk;
    if (j < 2 * (nk / EFFDET_TAL_MAX_TOPK)) { t.mm[j] = 0.f; continue; }
    j -= 2 * (nk / EFFDET_TAL_MAX_TOPK);
    t.slot[j] = 0ull;
  }
}

// One workgroup per (row, image); a pad row (or a row whose label names no class) exits at once.  atss_select_kernel's shape over the
// WHOLE table: every thread strides over the anchors, the centre test first (one 16-byte read for most anchors), then the pair
// through tal_pair, and keeps its K smallest keys ~bits(m) << 32 | a as a sorted list in registers (K >= topk at compile time: the
// insertion and the pop are fully unrolled, no runtime-indexed array); then up to topk rounds of the workgroup's arg-min over the list
// heads, which the owner pops.  A round that finds no key left ends the rounds (every thread reads the same minimum: the exit is
// uniform), so the sentinel is never a winner.  The winners go to keys[b][n][] in rank order; then thread j claims winner j's anchor
// for this row: atomicMax of bits(u) << 32 | (0xFFFFFFFF - n) -- u > 0 at a winner (m > 0), so a claim is never 0 -- the largest u,
// then the lowest row.
template <int K>
__global__ __launch_bounds__(256) void tal_select_kernel(const LossK p, const TalK t) {
  const int n = blockIdx.x, b = blockIdx.y;
  const float* rp = p.annots + ((long long)b * p.N + n) * 5;
  const int lab = tal_label(rp, p.nc);
  if (lab < 0) return;
  const float r[4] = {rp[0], rp[1], rp[2], rp[3]};
  __shared__ unsigned long long wmin[2][4];
  __shared__ unsigned long long win[EFFDET_TAL_MAX_TOPK];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float4* anc = (const float4*)p.anchors;
  unsigned long long keys[K];
#pragma unroll
  for (int j = 0; j < K; ++j) keys[j] = TAL_NO_KEY;
  for (long long a = threadIdx.x; a < p.A; a += 256) {
    const float4 an = anc[a];
    if (!atss_inside(an, r)) continue;
    const TalPair v = tal_pair(p, t, b, a, an, r, lab);
    if (!(v.m > 0.f)) continue;                              // (a NaN metric is no candidate)
    const unsigned long long key = ((unsigned long long)(~__float_as_uint(v.m)) << 32) | (unsigned)a;
    if (key < keys[K - 1]) {
#pragma unroll
      for (int j = K - 1; j > 0; --j) {                      // new[j] = min(old[j], max(old[j - 1], key)), from the top down
        const unsigned long long m = keys[j - 1] > key ? keys[j - 1] : key;
        keys[j] = keys[j] < m ? keys[j] : m;
      }
      keys[0] = keys[0] < key ? keys[0] : key;
    }
  }
  int cnt = 0;
  for (int q = 0; q < t.topk; ++q) {
    unsigned long long m = keys[0];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const unsigned long long v = shfl_xor_u64(m, o); m = v < m ? v : m; }
    unsigned long long* w = wmin[q & 1];                     // two slots: one barrier per round
    if (lane == 0) w[wave] = m;
    __syncthreads();
    const unsigned long long m01 = w[0] < w[1] ? w[0] : w[1], m23 = w[2] < w[3] ? w[2] : w[3];
    m = m01 < m23 ? m01 : m23;
    if (m == TAL_NO_KEY) break;                              // fewer candidates than topk
    if (keys[0] == m) {                                      // the owner pops its head (keys are distinct: the anchor index)
#pragma unroll
      for (int j = 0; j + 1 < K; ++j) keys[j] = keys[j + 1];
      keys[K - 1] = TAL_NO_KEY;
    }
    if (threadIdx.x == 0) {
      win[q] = m;
      t.keys[((long long)b * p.N + n) * EFFDET_TAL_MAX_TOPK + q] = m;
    }
    ++cnt;
  }
  __syncthreads();
  if ((int)threadIdx.x < cnt) {
    const long long a = (long long)(unsigned)win[threadIdx.x];
    const TalPair v = tal_pair(p, t, b, a, anc[a], r, lab);
    atomicMax(t.slot + (long long)b * p.A + a, ((unsigned long long)__float_as_uint(v.u) << 32) | (0xFFFFFFFFu - (unsigned)n));
  }
}

// loss_assign_kernel's grid: the anchor's claim names its row (none: negative), then the shared tail.  The valid rows are only
// counted here (the matcher has no per-anchor loop over them), 256 at a time.
__global__ __launch_bounds__(256) void tal_assign_kernel(const LossK p, const TalK t, const KneeBeta knee) {
  const int b = blockIdx.y;
  const long long a = blockIdx.x * 256LL + threadIdx.x;
  int total_valid = 0;
  for (int n0 = 0; n0 < p.N; n0 += 256) {
    const int n = n0 + (int)threadIdx.x;
    total_valid += __syncthreads_count(n < p.N && p.annots[((long long)b * p.N + n) * 5 + 4] != -1.0f);
  }
  const bool ok = a < p.A;
  float4 an = make_float4(0, 0, 0, 0);
  int barg = -1;
  if (ok) {
    an = ((const float4*)p.anchors)[a];
    const unsigned long long s = t.slot[(long long)b * p.A + a];
    if (s != 0ull) barg = (int)(0xFFFFFFFFu - (unsigned)s);
  }
  assign_tail(p, b, a, ok, ok && total_valid > 0, barg < 0, barg >= 0, barg, an, knee);
  if (blockIdx.x == 0 && threadIdx.x == 0) p.stat[b * SS + 3] = (float)total_valid;
}

// The aligned target, after loss_quality_kernel has stored q everywhere: one wave per (row, image), lane j < 16 holds winner j.  A
// winner whose anchor's claim names this row is finally assigned to it: its m is in its key, its u in the claim (no recomputation);
// mmax / umax over those lanes (shuffles: the 16 values never leave the wave), then q at their anchors.  A row without winners (a pad
// row has none) writes nothing: (mmax, umax) stay tal_zero_kernel's zeros.
__global__ __launch_bounds__(64) void tal_target_kernel(const LossK p, const TalK t, float* __restrict__ q) {
#pragma clang fp contract(off)
  const int n = blockIdx.x, b = blockIdx.y, j = threadIdx.x;
  const long long row = (long long)b * p.N + n;
  float m = 0.f, u = 0.f;
  bool mine = false;
  long long i = 0;
  if (j < EFFDET_TAL_MAX_TOPK) {
    const unsigned long long key = t.keys[row * EFFDET_TAL_MAX_TOPK + j];
    if (key != TAL_NO_KEY) {
      i = (long long)b * p.A + (long long)(unsigned)key;
      const unsigned long long s = t.slot[i];
      if (0xFFFFFFFFu - (unsigned)s == (unsigned)n) {
        mine = true;
        m = __uint_as_float(~(unsigned)(key >> 32));
        u = __uint_as_float((unsigned)(s >> 32));
      }
    }
  }
  const float mmax = wave_max(m), umax = wave_max(u);      // (m, u >= 0 at a winner; the other lanes hold 0)
  if (mine) q[i] = (m * umax) / (mmax + 1e-9f);
  if (j == 0 && mmax > 0.f) { t.mm[row * 2] = mmax; t.mm[row * 2 + 1] = umax; }
}

// inspection: one thread per (anchor, row, image) -> out[0][b][n][a] = m, out[1][b][n][a] = u through tal_pair; 0 where the anchor's
// centre is not inside the row's box and for a row without candidates
__global__ __launch_bounds__(256) void tal_metrics_kernel(const LossK p, const TalK t, float* __restrict__ out) {
  const int n = blockIdx.y, b = blockIdx.z;
  const long long a = blockIdx.x * 256LL + threadIdx.x;
  if (a >= p.A) return;
  const float* rp = p.annots + ((long long)b * p.N + n) * 5;
  const int lab = tal_label(rp, p.nc);
  TalPair v{0.f, 0.f};
  if (lab >= 0) {
    const float r[4] = {rp[0], rp[1], rp[2], rp[3]};
    const float4 an = ((const float4*)p.anchors)[a];
    if (atss_inside(an, r)) v = tal_pair(p, t, b, a, an, r, lab);
  }
  const long long o = ((long long)b * p.N + n) * p.A + a;
  out[o] = v.m;
  out[(long long)p.B * p.N * p.A + o] = v.u;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host side.  Every extern "C" loss function fills one LossCall and hands it to a driver (loss_forward, loss_bwd, loss_bwd_cls,
// loss_bwd_reg), which makes the entry point's checks, carves the workspace by the one rule loss_workspace and launches from the
// record: the matcher picks one of four assign paths, opts / ql the class policy, the box term smooth-L1 or the IoU-family kernels.

// workgroups per image of the assign pass / upper bound of the class pass (either kernel: dld <= 9*nc + 63)
inline long long assign_blocks(long long A) { return (A + 255) / 256; }
inline long long cls_blocks_max(long long A, int nc) { return ((A * nc + 3) / 4 + (A / 9 + 1) * 16 + 1023) / 1024 + 1; }

LossK loss_args(const float* cls, const float* reg, const float* anchors, const float* annots, int B, long long A, int nc, int N) {
  LossK k{}; k.cls = cls; k.reg = reg; k.anchors = anchors; k.annots = annots; k.B = B; k.nc = nc; k.N = N; k.A = A;
  return k;
}

TalK tal_args(const effdet_tal_t* tal) {
  TalK t{}; t.topk = tal->topk; t.alpha = tal->alpha; t.beta = tal->beta;
  return t;
}

// the assign path of a call: the reference's single pass, the bands of the options, ATSS, the task-aligned matcher
enum { MATCH_DEFAULT = 0, MATCH_BANDS, MATCH_ATSS, MATCH_TAL };

// What every loss entry point receives.  k holds what the CALLER fills of the kernels' arguments: the tensors, losses, dcls / dld,
// dreg / reg_ld, gscale, B, A, nc, N (a backward call leaves what it does not take null / 0); the drivers carve the rest.
struct LossCall {
  LossK k;
  const void* ws; long long ws_bytes;  // (the backward calls take no byte count)
  hipStream_t st;
  bool grad; int dtype;                // forward: also d(cls) into k.dcls, pixel-major; the dtype of k.dcls / k.dreg
  int matcher;                         // MATCH_*: which of opts / atss / tal the entry point REQUIRES (a null one is refused)
  const effdet_loss_opts_t* opts;      // null (MATCH_DEFAULT only): the reference's constants -- FocalDefault, KneeDefault, loss_assign_kernel
  const effdet_atss_t* atss; const effdet_tal_t* tal;
  const effdet_quality_loss_t* ql;     // the quality loss in the place of the focal term (include/effdet_quality_loss.h), or null
  bool need_ql;                        // the effdet_loss_quality_* calls: a null ql is refused
  bool box; int box_kind; float box_weight;      // the stand-alone box term of the effdet_box_loss_* calls
};

// the box term of a call: the stand-alone one, else the options' -> kind (0: smooth-L1) and its weight
inline int box_term(const LossCall& c, float& weight) {
  weight = c.box ? c.box_weight : c.opts ? c.opts->box_weight : 1.0f;
  return c.box ? c.box_kind : c.opts ? c.opts->box_kind : 0;
}

// the buffers of a workspace beyond LossK's: between the passes of the three matchers, and the quality target
struct LossBufs { OptsK o; AtssK t; TalK tal; float* q; };

// THE workspace rule: (matcher, quality loss or not; k.B, k.A, k.nc, k.N) -> the bytes a forward call needs, and with ws the carved
// pointers.  The five *_workspace_bytes exports and every driver come here.
//   every call     assign [B][A], stat [B][SS], part_reg [B][na], part_cls [B][cls_blocks_max] (num_classes only sizes this last
//                  buffer: a backward call or the box term, which know no class count, find the first three where the forward left them)
//   bands          then gtmax [B][N], best [B][A], barg [B][A]
//   ATSS           in their place kth [B][N][EFFDET_ATSS_MAX_LEVELS], thr [B][N]
//   quality loss   the target q [B][A] past the LONGER of the two matchers' layouts: the same place whichever matcher ran, so the
//                  class backward finds it without knowing the matcher
//   task-aligned   the quality layout (q where the class backward looks for it; one layout with or without a quality loss), then keys
//                  [B][N][EFFDET_TAL_MAX_TOPK], (mmax, umax) [B][N][2] and claims [B][A]
size_t loss_workspace(LossK& k, LossBufs& w, const void* ws, int matcher, bool quality) {
  const int B = k.B, N = k.N; const long long A = k.A;
  Carver c(const_cast<void*>(ws));
  k.assign = c.take<int>((size_t)B * A);
  k.stat = c.take<float>((size_t)B * SS);
  k.part_reg = c.take<float>((size_t)B * assign_blocks(A));
  k.part_cls = c.take<float>((size_t)B * cls_blocks_max(A, k.nc));
  k.na = (int)assign_blocks(A);
  if (matcher == MATCH_DEFAULT) return c.off;
  const size_t head = c.off;
  w.o.gtmax = c.take<int>((size_t)B * N);
  w.o.best = c.take<float>((size_t)B * A);
  w.o.barg = c.take<int>((size_t)B * A);
  const size_t bands = c.off;
  if (matcher == MATCH_BANDS && !quality) return bands;
  c.off = head;
  w.t.kth = c.take<unsigned long long>((size_t)B * N * EFFDET_ATSS_MAX_LEVELS);
  w.t.thr = c.take<float>((size_t)B * N);
  if (matcher == MATCH_ATSS && !quality) return c.off;
  if (c.off < bands) c.off = bands;
  float* q = c.take<float>((size_t)B * A);
  w.q = quality ? q : nullptr;
  if (matcher != MATCH_TAL) return c.off;
  w.tal.keys = c.take<unsigned long long>((size_t)B * N * EFFDET_TAL_MAX_TOPK);
  w.tal.mm = c.take<float>((size_t)B * N * 2);
  w.tal.slot = c.take<unsigned long long>((size_t)B * A);
  return c.off;
}

// ... the part every call has, alone: what a backward call and the box term need
void loss_workspace(LossK& k, const void* ws) { LossBufs w{}; loss_workspace(k, w, ws, MATCH_DEFAULT, false); }

// a *_workspace_bytes export
long long loss_workspace_bytes(int matcher, bool quality, int B, long long A, int num_classes, int N) {
  LossK k = loss_args(nullptr, nullptr, nullptr, nullptr, B, A, num_classes, N); LossBufs w{};
  return (long long)loss_workspace(k, w, nullptr, matcher, quality);
}

// ---- argument checks, each written once.  Every entry point makes all its EFFDET_EINVAL checks before the first
// EFFDET_EUNSUPPORTED one; check_dcls ends with the latter, so it comes last among an entry point's EINVAL checks.
inline bool finite_ge0(float v) { return v >= 0.f && v <= 3.402823466e38f; }      // (false for a NaN)

inline bool box_loss_args_ok(int kind, float weight) {
  return kind >= EFFDET_BOX_LOSS_IOU && kind <= EFFDET_BOX_LOSS_CIOU && finite_ge0(weight);
}

bool loss_opts_ok(const effdet_loss_opts_t* o) {
  if (!o) return false;
  if (!(o->alpha > 0.f && o->alpha < 1.f) || !(o->gamma >= 0.f && o->gamma <= 8.f)) return false;
  if (!(o->label_smoothing >= 0.f && o->label_smoothing < 1.f)) return false;
  if (!(o->beta > 0.f && o->beta <= 3.402823466e38f) || !finite_ge0(o->reg_weight) || !finite_ge0(o->box_weight)) return false;
  if (!(o->neg_iou >= 0.f && o->neg_iou <= o->pos_iou && o->pos_iou <= 1.f)) return false;
  if (o->low_quality != 0 && o->low_quality != 1) return false;
  return o->box_kind >= 0 && o->box_kind <= EFFDET_BOX_LOSS_CIOU;
}

bool quality_ok(const effdet_quality_loss_t* q) {
  if (!q || (q->kind != EFFDET_QUALITY_QFL && q->kind != EFFDET_QUALITY_VFL)) return false;
  return q->beta >= 1.f && q->beta <= 8.f && q->alpha > 0.f && q->alpha <= 1.f && q->gamma >= 0.f && q->gamma <= 8.f;    // (false for a NaN)
}

bool atss_ok(const effdet_atss_t* t, long long A) {
  if (!t || t->topk < 1 || t->topk > EFFDET_ATSS_MAX_TOPK || t->num_levels < 1 || t->num_levels > EFFDET_ATSS_MAX_LEVELS) return false;
  if (t->level_start[0] != 0 || t->level_start[t->num_levels] != A) return false;
  for (int l = 0; l < t->num_levels; ++l)
    if (t->level_start[l + 1] <= t->level_start[l]) return false;
  return true;
}

bool tal_ok(const effdet_tal_t* t) {
  if (!t || t->topk < 1 || t->topk > EFFDET_TAL_MAX_TOPK) return false;
  if (!(t->alpha >= 0.f && t->alpha <= 4.f) || !(t->beta >= 0.f && t->beta <= 16.f)) return false;      // (false for a NaN)
  return t->aligned_target == 0 || t->aligned_target == 1;
}

inline bool dtype_ok(int dtype, bool split) { return dtype == EFFDET_F32 || dtype == EFFDET_BF16 || (split && dtype == EFFDET_F32_SPLIT); }

// the d(cls) output: dtype, then with dld the pixel-major padded layout (split: whole [hi|lo] groups, aligned rows) and its extent
int check_dcls(const void* dcls, int dld, int dtype, bool split, long long A, int nc) {
  if (!dtype_ok(dtype, split)) return EFFDET_EINVAL;
  if (dld && (A % 9 || nc % 4 || dld % 4 || dld < 9 * nc)) return EFFDET_EINVAL;
  if (dtype == EFFDET_F32_SPLIT && (dld % 32 || ((unsigned long long)dcls & 127ull))) return EFFDET_EINVAL;
  if (dld && (A / 9) * dld >= 0x7fffffffLL) return EFFDET_EUNSUPPORTED;
  return EFFDET_OK;
}

// the d(reg) output: dtype and layout (the split layout exists pixel-major only)
int check_dreg(const void* dreg, int reg_ld, int dtype, long long A) {
  if (!dtype_ok(dtype, true)) return EFFDET_EINVAL;
  if (reg_ld && (reg_ld < 36 || reg_ld % 4 || A % 9)) return EFFDET_EINVAL;
  if (dtype == EFFDET_F32_SPLIT && (!reg_ld || reg_ld % 32 || ((unsigned long long)dreg & 127ull))) return EFFDET_EINVAL;
  return EFFDET_OK;
}

// ---- the one place where a dtype code becomes an element type: fn(Tag<T>{}).  SPLIT: the entry point also takes EFFDET_F32_SPLIT
// (the callers have checked the code with dtype_ok)
template <typename T> struct Tag { using type = T; };
template <bool SPLIT, typename Fn>
inline void by_dtype(int dtype, Fn&& fn) {
  if (dtype == EFFDET_F32) return fn(Tag<float>{});
  if constexpr (SPLIT) if (dtype == EFFDET_F32_SPLIT) return fn(Tag<split_t>{});
  fn(Tag<bf16_t>{});
}

// ---- drivers
// Where a call's values become the class policy's type: FocalDefault without options (the reference's constants), FocalP of the
// options, or with a quality loss (checked by the caller) its soft-target policy reading q, which loss_workspace has placed -> fn(policy)
template <typename Fn>
void with_class_policy(const LossCall& c, const float* q, Fn&& fn) {
  if (!c.opts) return fn(FocalDefault{});
  if (!c.ql) return fn(FocalP{c.opts->alpha, c.opts->gamma, c.opts->label_smoothing});
  if (c.ql->kind == EFFDET_QUALITY_QFL) return fn(FocalQfl{c.ql->beta, q});
  return fn(FocalVfl{c.ql->alpha, c.ql->gamma, q});
}

// The four assign paths: each zeroes what its passes accumulate into and enqueues its select / assign kernels; k and w are carved.
int assign_default(const LossK& k, hipStream_t st) {
  hipLaunchKernelGGL(loss_zero_stat_kernel, dim3((unsigned)((k.B * SS + 255) / 256)), dim3(256), 0, st, k.stat, k.B * SS);
  EFFDET_CHECK_LAUNCH();
  hipLaunchKernelGGL(loss_assign_kernel, dim3((unsigned)k.na, k.B), dim3(256), 0, st, k);
  EFFDET_CHECK_LAUNCH();
  return EFFDET_OK;
}

int assign_bands(const LossK& k, OptsK o, const effdet_loss_opts_t* opts, hipStream_t st) {
  o.pos_iou = opts->pos_iou; o.neg_iou = opts->neg_iou; o.low_quality = opts->low_quality;
  const int nz = k.B * SS, mz = k.B * k.N;
  hipLaunchKernelGGL(opts_zero_kernel, dim3((unsigned)((nz + mz + 255) / 256)), dim3(256), 0, st, k.stat, nz, o.gtmax, mz);
  EFFDET_CHECK_LAUNCH();
  hipLaunchKernelGGL(opts_iou_kernel, dim3((unsigned)k.na, k.B), dim3(256), 0, st, k, o);
  EFFDET_CHECK_LAUNCH();
  hipLaunchKernelGGL(opts_assign_kernel, dim3((unsigned)k.na, k.B), dim3(256), 0, st, k, o, KneeBeta{opts->beta});
  EFFDET_CHECK_LAUNCH();
  return EFFDET_OK;
}

int assign_atss(const LossK& k, AtssK t, const effdet_atss_t* atss, KneeBeta knee, hipStream_t st) {
  t.topk = atss->topk; t.num_levels = atss->num_levels;      // (A < 2^31 has been checked: an index within a level fits the low half of a key)
  for (int l = 0; l <= atss->num_levels; ++l) t.ls[l] = atss->level_start[l];
  hipLaunchKernelGGL(loss_zero_stat_kernel, dim3((unsigned)((k.B * SS + 255) / 256)), dim3(256), 0, st, k.stat, k.B * SS);
  EFFDET_CHECK_LAUNCH();
  if (t.topk <= 9) hipLaunchKernelGGL(atss_select_kernel<9>, dim3((unsigned)k.N, k.B), dim3(256), 0, st, k, t);
  else hipLaunchKernelGGL(atss_select_kernel<EFFDET_ATSS_MAX_TOPK>, dim3((unsigned)k.N, k.B), dim3(256), 0, st, k, t);
  EFFDET_CHECK_LAUNCH();
  hipLaunchKernelGGL(atss_assign_kernel, dim3((unsigned)k.na, k.B), dim3(256), 0, st, k, t, knee);
  EFFDET_CHECK_LAUNCH();
  return EFFDET_OK;
}

int assign_tal(const LossK& k, const TalK& t, KneeBeta knee, hipStream_t st) {      // (A < 2^31 has been checked: an anchor index fits the low half of a key)
  const long long ns = (long long)k.B * SS, nk = (long long)k.B * k.N * EFFDET_TAL_MAX_TOPK, na = (long long)k.B * k.A;
  hipLaunchKernelGGL(tal_zero_kernel, dim3(grid_for(ns + nk + nk / EFFDET_TAL_MAX_TOPK * 2 + na)), dim3(256), 0, st, k.stat, ns, t, nk, na);
  EFFDET_CHECK_LAUNCH();
  if (t.topk <= 13) hipLaunchKernelGGL(tal_select_kernel<13>, dim3((unsigned)k.N, k.B), dim3(256), 0, st, k, t);
  else hipLaunchKernelGGL(tal_select_kernel<EFFDET_TAL_MAX_TOPK>, dim3((unsigned)k.N, k.B), dim3(256), 0, st, k, t);
  EFFDET_CHECK_LAUNCH();
  hipLaunchKernelGGL(tal_assign_kernel, dim3((unsigned)k.na, k.B), dim3(256), 0, st, k, t, knee);
  EFFDET_CHECK_LAUNCH();
  return EFFDET_OK;
}

// after the forward kernels have been enqueued with an IoU-family box term: the per-workgroup partials over their assignment, then
// losses[1]
int box_loss_finish(const LossCall& c, int kind, float weight) {
  LossK k = loss_args(nullptr, c.k.reg, c.k.anchors, c.k.annots, c.k.B, c.k.A, 0, c.k.N); k.losses = c.k.losses;
  loss_workspace(k, c.ws);
  hipLaunchKernelGGL(box_loss_fwd_kernel, dim3((unsigned)k.na, k.B), dim3(256), 0, c.st, k, kind);
  EFFDET_CHECK_LAUNCH();
  hipLaunchKernelGGL(box_loss_final_kernel, dim3(1), dim3(1024), 0, c.st, k, weight);
  EFFDET_CHECK_LAUNCH();
  return EFFDET_OK;
}

// Every forward entry point (c.grad: the _fwd_grad ones).  The entry point's own EINVAL checks, the shared ones, the EUNSUPPORTED
// one; then the matcher's assign path, with a quality loss q for the class pass (and the task-aligned target behind it), the class
// pass (grad: forward + gradient into k.dcls, pixel-major), the final reduction, and with a box kind its term over the same assignment.
int loss_forward(const LossCall& c) {
  LossK k = c.k;
  const effdet_loss_opts_t* o = c.opts;
  hipStream_t st = c.st;
  if (c.box && !box_loss_args_ok(c.box_kind, c.box_weight)) return EFFDET_EINVAL;
  if ((c.need_ql || c.ql) && !quality_ok(c.ql)) return EFFDET_EINVAL;
  if (c.matcher != MATCH_DEFAULT) {               // (the default calls check neither B < 1 nor A, num_classes)
    if (!loss_opts_ok(o) || k.B < 1 || k.N < 1 || k.A < 1 || k.nc < 1) return EFFDET_EINVAL;
    if (c.matcher != MATCH_BANDS && o->low_quality != 0) return EFFDET_EINVAL;      // a matcher replaces the bands and their promotion
    if (c.matcher == MATCH_ATSS && !atss_ok(c.atss, k.A)) return EFFDET_EINVAL;
    if (c.matcher == MATCH_TAL && !tal_ok(c.tal)) return EFFDET_EINVAL;
  }
  LossBufs w{};
  if (c.matcher == MATCH_TAL) w.tal = tal_args(c.tal);
  const long long need = (long long)loss_workspace(k, w, c.ws, c.matcher, c.ql != nullptr);
  if (!k.cls || !k.reg || !k.anchors || !k.annots || !k.losses || !c.ws || (c.grad && !k.dcls)) return EFFDET_EINVAL;
  if (c.ws_bytes < need || k.B > 65535 || k.N < 1) return EFFDET_EINVAL;
  if (c.grad) {
    if (k.dld <= 0) return EFFDET_EINVAL;
    if (const int rc = check_dcls(k.dcls, k.dld, c.dtype, true, k.A, k.nc)) return rc;
  }
  if (k.A * k.nc >= 0x7fffffffLL) return EFFDET_EUNSUPPORTED;

  int rc = EFFDET_OK;
  if (c.matcher == MATCH_DEFAULT) rc = assign_default(k, st);
  else if (c.matcher == MATCH_BANDS) rc = assign_bands(k, w.o, o, st);
  else if (c.matcher == MATCH_ATSS) rc = assign_atss(k, w.t, c.atss, KneeBeta{o->beta}, st);
  else rc = assign_tal(k, w.tal, KneeBeta{o->beta}, st);
  if (rc != EFFDET_OK) return rc;
  if (w.q) {                                      // after whichever assign pass ran: q for the class pass
    hipLaunchKernelGGL(loss_quality_kernel, dim3((unsigned)k.na, k.B), dim3(256), 0, st, k, w.q);
    EFFDET_CHECK_LAUNCH();
    if (c.matcher == MATCH_TAL && c.tal->aligned_target) {
      hipLaunchKernelGGL(tal_target_kernel, dim3((unsigned)k.N, k.B), dim3(64), 0, st, k, w.tal, w.q);
      EFFDET_CHECK_LAUNCH();
    }
  }
  const long long groups = c.grad ? (k.A / 9) * k.dld / 4 : (k.A * k.nc + 3) / 4;
  const int it = c.grad ? FG_IT : CLS_IT;
  k.ncb = (int)((groups + 256 * it - 1) / (256 * it));
  if (k.ncb > cls_blocks_max(k.A, k.nc)) return EFFDET_EINVAL;
  const dim3 g1((unsigned)k.ncb, k.B);
  with_class_policy(c, w.q, [&](auto f) {
    using F = decltype(f);
    if (c.grad) by_dtype<true>(c.dtype, [&](auto t) {
      hipLaunchKernelGGL((loss_cls_pix_kernel<typename decltype(t)::type, F, false, FG_IT>), g1, dim3(256), 0, st, k, f);
    });
    else hipLaunchKernelGGL(loss_cls_kernel<F>, g1, dim3(256), 0, st, k, f);
  });
  EFFDET_CHECK_LAUNCH();
  hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(1024), 0, st, k, o ? o->reg_weight : 1.0f);
  EFFDET_CHECK_LAUNCH();
  float weight;
  const int kind = box_term(c, weight);
  return kind ? box_loss_finish(c, kind, weight) : EFFDET_OK;
}

// d(logits) of the call's class policy into k.dcls, flat or (k.dld) pixel-major, with the upstream gradient applied.  No launch check:
// the caller's follows.
void launch_bwd_cls(const LossK& k, const LossCall& c, const float* q) {
  const long long groups = k.dld ? (k.A / 9) * k.dld / 4 : (k.A * k.nc + 3) / 4;
  const dim3 g1((unsigned)((groups + 255) / 256), k.B);
  with_class_policy(c, q, [&](auto f) {
    using F = decltype(f);
    by_dtype<false>(c.dtype, [&](auto t) {
      using T = typename decltype(t)::type;
      if (k.dld) hipLaunchKernelGGL((loss_cls_pix_kernel<T, F, true, 1>), g1, dim3(256), 0, c.st, k, f);
      else hipLaunchKernelGGL((loss_bwd_cls_kernel<T, F>), g1, dim3(256), 0, c.st, k, f);
    });
  });
}

// d(reg) of the call's box term into k.dreg: the box kernel of an IoU kind, else smooth-L1 with the options' knee or the reference's
void launch_bwd_reg(const LossK& k, const LossCall& c) {
  float weight;
  const int kind = box_term(c, weight);
  const dim3 g(grid_for((long long)k.B * k.A));
  by_dtype<true>(c.dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    if (kind) hipLaunchKernelGGL(box_loss_bwd_reg_kernel<T>, g, dim3(256), 0, c.st, k, kind, weight);
    else if (c.opts) hipLaunchKernelGGL((loss_bwd_reg_kernel<T, KneeBeta>), g, dim3(256), 0, c.st, k, KneeBeta{c.opts->beta}, c.opts->reg_weight);
    else hipLaunchKernelGGL((loss_bwd_reg_kernel<T, KneeDefault>), g, dim3(256), 0, c.st, k, KneeDefault{}, 1.0f);
  });
}

// the reference's combined backward: d(logits) and the smooth-L1 d(reg) [B][A][4] of the default forward
int loss_bwd(const LossCall& c) {
  LossK k = c.k;
  if (!k.cls || !k.reg || !k.anchors || !k.annots || !k.gscale || !c.ws || !k.dcls || !k.dreg) return EFFDET_EINVAL;
  if (const int rc = check_dcls(k.dcls, k.dld, c.dtype, false, k.A, k.nc)) return rc;
  loss_workspace(k, c.ws);
  launch_bwd_cls(k, c, nullptr);
  launch_bwd_reg(k, c);
  EFFDET_CHECK_LAUNCH();
  return EFFDET_OK;
}

// the class backward of the options, and with ql of a quality loss (q: where loss_workspace says the forward call left it)
int loss_bwd_cls(const LossCall& c) {
  LossK k = c.k;
  if (c.need_ql && !quality_ok(c.ql)) return EFFDET_EINVAL;
  if (!k.cls || !k.annots || !k.gscale || !c.ws || !k.dcls) return EFFDET_EINVAL;
  if (!loss_opts_ok(c.opts) || k.B < 1 || k.B > 65535 || k.N < 1 || k.A < 1 || k.nc < 1 || k.dld < 0) return EFFDET_EINVAL;
  if (const int rc = check_dcls(k.dcls, k.dld, c.dtype, false, k.A, k.nc)) return rc;
  if (k.A * k.nc >= 0x7fffffffLL) return EFFDET_EUNSUPPORTED;
  LossBufs w{};
  loss_workspace(k, w, c.ws, c.ql ? MATCH_BANDS : MATCH_DEFAULT, c.ql != nullptr);
  launch_bwd_cls(k, c, w.q);
  EFFDET_CHECK_LAUNCH();
  return EFFDET_OK;
}

// every d(reg) entry point.  With a box kind in the options the call is the stand-alone box call: B, N, A are not checked.
int loss_bwd_reg(const LossCall& c) {
  LossK k = c.k;
  if (c.box && !box_loss_args_ok(c.box_kind, c.box_weight)) return EFFDET_EINVAL;
  if (c.matcher != MATCH_DEFAULT && !loss_opts_ok(c.opts)) return EFFDET_EINVAL;
  if (c.opts && c.opts->box_kind == 0 && (k.B < 1 || k.N < 1 || k.A < 1)) return EFFDET_EINVAL;
  if (!k.reg || !k.anchors || !k.annots || !k.gscale || !c.ws || !k.dreg) return EFFDET_EINVAL;
  if (const int rc = check_dreg(k.dreg, k.reg_ld, c.dtype, k.A)) return rc;
  loss_workspace(k, c.ws);
  launch_bwd_reg(k, c);
  EFFDET_CHECK_LAUNCH();
  return EFFDET_OK;
}

}  // namespace

extern "C" int effdet_positive_pixel_map(const float* anchors, const float* annots, int B, long long A, int N, int nlev, const int* H,
                                         const int* W, unsigned char* map, effdet_stream_t stream) {
  if (!anchors || !annots || !map || !H || !W) return EFFDET_EINVAL;
  if (B < 1 || B > 65535 || N < 1 || nlev < 1 || nlev > EFFDET_MAX_SEG) return EFFDET_EINVAL;
  PosMapK g{}; g.map = map; g.nlev = nlev;
  long long apix = 0, P = 0;
  for (int l = 0; l < nlev; ++l) {
    if (H[l] < 1 || W[l] < 1) return EFFDET_EINVAL;
    apix += (long long)H[l] * W[l];
  }
  if (A != 9 * apix) return EFFDET_EINVAL;
  if (apix * B >= 0x40000000LL) return EFFDET_EUNSUPPORTED;
  g.apix = (int)apix; apix = 0;
  for (int l = 0; l < nlev; ++l) {
    const long long hw = (long long)H[l] * W[l];
    g.hw[l] = (int)hw; g.poff[l] = (int)apix; g.pix0[l] = (int)P;
    apix += hw; P += hw * B;
  }
  const LossK k = loss_args(nullptr, nullptr, anchors, annots, B, A, 0, N);
  hipLaunchKernelGGL(loss_pos_map_kernel, dim3((unsigned)((apix + 255) / 256), B), dim3(256), 0, (hipStream_t)stream, k, g);
  EFFDET_CHECK_LAUNCH();
  return EFFDET_OK;
}

// ---- the loss entry points: each fills the record and makes one call
extern "C" long long effdet_loss_workspace_bytes(int B, long long A, int num_classes) {
  return loss_workspace_bytes(MATCH_DEFAULT, false, B, A, num_classes, 0);
}

extern "C" long long effdet_loss_opts_workspace_bytes(int B, long long A, int num_classes, int N) {
  return loss_workspace_bytes(MATCH_BANDS, false, B, A, num_classes, N);
}

extern "C" long long effdet_loss_atss_workspace_bytes(int B, long long A, int num_classes, int N, const effdet_atss_t* atss) {
  return atss_ok(atss, A) ? loss_workspace_bytes(MATCH_ATSS, false, B, A, num_classes, N) : EFFDET_EINVAL;
}

extern "C" long long effdet_loss_quality_workspace_bytes(int B, long long A, int num_classes, int N, const effdet_atss_t* atss) {
  return !atss || atss_ok(atss, A) ? loss_workspace_bytes(MATCH_BANDS, true, B, A, num_classes, N) : EFFDET_EINVAL;
}

extern "C" long long effdet_loss_tal_workspace_bytes(int B, long long A, int num_classes, int N, const effdet_tal_t* tal) {
  return tal_ok(tal) ? loss_workspace_bytes(MATCH_TAL, false, B, A, num_classes, N) : EFFDET_EINVAL;
}

extern "C" int effdet_focal_loss_fwd(const float* cls, const float* reg, const float* anchors, const float* annots,
                                     float* losses, void* workspace, long long workspace_bytes, int B, long long A,
                                     int num_classes, int N, effdet_stream_t stream) {
  LossCall c{loss_args(cls, reg, anchors, annots, B, A, num_classes, N), workspace, workspace_bytes, (hipStream_t)stream};
  c.k.losses = losses;
  return loss_forward(c);
}

extern "C" int effdet_focal_loss_fwd_grad(const float* cls, const float* reg, const float* anchors, const float* annots,
                                          float* losses, void* workspace, long long workspace_bytes, void* dcls_pix, int dld,
                                          int dtype, int B, long long A, int num_classes, int N, effdet_stream_t stream) {
  LossCall c{loss_args(cls, reg, anchors, annots, B, A, num_classes, N), workspace, workspace_bytes, (hipStream_t)stream};
  c.k.losses = losses; c.k.dcls = dcls_pix; c.k.dld = dld; c.dtype = dtype; c.grad = true;
  return loss_forward(c);
}

extern "C" int effdet_focal_loss_bwd(const float* cls, const float* reg, const float* anchors, const float* annots,
                                     const float* gscale, const void* workspace, void* dcls_logit, void* dreg, int dtype,
                                     int B, long long A, int num_classes, int N, effdet_stream_t stream) {
  LossCall c{loss_args(cls, reg, anchors, annots, B, A, num_classes, N), workspace, 0, (hipStream_t)stream};
  c.k.gscale = gscale; c.dtype = dtype; c.k.dcls = dcls_logit; c.k.dreg = dreg;
  return loss_bwd(c);
}

extern "C" int effdet_focal_loss_bwd_pix(const float* cls, const float* reg, const float* anchors, const float* annots,
                                         const float* gscale, const void* workspace, void* dcls_pix, int dld, void* dreg,
                                         int dtype, int B, long long A, int num_classes, int N, effdet_stream_t stream) {
  if (dld <= 0) return EFFDET_EINVAL;
  LossCall c{loss_args(cls, reg, anchors, annots, B, A, num_classes, N), workspace, 0, (hipStream_t)stream};
  c.k.gscale = gscale; c.dtype = dtype; c.k.dcls = dcls_pix; c.k.dld = dld; c.k.dreg = dreg;
  return loss_bwd(c);
}

extern "C" int effdet_focal_loss_bwd_reg(const float* reg, const float* anchors, const float* annots, const float* gscale,
                                         const void* workspace, void* dreg, int reg_ld, int dtype, int B, long long A, int N,
                                         effdet_stream_t stream) {
  LossCall c{loss_args(nullptr, reg, anchors, annots, B, A, 0, N), workspace, 0, (hipStream_t)stream};
  c.k.gscale = gscale; c.dtype = dtype; c.k.dreg = dreg; c.k.reg_ld = reg_ld;
  return loss_bwd_reg(c);
}

extern "C" int effdet_box_loss_fwd(const float* cls, const float* reg, const float* anchors, const float* annots, float* losses,
                                   void* workspace, long long workspace_bytes, int B, long long A, int num_classes, int N, int kind,
                                   float weight, effdet_stream_t stream) {
  LossCall c{loss_args(cls, reg, anchors, annots, B, A, num_classes, N), workspace, workspace_bytes, (hipStream_t)stream};
  c.k.losses = losses; c.box = true; c.box_kind = kind; c.box_weight = weight;
  return loss_forward(c);
}

extern "C" int effdet_box_loss_fwd_grad(const float* cls, const float* reg, const float* anchors, const float* annots, float* losses,
                                        void* workspace, long long workspace_bytes, void* dcls_pix, int dld, int dtype, int B,
                                        long long A, int num_classes, int N, int kind, float weight, effdet_stream_t stream) {
  LossCall c{loss_args(cls, reg, anchors, annots, B, A, num_classes, N), workspace, workspace_bytes, (hipStream_t)stream};
  c.k.losses = losses; c.k.dcls = dcls_pix; c.k.dld = dld; c.dtype = dtype; c.grad = true;
  c.box = true; c.box_kind = kind; c.box_weight = weight;
  return loss_forward(c);
}

extern "C" int effdet_box_loss_bwd_reg(const float* reg, const float* anchors, const float* annots, const float* gscale,
                                       const void* workspace, void* dreg, int reg_ld, int dtype, int B, long long A, int N, int kind,
                                       float weight, effdet_stream_t stream) {
  LossCall c{loss_args(nullptr, reg, anchors, annots, B, A, 0, N), workspace, 0, (hipStream_t)stream};
  c.k.gscale = gscale; c.dtype = dtype; c.k.dreg = dreg; c.k.reg_ld = reg_ld;
  c.box = true; c.box_kind = kind; c.box_weight = weight;
  return loss_bwd_reg(c);
}

extern "C" int effdet_loss_opts_fwd(const float* cls, const float* reg, const float* anchors, const float* annots, float* losses,
                                    void* workspace, long long workspace_bytes, int B, long long A, int num_classes, int N,
                                    const effdet_loss_opts_t* opts, effdet_stream_t stream) {
  LossCall c{loss_args(cls, reg, anchors, annots, B, A, num_classes, N), workspace, workspace_bytes, (hipStream_t)stream};
  c.k.losses = losses; c.matcher = MATCH_BANDS; c.opts = opts;
  return loss_forward(c);
}

extern "C" int effdet_loss_opts_fwd_grad(const float* cls, const float* reg, const float* anchors, const float* annots, float* losses,
                                         void* workspace, long long workspace_bytes, void* dcls_pix, int dld, int dtype, int B,
                                         long long A, int num_classes, int N, const effdet_loss_opts_t* opts, effdet_stream_t stream) {
  LossCall c{loss_args(cls, reg, anchors, annots, B, A, num_classes, N), workspace, workspace_bytes, (hipStream_t)stream};
  c.k.losses = losses; c.k.dcls = dcls_pix; c.k.dld = dld; c.dtype = dtype; c.grad = true;
  c.matcher = MATCH_BANDS; c.opts = opts;
  return loss_forward(c);
}

extern "C" int effdet_loss_opts_bwd_cls(const float* cls, const float* annots, const float* gscale, const void* workspace, void* dcls,
                                        int dld, int dtype, int B, long long A, int num_classes, int N, const effdet_loss_opts_t* opts,
                                        effdet_stream_t stream) {
  LossCall c{loss_args(cls, nullptr, nullptr, annots, B, A, num_classes, N), workspace, 0, (hipStream_t)stream};
  c.k.gscale = gscale; c.dtype = dtype; c.k.dcls = dcls; c.k.dld = dld; c.matcher = MATCH_BANDS; c.opts = opts;
  return loss_bwd_cls(c);
}

extern "C" int effdet_loss_opts_bwd_reg(const float* reg, const float* anchors, const float* annots, const float* gscale,
                                        const void* workspace, void* dreg, int reg_ld, int dtype, int B, long long A, int N,
                                        const effdet_loss_opts_t* opts, effdet_stream_t stream) {
  LossCall c{loss_args(nullptr, reg, anchors, annots, B, A, 0, N), workspace, 0, (hipStream_t)stream};
  c.k.gscale = gscale; c.dtype = dtype; c.k.dreg = dreg; c.k.reg_ld = reg_ld; c.matcher = MATCH_BANDS; c.opts = opts;
  return loss_bwd_reg(c);
}

extern "C" int effdet_loss_atss_fwd(const float* cls, const float* reg, const float* anchors, const float* annots, float* losses,
                                    void* workspace, long long workspace_bytes, int B, long long A, int num_classes, int N,
                                    const effdet_loss_opts_t* opts, const effdet_atss_t* atss, effdet_stream_t stream) {
  LossCall c{loss_args(cls, reg, anchors, annots, B, A, num_classes, N), workspace, workspace_bytes, (hipStream_t)stream};
  c.k.losses = losses; c.matcher = MATCH_ATSS; c.opts = opts; c.atss = atss;
  return loss_forward(c);
}

extern "C" int effdet_loss_atss_fwd_grad(const float* cls, const float* reg, const float* anchors, const float* annots, float* losses,
                                         void* workspace, long long workspace_bytes, void* dcls_pix, int dld, int dtype, int B,
                                         long long A, int num_classes, int N, const effdet_loss_opts_t* opts,
                                         const effdet_atss_t* atss, effdet_stream_t stream) {
  LossCall c{loss_args(cls, reg, anchors, annots, B, A, num_classes, N), workspace, workspace_bytes, (hipStream_t)stream};
  c.k.losses = losses; c.k.dcls = dcls_pix; c.k.dld = dld; c.dtype = dtype; c.grad = true;
  c.matcher = MATCH_ATSS; c.opts = opts; c.atss = atss;
  return loss_forward(c);
}

// (a null atss: the bands of the options)
extern "C" int effdet_loss_quality_fwd(const float* cls, const float* reg, const float* anchors, const float* annots, float* losses,
                                       void* workspace, long long workspace_bytes, int B, long long A, int num_classes, int N,
                                       const effdet_loss_opts_t* opts, const effdet_atss_t* atss, const effdet_quality_loss_t* quality,
                                       effdet_stream_t stream) {
  LossCall c{loss_args(cls, reg, anchors, annots, B, A, num_classes, N), workspace, workspace_bytes, (hipStream_t)stream};
  c.k.losses = losses; c.matcher = atss ? MATCH_ATSS : MATCH_BANDS; c.opts = opts; c.atss = atss; c.ql = quality; c.need_ql = true;
  return loss_forward(c);
}

extern "C" int effdet_loss_quality_fwd_grad(const float* cls, const float* reg, const float* anchors, const float* annots, float* losses,
                                            void* workspace, long long workspace_bytes, void* dcls_pix, int dld, int dtype, int B,
                                            long long A, int num_classes, int N, const effdet_loss_opts_t* opts,
                                            const effdet_atss_t* atss, const effdet_quality_loss_t* quality, effdet_stream_t stream) {
  LossCall c{loss_args(cls, reg, anchors, annots, B, A, num_classes, N), workspace, workspace_bytes, (hipStream_t)stream};
  c.k.losses = losses; c.k.dcls = dcls_pix; c.k.dld = dld; c.dtype = dtype; c.grad = true;
  c.matcher = atss ? MATCH_ATSS : MATCH_BANDS; c.opts = opts; c.atss = atss; c.ql = quality; c.need_ql = true;
  return loss_forward(c);
}

extern "C" int effdet_loss_quality_bwd_cls(const float* cls, const float* annots, const float* gscale, const void* workspace, void* dcls,
                                           int dld, int dtype, int B, long long A, int num_classes, int N,
                                           const effdet_loss_opts_t* opts, const effdet_quality_loss_t* quality, effdet_stream_t stream) {
  LossCall c{loss_args(cls, nullptr, nullptr, annots, B, A, num_classes, N), workspace, 0, (hipStream_t)stream};
  c.k.gscale = gscale; c.dtype = dtype; c.k.dcls = dcls; c.k.dld = dld;
  c.matcher = MATCH_BANDS; c.opts = opts; c.ql = quality; c.need_ql = true;
  return loss_bwd_cls(c);
}

extern "C" int effdet_loss_tal_fwd(const float* cls, const float* reg, const float* anchors, const float* annots, float* losses,
                                   void* workspace, long long workspace_bytes, int B, long long A, int num_classes, int N,
                                   const effdet_loss_opts_t* opts, const effdet_tal_t* tal, const effdet_quality_loss_t* quality,
                                   effdet_stream_t stream) {
  LossCall c{loss_args(cls, reg, anchors, annots, B, A, num_classes, N), workspace, workspace_bytes, (hipStream_t)stream};
  c.k.losses = losses; c.matcher = MATCH_TAL; c.opts = opts; c.tal = tal; c.ql = quality;
  return loss_forward(c);
}

extern "C" int effdet_loss_tal_fwd_grad(const float* cls, const float* reg, const float* anchors, const float* annots, float* losses,
                                        void* workspace, long long workspace_bytes, void* dcls_pix, int dld, int dtype, int B,
                                        long long A, int num_classes, int N, const effdet_loss_opts_t* opts, const effdet_tal_t* tal,
                                        const effdet_quality_loss_t* quality, effdet_stream_t stream) {
  LossCall c{loss_args(cls, reg, anchors, annots, B, A, num_classes, N), workspace, workspace_bytes, (hipStream_t)stream};
  c.k.losses = losses; c.k.dcls = dcls_pix; c.k.dld = dld; c.dtype = dtype; c.grad = true;
  c.matcher = MATCH_TAL; c.opts = opts; c.tal = tal; c.ql = quality;
  return loss_forward(c);
}

extern "C" int effdet_loss_tal_metrics(const float* cls, const float* reg, const float* anchors, const float* annots, float* out, int B,
                                       long long A, int num_classes, int N, const effdet_tal_t* tal, effdet_stream_t stream) {
  if (!cls || !reg || !anchors || !annots || !out || !tal_ok(tal)) return EFFDET_EINVAL;
  if (B < 1 || B > 65535 || N < 1 || N > 65535 || A < 1 || num_classes < 1) return EFFDET_EINVAL;
  if (A * num_classes >= 0x7fffffffLL) return EFFDET_EUNSUPPORTED;
  const LossK k = loss_args(cls, reg, anchors, annots, B, A, num_classes, N);
  hipLaunchKernelGGL(tal_metrics_kernel, dim3((unsigned)assign_blocks(A), N, B), dim3(256), 0, (hipStream_t)stream, k, tal_args(tal), out);
  EFFDET_CHECK_LAUNCH();
  return EFFDET_OK;
}
