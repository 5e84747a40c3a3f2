// Device-side COCO box mean AP (pycocotools' COCOeval, iouType='bbox', useCats=1): evaluateImg's per-(image, category) greedy
// matching over every IoU threshold and area range, accumulate's per-(category, area, maxDets) score sort, cumsums, precision
// envelope and recall-threshold lookups, and summarize's 12 means.  Compiled with -ffp-contract=off: the fp64 IoU of maskApi.c
// bbIou must round exactly like the C source's unfused operations, or IoUs at exactly a threshold change their decision.
//
//   effdet_coco_match (one workgroup per image): the image's ground truth is staged in LDS (fp64 xywh, per-area ignore bits, crowd
//     bit), grouped by category in annotation order.  Every detection row gets its rank within (image, category) in row order
//     (finalize_dets' rows are score-descending, so this is COCOeval's stable score sort); rows of rank >= maxDets[-1] are dropped.
//     The greedy matching runs one WAVE per category present and one LANE per (area a, threshold t) -- lane = a * T + t: the
//     lanes walk the category's detections in rank order in lockstep, each against the category's GTs in its own ignore-sorted
//     order (non-ignored first, both halves in annotation order) with its matched-GT bit in an LDS word per GT; one __ballot per
//     detection then gives the record's 64 matched bits and 64 ignored bits directly.  The image's records are compacted in
//     (category, rank) order into its own slots [b * S, b * S + kept) (S = min(max_det, maxDets[-1] * K)); the rest of the slots
//     are padding records that sort after every category.  Non-ignored GT counts go to npig[K][A] with integer atomics.
//   effdet_coco_accumulate: a stable LSD radix sort of all records by image id (the low bytes the largest id needs), then by the
//     64-bit (category, descending score) key: ties of one category's scores rank by (image id, rank), as COCOeval's mergesort over
//     the images in np.unique order does.  Category bounds come from the sorted keys; the sorted rank / bits are gathered into
//     contiguous arrays; then one workgroup per (k, a, m), per threshold t: a forward block reduction gives the TP / FP totals and
//     a reverse sweep rebuilds the exact integer cumsums from the right, recall / precision in fp64, the envelope (running max
//     from the right) and, at each point where recall steps, the recThrs it answers (searchsorted 'left').  A last launch reduces
//     the 12 summary statistics in a fixed order.  Every launch geometry follows from the arguments alone.
#include "box_geom.h"
#include "block_scan.h"
#include "radix_sort.h"
#include <limits.h>
#include <math.h>

namespace {

constexpr int COCO_MAX_GT = 2048;           // GT rows per image staged in LDS (as VOC_MAX_GT)
constexpr size_t COCO_GT_LDS = 4 * sizeof(double) + sizeof(unsigned long long) + sizeof(int);     // bytes per GT row: box, gtm, gflag
constexpr int COCO_MAX_CATEGORIES = 1024;   // categories; the category occupies 10 bits of the sort key (2 passes above 255)
constexpr int COCO_MAX_T = 16, COCO_MAX_A = 4, COCO_MAX_M = 3, COCO_MAX_R = 128, COCO_MAX_DETS = 100;

struct CocoMatchParams {
  double iou[COCO_MAX_T];                  // min(iouThrs[t], 1 - 1e-10): evaluateImg's starting `iou`
  double rng[2 * COCO_MAX_A];              // areaRng[a] = [lo, hi], both ends inclusive
  int T, A, max_det_last;
};

struct CocoAccParams {
  double iou[COCO_MAX_T];                  // iouThrs (summarize selects 0.5 / 0.75 by ==)
  double rec[COCO_MAX_R];                  // recThrs
  int max_dets[COCO_MAX_M];
  int T, R, A, M;
};

// maskApi.c bbIou for one (detection, GT) pair, fp64, in the C source's operation order
__device__ __forceinline__ double coco_iou(double dx, double dy, double dw, double dh, double da, const double* g, bool crowd) {
  const double w = fmin(dw + dx, g[2] + g[0]) - fmax(dx, g[0]);
  if (w <= 0) return 0.0;
  const double h = fmin(dh + dy, g[3] + g[1]) - fmax(dy, g[1]);
  if (h <= 0) return 0.0;
  const double i = w * h;
  const double u = crowd ? da : da + g[2] * g[3] - i;
  return i / u;
}

// dets [B][max_det][6] (x, y, w, h, score, label) fp32 + counts [B]; gt [B][G][7] fp64 (x, y, w, h, category, iscrowd, area;
// a category outside [0, K) = padding); records of image b at [b * S, (b + 1) * S).
__global__ __launch_bounds__(256) void coco_match_kernel(const float* __restrict__ dets, const int* __restrict__ counts,
                                                         const int* __restrict__ image_ids, const double* __restrict__ gt, int max_det,
                                                         int G, int K, int S, CocoMatchParams P, unsigned long long* __restrict__ rec_key,
                                                         unsigned* __restrict__ rec_image, unsigned char* __restrict__ rec_rank,
                                                         unsigned long long* __restrict__ rec_match,
                                                         unsigned long long* __restrict__ rec_ignore, int* __restrict__ npig_counter) {
  extern __shared__ double coco_lds[];
  double* gbox = coco_lds;                                       // [G][4], grouped by category
  unsigned long long* gtm = (unsigned long long*)(gbox + 4 * G); // [G] bit lane = matched by lane (a, t); phase 1: int category
  int* gflag = (int*)(gtm + G);                                  // [G] bits 0..3 ignored for area a, bit 4 crowd
  int* gt_counter = gflag + G;                                   // [K] GT per category
  int* cstart = gt_counter + K;                                  // [K + 1]
  int* det_counter = cstart + K + 1;                             // [K] detection rows per category
  int* dstart = det_counter + K;                                 // [K + 1] kept records per category, exclusive prefix
  int* present = dstart + K + 1;                                 // [K + 1] categories with kept detections; [K] = their number
  int* gcat = (int*)gtm;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int A = P.A, T = P.T;
  int n = counts[b];
  n = n < 0 ? 0 : (n > max_det ? max_det : n);
  const float* d = dets + (long long)b * max_det * 6;
  const double* g0 = gt + (long long)b * G * 7;
  for (int c = tid; c < K; c += 256) { gt_counter[c] = 0; det_counter[c] = 0; }
  __syncthreads();
  for (int j = tid; j < G; j += 256) {
    const double cv = g0[(long long)j * 7 + 4];
    const int c = (cv >= 0.0 && cv < (double)K && (double)(int)cv == cv) ? (int)cv : -1;
    gcat[j] = c;
    if (c >= 0) atomicAdd(&gt_counter[c], 1);
  }
  for (int k = tid; k < n; k += 256) {
    int c;
    if (label_class(d[(long long)k * 6 + 5], K, c)) atomicAdd(&det_counter[c], 1);
  }
  __syncthreads();
  if (tid == 0) {
    int gs = 0, ds = 0, np = 0;
    for (int c = 0; c < K; ++c) {
      cstart[c] = gs; gs += gt_counter[c];
      dstart[c] = ds;
      const int kept = det_counter[c] < P.max_det_last ? det_counter[c] : P.max_det_last;
      ds += kept;
      if (kept) present[np++] = c;
    }
    cstart[K] = gs; dstart[K] = ds; present[K] = np;
  }
  __syncthreads();
  for (int j = tid; j < G; j += 256) {                           // stable group-by-category of the GT rows
    const int c = gcat[j];
    if (c < 0) continue;
    int r = 0;
    for (int q = 0; q < j; ++q) r += gcat[q] == c;
    const int dst = cstart[c] + r;
    const double* src = g0 + (long long)j * 7;
    const double area = src[6];
    const bool crowd = src[5] != 0.0;
    int fl = crowd ? 16 : 0;
    for (int a = 0; a < A; ++a) {
      const bool ig = crowd || area < P.rng[2 * a] || area > P.rng[2 * a + 1];
      if (ig) fl |= 1 << a;
      else atomicAdd(&npig_counter[c * A + a], 1);
    }
    gbox[4 * dst] = src[0]; gbox[4 * dst + 1] = src[1]; gbox[4 * dst + 2] = src[2]; gbox[4 * dst + 3] = src[3];
    gflag[dst] = fl;
  }
  const long long base = (long long)b * S;
  for (int s = dstart[K] + tid; s < S; s += 256) {               // padding records: category K sorts after every category
    rec_key[base + s] = ((unsigned long long)K << 32) | 0xffffffffull;
    rec_image[base + s] = 0u;
    rec_rank[base + s] = 255;
    rec_match[base + s] = 0ull;
    rec_ignore[base + s] = 0ull;
  }
  __syncthreads();                                               // gcat (aliasing gtm) is dead from here on
  const unsigned iid = (unsigned)image_ids[b];
  const bool active = lane < A * T;
  const int la = active ? lane / T : 0, lt = active ? lane - la * T : 0;
  const double lo = P.rng[2 * la], hi = P.rng[2 * la + 1], thr0 = P.iou[lt];
  const int npresent = present[K];
  for (int p = wave; p < npresent; p += 4) {                     // one category per wave
    const int c = present[p];
    const int g_begin = cstart[c], g_end = cstart[c + 1];
    for (int gi = g_begin + lane; gi < g_end; gi += 64) gtm[gi] = 0ull;
    __builtin_amdgcn_wave_barrier();
    const int kept = dstart[c + 1] - dstart[c];
    const long long out0 = base + dstart[c];
    int rank = 0;
    for (int r0 = 0; r0 < n && rank < kept; r0 += 64) {          // (wave-uniform)
      const int k = r0 + lane;
      int ck;
      const bool mine = k < n && label_class(d[(long long)k * 6 + 5], K, ck) && ck == c;
      unsigned long long mask = __ballot(mine);
      while (mask && rank < kept) {
        const int j = __ffsll((long long)mask) - 1;
        mask &= mask - 1ull;
        const float* row = d + (long long)(r0 + j) * 6;
        const double dx = row[0], dy = row[1], dw = row[2], dh = row[3];
        const double da = dw * dh;
        double best = thr0;
        int m = -1, mig = 0;
        if (active) {
          for (int pass = 0; pass < 2 && m < 0; ++pass) {        // non-ignored GTs first, then ignored ones (a matched non-ignored
            for (int gi = g_begin; gi < g_end; ++gi) {           // GT ends the walk at the first ignored one: COCOeval's `break`)
              const int fl = gflag[gi];
              const int ig = (fl >> la) & 1;
              if (ig != pass) continue;
              const bool crowd = (fl >> 4) & 1;
              if (((gtm[gi] >> lane) & 1ull) && !crowd) continue;
              const double iou = coco_iou(dx, dy, dw, dh, da, gbox + 4 * gi, crowd);
              if (iou < best) continue;
              best = iou; m = gi; mig = ig;
            }
          }
          if (m >= 0) atomicOr(&gtm[m], 1ull << lane);
        }
        const bool matched = m >= 0;
        const bool ignored = matched ? (mig != 0) : (da < lo || da > hi);
        const unsigned long long bm = __ballot(active && matched), bi = __ballot(active && ignored);
        if (lane == 0) {
          const long long o = out0 + rank;
          rec_key[o] = ((unsigned long long)c << 32) | rs_score_key(row[4]);
          rec_image[o] = iid;
          rec_rank[o] = (unsigned char)rank;
          rec_match[o] = bm;
          rec_ignore[o] = bi;
        }
        ++rank;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ accumulate
// the (category, score) key of every record in image-id order
__global__ __launch_bounds__(256) void coco_key_gather_kernel(const unsigned long long* __restrict__ rec_key, const unsigned* __restrict__ v,
                                                              unsigned long long* __restrict__ k64, long long N) {
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < N; i += (long long)gridDim.x * 256) k64[i] = rec_key[v[i]];
}

// seg[2k], seg[2k + 1] = [first, last + 1) sorted position of category k; the sorted rank and bits made contiguous
__global__ __launch_bounds__(256) void coco_segments_kernel(const unsigned long long* __restrict__ skey, const unsigned* __restrict__ v,
                                                            const unsigned char* __restrict__ rec_rank,
                                                            const unsigned long long* __restrict__ rec_match,
                                                            const unsigned long long* __restrict__ rec_ignore, long long N, int K,
                                                            int* __restrict__ seg, unsigned char* __restrict__ s_rank,
                                                            unsigned long long* __restrict__ s_match, unsigned long long* __restrict__ s_ignore) {
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < N; i += (long long)gridDim.x * 256) {
    const unsigned r = v[i];
    s_rank[i] = rec_rank[r]; s_match[i] = rec_match[r]; s_ignore[i] = rec_ignore[r];
    rs_segment_bounds(skey, i, N, K, seg);
  }
}

// first index r of the sorted x[0..R) with x[r] > v
__device__ __forceinline__ int coco_upper(const double* x, int R, double v) {
  int lo = 0, hi = R;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (x[mid] > v) hi = mid; else lo = mid + 1; }
  return lo;
}

// one workgroup per (k, a, m): COCOeval.accumulate's inner loop over the thresholds t
__global__ __launch_bounds__(256) void coco_accumulate_kernel(const int* __restrict__ seg, const unsigned char* __restrict__ s_rank,
                                                              const unsigned long long* __restrict__ s_match,
                                                              const unsigned long long* __restrict__ s_ignore, const int* __restrict__ npig_,
                                                              int K, CocoAccParams P, double* __restrict__ precision,
                                                              double* __restrict__ recall) {
  __shared__ unsigned long long itot[4];
  __shared__ double dtot[4];
  __shared__ int fmin_[4];
  __shared__ double rthr[COCO_MAX_R];
  const int k = blockIdx.x, a = blockIdx.y, m = blockIdx.z, tid = threadIdx.x;
  const int T = P.T, R = P.R, A = P.A, M = P.M;
  for (int r = tid; r < R; r += 256) rthr[r] = P.rec[r];
  const long long kam = ((long long)k * A + a) * M + m;          // offset of (k, a, m) in [K][A][M]
  const long long rstride = (long long)K * A * M;                // stride of r in precision [T][R][K][A][M]
  const int npig = npig_[k * A + a];
  if (npig == 0) {                                               // accumulate's `continue`: the entries stay -1
    for (int t = 0; t < T; ++t) {
      for (int r = tid; r < R; r += 256) precision[((long long)t * R + r) * rstride + kam] = -1.0;
      if (tid == 0) recall[(long long)t * rstride + kam] = -1.0;
    }
    return;
  }
  const double np_ = (double)npig;
  const int maxdet = P.max_dets[m];
  const long long s0 = seg[2 * k], s1 = seg[2 * k + 1];
  // the first record of the sequence (rank < maxDet): precision's lookup for recall thresholds <= rc[0] lands on it
  int first = INT_MAX;
  for (long long i = s0 + tid; i < s1; i += 256)
    if ((int)s_rank[i] < maxdet) { first = (int)i; break; }
  {
    int x = first;
    for (int o = 32; o > 0; o >>= 1) { const int y = __shfl_xor(x, o, 64); x = y < x ? y : x; }
    if ((tid & 63) == 0) fmin_[tid >> 6] = x;
    __syncthreads();
    first = min(min(fmin_[0], fmin_[1]), min(fmin_[2], fmin_[3]));
    __syncthreads();
  }
  const bool nd = first != INT_MAX;
  for (int t = 0; t < T; ++t) {
    const int bit = a * T + t;
    // totals: TP in the high word, FP in the low word (a category holds < 2^31 records)
    unsigned long long part = 0;
    for (long long i = s0 + tid; i < s1; i += 256) {
      if ((int)s_rank[i] >= maxdet) continue;
      const unsigned long long mt = (s_match[i] >> bit) & 1ull, ig = (s_ignore[i] >> bit) & 1ull;
      if (!ig) part += mt ? (1ull << 32) : 1ull;
    }
    unsigned long long tot;
    {
      unsigned long long x = part;
      for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
      if ((tid & 63) == 0) itot[tid >> 6] = x;
      __syncthreads();
      tot = itot[0] + itot[1] + itot[2] + itot[3];
      __syncthreads();
    }
    const long long TP = (long long)(tot >> 32);
    // reverse sweep: cumsums at i rebuilt from the right, envelope = running max from the right
    unsigned long long carry = 0;
    double env = 0.0;
    for (long long top = s1; top > s0; top -= 256) {             // (uniform bounds: every thread reaches every barrier)
      const long long i = top - 1 - tid;
      bool incl = false;
      unsigned long long v = 0;
      if (i >= s0 && (int)s_rank[i] < maxdet) {
        incl = true;
        const unsigned long long mt = (s_match[i] >> bit) & 1ull, ig = (s_ignore[i] >> bit) & 1ull;
        if (!ig) v = mt ? (1ull << 32) : 1ull;
      }
      unsigned long long ctot;
      const unsigned long long suf = carry + block_scan_sum(v, itot, &ctot);    // sum over positions >= i
      const unsigned long long after = suf - v;                                  // sum over positions > i
      const long long tp = TP - (long long)(after >> 32);
      const long long fp = (long long)(tot & 0xffffffffull) - (long long)(after & 0xffffffffull);
      const double dtp = (double)tp;
      const double pr = incl ? dtp / (((double)fp + dtp) + 2.220446049250313e-16) : 0.0;
      double mtot;
      const double e = fmax(block_scan_max(pr, dtot, &mtot), env);
      if (incl) {
        const double rc = dtp / np_;
        const int r_lo = (i == (long long)first) ? 0 : coco_upper(rthr, R, (double)(tp - (long long)(v >> 32)) / np_);
        const int r_hi = coco_upper(rthr, R, rc);
        for (int r = r_lo; r < r_hi; ++r) precision[((long long)t * R + r) * rstride + kam] = e;
      }
      carry += ctot;
      env = fmax(env, mtot);
    }
    const double rc_last = nd ? (double)TP / np_ : 0.0;
    const int r_end = nd ? coco_upper(rthr, R, rc_last) : 0;      // thresholds above the last recall: precision 0
    for (int r = r_end + tid; r < R; r += 256) precision[((long long)t * R + r) * rstride + kam] = 0.0;
    if (tid == 0) recall[(long long)t * rstride + kam] = rc_last;
  }
}

// summarize(): stat s = the mean of the selected entries > -1 (or -1), reduced in a fixed order; one workgroup per stat
__global__ __launch_bounds__(256) void coco_stats_kernel(const double* __restrict__ precision, const double* __restrict__ recall, int K,
                                                         CocoAccParams P, double* __restrict__ stats) {
  __shared__ double ssum[256];
  __shared__ long long scnt[256];
  const int s = blockIdx.x, tid = threadIdx.x;
  const int T = P.T, R = P.R, A = P.A, M = P.M;
  // COCOeval._summarizeDets: (ap, iouThr (0 = all), area index, maxDets)
  const int md2 = P.max_dets[M > 2 ? 2 : M - 1];
  const int ap = s < 6;
  const double iou_sel = s == 1 ? 0.5 : (s == 2 ? 0.75 : 0.0);
  const int area = s >= 3 && s <= 5 ? s - 2 : (s >= 9 ? s - 8 : 0);
  const int mdv = s == 0 ? 100 : (s == 6 ? P.max_dets[0] : (s == 7 ? P.max_dets[M > 1 ? 1 : 0] : md2));
  double acc = 0.0;
  long long cnt = 0;
  if (area < A) {
    const long long per_t = (long long)(ap ? R : 1) * K * M;     // (r, k, m) per threshold; a fixed
    for (int t = 0; t < T; ++t) {
      if (iou_sel != 0.0 && !(P.iou[t] == iou_sel)) continue;
      for (long long e = tid; e < per_t; e += 256) {
        const int m = (int)(e % M);
        if (P.max_dets[m] != mdv) continue;
        const long long rk = e / M;
        const int kk = (int)(rk % K);
        double v;
        if (ap) {
          const long long r = rk / K;
          v = precision[((((long long)t * R + r) * K + kk) * A + area) * M + m];
        } else {
          v = recall[(((long long)t * K + kk) * A + area) * M + m];
        }
        if (v > -1.0) { acc += v; ++cnt; }
      }
    }
  }
  ssum[tid] = acc; scnt[tid] = cnt;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) { ssum[tid] += ssum[tid + h]; scnt[tid] += scnt[tid + h]; }
    __syncthreads();
  }
  if (tid == 0) stats[s] = scnt[0] ? ssum[0] / (double)scnt[0] : -1.0;
}

struct CocoWs {
  RsBufs<unsigned long long> rs;
  unsigned long long *s_match, *s_ignore;
  unsigned char* s_rank;
  int* seg;
};

size_t coco_carve(CocoWs& w, void* base, long long N, int K) {
  Carver c(base);
  const size_t n = (size_t)(N > 0 ? N : 1);
  rs_carve(w.rs, c, 1, n);
  w.s_match = c.take<unsigned long long>(n); w.s_ignore = c.take<unsigned long long>(n);
  w.s_rank = c.take<unsigned char>(n);
  w.seg = c.take<int>((size_t)2 * (K > 0 ? K : 1));
  return c.off;
}

}  // namespace

extern "C" int effdet_coco_match(const float* dets, const int* counts, const int* image_ids, const double* gt, int B, int max_det, int G,
                                 int num_categories, const double* iou_thrs, int num_iou_thrs, const double* area_rng, int num_areas,
                                 int max_dets_last, unsigned long long* rec_key, unsigned* rec_image, unsigned char* rec_rank,
                                 unsigned long long* rec_match, unsigned long long* rec_ignore, int* npig, effdet_stream_t stream) {
  const int K = num_categories;
  if (!dets || !counts || !image_ids || !gt || !iou_thrs || !area_rng || !rec_key || !rec_image || !rec_rank || !rec_match ||
      !rec_ignore || !npig || B < 1 || max_det < 1 || G < 1 || K < 1 || num_iou_thrs < 1 || num_areas < 1 || max_dets_last < 1)
    return EFFDET_EINVAL;
  if (G > COCO_MAX_GT || K > COCO_MAX_CATEGORIES || num_iou_thrs > COCO_MAX_T || num_areas > COCO_MAX_A ||
      max_dets_last > COCO_MAX_DETS)
    return EFFDET_EUNSUPPORTED;
  CocoMatchParams P;
  for (int t = 0; t < num_iou_thrs; ++t) P.iou[t] = iou_thrs[t] < 1 - 1e-10 ? iou_thrs[t] : 1 - 1e-10;
  for (int a = 0; a < 2 * num_areas; ++a) P.rng[a] = area_rng[a];
  P.T = num_iou_thrs; P.A = num_areas; P.max_det_last = max_dets_last;
  const long long S = effdet_coco_slots(max_det, K, max_dets_last);
  const size_t lds = (size_t)G * COCO_GT_LDS + (size_t)(5 * K + 3) * sizeof(int);
  EFFDET_SET_MAX_LDS(coco_match_kernel, (size_t)COCO_MAX_GT * COCO_GT_LDS + (size_t)(5 * COCO_MAX_CATEGORIES + 3) * sizeof(int));
  hipLaunchKernelGGL(coco_match_kernel, dim3(B), dim3(256), lds, (hipStream_t)stream, dets, counts, image_ids, gt, max_det, G, K, (int)S, P,
                     rec_key, rec_image, rec_rank, rec_match, rec_ignore, npig);
  EFFDET_CHECK_LAUNCH();
  return EFFDET_OK;
}

extern "C" long long effdet_coco_slots(int max_det, int num_categories, int max_dets_last) {
  const long long cap = (long long)max_dets_last * num_categories;
  return max_det < cap ? (long long)max_det : cap;
}

extern "C" long long effdet_coco_accumulate_workspace_bytes(long long num_records, int num_categories) {
  CocoWs w;
  return (long long)coco_carve(w, nullptr, num_records, num_categories);
}

extern "C" int effdet_coco_accumulate(const unsigned long long* rec_key, const unsigned* rec_image, const unsigned char* rec_rank,
                                      const unsigned long long* rec_match, const unsigned long long* rec_ignore, long long num_records,
                                      unsigned max_image_id, const int* npig, int num_categories, const double* iou_thrs,
                                      int num_iou_thrs, const double* rec_thrs, int num_rec_thrs, int num_areas, const int* max_dets,
                                      int num_max_dets, void* workspace, long long workspace_bytes, double* precision, double* recall,
                                      double* stats, effdet_stream_t stream) {
  const long long N = num_records;
  const int K = num_categories;
  if (!npig || !iou_thrs || !rec_thrs || !max_dets || !workspace || !precision || !recall || !stats || N < 0 || N > (long long)INT_MAX ||
      K < 1 || num_iou_thrs < 1 || num_rec_thrs < 1 || num_areas < 1 || num_max_dets < 1 ||
      (N > 0 && (!rec_key || !rec_image || !rec_rank || !rec_match || !rec_ignore)))
    return EFFDET_EINVAL;
  if (K > COCO_MAX_CATEGORIES || num_iou_thrs > COCO_MAX_T || num_rec_thrs > COCO_MAX_R || num_areas > COCO_MAX_A ||
      num_max_dets > COCO_MAX_M)
    return EFFDET_EUNSUPPORTED;
  CocoWs w;
  if ((long long)coco_carve(w, workspace, N, K) > workspace_bytes) return EFFDET_EINVAL;
  CocoAccParams P;
  for (int t = 0; t < num_iou_thrs; ++t) P.iou[t] = iou_thrs[t];
  for (int r = 0; r < num_rec_thrs; ++r) P.rec[r] = rec_thrs[r];
  for (int m = 0; m < num_max_dets; ++m) {
    if (max_dets[m] < 0) return EFFDET_EINVAL;
    P.max_dets[m] = max_dets[m];
  }
  P.T = num_iou_thrs; P.R = num_rec_thrs; P.A = num_areas; P.M = num_max_dets;
  hipStream_t st = (hipStream_t)stream;
  unsigned* ia = (unsigned*)w.rs.ka;                             // the image-id passes use the key buffers as 32-bit keys
  unsigned* ib = (unsigned*)w.rs.kb;
  hipLaunchKernelGGL(rs_init_kernel<unsigned>, dim3(grid_for(N > 2LL * K ? N : 2LL * K)), dim3(256), 0, st, rec_image, ia, w.rs.va, N,
                     w.seg, K);
  EFFDET_CHECK_LAUNCH();
  unsigned *vi = w.rs.va, *vo = w.rs.vb;
  if (N > 0) {
    const int id_passes = max_image_id == 0u ? 0 : (max_image_id < 0x100u ? 1 : (max_image_id < 0x10000u ? 2 : (max_image_id < 0x1000000u ? 3 : 4)));
    if (const int rc = rs_sort(ia, vi, ib, vo, w.rs.hist, 1, N, w.rs.T, 0, id_passes, st)) return rc;
    // (category, score) keys in image-id order (only the permutation vi of the image-id passes is still needed)
    unsigned long long *ki = w.rs.ka, *ko = w.rs.kb;
    hipLaunchKernelGGL(coco_key_gather_kernel, dim3(grid_for(N)), dim3(256), 0, st, rec_key, (const unsigned*)vi, ki, N);
    EFFDET_CHECK_LAUNCH();
    const int passes = 4 + (K <= 255 ? 1 : 2);                   // category values 0..K (K = padding record)
    if (const int rc = rs_sort(ki, vi, ko, vo, w.rs.hist, 1, N, w.rs.T, 0, passes, st)) return rc;
    hipLaunchKernelGGL(coco_segments_kernel, dim3(grid_for(N)), dim3(256), 0, st, (const unsigned long long*)ki, (const unsigned*)vi,
                       rec_rank, rec_match, rec_ignore, N, K, w.seg, w.s_rank, w.s_match, w.s_ignore);
    EFFDET_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(coco_accumulate_kernel, dim3(K, num_areas, num_max_dets), dim3(256), 0, st, (const int*)w.seg,
                     (const unsigned char*)w.s_rank, (const unsigned long long*)w.s_match, (const unsigned long long*)w.s_ignore, npig, K,
                     P, precision, recall);
  EFFDET_CHECK_LAUNCH();
  hipLaunchKernelGGL(coco_stats_kernel, dim3(12), dim3(256), 0, st, (const double*)precision, (const double*)recall, K, P, stats);
  EFFDET_CHECK_LAUNCH();
  return EFFDET_OK;
}
