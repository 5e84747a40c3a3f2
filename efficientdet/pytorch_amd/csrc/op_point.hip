// Operating-point metrics (include/effdet_op_point.h): precision / recall / F1 against a grid of confidence thresholds over the
// records of effdet_voc_match, and a confusion matrix over the rows of effdet_finalize_dets.  Compiled with -ffp-contract=off: every
// fp64 operation of the header's tables rounds once, and the IoU is voc_map.hip's expression in its operation order.
//
//   effdet_op_curves: the class sort of effdet_voc_ap (radix_sort.h's rs_class_sort(): rs_init_kernel, rs_sort(), then the
//     rs_segment_bounds() of rs_segments_kernel); then
//     op_sweep_kernel (one workgroup per class: exact integer inclusive cumsum of the TP bytes over the class's sorted segment, in
//     256-record chunks with a carry), op_count_kernel (a grid over (class, threshold): a binary search of the threshold's key in the
//     score-descending segment gives npred, the cumsum in front of it gives tp; precision, recall, f1 from them), op_mean_kernel (one
//     thread per threshold: the sequential sum over the classes with ground truth) and op_best_kernel (one workgroup per row of `best`:
//     the first maximum of an f1 row through a fixed LDS tree whose ties go to the lower j).
//   effdet_confusion_match (one workgroup per image): the GT rows are staged in LDS as voc_match_kernel stages them; nothing is kept
//     per detection, every pass recomputes a prediction's best object.  Pass 1: atomic max of the IoU bits per object; pass 2: atomic
//     min of the row among the predictions holding that IoU; pass 3: the counts.
#include "box_geom.h"
#include "block_scan.h"
#include "radix_sort.h"
#include "../../../include/effdet_op_point.h"
#include <float.h>
#include <limits.h>

namespace {

constexpr int OP_MAX_CLASSES = 65535;          // effdet_voc_ap's range: class values 0..C fit the two class passes of the sort
constexpr int CM_MAX_GT = 2048;                // GT rows per image staged in LDS
constexpr size_t CM_GT_LDS = 4 * sizeof(double) + sizeof(unsigned long long) + 2 * sizeof(int);   // box, winner's IoU bits, label, winner's row

// one workgroup per class: cum[i] = TP bytes of the class's sorted records up to and including position i
__global__ __launch_bounds__(256) void op_sweep_kernel(const unsigned* __restrict__ sval, const unsigned char* __restrict__ rec_tp,
                                                       const int* __restrict__ seg, int* __restrict__ cum) {
  __shared__ int itot[4];
  const int c = blockIdx.x, tid = threadIdx.x;
  const long long s0 = seg[2 * c], s1 = seg[2 * c + 1];
  int carry = 0;
  for (long long base = s0; base < s1; base += 256) {            // (uniform bounds: every thread reaches every barrier)
    const long long i = base + tid;
    const int v = i < s1 ? (int)rec_tp[sval[i]] : 0;
    int tot;
    const int incl = block_scan_sum(v, itot, &tot);
    if (i < s1) cum[i] = carry + incl;
    carry += tot;
  }
}

// grid (ceil(M / 256), C): class c = blockIdx.y against threshold j
__global__ __launch_bounds__(256) void op_count_kernel(const unsigned long long* __restrict__ skey, const int* __restrict__ cum,
                                                       const int* __restrict__ seg, const int* __restrict__ gt_counter,
                                                       const float* __restrict__ thresholds, int M, int* __restrict__ tp,
                                                       int* __restrict__ npred, double* __restrict__ precision,
                                                       double* __restrict__ recall, double* __restrict__ f1) {
  const int c = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
  if (j >= M) return;
  const unsigned tkey = rs_score_key(thresholds[j]);
  const int s0 = seg[2 * c];
  int lo = s0, hi = seg[2 * c + 1];
  while (lo < hi) {                                               // first position of the segment whose key is not below tkey
    const int mid = lo + ((hi - lo) >> 1);
    if ((unsigned)skey[mid] < tkey) lo = mid + 1; else hi = mid;
  }
  const int np = lo - s0;
  const int t = np > 0 ? cum[lo - 1] : 0;
  const int n = gt_counter[c];
  const double p = np == 0 ? 1.0 : (double)t / (double)np;
  const double r = n == 0 ? 0.0 : (double)t / (double)n;
  const double s = p + r;
  const double f = s == 0.0 ? 0.0 : (2.0 * p * r) / s;
  const long long o = (long long)c * M + j;
  tp[o] = t; npred[o] = np;
  precision[o] = p; recall[o] = r; f1[o] = f;
}

// one thread per threshold: mean_curves[q][j] over the classes with ground truth, ascending class order
__global__ __launch_bounds__(256) void op_mean_kernel(const double* __restrict__ precision, const double* __restrict__ recall,
                                                      const double* __restrict__ f1, const int* __restrict__ gt_counter, int C, int M,
                                                      double* __restrict__ mean_curves) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= M) return;
  double sp = 0.0, sr = 0.0, sf = 0.0;
  int K = 0;
  for (int c = 0; c < C; ++c) {
    if (gt_counter[c] <= 0) continue;
    const long long o = (long long)c * M + j;
    sp += precision[o]; sr += recall[o]; sf += f1[o];
    ++K;
  }
  const double k = (double)K;
  mean_curves[j] = K ? sp / k : 0.0;
  mean_curves[M + j] = K ? sr / k : 0.0;
  mean_curves[2LL * M + j] = K ? sf / k : 0.0;
}

// workgroup c < C: class c's row of `best`; workgroup C: the mean curves' row
__global__ __launch_bounds__(256) void op_best_kernel(const double* __restrict__ precision, const double* __restrict__ recall,
                                                      const double* __restrict__ f1, const double* __restrict__ mean_curves,
                                                      const int* __restrict__ gt_counter, int C, int M, double* __restrict__ best) {
  __shared__ double bv[256];
  __shared__ int bj[256];
  const int c = blockIdx.x, tid = threadIdx.x;
  int any = 0;
  if (c < C) any = gt_counter[c] > 0;
  else for (int q = tid; q < C; q += 256) any |= gt_counter[q] > 0;
  any = __syncthreads_or(any);
  double* row = best + 4LL * c;
  if (!any) {
    if (tid == 0) { row[0] = -1.0; row[1] = 0.0; row[2] = 0.0; row[3] = 0.0; }
    return;
  }
  const double* P = c < C ? precision + (long long)c * M : mean_curves;
  const double* R = c < C ? recall + (long long)c * M : mean_curves + M;
  const double* F = c < C ? f1 + (long long)c * M : mean_curves + 2LL * M;
  double v = -1.0;                                                // (every f1 is >= 0)
  int at = INT_MAX;
  for (int j = tid; j < M; j += 256) {
    const double f = F[j];
    if (f > v) { v = f; at = j; }                                 // ascending j: the first maximum of the thread's share
  }
  bv[tid] = v; bj[tid] = at;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) {
      const double ov = bv[tid + s];
      const int oj = bj[tid + s];
      if (ov > bv[tid] || (ov == bv[tid] && oj < bj[tid])) { bv[tid] = ov; bj[tid] = oj; }      // (block_best.h's order, on LDS slots)
    }
    __syncthreads();
  }
  if (tid == 0) {
    const int j = bj[0];                                          // (M >= 1: thread 0 holds j = 0 at least)
    row[0] = (double)j; row[1] = P[j]; row[2] = R[j]; row[3] = F[j];
  }
}

struct OpWs { RsBufs<unsigned long long> rs; int* seg; int* cum; };

size_t op_carve(OpWs& w, void* base, long long N) {
  Carver c(base);
  const size_t n = (size_t)(N > 0 ? N : 1);
  rs_carve(w.rs, c, 1, n);
  w.seg = c.take<int>(2 * (size_t)OP_MAX_CLASSES);
  w.cum = c.take<int>(n);
  return c.off;
}

// a row of dets that is a prediction of the confusion matrix -> its class, else -1
__device__ __forceinline__ int cm_pred_class(const float* r, int C, float conf) {
  int c;
  if (!label_class(r[5], C, c)) return -1;
  return r[4] > conf ? c : -1;
}

// the prediction's best candidate object: the first maximum of box_geom.h's box_overlap_f64 over the objects (gl[j] >= 0) among those
// with iou > thr; -1 without a candidate
__device__ __forceinline__ int cm_best_object(const float* r, const double* gb, const int* gl, int G, double thr, double& best) {
  const double a0 = r[0], a1 = r[1], a2 = r[2], a3 = r[3];
  const double aarea = (a2 - a0) * (a3 - a1);
  int arg = -1;
  best = thr;
  for (int j = 0; j < G; ++j) {
    if (gl[j] < 0) continue;
    const double iou = box_overlap_f64(a0, a1, a2, a3, aarea, gb + 4 * j);
    if (iou > best) { best = iou; arg = j; }       // strictly above the threshold, then the first maximum
  }
  return arg;
}

// a candidate's IoU is > thr; with a negative thr it can be +0.0 (bits 0) but never negative: its bits order like the value
__device__ __forceinline__ unsigned long long cm_bits(double iou) { return (unsigned long long)__double_as_longlong(iou); }

__global__ __launch_bounds__(256) void confusion_kernel(const float* __restrict__ dets, const int* __restrict__ counts,
                                                        const double* __restrict__ gt_boxes, const int* __restrict__ gt_labels,
                                                        int max_det, int G, int C, float conf, double thr,
                                                        unsigned long long* __restrict__ counter) {
  extern __shared__ double cm_lds[];
  double* gb = cm_lds;                                            // [G][4]
  unsigned long long* top = (unsigned long long*)(gb + 4 * G);    // [G] largest IoU bits among the predictions that kept the object
  int* gl = (int*)(top + G);                                      // [G] label, -1 = no object
  int* win = gl + G;                                              // [G] lowest row holding `top`
  const int b = blockIdx.x, tid = threadIdx.x;
  for (int j = tid; j < G; j += 256) {
    const double* src = gt_boxes + ((long long)b * G + j) * 4;
    gb[4 * j] = src[0]; gb[4 * j + 1] = src[1]; gb[4 * j + 2] = src[2]; gb[4 * j + 3] = src[3];
    const int lab = gt_labels[(long long)b * G + j];
    gl[j] = (lab >= 0 && lab < C) ? lab : -1;
    top[j] = 0ull;
    win[j] = INT_MAX;
  }
  __syncthreads();
  int n = counts[b];
  n = n < 0 ? 0 : (n > max_det ? max_det : n);
  const float* d = dets + (long long)b * max_det * 6;
  for (int k = tid; k < n; k += 256) {
    const float* r = d + (long long)k * 6;
    if (cm_pred_class(r, C, conf) < 0) continue;
    double best;
    const int a = cm_best_object(r, gb, gl, G, thr, best);
    if (a >= 0) atomicMax(&top[a], cm_bits(best));
  }
  __syncthreads();
  for (int k = tid; k < n; k += 256) {
    const float* r = d + (long long)k * 6;
    if (cm_pred_class(r, C, conf) < 0) continue;
    double best;
    const int a = cm_best_object(r, gb, gl, G, thr, best);
    if (a >= 0 && cm_bits(best) == top[a]) atomicMin(&win[a], k);
  }
  __syncthreads();
  const long long ld = (long long)C + 1;
  for (int k = tid; k < n; k += 256) {
    const float* r = d + (long long)k * 6;
    const int pc = cm_pred_class(r, C, conf);
    if (pc < 0) continue;
    double best;
    const int a = cm_best_object(r, gb, gl, G, thr, best);
    const int col = (a >= 0 && win[a] == k) ? gl[a] : C;
    atomicAdd(&counter[pc * ld + col], 1ull);
  }
  for (int j = tid; j < G; j += 256)
    if (gl[j] >= 0 && win[j] == INT_MAX) atomicAdd(&counter[C * ld + gl[j]], 1ull);
}

}  // namespace

extern "C" long long effdet_op_curves_workspace_bytes(long long num_records) {
  if (num_records < 0 || num_records > (long long)INT_MAX) return 0;
  OpWs w;
  return (long long)op_carve(w, nullptr, num_records);
}

extern "C" int effdet_op_curves(const unsigned long long* rec_key, const unsigned char* rec_tp, long long num_records, const int* gt_count,
                                int num_classes, const float* thresholds, int num_thresholds, void* workspace, long long workspace_bytes,
                                int* tp, int* npred, double* precision, double* recall, double* f1, double* mean_curves, double* best,
                                effdet_stream_t stream) {
  const long long N = num_records;
  const int C = num_classes, M = num_thresholds;
  if (!gt_count || !thresholds || !workspace || !tp || !npred || !precision || !recall || !f1 || !mean_curves || !best || N < 0 ||
      N > (long long)INT_MAX || C < 1 || (N > 0 && (!rec_key || !rec_tp)))
    return EFFDET_EINVAL;
  if (M < 1 || M > EFFDET_OP_MAX_THRESHOLDS || C > OP_MAX_CLASSES) return EFFDET_EUNSUPPORTED;
  OpWs w;
  if ((long long)op_carve(w, workspace, N) > workspace_bytes) return EFFDET_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* ki; unsigned* vi;
  if (const int rc = rs_class_sort(rec_key, N, C, w.rs, w.seg, ki, vi, st)) return rc;
  if (N > 0) {
    hipLaunchKernelGGL(op_sweep_kernel, dim3(C), dim3(256), 0, st, (const unsigned*)vi, rec_tp, (const int*)w.seg, w.cum);
    EFFDET_CHECK_LAUNCH();
  }
  const int mb = (M + 255) / 256;
  hipLaunchKernelGGL(op_count_kernel, dim3(mb, C), dim3(256), 0, st, (const unsigned long long*)ki, (const int*)w.cum, (const int*)w.seg,
                     gt_count, thresholds, M, tp, npred, precision, recall, f1);
  hipLaunchKernelGGL(op_mean_kernel, dim3(mb), dim3(256), 0, st, (const double*)precision, (const double*)recall, (const double*)f1,
                     gt_count, C, M, mean_curves);
  hipLaunchKernelGGL(op_best_kernel, dim3(C + 1), dim3(256), 0, st, (const double*)precision, (const double*)recall, (const double*)f1,
                     (const double*)mean_curves, gt_count, C, M, best);
  EFFDET_CHECK_LAUNCH();
  return EFFDET_OK;
}

extern "C" int effdet_confusion_match(const float* dets, const int* counts, const double* gt_boxes, const int* gt_labels, int B, int max_det,
                                      int G, int num_classes, float conf_threshold, double iou_threshold, long long* matrix,
                                      effdet_stream_t stream) {
  if (!dets || !counts || !gt_boxes || !gt_labels || !matrix || B < 1 || max_det < 1 || G < 1 || num_classes < 1 ||
      num_classes > OP_MAX_CLASSES || conf_threshold != conf_threshold || iou_threshold != iou_threshold)
    return EFFDET_EINVAL;
  if (G > CM_MAX_GT) return EFFDET_EUNSUPPORTED;
  const size_t lds = (size_t)G * CM_GT_LDS;
  EFFDET_SET_MAX_LDS(confusion_kernel, (size_t)CM_MAX_GT * CM_GT_LDS);
  hipLaunchKernelGGL(confusion_kernel, dim3(B), dim3(256), lds, (hipStream_t)stream, dets, counts, gt_boxes, gt_labels, max_det, G,
                     num_classes, conf_threshold, iou_threshold, (unsigned long long*)matrix);
  EFFDET_CHECK_LAUNCH();
  return EFFDET_OK;
}
