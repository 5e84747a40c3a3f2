// Device-side VOC mean AP (the reference's eval.py:165-257 `evaluate`, after `_get_detections`): greedy matching of every
// detection against the ground truth of its image and class, the per-class score sort, the TP / FP cumsums, recall / precision
// and `_compute_ap` (eval.py:46-73).  Compiled with -ffp-contract=off: the fp64 IoU of `compute_overlap` (eval.py:19-43) must
// round exactly like NumPy's unfused operations, or IoUs at exactly the threshold change their decision.
//
//   effdet_voc_match (one workgroup per image): the image's GT rows are staged in LDS; one thread per detection slot finds its
//     assigned GT (first maximum of the IoU over the class's GT rows, in row order) and cond = IoU >= threshold.  The reference
//     walks an image's detections of one class in score order and a detection whose best GT is already taken is a false positive
//     (no fall-back to the second best), so TP(d) = cond(d) and d is the FIRST slot with cond and that assigned GT: an LDS
//     atomicMin of the slot index per GT decides it order-independently.  One record per slot: 64-bit sort key
//     (class << 32 | descending-score key), TP byte; empty slots get class C (they sort after every real class).  GT rows are
//     counted per class with integer atomics.
//   effdet_voc_ap: a stable LSD radix sort of all records by (class, score key) -- 4 score passes + 1 class pass (2 above 255
//     classes) -- so ties keep insertion order (image, then slot); per-class segment bounds from the class changes of the sorted
//     keys; then one workgroup per class: forward sweep (exact integer TP / FP cumsums -> fp64 recall, precision), reverse sweep
//     (precision envelope = running max from the right, AP terms (r_k - r_{k-1}) * env_k at the TP positions k), and a fixed
//     LDS tree over the per-thread partial sums.  Every launch geometry follows from (B, max_det, G, C, N) alone.
#include "box_geom.h"
#include "block_scan.h"
#include "radix_sort.h"
#include <float.h>
#include <limits.h>

namespace {

constexpr int VOC_MAX_GT = 2048;              // GT rows per image staged in LDS
constexpr size_t VOC_GT_LDS = 4 * sizeof(double) + 2 * sizeof(int);     // bytes per GT row: 4 fp64 box, label, claim
constexpr int VOC_MAX_CLASSES = 65535;        // class values 0..C fit the two class passes of the sort

// compute_overlap(d, gts of class c) (box_geom.h's box_overlap_f64) and np.argmax
__device__ __forceinline__ int voc_assign(const double a0, const double a1, const double a2, const double a3, int c,
                                          const double* gb, const int* gl, int G, double& best) {
  const double aarea = (a2 - a0) * (a3 - a1);
  int arg = -1;
  best = -1.0;
  for (int j = 0; j < G; ++j) {
    if (gl[j] != c) continue;
    const double iou = box_overlap_f64(a0, a1, a2, a3, aarea, gb + 4 * j);
    if (iou > best) { best = iou; arg = j; }       // first maximum
  }
  return arg;
}

// dets [B][max_det][6] (x1, y1, x2, y2, score, label) fp32, counts [B]; gt_boxes [B][G][4] fp64, gt_labels [B][G] (-1 = pad).
// rec_key / rec_tp point at the B * max_det records of this batch.
__global__ __launch_bounds__(256) void voc_match_kernel(const float* __restrict__ dets, const int* __restrict__ counts,
                                                        const double* __restrict__ gt_boxes, const int* __restrict__ gt_labels,
                                                        int max_det, int G, int C, double thr, unsigned long long* __restrict__ rec_key,
                                                        unsigned char* __restrict__ rec_tp, int* __restrict__ gt_counter) {
  extern __shared__ double voc_lds[];
  double* gb = voc_lds;                       // [G][4]
  int* gl = (int*)(gb + 4 * G);               // [G]
  int* claim = gl + G;                        // [G] first slot claiming the GT
  const int b = blockIdx.x, tid = threadIdx.x;
  for (int j = tid; j < G; j += 256) {
    const double* src = gt_boxes + ((long long)b * G + j) * 4;
    gb[4 * j] = src[0]; gb[4 * j + 1] = src[1]; gb[4 * j + 2] = src[2]; gb[4 * j + 3] = src[3];
    const int lab = gt_labels[(long long)b * G + j];
    gl[j] = lab;
    claim[j] = INT_MAX;
    if (lab >= 0 && lab < C) atomicAdd(&gt_counter[lab], 1);
  }
  __syncthreads();
  int n = counts[b];
  n = n < 0 ? 0 : (n > max_det ? max_det : n);
  const float* d = dets + (long long)b * max_det * 6;
  for (int k = tid; k < n; k += 256) {
    const float* r = d + (long long)k * 6;
    int c;
    if (!label_class(r[5], C, c)) continue;
    double best;
    const int a = voc_assign(r[0], r[1], r[2], r[3], c, gb, gl, G, best);
    if (a >= 0 && best >= thr) atomicMin(&claim[a], k);
  }
  __syncthreads();
  for (int k = tid; k < max_det; k += 256) {
    const long long o = (long long)b * max_det + k;
    unsigned long long key = ((unsigned long long)C << 32) | 0xffffffffull;
    unsigned char tp = 0;
    if (k < n) {
      const float* r = d + (long long)k * 6;
      int c;
      if (label_class(r[5], C, c)) {
        double best;
        const int a = voc_assign(r[0], r[1], r[2], r[3], c, gb, gl, G, best);
        tp = (a >= 0 && best >= thr && claim[a] == k) ? 1 : 0;
        key = ((unsigned long long)c << 32) | rs_score_key(r[4]);
      }
    }
    rec_key[o] = key;
    rec_tp[o] = tp;
  }
}

// one workgroup per class: eval.py:225-241 + _compute_ap on the class's sorted records [seg[2c], seg[2c+1])
__global__ __launch_bounds__(256) void voc_ap_kernel(const unsigned* __restrict__ sval, const unsigned char* __restrict__ rec_tp,
                                                     const int* __restrict__ seg, const int* __restrict__ gt_counter,
                                                     double* __restrict__ recall, double* __restrict__ precision,
                                                     double* __restrict__ ap, double* __restrict__ num_ann) {
  __shared__ int itot[4];
  __shared__ double dtot[4];
  __shared__ double red[256];
  const int c = blockIdx.x, tid = threadIdx.x;
  const int ngt = gt_counter[c];
  if (ngt == 0) {                                    // eval.py:221-223: AP 0 (the class still counts in the mean)
    if (tid == 0) { ap[c] = 0.0; num_ann[c] = 0.0; }
    return;
  }
  const double n = (double)ngt;
  const long long s0 = seg[2 * c], s1 = seg[2 * c + 1];
  int carry = 0;
  for (long long base = s0; base < s1; base += 256) {            // (uniform bounds: every thread reaches every barrier)
    const long long i = base + tid;
    const int v = i < s1 ? (int)rec_tp[sval[i]] : 0;
    int tot;
    const int incl = block_scan_sum(v, itot, &tot);
    if (i < s1) {
      const int tp = carry + incl;
      const int fp = (int)(i - s0 + 1) - tp;
      recall[i] = (double)tp / n;
      precision[i] = (double)tp / fmax((double)tp + (double)fp, DBL_EPSILON);
    }
    carry += tot;
  }
  __syncthreads();                                   // recall / precision of the whole segment visible to the block
  double env = 0.0, acc = 0.0;
  for (long long top = s1; top > s0; top -= 256) {
    const long long i = top - 1 - tid;
    const bool valid = i >= s0;
    double tot;
    const double m = block_scan_max(valid ? precision[i] : 0.0, dtot, &tot);
    if (valid && rec_tp[sval[i]]) {
      const double rprev = i > s0 ? recall[i - 1] : 0.0;
      acc += (recall[i] - rprev) * fmax(m, env);
    }
    env = fmax(env, tot);
  }
  red[tid] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) { ap[c] = red[0]; num_ann[c] = n; }
}

typedef RsBufs<unsigned long long> VocWs;     // the workspace is the sort's buffers for one segment of max(N, 1) keys

size_t voc_carve(VocWs& w, void* base, long long N) {
  Carver c(base);
  rs_carve(w, c, 1, (size_t)(N > 0 ? N : 1));
  return c.off;
}

}  // namespace

extern "C" int effdet_voc_match(const float* dets, const int* counts, const double* gt_boxes, const int* gt_labels, int B, int max_det,
                                int G, int num_classes, double iou_threshold, unsigned long long* rec_key, unsigned char* rec_tp,
                                int* gt_count, effdet_stream_t stream) {
  if (!dets || !counts || !gt_boxes || !gt_labels || !rec_key || !rec_tp || !gt_count || B < 1 || max_det < 1 || G < 1 ||
      num_classes < 1 || num_classes > VOC_MAX_CLASSES)
    return EFFDET_EINVAL;
  if (G > VOC_MAX_GT) return EFFDET_EUNSUPPORTED;
  const size_t lds = (size_t)G * VOC_GT_LDS;
  EFFDET_SET_MAX_LDS(voc_match_kernel, (size_t)VOC_MAX_GT * VOC_GT_LDS);
  hipLaunchKernelGGL(voc_match_kernel, dim3(B), dim3(256), lds, (hipStream_t)stream, dets, counts, gt_boxes, gt_labels, max_det, G,
                     num_classes, iou_threshold, rec_key, rec_tp, gt_count);
  EFFDET_CHECK_LAUNCH();
  return EFFDET_OK;
}

extern "C" long long effdet_voc_ap_workspace_bytes(long long num_records) {
  VocWs w;
  return (long long)voc_carve(w, nullptr, num_records);
}

extern "C" int effdet_voc_ap(const unsigned long long* rec_key, const unsigned char* rec_tp, long long num_records, const int* gt_count,
                             int num_classes, void* workspace, long long workspace_bytes, double* ap, double* num_annotations,
                             double* recall, double* precision, int* seg, effdet_stream_t stream) {
  const long long N = num_records;
  if (!gt_count || !workspace || !ap || !num_annotations || !seg || N < 0 || N > (long long)INT_MAX || num_classes < 1 ||
      num_classes > VOC_MAX_CLASSES || (N > 0 && (!rec_key || !rec_tp || !recall || !precision)))
    return EFFDET_EINVAL;
  VocWs w;
  if ((long long)voc_carve(w, workspace, N) > workspace_bytes) return EFFDET_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int C = num_classes;
  unsigned long long* ki; unsigned* vi;
  if (const int rc = rs_class_sort(rec_key, N, C, w, seg, ki, vi, st)) return rc;
  hipLaunchKernelGGL(voc_ap_kernel, dim3(C), dim3(256), 0, st, (const unsigned*)vi, rec_tp, (const int*)seg, gt_count, recall, precision,
                     ap, num_annotations);
  EFFDET_CHECK_LAUNCH();
  return EFFDET_OK;
}
