/* effdet_wbf.h -- Weighted Boxes Fusion (Solovyev et al.) of libeffdet_hip.so: merges the detection lists of several views of one
 * batch (an image and its mirror image, several detectors) on the device.  Entry points added to ABI generation 11 after
 * effdet_hip.h's own set; its conventions (device pointers, 0 or a negative EFFDET_E* code, work enqueued on `stream`) hold here.  A
 * library of the same generation built before this header lacks the two symbols, so a binding looks them up by name first.
 *
 * A view is what the NMS stage emits: score [B][A_v] fp32, label [B][A_v] int64 (class indices: they must fit an int), boxes
 * [B][A_v][4] fp32 (x1, y1, x2, y2), count [B] int32, rows score-descending; of each view only the first min(count[b], top_n, A_v)
 * rows of image b take part.  Every view has a weight w_v > 0 and a transform: an optional horizontal flip about width W_v, then a
 * multiplier m_v > 0.  Semantics, all in fp32, in this order of operations, nothing contracted into an FMA:
 *
 *  1. transform   flip: x1' = W_v - x2, x2' = W_v - x1; then every coordinate is multiplied by m_v; conf = score * w_v.  A row takes
 *                 part when score >= skip_thr, conf is positive and finite, and the transformed box's area (x2 - x1) * (y2 - y1) is
 *                 positive and finite (so NaN scores and degenerate boxes drop out).
 *  2. order       the image's surviving candidates by conf descending, then view ascending, then row ascending.
 *  3. clustering  candidates are taken in that order.  Among the existing clusters with the candidate's label the one whose CURRENT
 *                 fused box has the largest IoU with the candidate is taken (ties: the lowest cluster index; a NaN IoU never wins);
 *                 IoU = inter / (area_a + area_b - inter), 0 when iw <= 0 || ih <= 0 -- effdet_nms's rule.  If that IoU is
 *                 > iou_thr the candidate joins, else it founds cluster number (clusters so far).  Clusters of different labels never
 *                 interact, so this equals the published per-label loop.
 *  4. state       S[k] += conf * coord[k] (k = 0..3; multiply, then add), sc += conf, cmax = max(cmax, conf), cnt += 1.  The fused
 *                 box of a cluster with cnt == 1 is its member's transformed box AS IT IS (the published code divides (conf * x) /
 *                 conf; here a single view passes through unchanged); with cnt >= 2 it is S[k] / sc, recomputed after every join.
 *  5. score       EFFDET_WBF_AVG: ((sc / float(cnt)) * float(min(cnt, V))) / wsum, wsum = the fp32 sum of the w_v in view order;
 *                 EFFDET_WBF_MAX: cmax / wmax, wmax = the largest w_v.
 *  6. output      clusters by score descending, then cluster index ascending: out_score [B][N], out_label [B][N] int64, out_boxes
 *                 [B][N][4], out_count [B] with N = V * top_n; rows past the count are zero.  effdet_finalize_dets takes them as
 *                 they are.
 *
 * One 1024-thread workgroup per image holds the candidates in LDS, which is where the limit on V * top_n comes from. */
#ifndef EFFDET_WBF_H
#define EFFDET_WBF_H
#include "effdet_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

enum { EFFDET_WBF_AVG = 0, EFFDET_WBF_MAX = 1 };   /* conf_type */
#define EFFDET_WBF_MAX_VIEWS 8
#define EFFDET_WBF_MAX_IN 4096                     /* V * top_n: the candidates of an image live in one workgroup's LDS */

typedef struct {
  const float* score[EFFDET_WBF_MAX_VIEWS];        /* per view: [B][A_v] */
  const long long* label[EFFDET_WBF_MAX_VIEWS];    /*           [B][A_v] */
  const float* boxes[EFFDET_WBF_MAX_VIEWS];        /*           [B][A_v][4], 16-byte aligned */
  const int* count[EFFDET_WBF_MAX_VIEWS];          /*           [B] */
  long long A[EFFDET_WBF_MAX_VIEWS];               /* rows per image of the view's arrays */
  float weight[EFFDET_WBF_MAX_VIEWS];              /* w_v > 0 */
  float width[EFFDET_WBF_MAX_VIEWS];               /* W_v, read with flip only */
  float mul[EFFDET_WBF_MAX_VIEWS];                 /* m_v > 0 */
  int flip[EFFDET_WBF_MAX_VIEWS];                  /* 0 | 1 */
  int V, B, top_n, conf_type;
  float iou_thr, skip_thr;
  float* out_score;                                /* [B][V * top_n] */
  long long* out_label;                            /* [B][V * top_n] */
  float* out_boxes;                                /* [B][V * top_n][4] */
  int* out_count;                                  /* [B] */
} effdet_wbf_t;

/* bytes of workspace for B images of V views; 0 today (candidates live in LDS, cluster state in registers): workspace may then be NULL */
long long effdet_wbf_workspace_bytes(int B, int V, int top_n);
/* p in HOST memory.  1 <= V <= 8, top_n >= 1, V * top_n <= 4096, conf_type 0..1, 0 <= iou_thr <= 1, skip_thr not NaN, weights and
 * multipliers positive and finite, a flip's width finite: anything else is EFFDET_EUNSUPPORTED; a NULL or misaligned pointer, B < 1,
 * A_v < 1 or a workspace smaller than effdet_wbf_workspace_bytes is EFFDET_EINVAL.  Nothing is launched in either case. */
int effdet_wbf(const effdet_wbf_t* p, void* workspace, long long workspace_bytes, effdet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EFFDET_WBF_H */
