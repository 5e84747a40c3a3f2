/* effdet_op_point.h -- operating-point metrics of libeffdet_hip.so: precision / recall / F1 against a grid of confidence thresholds
 * (effdet_op_curves) and a confusion matrix at one threshold (effdet_confusion_match), over the same rows and records the VOC metric
 * works on (effdet_finalize_dets, effdet_voc_match).  They answer what the mean AP cannot: which score threshold to deploy with, what
 * each class's precision and recall are there, and which classes are mistaken for each other or for background.  Entry points added to
 * ABI generation 11 after effdet_hip.h's own set; its conventions (device pointers, 0 or a negative EFFDET_E* code, work enqueued on
 * `stream`) hold here.  A library of the same generation built before this header lacks the three symbols, so a binding looks them up
 * by name first.
 *
 * The reference has no such tool; the semantics are this project's, stated here and restated in tests/op_point_restated.py.
 *
 * ---- effdet_op_curves: confidence curves
 * Input.  The num_records records of effdet_voc_match (rec_key, rec_tp) and its gt_count[C], C = num_classes; thresholds[M] fp32 on
 *   the device, M = num_thresholds.  The call does not look at the thresholds' values: any order, any value.  (The Python binding
 *   wants them finite and strictly ascending and turns -0.0 into +0.0.)
 * Sort.  The records are sorted exactly as effdet_voc_ap sorts them: csrc/radix_sort.h's rs_sort, stable, by (class, descending-score
 *   key), 4 score passes + 1 class pass (2 above 255 classes), and the same segment bounds of the sorted keys.  Tied scores keep record
 *   order.  Empty slots (class C) sort behind every class and are never counted.
 * Counts, int32 [C][M].  With key(x) = the descending-score key of rec_key's low word (rs_score_key: ascending keys = descending
 *   scores, +0 before -0):
 *       npred[c][j] = the number of class c's records whose key is BELOW key(thresholds[j]);
 *       tp[c][j]    = the number of TP bytes among them (an exact integer cumsum over that prefix of the class's sorted segment).
 *   For every score that is not a NaN, and a threshold t that is not -0.0, "key below key(t)" is `score > t`, the strict rule of
 *   effdet_finalize_dets' score_threshold.  (For t = -0.0 a score of +0.0 counts although +0.0 > -0.0 is false.)  A NaN score with the
 *   sign bit clear has a key below every number's and counts at every threshold; one with the sign bit set has a key above every
 *   number's and counts at none.  effdet_finalize_dets emits neither.
 * Why this is the count at threshold t.  effdet_voc_match decides whether a detection is a TP from the rows of its image in front of
 *   it alone (the first of its class to qualify for its assigned GT).  PRECONDITION: the rows of an image are score-descending, as
 *   effdet_finalize_dets writes them.  Then the detections of an image with score > t are a prefix of its rows, a re-evaluation over
 *   only those detections gives each of them the TP byte it has here, and tp[c][j] and npred[c][j] - tp[c][j] are the TP and FP that a
 *   full evaluation over the detections with score > thresholds[j] would count.  With rows in another order the outputs are still the
 *   counts defined above, but no longer that.
 * Curves, fp64 [C][M], every operation rounded once (nothing contracted), with n = gt_count[c]:
 *       precision = (double)tp / (double)npred             1.0 when npred == 0
 *       recall    = (double)tp / (double)n                 0.0 when n == 0
 *       f1        = (2.0 * p * r) / (p + r)                evaluated left to right; 0.0 when p + r == 0
 * mean_curves [3][M] fp64: the mean of precision (row 0), recall (row 1) and f1 (row 2) over the classes with n > 0 -- a sequential sum
 *   in ascending class order starting from 0.0, divided by (double)K, K = the number of such classes; zeros when K = 0.
 * best [C + 1][4] fp64: row c < C is (j*, precision[c][j*], recall[c][j*], f1[c][j*]) with j* the FIRST j that maximises f1[c][.];
 *   (-1, 0, 0, 0) for a class with n == 0.  Row C is (j*, mean precision, mean recall, mean f1 at j*) with j* the first j that
 *   maximises the mean f1; (-1, 0, 0, 0) when K = 0.
 * Every element of tp, npred, precision, recall, f1, mean_curves and best is written on every call, num_records == 0 included.  Launch
 *   geometry follows from (num_records, C, M) alone.  No floating-point atomics: two calls on the same input give the same bits.
 *
 * ---- effdet_confusion_match: confusion matrix
 * Input.  effdet_voc_match's: dets [B][max_det][6] fp32 (x1, y1, x2, y2, score, label) + counts [B], gt_boxes [B][G][4] fp64,
 *   gt_labels [B][G] int32, 1 <= G <= 2048.  max_det is unbounded.
 * Output.  The call ADDS to matrix [(C + 1)][(C + 1)] int64 (integer atomics; the caller zeroes it once): row = predicted class, column =
 *   true class, index C = background.  So column c sums to the objects of class c, row r to the predictions of class r.
 * Rule (Ultralytics' ConfusionMatrix.process_batch, with its ties decided), per image b:
 *   predictions  its first min(max(counts[b], 0), max_det) rows whose label is an integer in [0, C) and whose score > conf_threshold
 *                (fp32 comparison, strict; a NaN score is no prediction);
 *   objects      its GT rows whose label is in [0, C);
 *   IoU          effdet_voc_match's fp64 expression in its operation order, between any prediction and any object whatever their
 *                labels:  iw = max(min(a2, b2) - max(a0, b0), 0), ih likewise, ua = max(area_a + area_b - iw * ih, DBL_EPSILON),
 *                iou = iw * ih / ua;
 *   candidates   the pairs with iou > iou_threshold (strict; a NaN is none);
 *   step 1       every prediction keeps only its best candidate object: the largest IoU, the FIRST such object in GT row order;
 *   step 2       every object keeps, among the predictions that kept it, the one with the largest IoU, the LOWEST row among equals;
 *                a prediction whose object went to another prediction gets no second choice;
 *   counts       a surviving pair adds 1 at [label of the prediction][label of the object]; every other object adds 1 at
 *                [C][its label] (missed); every other prediction adds 1 at [its label][C] (background false positive).
 * One workgroup per image holds the GT rows (32 bytes of box, 4 of label) and, per object, the winner's IoU bits (8) and row (4) in
 * LDS: 48 bytes * 2048 = 96 KiB, where the limit on G comes from.  The winner of an object is decided by integer LDS atomics (a
 * non-negative fp64 orders like its bit pattern: atomic max; then atomic min of the row among the predictions with that IoU), so the
 * result does not depend on the order the predictions are visited in. */
#ifndef EFFDET_OP_POINT_H
#define EFFDET_OP_POINT_H
#include "effdet_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define EFFDET_OP_MAX_THRESHOLDS 4096                  /* M */

/* bytes of workspace for num_records records (the sort's buffers, the segment bounds, the TP cumsum); 0 for num_records outside
 * [0, 2^31) */
long long effdet_op_curves_workspace_bytes(long long num_records);
/* EFFDET_EUNSUPPORTED: num_thresholds outside 1..4096 or num_classes above 65535 (effdet_voc_ap's range).  EFFDET_EINVAL: a NULL
 * gt_count, thresholds, workspace or output, num_records outside [0, 2^31), num_classes < 1, rec_key or rec_tp NULL with
 * num_records > 0, or a workspace smaller than effdet_op_curves_workspace_bytes(num_records).  Nothing is enqueued in either case. */
int effdet_op_curves(const unsigned long long* rec_key, const unsigned char* rec_tp, long long num_records, const int* gt_count,
                     int num_classes, const float* thresholds, int num_thresholds, void* workspace, long long workspace_bytes,
                     int* tp, int* npred, double* precision, double* recall, double* f1, double* mean_curves, double* best,
                     effdet_stream_t stream);

/* EFFDET_EUNSUPPORTED: G > 2048.  EFFDET_EINVAL: a NULL pointer, B, max_det, G or num_classes < 1, num_classes > 65535, or a NaN
 * threshold.  Nothing is enqueued in either case. */
int effdet_confusion_match(const float* dets, const int* counts, const double* gt_boxes, const int* gt_labels, int B, int max_det,
                           int G, int num_classes, float conf_threshold, double iou_threshold, long long* matrix,
                           effdet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EFFDET_OP_POINT_H */
