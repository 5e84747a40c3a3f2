/* effdet_soft_nms.h -- the rescoring NMS of libeffdet_hip.so (Soft-NMS and per-class suppression): the entry points added to ABI
 * generation 11 after effdet_hip.h's own set.  effdet_hip.h documents the semantics next to effdet_nms, whose keys, sort and IoU they
 * share; its conventions (device pointers, 0 or a negative EFFDET_E* code, work enqueued on `stream`) hold here.  A library of the
 * same generation built before this header lacks the two symbols, so a binding looks them up by name before the first call. */
#ifndef EFFDET_SOFT_NMS_H
#define EFFDET_SOFT_NMS_H
#include "effdet_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

enum { EFFDET_NMS_HARD = 0, EFFDET_NMS_LINEAR = 1, EFFDET_NMS_GAUSSIAN = 2 };   /* method */
#define EFFDET_SOFT_NMS_MAX_TOP_N 4096                                          /* one workgroup's LDS holds the top-N of an image */

/* bytes of workspace for B images of A anchors: the sort's buffers (~20 B per anchor; the top-N live in LDS) */
long long effdet_soft_nms_workspace_bytes(int B, long long A, int pre_nms_top_n);
/* label [B][A] with class_aware, NULL without (else EFFDET_EINVAL); method 0..2, 1 <= pre_nms_top_n <= 4096,
 * 1 <= max_det <= pre_nms_top_n, sigma > 0: anything else is EFFDET_EUNSUPPORTED and nothing is launched.
 * out_idx [B][A], out_score [B][A], out_count [B]; effdet_gather_dets takes out_idx / out_count as they are. */
int effdet_soft_nms(const float* boxes, const float* score, const int* label, float threshold, float iou_threshold,
                    int method, float sigma, int class_aware, int pre_nms_top_n, int max_det, int* out_idx,
                    float* out_score, int* out_count, void* workspace, long long workspace_bytes, int B, long long A,
                    effdet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EFFDET_SOFT_NMS_H */
