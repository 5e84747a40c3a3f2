/* effdet_atss.h -- Adaptive Training Sample Selection (Zhang et al., CVPR 2020) as the matcher of the detection loss of
 * libeffdet_hip.so, in place of the IoU bands.  Entry points added to ABI generation 11; a companion of effdet_loss_opts.h: the forward
 * entry points are effdet_loss_opts_fwd / _fwd_grad with an effdet_atss_t between the options and the stream, the same buffers, layouts
 * and conventions (device pointers, 0 or a negative EFFDET_E* code, kernel launches only on `stream`: no memset, copy or sync; no float
 * atomics; two runs give bitwise-equal results).  Both structs are read from HOST memory at call time.  A library of the same
 * generation built before this header lacks the symbols, so a binding looks them up by name before the first call.  There is no
 * reference implementation to pin against: this header is the specification.
 *
 * Semantics, every quantity fp32, no multiply-add contracted.  Per image, over its valid rows (label != -1):
 *
 * Centres.     cx = 0.5f * (x1 + x2), cy = 0.5f * (y1 + y2) for anchors and annotations alike; dx = cx_a - cx_n, dy = cy_a - cy_n,
 *              d2(a, n) = dx * dx + dy * dy.
 * Candidates.  The anchor table is cut into num_levels levels: level l = anchors [level_start[l], level_start[l + 1]).  For row n and
 *              level l, C(n, l) = the min(topk, level size) anchors of the level that are smallest under the lexicographic key
 *              (d2(a, n), a): a distance tie goes to the LOWER anchor index (the 9 anchors of a pixel share a centre, so ties are the
 *              normal case).  The key involves only fp32 subtract, multiply and add: it is the same bits on any IEEE machine.
 * Threshold.   Visit the candidates of n in level order, then rank order; m = their number; iou(a, n) = effdet_loss_opts.h's
 *              (the expression every matcher of the library evaluates).
 *                mean = (sequential sum of iou) / m
 *                var  = (sequential sum of (iou - mean) * (iou - mean)) / (m - 1), or 0 for m < 2      (the UNBIASED estimate)
 *                thr[n] = mean + sqrtf(var)
 * Positive.    A candidate a of n is positive for n when iou(a, n) >= thr[n] and its centre lies inside the box by mmdet's rule:
 *                min(cx_a - x1, cy_a - y1, x2 - cx_a, y2 - cy_a) > 0.01f
 * Code.        An anchor positive for several rows takes the row with the largest iou(a, n), the FIRST such n on a tie; its code is
 *              that n.  Every other anchor is negative (code -1): ATSS has no ignore band.  In an image without a valid row every
 *              anchor is ignored (code -2) and the image contributes 0, as on the other paths.  num_pos counts the positives.
 *
 * Everything downstream of the assignment -- the class term, the box term (smooth-L1 with beta / reg_weight, or box_kind 1..4 with
 * box_weight), the reductions, the gradients -- is effdet_loss_opts.h's with the effdet_loss_opts_t passed alongside.  pos_iou and
 * neg_iou are not read (they must still be in range); low_quality != 0 is EFFDET_EINVAL. */
#ifndef EFFDET_ATSS_H
#define EFFDET_ATSS_H
#include "effdet_loss_opts.h"
#ifdef __cplusplus
extern "C" {
#endif

#define EFFDET_ATSS_MAX_LEVELS 8
#define EFFDET_ATSS_MAX_TOPK   16

typedef struct effdet_atss {
  int topk;                                            /* default 9; 1 .. EFFDET_ATSS_MAX_TOPK */
  int num_levels;                                      /* 1 .. EFFDET_ATSS_MAX_LEVELS */
  long long level_start[EFFDET_ATSS_MAX_LEVELS + 1];   /* level_start[0] = 0, strictly increasing, level_start[num_levels] = A */
} effdet_atss_t;

/* A null atss, a topk or num_levels outside its range, a level_start that is not as described, a null or out-of-range opts,
 * opts->low_quality != 0 and every condition of the twin entry point are EFFDET_EINVAL; nothing is launched when a code is returned
 * for an argument.
 * Workspace: the layout starts with effdet_loss_workspace_bytes' (assign [B][A] int32, the per-image stat lines, the partials); the
 * matcher's own buffers follow (per valid row the topk-th key of every level, [B][N][EFFDET_ATSS_MAX_LEVELS] 64-bit, and thr [B][N]).
 * So the backward passes need no entry points of their own: effdet_loss_opts_bwd_cls, effdet_loss_opts_bwd_reg and
 * effdet_box_loss_bwd_reg read the workspace a forward call left, with the same opts.  Nothing in the workspace has to be
 * initialised by the caller.
 * effdet_loss_atss_workspace_bytes returns EFFDET_EINVAL (negative) for a null or invalid atss (checked against this A). */
long long effdet_loss_atss_workspace_bytes(int B, long long A, int num_classes, int N, const effdet_atss_t* atss);
int effdet_loss_atss_fwd(const float* cls, const float* reg, const float* anchors, const float* annots, float* losses,
                         void* workspace, long long workspace_bytes, int B, long long A, int num_classes, int N,
                         const effdet_loss_opts_t* opts, const effdet_atss_t* atss, effdet_stream_t stream);
/* one pass over cls: losses and d(logit) for an upstream gradient of ONE, pixel-major [B][A/9][dld] (F32, BF16 or F32_SPLIT) */
int effdet_loss_atss_fwd_grad(const float* cls, const float* reg, const float* anchors, const float* annots, float* losses,
                              void* workspace, long long workspace_bytes, void* dcls_pix, int dld, int dtype, int B,
                              long long A, int num_classes, int N, const effdet_loss_opts_t* opts, const effdet_atss_t* atss,
                              effdet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EFFDET_ATSS_H */
