/* effdet_loss_opts.h -- the options of the detection loss of libeffdet_hip.so: focal alpha / gamma, label smoothing, the smooth-L1
 * knee and weight, the matcher's IoU bands and low-quality matches.  Entry points added to ABI generation 11 after effdet_hip.h's own
 * set; they are the twins of effdet_focal_loss_fwd / _fwd_grad / _bwd / _bwd_pix / _bwd_reg with an effdet_loss_opts_t in front of
 * the stream: the same buffers, layouts and conventions (device pointers, 0 or a negative EFFDET_E* code, kernel launches only on
 * `stream`: no memset, copy or sync).  The struct is read from HOST memory at call time; its values become launch arguments.  A
 * library of the same generation built before this header lacks the symbols, so a binding looks them up by name before the first call.
 *
 * Semantics, every quantity fp32.
 *
 * Matcher.  iou(a, n) is the expression of the reference's calc_iou as effdet_focal_loss_fwd evaluates it
 *   (iw ih / max(area_a + area_n - iw ih, 1e-8), iw and ih clamped at 0).  Per anchor a of an image, over its valid rows (label != -1):
 *     best = max_n iou(a, n), barg = the FIRST n that reaches it
 *     best <  neg_iou            -> negative (code -1)
 *     best >= pos_iou            -> positive (code barg)
 *     otherwise                  -> ignored  (code -2);   an image without a valid row: every anchor ignored
 *   With low_quality, in addition: gtmax[n] = max_a iou(a, n) per valid row; an anchor with iou(a, n) == gtmax[n] and gtmax[n] > 0
 *   for ANY valid n becomes positive with code = its own barg (torchvision's Matcher(allow_low_quality_matches=True); the anchor
 *   takes its own arg-max row, which may be another row than the one it is the best anchor of).  gtmax[n] > 0 is a stated
 *   deviation: without it a box that overlaps no anchor would promote every anchor.  num_pos counts the promoted anchors.
 *
 * Class term, per element with hard target h (1 on the assigned row's label of a positive anchor, else 0), p clamped to
 * [1e-4, 1 - 1e-4] as in effdet_focal_loss_fwd:
 *     t   = h (1 - eps) + eps / 2                                   (eps = label_smoothing)
 *     u   = 1 - p_t, p_t = h p + (1 - h)(1 - p):  u = 1 - p for h = 1, u = p for h = 0
 *     w   = (h alpha + (1 - h)(1 - alpha)) * exp2(gamma * log2(u))
 *     l   = -w (t log p + (1 - t) log(1 - p))
 *   losses[0] = mean over the B images of (sum over the image's non-ignored anchors and all classes of l) / max(num_pos, 1); an image
 *   without a valid row contributes 0.  d(logit) = d l / d p * p (1 - p) with p the unclamped probability; the clamp passes the
 *   gradient on the closed range.  Elements the loss does not reach (ignored anchors, images without a valid row) get p - p: +0.0,
 *   or NaN for a non-finite p, as in effdet_focal_loss_bwd.  At eps = 0, gamma = 2, alpha = 0.25 l is the reference's value.
 *
 * Box term, box_kind 0 (smooth-L1 on the encoded deltas, targets as in effdet_focal_loss_fwd), d = |target - r| per delta:
 *     d <= beta ? 0.5 d d / beta : d - 0.5 beta
 *   losses[1] = reg_weight * mean over the B images of (sum over positives and the 4 deltas) / (4 num_pos); an image without a valid
 *   row or a positive contributes 0.  d(reg) = gscale[1] * reg_weight / (B * 4 num_pos) * (d <= beta ? (r - target) / beta : sign).
 * Box term, box_kind EFFDET_BOX_LOSS_IOU .. _CIOU: include/effdet_box_loss.h's loss over THIS assignment, times box_weight;
 *   reg_weight does not apply.
 * d(reg) is exact +0.0 for every anchor that is not positive and in every pad channel. */
#ifndef EFFDET_LOSS_OPTS_H
#define EFFDET_LOSS_OPTS_H
#include "effdet_box_loss.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct effdet_loss_opts {
  float alpha;            /* default 0.25        0 < alpha < 1 */
  float gamma;            /* default 2           0 <= gamma <= 8 */
  float label_smoothing;  /* default 0           0 <= eps < 1 */
  float beta;             /* default 1.0f / 9.0f finite, > 0 */
  float reg_weight;       /* default 1           finite, >= 0 */
  float pos_iou;          /* default 0.5         0 <= neg_iou <= pos_iou <= 1 */
  float neg_iou;          /* default 0.4 */
  int low_quality;        /* default 0           0 / 1 */
  int box_kind;           /* default 0           0 (smooth-L1) or EFFDET_BOX_LOSS_IOU .. EFFDET_BOX_LOSS_CIOU */
  float box_weight;       /* default 1           finite, >= 0; box_kind 1..4 only */
} effdet_loss_opts_t;

/* A null opts or any value outside the ranges above (a NaN included) is EFFDET_EINVAL, as is every condition of the twin; nothing is
 * launched when a code is returned for an argument.
 * Workspace: the layout starts with effdet_loss_workspace_bytes' (assign [B][A] int32, the per-image stat lines, the partials), so
 * effdet_box_loss_bwd_reg and every reader of the assignment work on it; gtmax [B][N] and the per-anchor best / barg follow.  The
 * backward entry points read the workspace a forward call with the same options left. */
long long effdet_loss_opts_workspace_bytes(int B, long long A, int num_classes, int N);
int effdet_loss_opts_fwd(const float* cls, const float* reg, const float* anchors, const float* annots, float* losses,
                         void* workspace, long long workspace_bytes, int B, long long A, int num_classes, int N,
                         const effdet_loss_opts_t* opts, effdet_stream_t stream);
/* one pass over cls: losses and d(logit) for an upstream gradient of ONE, pixel-major [B][A/9][dld] (F32, BF16 or F32_SPLIT) */
int effdet_loss_opts_fwd_grad(const float* cls, const float* reg, const float* anchors, const float* annots, float* losses,
                              void* workspace, long long workspace_bytes, void* dcls_pix, int dld, int dtype, int B,
                              long long A, int num_classes, int N, const effdet_loss_opts_t* opts, effdet_stream_t stream);
/* d(logit) times gscale[0]: dld == 0 -> [B][A][num_classes], dld > 0 -> pixel-major [B][A/9][dld] (F32 or BF16) */
int effdet_loss_opts_bwd_cls(const float* cls, const float* annots, const float* gscale, const void* workspace, void* dcls,
                             int dld, int dtype, int B, long long A, int num_classes, int N, const effdet_loss_opts_t* opts,
                             effdet_stream_t stream);
/* d(reg) times gscale[1] in the three layouts of effdet_focal_loss_bwd_reg */
int effdet_loss_opts_bwd_reg(const float* reg, const float* anchors, const float* annots, const float* gscale,
                             const void* workspace, void* dreg, int reg_ld, int dtype, int B, long long A, int N,
                             const effdet_loss_opts_t* opts, effdet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EFFDET_LOSS_OPTS_H */
