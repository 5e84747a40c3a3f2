/* effdet_tal.h -- task-aligned anchor assignment (TOOD, Feng et al., ICCV 2021; the assigner of PP-YOLOE, YOLOv8 and RTMDet's family) as
 * the matcher of the detection loss of libeffdet_hip.so, in place of the IoU bands or ATSS.  Entry points added to ABI generation 11; a
 * companion of effdet_atss.h and effdet_quality_loss.h: the forward entry points are effdet_loss_quality_fwd / _fwd_grad with an
 * effdet_tal_t in the place of the effdet_atss_t, the same buffers, layouts and conventions (device pointers, 0 or a negative EFFDET_E*
 * code, kernel launches only on `stream`: no memset, copy or sync; no float atomics; two runs give bitwise-equal results).  The structs
 * are read from HOST memory at call time.  A library of the same generation built before this header lacks the symbols, so a binding
 * looks them up by name before the first call.  There is no reference implementation to pin against: this header is the specification.
 *
 * Semantics, every quantity fp32, no multiply-add contracted.  Per image b, over its valid rows n (label != -1); everything below is a
 * CONSTANT of the gradient.
 *
 * Pair.        For anchor a and row n:
 *                u(a, n) = the IoU between the DECODED prediction of a and row n, clamped to [0, 1]: effdet_quality_loss.h's q expression
 *                          (effdet_box_loss.h's `decode` and `overlap`, clampnan, NaN for a non-finite regression row) with row n in the
 *                          place of the assigned row
 *                s(a, n) = cls[b][a][label_n], the class pass's unclamped probability
 *                m(a, n) = pow(s, alpha) * pow(u, beta), pow(x, e) = exp2(e * log2(x)) as in the options' focal term, 0 for x == 0
 *              A row whose label is outside [0, num_classes) has no candidates.  ONE device function evaluates the pair for every kernel.
 * Candidates.  The anchors of row n whose centre lies inside the row's box by effdet_atss.h's rule
 *                min(cx_a - x1, cy_a - y1, x2 - cx_a, y2 - cy_a) > 0.01f
 *              and whose m(a, n) > 0 (a NaN m is no candidate).  The centre test comes FIRST and the top-k is taken among the anchors
 *              that pass it (PaddleDetection, Ultralytics); mmdet takes the top-k over all anchors and masks afterwards.
 * Selection.   The min(topk, number of candidates) candidates with the smallest 64-bit key (~bits(m) << 32) | a: the largest metric
 *              first, the LOWER anchor index on equal bits (m > 0, so its bit pattern orders as an unsigned integer).
 * Code.        An anchor selected by several rows takes the row with the largest u(a, n), the FIRST such n on a tie; its code is that n.
 *              Every other anchor is negative (code -1): there is no ignore band.  In an image without a valid row every anchor is
 *              ignored (code -2) and the image contributes 0, as on the other paths.  num_pos counts the positives.
 * Target.      Only with a quality loss and aligned_target != 0.  Per row n, over the anchors FINALLY assigned to it:
 *                mmax = max m(a, n), umax = max u(a, n)
 *                q(b, a) = (m(a, n) * umax) / (mmax + 1e-9f), evaluated in that order,
 *              and q = 0 at every other anchor.  With aligned_target == 0 q is effdet_quality_loss.h's, and without a quality loss
 *              there is no q.
 *
 * Everything downstream of the assignment -- the class term (the focal term of opts, or the quality loss on q), the box term, the
 * reductions, d(logit) and d(reg) in their three layouts, the exact zeros away from the positives -- is effdet_loss_opts.h's /
 * effdet_box_loss.h's / effdet_quality_loss.h's with the structs passed alongside.  pos_iou and neg_iou are not read (they must still be
 * in range); low_quality != 0 is EFFDET_EINVAL. */
#ifndef EFFDET_TAL_H
#define EFFDET_TAL_H
#include "effdet_quality_loss.h"
#ifdef __cplusplus
extern "C" {
#endif

#define EFFDET_TAL_MAX_TOPK 16

typedef struct effdet_tal {
  int   topk;            /* default 13   1 .. EFFDET_TAL_MAX_TOPK */
  float alpha;           /* default 1    0 <= alpha <= 4    exponent of the class score */
  float beta;            /* default 6    0 <= beta  <= 16   exponent of the IoU */
  int   aligned_target;  /* default 1    0 / 1: with a quality loss, q = the normalised metric instead of the IoU */
} effdet_tal_t;

/* A null tal, a topk outside its range, an alpha or beta outside its range (a NaN included), an aligned_target other than 0 / 1, a null
 * or out-of-range opts, opts->low_quality != 0, a non-null quality that is out of range and every condition of the twin entry point are
 * EFFDET_EINVAL; nothing is launched when a code is returned for an argument.
 * Workspace, ONE layout with or without a quality loss: effdet_loss_workspace_bytes' prefix (assign [B][A] int32, the per-image stat
 * lines, the partials); q [B][A] fp32 where effdet_loss_quality_bwd_cls looks for it, i.e. the layout of
 * effdet_loss_quality_workspace_bytes(B, A, num_classes, N, NULL), whose size is the offset K of the matcher's own buffers, each rounded
 * up to 256 bytes:
 *   K                                    keys [B][N][EFFDET_TAL_MAX_TOPK] 64-bit: the row's winners in rank order, padded with the no-key
 *                                        value ~0 (a pad row: all padding)
 *   K + round_up(128 B N, 256)           (mmax, umax) [B][N][2] fp32 (0, 0 where no anchor is finally assigned to the row, and for every
 *                                        row where no aligned target is formed)
 *   ...  + round_up(8 B N, 256)          the conflict slots [B][A] 64-bit: (bits(u) << 32) | (0xFFFFFFFF - n) of the row an anchor takes,
 *                                        0 where no row selected it
 * So effdet_loss_opts_bwd_cls, effdet_loss_opts_bwd_reg, effdet_box_loss_bwd_reg and effdet_loss_quality_bwd_cls read the workspace a
 * forward call left, with the same opts / quality: there are no backward entry points here.  Nothing in the workspace has to be
 * initialised by the caller.
 * effdet_loss_tal_workspace_bytes returns EFFDET_EINVAL (negative) for a null or invalid tal. */
long long effdet_loss_tal_workspace_bytes(int B, long long A, int num_classes, int N, const effdet_tal_t* tal);
/* quality == NULL: the focal term of opts */
int effdet_loss_tal_fwd(const float* cls, const float* reg, const float* anchors, const float* annots, float* losses,
                        void* workspace, long long workspace_bytes, int B, long long A, int num_classes, int N,
                        const effdet_loss_opts_t* opts, const effdet_tal_t* tal, const effdet_quality_loss_t* quality,
                        effdet_stream_t stream);
/* one pass over cls: losses and d(logit) for an upstream gradient of ONE, pixel-major [B][A/9][dld] (F32, BF16 or F32_SPLIT) */
int effdet_loss_tal_fwd_grad(const float* cls, const float* reg, const float* anchors, const float* annots, float* losses,
                             void* workspace, long long workspace_bytes, void* dcls_pix, int dld, int dtype, int B,
                             long long A, int num_classes, int N, const effdet_loss_opts_t* opts, const effdet_tal_t* tal,
                             const effdet_quality_loss_t* quality, effdet_stream_t stream);
/* inspection: m and u of every pair through the same device function; out [2][B][N][A] fp32 (m, then u), 0 where a is not inside n,
 * where n is a pad row and where its label is outside [0, num_classes) */
int effdet_loss_tal_metrics(const float* cls, const float* reg, const float* anchors, const float* annots, float* out, int B,
                            long long A, int num_classes, int N, const effdet_tal_t* tal, effdet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EFFDET_TAL_H */
