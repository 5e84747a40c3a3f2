/* effdet_quality_loss.h -- IoU-aware class losses of the detection loss of libeffdet_hip.so: the quality focal loss of GFL (Li et al.,
 * NeurIPS 2020) and the varifocal loss of VarifocalNet (Zhang et al., CVPR 2021) in place of the hard-target focal term.  Entry points
 * added to ABI generation 11; a companion of effdet_loss_opts.h and effdet_atss.h: the forward entry points are effdet_loss_opts_fwd /
 * _fwd_grad with an effdet_atss_t (or NULL: the IoU bands of the options) and an effdet_quality_loss_t between the options and the
 * stream, the same buffers, layouts and conventions (device pointers, 0 or a negative EFFDET_E* code, kernel launches only on `stream`:
 * no memset, copy or sync; no float atomics; two runs give bitwise-equal results).  The structs are read from HOST memory at call time.
 * A library of the same generation built before this header lacks the symbols, so a binding looks them up by name before the first
 * call.  There is no reference implementation to pin against: this header is the specification.
 *
 * Semantics, every quantity fp32.
 *
 * Quality.  For a positive anchor a of image b (assignment code n >= 0) with regression row r and annotation row g taken raw:
 *     q(b, a) = clampnan(iou, 0, 1), iou = effdet_box_loss.h's: its `decode` (the EFFDET_BOX_LOSS_DW_MAX cap included) and its
 *               `overlap` line, I / (U + 1e-7) -- the device function the box-loss kernels evaluate.  clampnan keeps a NaN.
 *   q = 0 for every anchor that is not positive.  q is a CONSTANT of the gradient: nothing flows into d(reg) through it.
 *   A non-finite r at a positive anchor makes q NaN (the sum of r_k - r_k over the row is added to it), and losses[0] with it; that
 *   anchor's class-gradient row is then unspecified.
 *
 * Class term, per element of a non-ignored anchor of an image with a valid row; p clamped to [1e-4, 1 - 1e-4] as in
 * effdet_focal_loss_fwd; soft target t = q on the assigned row's label of a positive anchor, t = 0 elsewhere;
 * BCE(p, t) = -(t log p + (1 - t) log(1 - p)):
 *   EFFDET_QUALITY_QFL   l = |t - p|^beta BCE(p, t), no alpha.  The power is exp2(beta * log2(u)), u = |t - p|, no multiply-add
 *                        contracted (as the options' focal term); at u == 0 the power and its derivative are 0.
 *   EFFDET_QUALITY_VFL   t > 0 (or NaN):  l = t BCE(p, t)
 *                        otherwise -- a positive anchor whose q is exactly 0 included --:  l = alpha p^gamma BCE(p, 0), the power as
 *                        exp2(gamma * log2(p))
 *   losses[0] = mean over the B images of (sum over the image's non-ignored anchors and all classes of l) / max(num_pos, 1); an image
 *   without a valid row contributes 0.  This is the normaliser of every class term of the library; mmdet's GFL / VFNet heads divide
 *   the batch's sum by a batch-wide normaliser (the sum of the positives' qualities, resp. their number).
 *   d(logit) = d l / d p * p (1 - p) with p the unclamped probability, t held constant; the clamp passes the gradient on the closed
 *   range.  Elements the loss does not reach (ignored anchors, images without a valid row) get p - p: +0.0, or NaN for a non-finite p.
 *
 * Everything else -- the assignment (bands / low-quality matches of opts, or ATSS with atss), num_pos, losses[1], d(reg) -- is
 * effdet_loss_opts_fwd's resp. effdet_loss_atss_fwd's with the same opts, BIT FOR BIT: the same kernels run.  The alpha, gamma and
 * label_smoothing of opts are not read (they must still be in range): the quality loss replaces the term they parameterise. */
#ifndef EFFDET_QUALITY_LOSS_H
#define EFFDET_QUALITY_LOSS_H
#include "effdet_atss.h"
#ifdef __cplusplus
extern "C" {
#endif

enum { EFFDET_QUALITY_QFL = 1, EFFDET_QUALITY_VFL = 2 };

typedef struct effdet_quality_loss {
  int kind;     /* EFFDET_QUALITY_QFL or EFFDET_QUALITY_VFL */
  float beta;   /* default 2      1 <= beta <= 8         QFL's exponent (must be in range for either kind) */
  float alpha;  /* default 0.75   0 < alpha <= 1         VFL's weight of the negatives (likewise) */
  float gamma;  /* default 2      0 <= gamma <= 8        VFL's exponent of the negatives (likewise) */
} effdet_quality_loss_t;

/* A null quality, a kind outside the two or any value outside the ranges above (a NaN included) is EFFDET_EINVAL, as is every
 * condition of effdet_loss_opts_fwd / _fwd_grad / _bwd_cls (atss == NULL) resp. effdet_loss_atss_fwd / _fwd_grad; nothing is
 * launched when a code is returned for an argument.
 * Workspace: the layout starts with effdet_loss_workspace_bytes' (assign [B][A] int32, the per-image stat lines, the partials), so
 * effdet_loss_opts_bwd_reg / effdet_box_loss_bwd_reg and every reader of the assignment work on it: there is no d(reg) entry point
 * here.  The matcher's buffers follow, and q [B][A] fp32 follows them as the LAST buffer, at the same offset for either matcher (past
 * the longer of the two matchers' layouts): it starts workspace_bytes - round_up(4 B A, 256) bytes into the workspace.  The forward
 * calls write q with one more launch than their twins (one thread per anchor, after the assign pass); effdet_loss_quality_bwd_cls
 * reads the workspace a forward call with the same arguments left.
 * effdet_loss_quality_workspace_bytes returns EFFDET_EINVAL (negative) for an invalid atss (checked against this A); NULL: the bands. */
long long effdet_loss_quality_workspace_bytes(int B, long long A, int num_classes, int N, const effdet_atss_t* atss);
int effdet_loss_quality_fwd(const float* cls, const float* reg, const float* anchors, const float* annots, float* losses,
                            void* workspace, long long workspace_bytes, int B, long long A, int num_classes, int N,
                            const effdet_loss_opts_t* opts, const effdet_atss_t* atss, const effdet_quality_loss_t* quality,
                            effdet_stream_t stream);
/* one pass over cls: losses and d(logit) for an upstream gradient of ONE, pixel-major [B][A/9][dld] (F32, BF16 or F32_SPLIT) */
int effdet_loss_quality_fwd_grad(const float* cls, const float* reg, const float* anchors, const float* annots, float* losses,
                                 void* workspace, long long workspace_bytes, void* dcls_pix, int dld, int dtype, int B,
                                 long long A, int num_classes, int N, const effdet_loss_opts_t* opts, const effdet_atss_t* atss,
                                 const effdet_quality_loss_t* quality, effdet_stream_t stream);
/* d(logit) times gscale[0]: dld == 0 -> [B][A][num_classes], dld > 0 -> pixel-major [B][A/9][dld] (F32 or BF16) */
int effdet_loss_quality_bwd_cls(const float* cls, const float* annots, const float* gscale, const void* workspace, void* dcls,
                                int dld, int dtype, int B, long long A, int num_classes, int N, const effdet_loss_opts_t* opts,
                                const effdet_quality_loss_t* quality, effdet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EFFDET_QUALITY_LOSS_H */
