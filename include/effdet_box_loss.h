/* effdet_box_loss.h -- the IoU-family box regression losses of libeffdet_hip.so (IoU / GIoU / DIoU / CIoU in place of the reference's
 * smooth-L1 on encoded deltas): entry points added to ABI generation 11 after effdet_hip.h's own set.  They are the twins of
 * effdet_focal_loss_fwd / _fwd_grad / _bwd_reg: the same buffers, layouts, workspace (effdet_loss_workspace_bytes), conventions
 * (device pointers, 0 or a negative EFFDET_E* code, kernel launches only on `stream`) and the same anchor assignment and focal class
 * term; only losses[1] and d(reg) differ.  A library of the same generation built before this header lacks the three symbols, so a
 * binding looks them up by name before the first call.
 *
 * Semantics, every quantity fp32, for a positive anchor (x1, y1, x2, y2) with regression row r and its assigned annotation row
 * g = (gx1, gy1, gx2, gy2) taken raw (no width clamp); gw = gx2 - gx1, gh = gy2 - gy1:
 *   decode   aw = x2 - x1, ah = y2 - y1, acx = x1 + 0.5 aw, acy = y1 + 0.5 ah        (models/module.py BBoxTransform, std .1 .1 .2 .2)
 *            pcx = acx + 0.1 r0 aw, pcy = acy + 0.1 r1 ah
 *            dw = min(0.2 r2, EFFDET_BOX_LOSS_DW_MAX), dh likewise; pw = exp(dw) aw, ph = exp(dh) ah; corners pc -+ 0.5 p{w,h}
 *   overlap  iw = max(min(px2, gx2) - max(px1, gx1), 0), ih likewise; I = iw ih, U = pw ph + gw gh - I, iou = I / (U + 1e-7)
 *   hull     cw = max(px2, gx2) - min(px1, gx1), ch likewise
 *   IOU      L = 1 - iou
 *   GIOU     C = cw ch, L = 1 - iou + (C - U) / (C + 1e-7)
 *   DIOU     L = 1 - iou + rho2 / (cw^2 + ch^2 + 1e-7), rho2 = (pcx - (gx1 + gx2) / 2)^2 + (pcy - (gy1 + gy2) / 2)^2
 *   CIOU     the DIOU loss + alpha v, v = 4 / pi^2 (atan(gw / gh) - atan(pw / ph))^2, alpha = v / (1 - iou + v + 1e-7) held constant
 *            in the gradient
 *   losses[1] = weight * mean over the B images of (sum over the image's positives of L) / num_pos; an image without a valid
 *            annotation row or without a positive anchor contributes 0.  losses[0] is effdet_focal_loss_fwd's.
 *   d(reg)   what autograd gives for the formulas above, times gscale[1] * weight / (B * num_pos): min / max split a tie 0.5 / 0.5,
 *            the clamp of iw / ih at 0 passes the gradient at exactly 0, the dw / dh cap passes at equality and is 0 beyond it.
 *            Exact +0.0 for every anchor that is not positive and in every pad channel.
 * A non-finite r at a positive anchor makes losses[1] non-finite; the gradient row is then unspecified. */
#ifndef EFFDET_BOX_LOSS_H
#define EFFDET_BOX_LOSS_H
#include "effdet_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

enum { EFFDET_BOX_LOSS_IOU = 1, EFFDET_BOX_LOSS_GIOU = 2, EFFDET_BOX_LOSS_DIOU = 3, EFFDET_BOX_LOSS_CIOU = 4 };   /* kind (0, the
                                                    reference's smooth-L1, is what the effdet_focal_loss_* entry points compute) */
#define EFFDET_BOX_LOSS_DW_MAX 4.135166556742356f   /* log(1000 / 16), rounded to fp32 */

/* Arguments and error codes as effdet_focal_loss_fwd / _fwd_grad / _bwd_reg; in addition a kind outside 1..4 or a weight that is
 * negative or not finite is EFFDET_EINVAL.  Nothing is launched when a code is returned for an argument.  bwd_reg reads the workspace
 * a forward call of any kind (or effdet_focal_loss_fwd / _fwd_grad) left: the assignment does not depend on the kind. */
int effdet_box_loss_fwd(const float* cls, const float* reg, const float* anchors, const float* annots, float* losses,
                        void* workspace, long long workspace_bytes, int B, long long A, int num_classes, int N, int kind,
                        float weight, effdet_stream_t stream);
int effdet_box_loss_fwd_grad(const float* cls, const float* reg, const float* anchors, const float* annots, float* losses,
                             void* workspace, long long workspace_bytes, void* dcls_pix, int dld, int dtype, int B,
                             long long A, int num_classes, int N, int kind, float weight, effdet_stream_t stream);
int effdet_box_loss_bwd_reg(const float* reg, const float* anchors, const float* annots, const float* gscale,
                            const void* workspace, void* dreg, int reg_ld, int dtype, int B, long long A, int N, int kind,
                            float weight, effdet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EFFDET_BOX_LOSS_H */
