"""The IoU-family box regression losses of include/effdet_box_loss.h restated in torch: decode -> loss -> .backward(), in any
precision.  float64 is the reference of tests/test_gpu_box_loss.py, float32 (the same code) the yardstick that sizes its tolerance.

The header fixes every quantity as fp32, so the constants here are the fp32 ones (0.1f, 0.2f, 1e-7f, the rounded cap and 4 / pi^2)
taken as they are into either precision: the float64 run is then the exactly-rounded evaluation of the same program, and an input that
sits exactly on a kink in fp32 sits on it in float64 too.

The subgradients are autograd's: torch.minimum / torch.maximum split a tie 0.5 / 0.5, clamp(min=0) passes at exactly 0 and
clamp(max=cap) passes at equality (tests/test_box_loss_host.py pins all three on hand-derived cases).

The assignment is loss.hip's loss_assign_kernel, restated by tests/loss_cases.oracle_states."""
import math

import numpy as np
import torch

from tests import loss_cases as LC

KINDS = ('iou', 'giou', 'diou', 'ciou')


def _f32(v):
    return float(np.float32(v))


STD_XY, STD_WH, EPS = _f32(0.1), _f32(0.2), _f32(1e-7)
DW_MAX = _f32(math.log(1000.0 / 16.0))               # EFFDET_BOX_LOSS_DW_MAX
C_4_PI2 = _f32(4.0 / math.pi ** 2)


def decode(anc, r):
    """anc [P, 4], r [P, 4] -> (pcx, pcy, pw, ph) of the predicted boxes (models/module.py BBoxTransform + the dw / dh cap)."""
    aw, ah = anc[:, 2] - anc[:, 0], anc[:, 3] - anc[:, 1]
    acx, acy = anc[:, 0] + 0.5 * aw, anc[:, 1] + 0.5 * ah
    pcx, pcy = acx + STD_XY * r[:, 0] * aw, acy + STD_XY * r[:, 1] * ah
    pw = torch.exp(torch.clamp(STD_WH * r[:, 2], max=DW_MAX)) * aw
    ph = torch.exp(torch.clamp(STD_WH * r[:, 3], max=DW_MAX)) * ah
    return pcx, pcy, pw, ph


def selects(anc, gt, r):
    """The operand pairs of every min / max / clamp select of the loss as differences [P, 8]: the four corner pairs (the intersection
    and the hull select among the same pairs), the two clamps at 0 and the two caps.  A case is away from the kinks when no entry is
    near 0."""
    pcx, pcy, pw, ph = decode(anc, r)
    px1, px2, py1, py2 = pcx - 0.5 * pw, pcx + 0.5 * pw, pcy - 0.5 * ph, pcy + 0.5 * ph
    iwr = torch.minimum(px2, gt[:, 2]) - torch.maximum(px1, gt[:, 0])
    ihr = torch.minimum(py2, gt[:, 3]) - torch.maximum(py1, gt[:, 1])
    return torch.stack([px1 - gt[:, 0], py1 - gt[:, 1], px2 - gt[:, 2], py2 - gt[:, 3], iwr, ihr,
                        STD_WH * r[:, 2] - DW_MAX, STD_WH * r[:, 3] - DW_MAX], 1)


def anchor_loss(kind, anc, gt, r):
    """Per-anchor loss [P] of positives with anchors anc [P, 4], assigned annotation boxes gt [P, 4], regression rows r [P, 4]."""
    pcx, pcy, pw, ph = decode(anc, r)
    px1, px2, py1, py2 = pcx - 0.5 * pw, pcx + 0.5 * pw, pcy - 0.5 * ph, pcy + 0.5 * ph
    gx1, gy1, gx2, gy2 = gt[:, 0], gt[:, 1], gt[:, 2], gt[:, 3]
    gw, gh = gx2 - gx1, gy2 - gy1
    iw = torch.clamp(torch.minimum(px2, gx2) - torch.maximum(px1, gx1), min=0)
    ih = torch.clamp(torch.minimum(py2, gy2) - torch.maximum(py1, gy1), min=0)
    inter = iw * ih
    union = pw * ph + gw * gh - inter
    iou = inter / (union + EPS)
    loss = 1 - iou
    if kind == 'iou':
        return loss
    cw = torch.maximum(px2, gx2) - torch.minimum(px1, gx1)
    ch = torch.maximum(py2, gy2) - torch.minimum(py1, gy1)
    if kind == 'giou':
        hull = cw * ch
        return loss + (hull - union) / (hull + EPS)
    dx, dy = pcx - (gx1 + gx2) / 2, pcy - (gy1 + gy2) / 2
    loss = loss + (dx * dx + dy * dy) / (cw * cw + ch * ch + EPS)
    if kind == 'diou':
        return loss
    assert kind == 'ciou', kind
    da = torch.atan(gw / gh) - torch.atan(pw / ph)
    v = C_4_PI2 * da * da
    alpha = (v / (1 - iou + v + EPS)).detach()
    return loss + alpha * v


def positives(case, codes=None):
    """-> (image [P], anchor [P], row [P]) of the positive anchors, image-major in anchor order; codes default to the float64
    assignment."""
    codes = LC.oracle_states(case, torch.float64) if codes is None else codes
    b, a = torch.nonzero(codes >= 0, as_tuple=True)
    return b, a, codes[b, a]


def run(case, kind, weight=1.0, gscale=1.0, dtype=torch.float64, codes=None):
    """-> dict: loss (losses[1], a python float), per_anchor [P] (dtype), image_sum [B], num_pos [B], grad [B, A, 4] (dtype) =
    d(gscale * losses[1]) / d(reg), pos = positives(case)."""
    B, A = case['reg'].shape[:2]
    b, a, row = positives(case, codes)
    reg = case['reg'].to(dtype).clone().requires_grad_(True)
    anc, ann = case['anc'][0].to(dtype), case['ann'].to(dtype)
    la = anchor_loss(kind, anc[a], ann[b, row, :4], reg[b, a])
    num_pos = torch.bincount(b, minlength=B)
    image_sum = torch.zeros(B, dtype=dtype).index_add(0, b, la)
    live = num_pos > 0                                  # (an image without valid rows has no positive either)
    per_image = torch.where(live, image_sum / num_pos.clamp(min=1).to(dtype), torch.zeros((), dtype=dtype))
    loss = weight * per_image.mean()
    (gscale * loss).backward()
    return {'loss': float(loss.detach()), 'per_anchor': la.detach(), 'image_sum': image_sum.detach(), 'num_pos': num_pos,
            'grad': reg.grad.detach(), 'pos': (b, a, row)}
