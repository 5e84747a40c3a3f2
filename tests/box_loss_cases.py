"""Seeded inputs of the IoU-family box loss tests (tests/test_box_loss_host.py on the CPU, tests/test_gpu_box_loss.py on the device).
A case is a tests/loss_cases.py case dict (S, cls, reg, anc, ann, ...) plus
  tags: what the construction reaches ('tail_workgroup', 'chunk_crossing', 'empty_image', 'no_positive_image', 'capped_dw', ...),
  tie:  True where inputs sit on kinks on purpose (every coordinate exactly representable, so fp32 and fp64 take the same branch);
        the other cases keep every min / max / clamp select at least MARGIN px (resp. MARGIN in dw) away from a tie, which
        tests/test_box_loss_host.py checks, so precision cannot flip a branch and no element is excluded from a comparison.
The draws are fixed by the seeds below; they were chosen so that the margin condition holds."""
import functools

import numpy as np
import torch

from tests import box_loss_restated as R
from tests import loss_cases as LC

MARGIN = 1e-2
NC = 4


def _cls(B, A, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.sigmoid((torch.randn(B, A, NC, generator=g) * 2.0).clamp(-6.0, 6.0))


def _case(anc, ann, reg, seed, tags, tie=False):
    return {'S': 128, 'cls': _cls(ann.shape[0], anc.shape[1], seed), 'reg': reg.float(), 'anc': anc, 'ann': ann.float(), 'expect': [],
            'expect_all': {}, 'state_check': 'exact', 'tags': tuple(tags), 'tie': tie}


# --------------------------------------------------------------------------- straddle
STRADDLE_A = 9 * 29                                  # one full 256-thread workgroup + a 5-anchor tail
STRADDLE_N = 65                                      # crosses the 64-row chunk of loss_assign_kernel
STRADDLE_SEED = 1
STRADDLE_TAIL_ANCHOR = 9 * 28 + 7                    # 259: in the tail workgroup, assigned row 64


def straddle():
    """A synthetic table of 261 anchors (the 29 level-3 pixels from (y 6, x 0) on of the S = 128 table), B = 3: image 0 with 20 valid
    rows scattered over the 65 -- jittered copies of anchors, row 64 a copy of tail anchor 259 --, image 1 all pad rows, image 2 one
    4 x 4 box that no anchor reaches (valid rows, no positive)."""
    anc = LC.anchors(128)[:, 9 * 96: 9 * 96 + STRADDLE_A].clone()
    rng = np.random.RandomState(STRADDLE_SEED)
    ann = torch.full((3, STRADDLE_N, 5), -1.0)
    rows = np.concatenate([np.sort(rng.permutation(64)[:19]), [64]])
    src = np.concatenate([rng.permutation(256)[:19], [STRADDLE_TAIL_ANCHOR]])
    jitter = torch.from_numpy(rng.uniform(-2.5, 2.5, (20, 4)).astype(np.float32))
    ann[0, rows, :4] = anc[0, src] + jitter
    ann[0, rows, 4] = torch.from_numpy(rng.randint(0, NC, 20).astype(np.float32))
    ann[2, 5] = torch.tensor([60.3, 60.7, 64.3, 64.7, 1.0])
    g = torch.Generator().manual_seed(STRADDLE_SEED)
    reg = torch.randn(3, STRADDLE_A, 4, generator=g) * 0.5
    return _case(anc, ann, reg, 11, ('tail_workgroup', 'chunk_crossing', 'empty_image', 'no_positive_image'))


# --------------------------------------------------------------------------- s128
S128_BOX_SEED = 6
S128_REG_SEED = {0.5: 4, 2.0: 3}                     # reg scale -> seed of the draw


def s128(scale):
    """The S = 128 model anchors (A = 3069), 40 random boxes, reg ~ scale * randn: scale 0.5 is a plausible early-training head,
    scale 2.0 throws a share of the predictions off their annotation (zero intersection: the IoU term's gradient vanishes there and
    only the GIoU / DIoU / CIoU terms pull)."""
    anc = LC.anchors(128)
    rng = np.random.RandomState(S128_BOX_SEED)
    ann = torch.full((1, 40, 5), -1.0)
    ann[0, :, :4] = LC._random_boxes(rng, 40, 128)
    ann[0, :, 4] = torch.from_numpy(rng.randint(0, NC, 40).astype(np.float32))
    g = torch.Generator().manual_seed(S128_REG_SEED[scale])
    reg = torch.randn(1, anc.shape[1], 4, generator=g) * scale
    return _case(anc, ann, reg, 12, ('zero_intersection',) if scale == 2.0 else ())


# --------------------------------------------------------------------------- ties
TIE_T = LC.int_anchor(8, 8)                          # the integer anchor (52, 52, 84, 84)
TIE_SHIFTED = 100                                    # table entry replaced by the anchor (0, 52, 32, 84)
TIE_GX1 = float(np.float32(16.0) + np.float32(0.1) * np.float32(-8.0) * np.float32(32.0) + np.float32(16.0))    # 6.3999996...
CAP_R_AT = None                                      # set below: fp32 r with fl(0.2f * r) == the cap, the exact product just below it
CAP_R_ABOVE = None                                   # the next fp32 r whose product lies above the cap in both precisions


def _cap_values():
    std, cap = np.float32(0.2), np.float32(R.DW_MAX)
    r = np.float32(float(cap) / float(std))
    r = np.nextafter(r, np.float32(0), dtype=np.float32)
    r = np.nextafter(r, np.float32(0), dtype=np.float32)
    at = None
    for _ in range(8):
        exact = float(std) * float(r)
        if np.float32(std * r) == cap and exact <= float(cap):
            at = r
        if np.float32(std * r) > cap and exact > float(cap):
            return at, r
        r = np.nextafter(r, np.float32(100), dtype=np.float32)
    raise AssertionError('no fp32 r around the cap')


CAP_R_AT, CAP_R_ABOVE = _cap_values()


def ties():
    """Three images on the S = 128 table, reg = 0 but for the rows named here, every coordinate exactly representable.
    image 0: the annotation IS anchor TIE_T and reg = 0: prediction == annotation, all four min / max pairs tie; loss 0, gradient 0.
    image 1: table entry TIE_SHIFTED is the anchor (0, 52, 32, 84) with r0 = -8: the prediction is (-25.6, 52, 6.4, 84) in fp32
             arithmetic without a rounding (0.1f * -8 * 32 and 16 + that are exact), the annotation (6.4f, 52, 38.5, 84) starts where
             it ends: iw == 0 exactly, the clamp passes the gradient.
    image 2: anchor TIE_T with 0.2f * r2 == the cap in fp32 (the exact product a hair below: both precisions pass the gradient) and
             0.2f * r3 above it (no gradient)."""
    anc = LC.anchors(128).clone()
    anc[0, TIE_SHIFTED] = torch.tensor([0.0, 52.0, 32.0, 84.0])
    ann = torch.full((3, 2, 5), -1.0)
    ann[0, 1] = torch.tensor([52.0, 52.0, 84.0, 84.0, 1.0])
    ann[1, 0] = torch.tensor([TIE_GX1, 52.0, 38.5, 84.0, 2.0])
    ann[2, 1] = torch.tensor([50.0, 52.0, 86.0, 84.0, 3.0])
    reg = torch.zeros(3, anc.shape[1], 4)
    reg[1, TIE_SHIFTED, 0] = -8.0
    reg[2, TIE_T, 2] = float(CAP_R_AT)
    reg[2, TIE_T, 3] = float(CAP_R_ABOVE)
    return _case(anc, ann, reg, 13, ('all_ties', 'touching', 'capped_dw'), tie=True)


# --------------------------------------------------------------------------- aspect
ASPECT_SEED = 0


def aspect():
    """Annotations with gw / gh in {1/8, 1, 8} (for ciou's v and alpha) on a table whose entries 100, 1500 and 3000 are replaced by
    anchors of about those shapes (no model anchor is 1:8), reg ~ 0.5 * randn."""
    anc = LC.anchors(128).clone()
    boxes = [(60.0, 20.0, 68.0, 84.0), (40.0, 40.0, 72.0, 72.0), (20.0, 90.0, 84.0, 98.0)]
    for i, bx, d in zip((100, 1500, 3000), boxes, ((1.5, -2.0, 0.5, 3.0), (-1.0, 2.0, 2.5, -1.5), (2.0, 0.5, -3.0, 1.0))):
        anc[0, i] = torch.tensor(bx) + torch.tensor(d)
    ann = torch.full((1, 5, 5), -1.0)
    for n, bx in zip((0, 2, 3), boxes):
        ann[0, n] = torch.tensor(list(bx) + [float(n % NC)])
    g = torch.Generator().manual_seed(ASPECT_SEED)
    reg = torch.randn(1, anc.shape[1], 4, generator=g) * 0.5
    return _case(anc, ann, reg, 14, ('aspect',))


CASES = {'straddle': straddle, 's128_r05': functools.partial(s128, 0.5), 's128_r20': functools.partial(s128, 2.0), 'ties': ties,
         'aspect': aspect}


@functools.lru_cache(maxsize=None)
def get(name):
    """The case, built once; treat it as read-only."""
    return CASES[name]()


def select_margin(case):
    """-> the smallest |difference| between the operands of any min / max / clamp select over the positives (float64)."""
    b, a, row = R.positives(case)
    d = R.selects(case['anc'][0].double()[a], case['ann'].double()[b, row, :4], case['reg'].double()[b, a])
    return float(d.abs().min())


def assignment_margin(case):
    """-> the smallest float64 distance of any anchor's best IoU from the thresholds 0.4 / 0.5 and, over the positives, of the best
    from the second-best IoU: while it is far above fp32 rounding (~1e-7) the device assigns exactly what the float64 rule does."""
    m = 1.0
    for b in range(case['ann'].shape[0]):
        iou, rows = LC.oracle_iou(case, b, torch.float64)
        if len(rows) == 0:
            continue
        top = iou.topk(min(2, len(rows)), dim=1)[0]
        m = min(m, float((top[:, 0] - 0.4).abs().min()), float((top[:, 0] - 0.5).abs().min()))
        pos = top[:, 0] >= 0.5
        if len(rows) > 1 and bool(pos.any()):
            m = min(m, float((top[pos, 0] - top[pos, 1]).min()))
    return m
