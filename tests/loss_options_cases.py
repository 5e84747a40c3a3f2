"""Inputs and option sets of the loss-option tests (tests/test_loss_options_host.py on the CPU, tests/test_gpu_loss_options.py on the
device), built from tests/loss_cases.py and tests/box_loss_cases.py (S = 128, A = 3069, nc = 4 unless the name says otherwise).

A case is a tests/loss_cases.py case dict plus
  exact: [(image, anchor)] anchors that sit ON a band or tie for a row's maximum on purpose.  Their products are exactly representable
         (integer anchor, integer box), so fp32 and float64 agree and fused multiply-add cannot matter; margin() leaves them out and
         tests/test_loss_options_host.py pins them by hand instead.
Everything else keeps its IoUs at least MARGIN (the margin of tests/loss_cases.skip_mask) away from a band, from the runner-up row of
a positive, and -- with low_quality -- every row's maximum away from its runner-up anchor, so the device assigns exactly what the
float64 restatement does and no element is excluded from any comparison.

Why the low-quality cases replace an anchor: a box that no anchor reaches at IoU 0.5 is typically CONTAINED in many anchors of the
model's table, whose IoUs differ only through their areas -- 1024 up to rounding for the three ratios of a level-3 pixel -- so a row's
maximum is a near-tie that fp32 and float64 resolve differently.  One replaced table entry that overlaps the box far more than any
other (still under 0.5) gives the row a maximum with room; the C ABI takes any [A, 4] table."""
import functools

import torch

from oracle import effdet_oracle as O
from tests import box_loss_cases as BC
from tests import loss_cases as LC
from tests import loss_options_restated as R

MARGIN = 1e-6                                        # LC.skip_mask's
NC = 4

# --------------------------------------------------------------------------- option sets
OPTS = {
    'paper': dict(alpha=0.25, gamma=1.5, beta=0.1, reg_weight=50.0, low_quality=True),      # the EfficientDet paper's loss
    'paper_nolq': dict(alpha=0.25, gamma=1.5, beta=0.1, reg_weight=50.0),                   # ... where a row's maximum has no margin
    'lq': dict(low_quality=True),
    'smooth': dict(label_smoothing=0.1),
    'gamma0': dict(alpha=0.5, gamma=0.0, label_smoothing=0.05, beta=0.5),
    'bands': dict(pos_iou=0.75, neg_iou=0.25),                                              # exactly representable bands
    'high_bands_lq': dict(pos_iou=0.875, neg_iou=0.8125, low_quality=True, gamma=1.5),
}


def opts(name):
    return R.options(**OPTS[name])


def _with(case, **kw):
    c = dict(case)
    c.update(kw)
    c.setdefault('exact', [])
    return c


# --------------------------------------------------------------------------- the cases
STRADDLE_SMALL = 258                                 # in the 5-anchor tail workgroup of the 261-anchor table


def straddle_lq():
    """BC.straddle (261 anchors, N = 65: the tail workgroup and the 64-row chunk are crossed) with tail anchor 258 replaced by the
    7 x 7 box (59, 59, 66, 66): IoU 16 / 49 with the 4 x 4 box of image 2 (row 5), which no anchor reaches at 0.5 -- the only anchor
    low_quality promotes there; the row's maximum comes from the tail workgroup, every other anchor from the first."""
    c = BC.get('straddle')
    anc = c['anc'].clone()
    anc[0, STRADDLE_SMALL] = torch.tensor([59.0, 59.0, 66.0, 66.0])
    return _with(c, anc=anc)


TINY_SMALL = 1500


def tiny_lq():
    """LC.tiny_box's annotations (a 0.5 x 0.5 box, row 2, inside a 0.6 x 0.6 one, row 0) on the model's table with entry 1500 replaced
    by (60, 60, 61.5, 61.5): IoU 0.36 / 2.25 = 0.16 with row 0 and 0.25 / 2.25 = 0.111 with row 2, both rows' maximum.  Without
    low_quality the image has no positive; with it anchor 1500 is promoted and takes its OWN arg-max row 0, not row 2."""
    c = LC.CASES['tiny_box']()
    anc = LC.anchors(128).clone()
    anc[0, TINY_SMALL] = torch.tensor([60.0, 60.0, 61.5, 61.5])
    return _with(c, anc=anc, expect=[], expect_all={})


TIE_A, TIE_B = LC.int_anchor(8, 8), LC.int_anchor(8, 9)     # (52, 52, 84, 84) and (60, 52, 92, 84)
FAR_BOX = (5000.0, 5000.0, 5010.0, 5010.0)


def lq_ties():
    """Image 0: the 32 x 32 box (56, 52, 88, 84) half-way between the integer anchors TIE_A and TIE_B: intersection 28 x 32 = 896,
    union 1152 with either -- the same operands, so the same IoU 0.7777.. in any precision --, 0.63 at most with any other anchor.
    With the bands of 'high_bands_lq' (0.8125 / 0.875) every anchor is negative by the bands and exactly those two are promoted.
    Image 1: one box that overlaps no anchor (gtmax 0): nothing is promoted, every anchor negative, no positive."""
    ann = torch.full((2, 3, 5), -1.0)
    ann[0, 1] = torch.tensor([56.0, 52.0, 88.0, 84.0, 2.0])
    ann[1, 2] = torch.tensor(list(FAR_BOX) + [1.0])
    c = LC._case(128, NC, ann, 811)
    return _with(c, exact=[(0, TIE_A), (0, TIE_B)])


BAND_BOXES = [   # against the integer anchor (52, 52, 84, 84), 32 rows tall and sticking out to the right as LC.THRESHOLD_BOXES: intersection
    # (84 - x1) * 32; every product an exact integer, the two band ratios exactly representable
    ((57, 52, 88, 84), LC.POS),     # 864 / (1024 + 992 - 864) = 864 / 1152 = 0.75 exactly -> positive (>=)
    ((56, 52, 87, 84), LC.POS),     # 896 / 1120 = 0.8; and with the next integer anchor (60, 52, 92, 84) 864 / 1152 = 0.75 exactly again
    ((58, 52, 89, 84), LC.IGN),     # 832 / 1184 = 0.703
    ((74, 52, 92, 84), LC.IGN),     # 320 / (1024 + 576 - 320) = 320 / 1280 = 0.25 exactly -> NOT < 0.25 -> ignored
    ((73, 52, 91, 84), LC.IGN),     # 352 / 1248 = 0.282
    ((75, 52, 93, 84), LC.NEG),     # 288 / 1312 = 0.2195
]


def bands():
    """LC.thresholds' construction for the bands 0.25 / 0.75: one image per box of BAND_BOXES (row 1 of 3), nc = 6."""
    t = LC.int_anchor(8, 8)
    ann = torch.full((len(BAND_BOXES), 3, 5), -1.0)
    expect = []
    for b, (box, state) in enumerate(BAND_BOXES):
        ann[b, 1] = torch.tensor(list(box) + [b], dtype=torch.float32)
        expect.append((b, t, state, 1 if state == LC.POS else None))
    c = LC._case(128, 6, ann, 821, expect=expect)
    return _with(c, exact=[(0, t), (1, TIE_B), (3, t)])


def nc80():
    """nc = 80 at S = 128, B = 2: the 16-byte loads of the class kernels, dld = 768."""
    _, ann = O.synthetic_batch(2, 128, seed=43, num_classes=80)
    return _with(LC._case(128, 80, ann, 831))


TAIL_NC = LC.TAIL_NC[1]                              # 3: A * nc % 4 == 3, scalar loads and stores on every group, [B][A][nc] only


def tail_nc():
    return _with(LC.tails(TAIL_NC))


CASES = {'straddle_lq': straddle_lq, 'tiny_lq': tiny_lq, 'lq_ties': lq_ties, 'bands': bands, 'nc80': nc80, 'tail_nc%d' % TAIL_NC: tail_nc,
         'straddle': lambda: _with(BC.get('straddle')), 's128_r05': lambda: _with(BC.get('s128_r05')),
         'tiny_box': lambda: _with(LC.CASES['tiny_box']())}

# (case, option set) pairs the device tests run; every one is proven by tests/test_loss_options_host.py to have its margin
RUNS = [('straddle_lq', 'paper'), ('straddle_lq', 'lq'), ('straddle', 'smooth'), ('straddle', 'gamma0'), ('tiny_lq', 'lq'),
        ('tiny_lq', 'paper'), ('tiny_box', 'paper'), ('lq_ties', 'high_bands_lq'), ('bands', 'bands'), ('s128_r05', 'paper_nolq'),
        ('s128_r05', 'bands'), ('nc80', 'paper_nolq'), ('tail_nc%d' % TAIL_NC, 'gamma0'), ('tail_nc%d' % TAIL_NC, 'smooth')]
# (the seeded tables -- s128_r05, nc80, tail_nc -- run without low_quality: their boxes lie inside several anchors of equal area, so
# a row's maximum is a tie or a near-tie there, see the module docstring)
# the existing cases on which the default options are compared with the existing entry points
DEFAULT_CASES = ['straddle', 's128_r05', 'tiny_box']


@functools.lru_cache(maxsize=None)
def get(name):
    """The case, built once; treat it as read-only."""
    return CASES[name]()


def margin(case, o):
    """-> the smallest float64 distance that a rounding would have to bridge to change the assignment under options o, the `exact`
    anchors left out: any anchor's best IoU from either band; a positive's best from its second-best row; with low_quality each valid
    row's maximum (> 0) from its runner-up anchor, and a row without overlap must have maximum exactly 0."""
    m = 1.0
    codes, _ = R.assign(case, o, torch.float64)
    for b in range(case['ann'].shape[0]):
        iou, rows = LC.oracle_iou(case, b, torch.float64)
        if len(rows) == 0:
            continue
        keep = torch.ones(iou.shape[0], dtype=torch.bool)
        for (eb, ea) in case['exact']:
            if eb == b:
                keep[ea] = False
        top = iou.topk(min(2, len(rows)), dim=1)[0]
        m = min(m, float((top[keep, 0] - o['neg_iou']).abs().min()), float((top[keep, 0] - o['pos_iou']).abs().min()))
        pos = (codes[b] >= 0) & keep
        if len(rows) > 1 and bool(pos.any()):
            m = min(m, float((top[pos, 0] - top[pos, 1]).min()))
        if o['low_quality']:
            for j in range(len(rows)):
                col = iou[keep, j]
                t2 = col.topk(2)[0]
                exact_max = max([float(iou[ea, j]) for (eb, ea) in case['exact'] if eb == b] or [0.0])
                if float(t2[0]) == 0.0 and exact_max == 0.0:
                    continue                                    # no overlap at all: exactly 0 in any precision
                if exact_max > float(t2[0]):
                    m = min(m, exact_max - float(t2[0]))        # the exact anchors hold the maximum: room to the best of the rest
                else:
                    m = min(m, float(t2[0] - t2[1]), float(t2[0]) - exact_max if exact_max > 0.0 else 1.0)
    return m
