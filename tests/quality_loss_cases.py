"""Inputs, option sets and runs of the quality-loss tests (tests/test_quality_loss_host.py on the CPU, tests/test_gpu_quality_loss.py on
the device), built from tests/loss_cases.py, tests/box_loss_cases.py, tests/loss_options_cases.py and tests/atss_cases.py: the
smallest tables those files have (S = 128: A = 3069, nc = 4; the 261-anchor `straddle` table with N = 65; nc = 3 for the scalar path of
the flat kernels).

A case is a tests/loss_options_cases.py case dict (with `exact`: the anchors that sit on a band on purpose, left out of margin()) or a
tests/atss_cases.py one (with level_start / topk), plus
  tags: what the construction reaches; tests/test_quality_loss_host.py checks each.
Every other IoU keeps MARGIN from a band (OC.margin / AC.margin), so the device assigns what the float64 restatement does and no
element is excluded from a comparison.  The varifocal loss jumps where q leaves 0, so every positive's q is either exactly 0 with the
prediction at least Q_ZERO_PX off its box, or at least Q_MIN (tests/test_quality_loss_host.py checks that too)."""
import functools

import torch

from tests import atss_cases as AC
from tests import box_loss_cases as BC
from tests import loss_cases as LC
from tests import loss_options_cases as OC
from tests import loss_options_restated as R
from tests import quality_loss_restated as QR

MARGIN = OC.MARGIN
Q_MIN, Q_ZERO_PX = 1e-4, BC.MARGIN
NC = 4
GS = (0.7, 1.3)                                      # upstream gradients of the two losses

# --------------------------------------------------------------------------- option sets
OPTS = {
    'default': dict(),
    'huber': dict(beta=0.1, reg_weight=50.0),
    'lq': dict(beta=0.1, reg_weight=50.0, low_quality=True),
}
QUALITY = {
    'qfl': dict(kind='qfl'),
    'qfl15': dict(kind='qfl', beta=1.5),
    'vfl': dict(kind='vfl'),
    'vfl15': dict(kind='vfl', alpha=0.5, gamma=1.5),
}


def opts(name):
    return R.options(**OPTS[name])


def quality(name):
    return QR.options(**QUALITY[name])


# --------------------------------------------------------------------------- edges
T, T_CAP, T_OFF, T_LOW = LC.int_anchor(8, 8), LC.int_anchor(8, 9), LC.int_anchor(9, 8), LC.int_anchor(7, 8)
EDGE_BOX = (52.0, 52.0, 84.0, 84.0)                  # == anchor T
HALF_BOX = (60.0, 52.0, 100.0, 84.0)                 # LC.THRESHOLD_BOXES[0]: IoU 768 / 1536 = 0.5 exactly with anchor T
HALF_ON_BAND = [LC.int_anchor(y, x) for y, x in ((7, 9), (7, 10), (8, 8), (8, 11), (9, 9), (9, 10))]
P_BELOW, P_ABOVE = 1e-5, 1.0 - 1e-5


def edges():
    """Five images on the S = 128 table, nc = 4, every named coordinate an integer.
    image 0: the box IS the integer anchor T (52, 52, 84, 84), label 1.
      T      r = 0: prediction == box, I = U = 1024, q = 1024 / (1024 + 1e-7) -- exactly 1 in fp32.  Its four probabilities: below the
             clamp, above it (on the label), and exactly on either end.
      T_CAP  the integer anchor one pixel to the right (IoU 768 / 1280 = 0.6: positive), r2 = 25: 0.2 r2 = 5 is beyond the dw cap.
             Probabilities exactly on the clamp ends (the low end on the label), and 1 - 1e-6 / 1e-6.
      T_OFF  the integer anchor one pixel down (0.6 too), r0 = 30: the prediction's centre moves 96 px right, off the box: iw < 0,
             q exactly 0 -- a positive anchor whose label element takes the varifocal loss's NEGATIVE branch.
      T_LOW  the integer anchor one pixel up (0.6 too): its label probability lies below the clamp.
    image 1: the box (60, 52, 100, 84), label 2: IoU exactly 0.5 with T -- ON the pos_iou band, so (1, T) is `exact` -- and r = 0,
             p = 0.5 on the label: p == t exactly in fp32 (768 / (1536 + 1e-7) rounds to 0.5), u = 0.  The five other integer anchors
             of HALF_ON_BAND meet the box in 768 of 1536 px too (32 x 24 or 24 x 32): `exact` as well, with random inputs.
    image 2: no valid row.  image 3: one box that overlaps no anchor (rows, no positive).  image 4: image 0's box, random inputs."""
    ann = torch.full((5, 3, 5), -1.0)
    ann[0, 1] = torch.tensor(list(EDGE_BOX) + [1.0])
    ann[1, 2] = torch.tensor(list(HALF_BOX) + [2.0])
    ann[3, 0] = torch.tensor(list(OC.FAR_BOX) + [3.0])
    ann[4, 1] = ann[0, 1]
    c = LC._case(128, NC, ann, 1001)
    cls, reg = c['cls'], c['reg']
    hi, lo = R.P_HI, R.P_LO
    reg[0, T] = 0.0
    cls[0, T] = torch.tensor([P_BELOW, P_ABOVE, lo, hi])
    reg[0, T_CAP] = torch.tensor([0.25, -0.5, 25.0, -3.0])
    cls[0, T_CAP] = torch.tensor([hi, lo, 1.0 - 1e-6, 1e-6])
    reg[0, T_OFF] = torch.tensor([30.0, 0.0, 0.0, 0.0])
    cls[0, T_OFF] = torch.tensor([lo, hi, P_BELOW, 0.3])
    cls[0, T_LOW, 1] = P_BELOW
    reg[1, T] = 0.0
    cls[1, T, 2] = 0.5
    c.update(exact=[(1, a) for a in HALF_ON_BAND], tags=('q_zero', 'q_one', 'p_equals_t', 'p_clamp', 'dw_cap', 'empty_image', 'no_positive_image'))
    return c


def _tagged(case, *tags):
    c = dict(case)
    c.setdefault('exact', [])
    c['tags'] = tuple(tags)
    return c


CASES = {
    'edges': edges,
    's128_r05': lambda: _tagged(OC.get('s128_r05'), 's128'),
    's128_r20': lambda: _tagged(BC.get('s128_r20'), 's128', 'q_zero'),
    'straddle_lq': lambda: _tagged(OC.get('straddle_lq'), 'tail_workgroup', 'chunk_crossing', 'empty_image', 'low_quality'),
    'straddle': lambda: _tagged(OC.get('straddle'), 'tail_workgroup', 'chunk_crossing', 'empty_image', 'no_positive_image'),
    'tail_nc3': lambda: _tagged(OC.get('tail_nc%d' % OC.TAIL_NC), 'scalar_path'),
    'atss_nested': lambda: _tagged(AC.get('nested'), 'atss'),
    'atss_straddle': lambda: _tagged(AC.get('straddle'), 'atss', 'tail_workgroup', 'chunk_crossing', 'empty_image'),
}

# (case, option set, quality set, box term or None) the device tests run; a case with level_start runs under ATSS with its topk
RUNS = [('edges', 'default', 'qfl', None), ('edges', 'huber', 'vfl', ('giou', 2.0)),
        ('s128_r05', 'huber', 'qfl', ('giou', 2.0)), ('s128_r20', 'default', 'vfl', None), ('s128_r20', 'default', 'qfl15', ('ciou', 1.0)),
        ('straddle_lq', 'lq', 'qfl', None), ('straddle_lq', 'lq', 'vfl15', ('ciou', 2.0)), ('straddle', 'default', 'vfl', None),
        ('tail_nc3', 'default', 'qfl', None), ('tail_nc3', 'huber', 'vfl15', None),
        ('atss_nested', 'huber', 'qfl', ('giou', 2.0)), ('atss_straddle', 'default', 'vfl', None),
        ('atss_straddle', 'default', 'qfl', None), ('atss_straddle', 'huber', 'vfl', ('giou', 2.0))]      # ATSS x {QFL, smooth-L1} / {VFL, box kind}


@functools.lru_cache(maxsize=None)
def get(name):
    """The case, built once; treat it as read-only."""
    return CASES[name]()


def is_atss(case):
    return 'level_start' in case


@functools.lru_cache(maxsize=None)
def codes(name, on):
    """The assignment of the case under option set `on`: the float32 ATSS mirror's for an ATSS case, else the float64 bands'."""
    c = get(name)
    return AC.AR.assign(c) if is_atss(c) else R.assign(c, opts(on), torch.float64)[0]


def margin(name, on):
    c = get(name)
    return AC.margin(c) if is_atss(c) else OC.margin(c, opts(on))


@functools.lru_cache(maxsize=None)
def reference(name, on, qn, box=None):
    """-> (float64 run, float32 run) of the restatement with the upstream gradients GS on one assignment; computed once, read-only."""
    c, cd = get(name), codes(name, on)
    return tuple(QR.run(c, opts(on), quality(qn), box=box, gscale=GS, dtype=dt, codes=cd) for dt in (torch.float64, torch.float32))
