"""Inputs of the ATSS matcher tests (tests/test_atss_host.py on the CPU, tests/test_gpu_atss.py on the device).  A case is a
tests/loss_cases.py case dict plus
  level_start, topk: the matcher's arguments (where no table is named it is the S = 128 one: A = 3069, levels 2304 / 576 / 144 / 36 / 9,
         whose 2880 boundary falls inside a 256-anchor workgroup);
  tags:  what the construction reaches (tests/test_atss_host.py checks each);
  exact: [(image, anchor)] anchors that tie on purpose with exactly representable operands; margin() leaves them out and the host
         test pins them by hand.
Everything else keeps tests/atss_restated.margin() >= MARGIN, so the device assigns exactly what the float32 mirror does and no
element is excluded from any comparison.  The seeds below were chosen so that this holds."""
import functools

import numpy as np
import torch

from oracle import effdet_oracle as O
from tests import atss_restated as AR
from tests import box_loss_cases as BC
from tests import loss_cases as LC
from tests import loss_options_cases as OC

MARGIN = 1e-6                                        # LC.skip_mask's
S128_LEVELS = [0, 2304, 2880, 3024, 3060, 3069]


def _with(case, level_start, topk, tags, exact=()):
    c = dict(case)
    c.update(level_start=list(level_start), topk=topk, tags=tuple(tags), exact=list(exact))
    assert c['level_start'][-1] == c['anc'].shape[1]
    return c


# --------------------------------------------------------------------------- hand
HAND_SHAPES = [(4, 4), (5, 5), (6, 6), (3, 6), (4, 8), (5, 10), (6, 3), (8, 4), (10, 5)]      # (half width, half height) of a pixel's 9
HAND_LEVELS = [0, 144, 180]
HAND_TOPK = 12
HAND_BOX = (16.0, 8.0, 32.0, 24.0)
HAND_CAND = list(range(54, 66)) + list(range(153, 162)) + [171, 172, 173]


def hand_table():
    """Level 0: 4 x 4 pixels of stride 8 (centres 8x + 4, 8y + 4), level 1: 2 x 2 of stride 16 (centres 16x + 8, 16y + 8) with
    HAND_SHAPES doubled; pixel-major, 9 anchors per pixel, every coordinate an integer.  A = 144 + 36 = 180."""
    rows = []
    for stride, n, mul in ((8, 4, 1), (16, 2, 2)):
        for y in range(n):
            for x in range(n):
                cx, cy = stride * x + stride // 2, stride * y + stride // 2
                rows += [(cx - mul * hw, cy - mul * hh, cx + mul * hw, cy + mul * hh) for hw, hh in HAND_SHAPES]
    return torch.tensor(rows, dtype=torch.float32)[None]


def hand():
    """One valid row (row 1 of 3) on hand_table(), topk 12: the 16 x 16 box (16, 8, 32, 24), centre (24, 16).

    Level 0.  The centre is the corner shared by pixels 6, 7 (y 1, x 2 / 3: centres (20, 12), (28, 12)) and 10, 11 (centres (20, 20),
    (28, 20)): d2 = 16 + 16 = 32 for all 36 anchors of the four, 160 or more for every other pixel.  Index order decides: the 12
    candidates are anchors 54 .. 62 (pixel 6) and 63, 64, 65 (pixel 7) -- 54 .. 63 are held by wave 0 of the selection, 64 and 65 by
    wave 1.  IoUs with the box (area 256), slot by slot of pixel 6, intersection / union:
      (4,4) 64/256 = .25   (5,5) 81/275 = .294545   (6,6) 100/300 = .333333   (3,6) 60/268 = .223881   (4,8) 96/288 = .333333
      (5,10) 126/330 = .381818   (6,3) 60/268 = .223881   (8,4) 96/288 = .333333   (10,5) 126/330 = .381818
    and by symmetry .25, .294545, .333333 for slots 0 .. 2 of pixel 7.
    Level 1.  Pixels 1 and 3 (centres (24, 8), (24, 24)) are at d2 = 64, the other two at 320: candidates 153 .. 161 (pixel 1) and 171,
    172, 173 (pixel 3).  IoUs of pixel 1:
      (8,8) 128/384 = .333333   (10,10) 160/496 = .322581   (12,12) 192/640 = .3   (6,12) 144/400 = .36   (8,16) 256/512 = .5
      (10,20) 256/800 = .32   (12,6) 96/448 = .214286   (16,8) 128/640 = .2   (20,10) 160/896 = .178571
    and .333333, .322581, .3 for slots 0 .. 2 of pixel 3.
    Threshold.  m = 24, sum = 7.318507, mean = .304938; sum of squared deviations = .113229, / 23 = .004923, std = .070164;
    thr = .375102.
    Positives.  IoU >= thr: anchors 59 and 62 (.381818) and 157 (.5).  Anchor 157's centre (24, 8) lies ON the box's upper side
    (cy - y1 = 0, not > 0.01): not positive.  So the positives are 59 and 62 with code 1 (the row), every other anchor is negative."""
    ann = torch.full((1, 3, 5), -1.0)
    ann[0, 1] = torch.tensor(list(HAND_BOX) + [2.0])
    c = LC._case(32, 4, ann, 901, anc=hand_table())
    return _with(c, HAND_LEVELS, HAND_TOPK, ('integer_table', 'level_start_not_64', 'four_way_tie', 'winners_in_two_waves', 'centre_on_side'))


HAND_IOU = [(64, 256), (81, 275), (100, 300), (60, 268), (96, 288), (126, 330), (60, 268), (96, 288), (126, 330), (64, 256), (81, 275),
            (100, 300), (128, 384), (160, 496), (192, 640), (144, 400), (256, 512), (256, 800), (96, 448), (128, 640), (160, 896),
            (128, 384), (160, 496), (192, 640)]                   # intersection / union per candidate, in HAND_CAND's order
HAND_THR = 0.375102
HAND_POS = [59, 62]


# --------------------------------------------------------------------------- the S = 128 table
def _boxes_case(boxes, labels, seed, nc=4, B=1, N=None):
    N = len(boxes) if N is None else N
    ann = torch.full((B, N, 5), -1.0)
    for n, (bx, lab) in enumerate(zip(boxes, labels)):
        ann[0, n] = torch.tensor(list(bx) + [float(lab)])
    return LC._case(128, nc, ann, seed)


SMALL_BOXES = [(30.3, 41.7, 77.9, 90.2), (70.1, 12.6, 118.4, 50.3), (8.2, 60.5, 40.9, 120.7)]


def small_level():
    """topk = 16 against the 9-anchor top level: min(topk, level size) = 9 candidates there, 16 on the other four levels."""
    return _with(_boxes_case(SMALL_BOXES, (0, 1, 2), 911), S128_LEVELS, 16, ('topk_above_level_size', 'wide_list'))


def single():
    """topk = 1 with the whole table as ONE level: m = 1, std 0, thr = the nearest anchor's own IoU -- positive iff its centre is inside."""
    return _with(_boxes_case(SMALL_BOXES, (3, 1, 0), 912), [0, 3069], 1, ('one_candidate', 'one_level'))


def straddle():
    """BC.straddle (261 anchors, N = 65, B = 3) as two levels 252 + 9: the tail workgroup, the 64-row chunk boundary, pad rows between
    valid ones, an image of pad rows only and one whose only box no anchor reaches at 0.5."""
    return _with(BC.get('straddle'), [0, 252, 261], 9, ('tail_workgroup', 'chunk_crossing', 'pads_between', 'empty_image'))


NESTED_BOXES = [(36.3, 40.2, 90.1, 86.4), (38.7, 41.9, 84.4, 81.2)]


def nested():
    """Two overlapping boxes that share candidates: 7 anchors are positive for both and take the row of the larger IoU (4 go to row
    0, 3 to row 1), and either row keeps the positives the other does not claim."""
    return _with(_boxes_case(NESTED_BOXES, (1, 3), 921), S128_LEVELS, 9, ('shared_candidates', 'loser_keeps_others'))


def dup():
    """The same box in rows 0 and 2 with different labels (a pad row between): the same candidates, threshold and IoUs -- an exact tie
    on every positive, so the first row wins.  Those anchors are `exact`."""
    ann = torch.full((1, 3, 5), -1.0)
    ann[0, 0] = torch.tensor([30.3, 41.7, 77.9, 90.2, 1.0])
    ann[0, 2] = ann[0, 0]
    ann[0, 2, 4] = 3.0
    c = _with(LC._case(128, 4, ann, 931), S128_LEVELS, 9, ('exact_tie',))
    r = AR.row_view(c, 0, 0)
    c['exact'] = [(0, a) for a, p in zip(r['cand'], r['pos']) if p]
    return c


NARROW_BOX = (60.0, 40.0, 60.015625, 80.0)


def none():
    """Image 0: one box narrower than 0.02 px -- no centre is more than 0.01 inside it: candidates but no positive.  Image 1: a box far
    outside the table (every IoU 0, thr 0, no centre inside).  Image 2: no valid row (every anchor ignored)."""
    ann = torch.full((3, 2, 5), -1.0)
    ann[0, 1] = torch.tensor(list(NARROW_BOX) + [1.0])
    ann[1, 0] = torch.tensor(list(OC.FAR_BOX) + [2.0])
    return _with(LC._case(128, 4, ann, 941), S128_LEVELS, 9, ('no_positive', 'far_box', 'empty_image'))


S128_SEEDS = {4: 51, 80: 52}


def s128_seeded(nc):
    _, ann = O.synthetic_batch(2, 128, seed=S128_SEEDS[nc], num_classes=nc)
    return _with(LC._case(128, nc, ann, 950 + nc), S128_LEVELS, 9, ('seeded',))


CASES = {'hand': hand, 'small_level': small_level, 'single': single, 'straddle': straddle, 'nested': nested, 'dup': dup, 'none': none,
         's128_nc4': functools.partial(s128_seeded, 4), 's128_nc80': functools.partial(s128_seeded, 80)}


@functools.lru_cache(maxsize=None)
def get(name):
    """The case, built once; treat it as read-only."""
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def codes(name):
    """The float32 mirror's codes of the case; read-only."""
    return AR.assign(get(name))


def margin(case, topk=None):
    return AR.margin(case, topk)


def levels(case):
    return np.diff(case['level_start']).tolist()
