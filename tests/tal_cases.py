"""Inputs of the task-aligned matcher tests (tests/test_tal_host.py on the CPU, tests/test_gpu_tal.py on the device).  A case is a
tests/loss_cases.py case dict plus
  tal:   the matcher's options (tests/tal_restated.options);
  tags:  what the construction reaches (tests/test_tal_host.py checks each).
Every case but `hand` lives on the S = 128 table (A = 3069 = 11 workgroups + 253 anchors, levels 2304 / 576 / 144 / 36 / 9).  The
predictions are seeded; the seeds below were chosen so that tests/tal_restated.gaps holds on every case: each decision of the matcher is
either between equal operands (duplicated rows: the index rule decides) or clear by 1e-3 relative in float64, so the float64 codes are
the only admissible device answer and no anchor is excluded from any comparison."""
import functools

import torch

from oracle import effdet_oracle as O
from tests import atss_cases as AC
from tests import loss_cases as LC
from tests import tal_restated as TR


def _with(case, tags, **tal):
    c = dict(case)
    c.update(tal=TR.options(**tal), tags=tuple(tags))
    return c


def _boxes_case(rows, seed, nc=4, B=2, N=None):
    """rows: [(image, box, label)] in row order per image; the other rows are pads."""
    N = max(sum(1 for r in rows if r[0] == b) for b in range(B)) if N is None else N
    ann = torch.full((B, N, 5), -1.0)
    at = [0] * B
    for b, box, lab in rows:
        ann[b, at[b]] = torch.tensor(list(box) + [float(lab)])
        at[b] += 1
    return LC._case(128, nc, ann, seed)


# --------------------------------------------------------------------------- hand
HAND_BOXES = {0: ((16.0, 8.0, 32.0, 24.0), 2), 2: ((16.0, 8.0, 24.0, 16.0), 0), 3: ((0.0, 0.0, 16.0, 16.0), 1)}      # row -> (box, label)
HAND_SCORES = {(54, 2): 0.5, (63, 2): 0.5, (90, 2): 0.25, (99, 2): 0.125, (54, 0): 0.5, (58, 0): 0.25, (144, 1): 0.5, (0, 1): 0.5}
HAND_TAL = dict(topk=12, alpha=1.0, beta=2.0)
HAND_WINNERS = {0: [54, 63, 90, 99], 2: [54, 58], 3: [144, 0]}
HAND_METRIC = {(0, 54): (1 / 32, 0.25), (0, 63): (1 / 32, 0.25), (0, 90): (1 / 64, 0.25), (0, 99): (1 / 128, 0.25),
               (2, 54): (0.5, 1.0), (2, 58): (1 / 16, 0.5), (3, 144): (0.5, 1.0), (3, 0): (1 / 32, 0.25)}      # (row, anchor) -> (m, u)
HAND_CODES = {63: 0, 90: 0, 99: 0, 54: 2, 58: 2, 144: 3, 0: 3}
HAND_Q = {63: 0.25, 90: 0.125, 99: 0.0625, 54: 1.0, 58: 0.125, 144: 1.0, 0: 0.0625}
HAND_MM = {0: (1 / 32, 0.25), 2: (0.5, 1.0), 3: (0.5, 1.0)}


def hand():
    """tests/atss_cases.hand_table (two levels, every coordinate an integer, A = 180), one image, rows 0, 2, 3 valid and row 1 a pad,
    every regression value 0 (the decoded prediction IS the anchor) and every probability 0 except HAND_SCORES (s == 0 gives m == 0:
    no candidate), topk 12, alpha 1, beta 2: m = s u^2 with s and u powers of two, so every figure below is exact in fp32.

    Row 0, the 16 x 16 box (16, 8, 32, 24), label 2.  Inside: the four level-0 pixels 6, 7, 10, 11 (centres (20, 12), (28, 12), (20, 20),
      (28, 20)); the level-1 centres (24, 8) and (24, 24) lie ON its sides.  Slot 0 of each pixel is the 8 x 8 quadrant of the box:
      u = 64 / 256 = 1/4.  Scores 1/2, 1/2, 1/4, 1/8 at anchors 54, 63, 90, 99: m = 1/32, 1/32, 1/64, 1/128.  Four candidates (< topk):
      all selected, 54 ahead of 63 on equal bits.
    Row 2, the box (16, 8, 24, 16) = anchor 54 itself, label 0.  Inside: pixel 6 alone -- nine anchors, FEWER than topk.  u(54) = 1,
      u(58) = 64 / 128 = 1/2 (slot 4, (16, 4, 24, 20)); scores 1/2 and 1/4: m = 1/2 and 1/16.  Two candidates, both selected.
    Row 3, the box (0, 0, 16, 16) = level-1 anchor 144, label 1: u(144) = 1, and anchor 0 = (0, 0, 8, 8) has u = 1/4; scores 1/2:
      m = 1/2 and 1/32.
    Conflict: anchor 54 is selected by rows 0 (u = 1/4) and 2 (u = 1): row 2 takes it.
    Codes: 63, 90, 99 -> 0; 54, 58 -> 2; 144, 0 -> 3; every other anchor negative.  num_pos = 7.
    Target (fp32: 1/32 + 1e-9 and 1/2 + 1e-9 round back to 1/32 and 1/2):
      row 0 over {63, 90, 99}: mmax 1/32, umax 1/4 -> q = 1/4, 1/8, 1/16
      row 2 over {54, 58}:     mmax 1/2,  umax 1   -> q = 1, 1/8
      row 3 over {144, 0}:     mmax 1/2,  umax 1   -> q = 1, 1/16"""
    anc = AC.hand_table()
    A = anc.shape[1]
    ann = torch.full((1, 4, 5), -1.0)
    for n, (box, lab) in HAND_BOXES.items():
        ann[0, n] = torch.tensor(list(box) + [float(lab)])
    cls = torch.zeros(1, A, 4)
    for (a, k), v in HAND_SCORES.items():
        cls[0, a, k] = v
    c = {'S': 32, 'cls': cls, 'reg': torch.zeros(1, A, 4), 'anc': anc, 'ann': ann, 'expect': [], 'expect_all': {}, 'state_check': 'exact'}
    return _with(c, ('hand', 'two_levels', 'inside_below_topk', 'conflict', 'zero_base', 'pads_between'), **HAND_TAL)


# --------------------------------------------------------------------------- the S = 128 table
STRADDLE_BOX = (20.3, 24.7, 100.9, 93.2)              # centres of four levels inside
WHOLE_BOX = (0.0, 0.0, 128.0, 128.0)
FEW_BOX = (19.0, 19.0, 21.0, 21.0)                    # around the level-0 centre (20, 20) alone: 9 anchors inside


def straddle():
    """One large box per image whose inside set spans several levels, a smaller one beside it."""
    return _with(_boxes_case([(0, STRADDLE_BOX, 1), (0, AC.SMALL_BOXES[1], 3), (1, STRADDLE_BOX, 0)], 1003), ('levels_crossed',))


def whole():
    """The whole image as a box: every anchor's centre is inside, the per-thread lists see all 3069 anchors."""
    return _with(_boxes_case([(0, WHOLE_BOX, 2), (1, WHOLE_BOX, 0), (1, AC.SMALL_BOXES[0], 1)], 1011), ('all_inside',))


def narrow():
    """ATSS's NARROW_BOX (0.0156 px wide): no centre is more than 0.01 inside it -- no candidate, no positive, every anchor negative;
    image 1 has no valid row (every anchor ignored)."""
    return _with(_boxes_case([(0, AC.NARROW_BOX, 1)], 1021), ('no_inside', 'empty_image'))


def few():
    """A 2 x 2 box around one level-0 centre: 9 anchors inside, fewer than topk = 13; a normal box beside it."""
    return _with(_boxes_case([(0, FEW_BOX, 0), (0, AC.SMALL_BOXES[2], 2), (1, FEW_BOX, 3)], 1031), ('inside_below_topk',))


def nested():
    """ATSS's two nested boxes: anchors selected by both rows take the row with the larger IoU."""
    return _with(_boxes_case([(0, AC.NESTED_BOXES[0], 1), (0, AC.NESTED_BOXES[1], 3), (1, AC.NESTED_BOXES[1], 1),
                              (1, AC.NESTED_BOXES[0], 1)], 1041), ('conflict',))


def dup():
    """Exact ties.  Every anchor of image 0 carries the SAME class row and beta = 0 (m = s: equal bits in, equal bits out): the
    winners of a row are its topk inside anchors of LOWEST index.  Rows 0 and 2 are the same box with the same label (a pad row
    between): the same winners with the same u -- every conflict is an exact tie, and the FIRST row takes them all.  Image 1: the same
    with duplicated regression rows as well."""
    c = _boxes_case([(0, AC.SMALL_BOXES[0], 1), (1, AC.SMALL_BOXES[1], 2)], 1051, N=3)
    c['ann'][0, 2] = c['ann'][0, 0]
    c['ann'][1, 2] = c['ann'][1, 0]
    c['cls'][0, :] = c['cls'][0, 0]
    c['cls'][1, :] = c['cls'][1, 5]
    c['reg'][1, :] = c['reg'][1, 5]
    return _with(c, ('metric_tie', 'conflict_tie', 'pads_between'), beta=0.0)


def bad_label():
    """Row 0 of image 0 carries label 9 at nc = 4 (no class: no candidates, but the image counts it as a valid row), row 1 a good
    one; image 1 has ONLY a bad-label row: every anchor negative, none ignored."""
    return _with(_boxes_case([(0, AC.SMALL_BOXES[0], 9), (0, AC.SMALL_BOXES[1], 2), (1, AC.SMALL_BOXES[2], 4)], 1061), ('label_outside',))


N70_SEED = 7


def n70():
    """N = 70 with 66 valid rows in image 0 (pads at rows 3, 20, 64, 69): a second 64-row chunk, many conflicts.  Image 1: 3 rows."""
    g = torch.Generator().manual_seed(N70_SEED)
    ann = torch.full((2, 70, 5), -1.0)
    for n in range(70):
        if n in (3, 20, 64, 69):
            continue
        wh = 14.0 + 50.0 * torch.rand(2, generator=g)
        xy = torch.rand(2, generator=g) * (126.0 - wh) + 1.0
        ann[0, n] = torch.cat([xy, xy + wh, torch.randint(0, 4, (1,), generator=g).float()])
    for n, box in enumerate(AC.SMALL_BOXES):
        ann[1, 2 * n] = torch.tensor(list(box) + [float(n)])
    return _with(LC._case(128, 4, ann, 1141), ('second_chunk', 'conflict', 'pads_between'))


S128_SEEDS = {4: 51, 80: 52}


def seeded(nc, seed, **tal):
    _, ann = O.synthetic_batch(2, 128, seed=S128_SEEDS[nc], num_classes=nc)
    return _with(LC._case(128, nc, ann, seed), ('seeded',), **tal)


CASES = {'hand': hand, 'straddle': straddle, 'whole': whole, 'narrow': narrow, 'few': few, 'nested': nested, 'dup': dup,
         'bad_label': bad_label, 'n70': n70,
         's128_nc4': functools.partial(seeded, 4, 1111), 's128_nc80': functools.partial(seeded, 80, 1102),
         'topk1': functools.partial(seeded, 4, 1103, topk=1), 'topk16': functools.partial(seeded, 80, 1104, topk=16),
         'alpha0': functools.partial(seeded, 4, 1105, alpha=0.0), 'beta0': functools.partial(seeded, 4, 1166, beta=0.0),
         'soft': functools.partial(seeded, 4, 1107, alpha=0.5, beta=2.0, topk=9)}


@functools.lru_cache(maxsize=None)
def get(name):
    """The case, built once; treat it as read-only."""
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 form's result (tests/tal_restated.assign) on the case; read-only."""
    c = get(name)
    return TR.assign(c, c['tal'])


@functools.lru_cache(maxsize=None)
def gaps(name):
    c = get(name)
    return TR.gaps(c, c['tal'])
