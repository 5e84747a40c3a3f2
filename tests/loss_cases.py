"""Shared inputs of the detection-loss edge tests (tests/test_loss_cases_host.py on the CPU, tests/test_gpu_loss_edges.py on the
device): one builder per branch of loss.hip that the synthetic 8-row batches never reach.  A case is a dict
  S, cls [B, A, nc] (probabilities), reg [B, A, 4], anc [1, A, 4], ann [B, N, 5] (pad rows label == -1)  -- all fp32 CPU tensors --
  expect: [(image, anchor, state, row)] hand-derived from the construction: state POS / NEG / IGN, row = the annotation row a
          positive anchor is assigned (its label is ann[image, row, 4]);
  expect_all: {image: state} where the construction fixes the state of EVERY anchor of the image;
  state_check: 'exact' -- the device's state of every anchor must equal the fp64 oracle's; 'skip' -- the same except on the
          near-threshold / near-tie anchors of skip_mask(); None -- no per-anchor comparison (losses and gradients only).
States are also available from the oracle in any precision through oracle_states()."""
import functools

import numpy as np
import torch

from oracle import effdet_oracle as O

POS, NEG, IGN = 'pos', 'neg', 'ign'
CODE_IGN, CODE_NEG = -2, -1                          # loss.hip's per-anchor code: -2 ignored, -1 negative, >= 0 the annotation row

# loss.hip constants the host test recomputes launch sizes from
CHUNK = 64                                           # annotation rows compacted into LDS per pass of loss_assign_kernel
CLS_IT, FG_IT = 8, 4                                 # 4-element groups per thread: loss_cls_kernel / loss_cls_pix_kernel (forward + gradient)
LANE_SUM_CHAINS = 192                                # loss_final_kernel's four-chain loop runs while i + 192 < n


def dld_for(nc):
    return (9 * nc + 63) // 64 * 64


def ncb_fwd(A, nc):
    """Workgroups (= partial sums) per image of loss_cls_kernel."""
    groups = (A * nc + 3) // 4
    return (groups + 256 * CLS_IT - 1) // (256 * CLS_IT)


def ncb_fwd_grad(A, nc):
    """Workgroups per image of the forward + gradient loss_cls_pix_kernel at the padded pitch dld_for(nc)."""
    groups = (A // 9) * dld_for(nc) // 4
    return (groups + 256 * FG_IT - 1) // (256 * FG_IT)


@functools.lru_cache(maxsize=None)
def anchors(S):
    return O.anchors_for_image(S, S)


def int_anchor(y, x):
    """Index at S=128 of the ratio-1 scale-1 level-3 anchor of pixel (y, x): the 32 x 32 square centred on (8x+4, 8y+4), all four
    coordinates integers (order: level, y, x, ratio-major, scale-minor -> slot 3 of the pixel's 9)."""
    return 9 * (y * 16 + x) + 3


def _cls_reg(B, A, nc, seed):
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(B, A, nc, generator=g) * 2.0).clamp(-6.0, 6.0)      # inside the clamp: every live gradient is non-zero
    return torch.sigmoid(logits), torch.randn(B, A, 4, generator=g) * 0.5


def _case(S, nc, ann, seed, anc=None, expect=(), expect_all=None, state_check='exact'):
    anc = anchors(S) if anc is None else anc
    cls, reg = _cls_reg(ann.shape[0], anc.shape[1], nc, seed)
    return {'S': S, 'cls': cls, 'reg': reg, 'anc': anc, 'ann': ann.float(), 'expect': list(expect), 'expect_all': expect_all or {},
            'state_check': state_check}


def _random_boxes(rng, n, S, lo=10.0, hi=70.0):
    """n boxes with fractional fp32 coordinates inside [0, S)."""
    wh = rng.uniform(lo, hi, (n, 2))
    xy = rng.uniform(0.0, S - 1.0, (n, 2)) - 0.3 * wh
    b = np.concatenate([xy, xy + wh], 1).clip(0.0, S - 1.0)
    return torch.from_numpy(b.astype(np.float32))


# --------------------------------------------------------------------------- the cases
def chunks():
    """Three 64-row chunks (N = 130), valid rows scattered between pad rows, A*nc odd (the scalar tail of the class kernels).
    Image 0: 90 valid rows scattered over all 130.  Image 1: rows 64..127 all pad (a chunk without a valid row), 40 valid rows
    scattered over 0..63 and both rows of the last chunk valid."""
    S, nc, N = 128, 5, 130
    rng = np.random.RandomState(7)
    ann = torch.full((2, N, 5), -1.0)
    rows0 = np.sort(rng.permutation(N)[:90])
    rows1 = np.concatenate([np.sort(rng.permutation(64)[:40]), [128, 129]])
    for b, rows in enumerate((rows0, rows1)):
        ann[b, rows, :4] = _random_boxes(rng, len(rows), S)
        ann[b, rows, 4] = torch.from_numpy(rng.randint(0, nc, len(rows)).astype(np.float32))
    return _case(S, nc, ann, 101, state_check='skip')


TIE_VARIANTS = {64: 63, 65: 64, 72: 70}              # N -> the later row: last of the only chunk / alone in chunk 2 / row 70


def chunk_ties(N):
    """First-argmax across the chunk boundary.  Image 0: rows 3 and `late` hold the SAME box with different labels -> row 3 wins
    on every anchor either reaches.  Image 1 (the mirror): row 3 holds a box of IoU 17/32 with the target anchor, row `late` the
    anchor itself (IoU 1) -> row `late` wins there.  Pad rows and far-away boxes in between."""
    S, nc, late = 128, 6, TIE_VARIANTS[N]
    t = int_anchor(8, 8)                                               # (52, 52, 84, 84)
    ann = torch.full((2, N, 5), -1.0)
    ann[:, 1] = torch.tensor([2.5, 3.25, 30.0, 40.5, 4.0])             # filler rows far from the target anchor, pads around them
    ann[:, 5] = torch.tensor([90.25, 4.0, 126.0, 37.5, 5.0])
    if late - 1 > 5:
        ann[:, late - 1] = torch.tensor([3.0, 88.5, 41.0, 125.0, 3.0])
    ann[0, 3] = torch.tensor([50.5, 51.25, 85.0, 83.5, 1.0]); ann[0, late] = ann[0, 3]; ann[0, late, 4] = 2.0
    ann[1, 3] = torch.tensor([52.0, 52.0, 84.0, 69.0, 1.0]); ann[1, late] = torch.tensor([52.0, 52.0, 84.0, 84.0, 2.0])
    return _case(S, nc, ann, 200 + N, expect=[(0, t, POS, 3), (1, t, POS, late)])


THRESHOLD_BOXES = [   # against the integer anchor (52, 52, 84, 84), area 1024; every product below is an exact integer in fp32.
    # 32 rows tall like the anchor and sticking out to the right: intersection (84 - x1) * 32.  (Not nested boxes: a box that
    # contains, or is contained in, the anchor also nests the pixel's ratio-0.5 / ratio-2 anchors, whose area is 1024 only up to
    # rounding -- they would land within 1e-7 of the same threshold, on either side of it.)
    ((60, 52, 100, 84), POS),     # 768 / (1024 + 1280 - 768) = 768 / 1536 = 0.5 exactly -> positive (>=)
    ((59, 52, 100, 84), POS),     # one column more: 800 / 1536 = 0.521
    ((61, 52, 100, 84), IGN),     # one column less: 736 / 1536 = 0.479
    ((60, 52, 112, 84), IGN),     # 768 / (1024 + 1664 - 768) = 768 / 1920 = float32(0.4) -> NOT < 0.4 -> ignored
    ((59, 52, 112, 84), IGN),     # 800 / 1920 = 0.417
    ((61, 52, 112, 84), NEG),     # 736 / 1920 = 0.383 -> negative
]


NESTED_THRESHOLD_BOXES = [   # the same two IoUs from nested boxes.  On the integer anchor they are as exact as above, but each image
    # also has up to five non-integer anchors within 2e-8 of the threshold (see THRESHOLD_BOXES): only the anchors outside
    # skip_mask() are compared on the device, and no loss (state_check 'skip').
    ((52, 52, 84, 68), POS),      # exactly the upper half of the anchor: 512 / 1024 = 0.5
    ((52, 52, 84, 69), POS),      # one row more: 544 / 1024
    ((52, 52, 84, 67), IGN),      # one row less: 480 / 1024 = 0.469
    ((52, 52, 84, 132), IGN),     # the anchor stretched from 32 to 80 tall: 1024 / 2560 = float32(0.4)
    ((52, 52, 84, 131), IGN),     # 79 tall: 1024 / 2528 = 0.405
    ((52, 52, 84, 133), NEG),     # 81 tall: 1024 / 2592 = 0.395
]


def thresholds(nested=False):
    """One image per box of THRESHOLD_BOXES (row 1 of 3, pads around it), label = the image index."""
    S, nc = 128, 6
    t = int_anchor(8, 8)
    boxes = NESTED_THRESHOLD_BOXES if nested else THRESHOLD_BOXES
    ann = torch.full((len(boxes), 3, 5), -1.0)
    expect = []
    for b, (box, state) in enumerate(boxes):
        ann[b, 1] = torch.tensor(list(box) + [b], dtype=torch.float32)
        expect.append((b, t, state, 1 if state == POS else None))
    return _case(S, nc, ann, 301, expect=expect, state_check='skip' if nested else 'exact')


TINY_ANCHORS = {100: (60.25, 60.25, 60.75, 60.75),   # the tiny box itself
                1500: (60.25, 60.25, 60.75, 60.875),  # a quarter taller: IoU 0.8 with the tiny box, 0.69 with the enclosing one
                3000: (60.2, 60.2, 60.8, 60.8)}       # the enclosing box itself


def tiny_box():
    """A 0.5 x 0.5 px box (row 2) and a 0.6 x 0.6 one enclosing it (row 0): the regression target's gw = max(gw, 1) clamp.  No
    anchor of the model's table (sides >= 22 px) can reach IoU 0.5 with a sub-pixel box, so three entries of the table are replaced
    by sub-pixel anchors -- the C ABI takes any [A, 4] table.  Anchors 100 and 1500 must pick the tiny box (IoU 1 / 0.8 against
    0.69 / 0.69 for the near-duplicate), anchor 3000 the enclosing one; every other anchor is negative."""
    S, nc = 128, 4
    anc = anchors(S).clone()
    for i, a in TINY_ANCHORS.items():
        anc[0, i] = torch.tensor(a)
    ann = torch.full((1, 4, 5), -1.0)
    ann[0, 0] = torch.tensor([60.2, 60.2, 60.8, 60.8, 3.0])
    ann[0, 2] = torch.tensor([60.25, 60.25, 60.75, 60.75, 1.0])
    return _case(S, nc, ann, 401, anc=anc, expect=[(0, 100, POS, 2), (0, 1500, POS, 2), (0, 3000, POS, 0)])


TAIL_NC = (1, 3, 7, 6)                               # A*nc % 4 at A = 3069: 1, 3, 3, 2


def tails(nc):
    """A*nc not a multiple of 4: loss_cls_kernel / loss_bwd_cls_kernel take scalar loads and stores on every group."""
    S = 128
    _, ann = O.synthetic_batch(2, S, seed=20 + nc, num_classes=nc)
    return _case(S, nc, ann, 500 + nc, state_check=None)


def many_images():
    """B = 18 > the 16 waves of loss_final_kernel.  Image 16 has no annotations (all ignored, no loss); image 17 has one 4 x 4 box
    (IoU < 0.02 with every anchor: all negative, no positive)."""
    S, nc = 128, 4
    _, ann = O.synthetic_batch(18, S, seed=31, num_classes=nc)
    ann[16] = -1.0
    ann[17] = -1.0
    ann[17, 2] = torch.tensor([60.3, 60.7, 64.3, 64.7, 1.0])
    return _case(S, nc, ann, 601, expect_all={16: IGN, 17: NEG})


MANY_PARTIALS = {'fwd_grad': (256, 2), 'fwd': (384, 1)}     # path -> (S, B) at nc = 80


def many_partials(path):
    """More than 192 per-image class partials, so loss_final_kernel's four-chain loop runs: 'fwd_grad' sizes it for
    focal_loss_fwd_grad (256 partials), 'fwd' for focal_loss_fwd (270)."""
    S, B = MANY_PARTIALS[path]
    nc = 80
    _, ann = O.synthetic_batch(B, S, seed=41, num_classes=nc)
    return _case(S, nc, ann, 701, state_check=None)


CASES = {'chunks': chunks, 'thresholds': thresholds, 'thresholds_nested': functools.partial(thresholds, True), 'tiny_box': tiny_box, 'many_images': many_images}
CASES.update({'chunk_ties_N%d' % n: functools.partial(chunk_ties, n) for n in TIE_VARIANTS})
CASES.update({'tails_nc%d' % nc: functools.partial(tails, nc) for nc in TAIL_NC})
CASES.update({'many_partials_%s' % p: functools.partial(many_partials, p) for p in MANY_PARTIALS})


# --------------------------------------------------------------------------- oracle views of a case
def oracle_iou(case, b, dtype):
    """-> (iou [A, valid rows], rows [valid rows] original row indices) of image b through the oracle's calc_iou in dtype."""
    ann = case['ann'][b]
    rows = torch.nonzero(ann[:, 4] != -1).reshape(-1)
    return O.calc_iou(case['anc'][0].to(dtype), ann[rows, :4].to(dtype)), rows


def oracle_states(case, dtype):
    """-> int64 [B, A]: loss.hip's code per anchor (CODE_IGN / CODE_NEG / assigned annotation row) by the oracle's rule in dtype:
    first argmax, positive >= 0.5, negative < 0.4; an image without annotations takes no part in the loss (all ignored)."""
    B, A = case['cls'].shape[:2]
    code = torch.full((B, A), CODE_IGN, dtype=torch.int64)
    for b in range(B):
        iou, rows = oracle_iou(case, b, dtype)
        if len(rows) == 0:
            continue
        best, arg = iou.max(dim=1)
        code[b, best < 0.4] = CODE_NEG
        pos = best >= 0.5
        code[b, pos] = rows[arg[pos]]
    return code


def skip_mask(case, margin=1e-6):
    """-> bool [B, A]: anchors whose fp64 best IoU lies within `margin` of a threshold, or whose two best fp64 IoUs differ by less
    than `margin` -- the only anchors where fp32 rounding (or FMA contraction) may legitimately change the state or the row."""
    B, A = case['cls'].shape[:2]
    skip = torch.zeros(B, A, dtype=torch.bool)
    for b in range(B):
        iou, rows = oracle_iou(case, b, torch.float64)
        if len(rows) == 0:
            continue
        top = iou.topk(min(2, len(rows)), dim=1)[0]
        skip[b] = ((top[:, 0] - 0.4).abs() < margin) | ((top[:, 0] - 0.5).abs() < margin)
        if len(rows) > 1:
            skip[b] |= (top[:, 0] - top[:, 1]) < margin
    return skip


def state_code(state, row):
    return {POS: row, NEG: CODE_NEG, IGN: CODE_IGN}[state]
