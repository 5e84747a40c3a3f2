"""Seeded inputs of the rescoring-NMS tests at the smallest sizes where the kernel can still go wrong.  The kernel runs one
1024-thread workgroup per image: 63 / 64 / 65 straddle a wave, 1023 / 1024 / 1025 the workgroup (a thread then owns a second
candidate), 3000 gives every thread three, and the top-N cap is met exactly and exceeded by one.

A case is a dict: name, boxes [B,A,4] f32, score [B,A] f32, label [B,A] int32, threshold, iou_threshold, pre_nms_top_n, max_det,
n (candidates per image, the largest over the batch)."""
import numpy as np

THR = 0.05


def _boxes(rng, A, extent=512.0, lo=8.0, hi=98.0):
    xy = rng.uniform(0, extent - lo, size=(A, 2))
    wh = rng.uniform(lo, hi, size=(A, 2))
    return np.concatenate([xy, xy + wh], 1).astype(np.float32)


def _scores(rng, A, n):
    """n candidates (distinct scores in (0.06, 1)) at random anchors, everything else at or below the threshold."""
    s = rng.uniform(0.0, THR, size=A).astype(np.float32)
    s[0] = np.float32(THR)                                            # exactly the threshold: not a candidate (the test is >)
    where = rng.permutation(np.arange(1, A))[:n]
    s[where] = rng.permutation(np.linspace(0.06, 0.999, max(n, 1)))[:n].astype(np.float32)
    return s


def _case(name, boxes, score, label, top_n, max_det, iou=0.5):
    boxes, score, label = np.asarray(boxes, np.float32), np.asarray(score, np.float32), np.asarray(label, np.int32)
    if boxes.ndim == 2:
        boxes, score, label = boxes[None], score[None], label[None]
    with np.errstate(invalid='ignore'):
        n = int((score > np.float32(THR)).sum(1).max())
    return dict(name=name, boxes=boxes, score=score, label=label, threshold=THR, iou_threshold=iou, pre_nms_top_n=top_n, max_det=max_det, n=n)


def _random(name, seed, n, top_n, max_det, A=None, extent=512.0):
    rng = np.random.default_rng(seed)
    A = A or max(n + 9, 16)
    return _case(name, _boxes(rng, A, extent), _scores(rng, A, n), rng.integers(0, 4, size=A), top_n, max_det)


def make_cases():
    cases = []
    for n in (0, 1, 2, 63, 64, 65, 1023, 1024, 1025):
        cases.append(_random('n%d' % n, 100 + n, n, 4096, 100))
    cases.append(_random('n64_top64', 1, 64, 64, 50))
    cases.append(_random('n65_top64', 2, 65, 64, 50))
    cases.append(_random('n1000_top1000', 3, 1000, 1000, 100))
    cases.append(_random('n1001_top1000', 4, 1001, 1000, 100))
    cases.append(_random('n3000_three_per_thread', 5, 3000, 4096, 100, extent=1024.0))
    cases.append(_random('n4100_top4096', 6, 4100, 4096, 100, A=4200, extent=1024.0))
    cases.append(_random('max_det_below_survivors', 7, 300, 1000, 10, extent=2048.0))         # sparse: far more than 10 survive
    # B = 3 with different counts per image, one of them empty
    rng = np.random.default_rng(8)
    A = 600
    cases.append(_case('batch3_500_0_37', np.stack([_boxes(rng, A) for _ in range(3)]),
                       np.stack([_scores(rng, A, 500), rng.uniform(0, THR, A).astype(np.float32), _scores(rng, A, 37)]),
                       rng.integers(0, 4, size=(3, A)), 1000, 100))
    # clusters of identical boxes
    rng = np.random.default_rng(9)
    cl = np.repeat(_boxes(rng, 20), 30, axis=0)
    cases.append(_case('identical_clusters', cl, rng.permutation(np.linspace(0.06, 0.99, 600)).astype(np.float32), rng.integers(0, 3, size=600), 1000, 100))
    # exact score ties (16 levels) on overlapping boxes: order by anchor index
    rng = np.random.default_rng(10)
    cases.append(_case('score_ties', _boxes(rng, 700, 256.0), (np.floor(rng.uniform(0, 1, 700) * 16) / 16).astype(np.float32),
                       rng.integers(0, 4, size=700), 1000, 100))
    # degenerate boxes and a NaN score among ordinary candidates
    rng = np.random.default_rng(11)
    b = _boxes(rng, 200, 128.0); s = rng.uniform(0.06, 0.99, 200).astype(np.float32)
    b[3, 2:] = b[3, :2]                                               # zero area
    b[5, 2] = b[5, 0]                                                 # zero width only
    b[7, 2] = b[7, 0] - 5.0                                           # negative area
    b[9, 2:] = b[9, :2] - 5.0                                         # inverted in x and y: positive product, no overlap with anything
    b[11, 2] = np.inf; b[13, 0] = -np.inf; b[13, 2] = np.inf          # infinite area
    b[15] = [0.0, 0.0, 3.0e19, 3.0e19]                                # finite coordinates, fp32 area overflows
    b[17] = np.nan
    b[19] = b[21] = [np.inf, 0.0, np.inf, 10.0]                       # inf - inf = NaN area, twice
    s[23] = np.nan; s[27] = -np.inf
    s[[3, 11, 15, 19]] = [0.995, 0.994, 0.993, 0.992]                 # degenerate boxes are picked early: they must rescore nothing
    cases.append(_case('degenerate_and_nan', b, s, rng.integers(0, 2, size=200), 1000, 100))
    # two classes on identical boxes: class-aware keeps both of a pair, class-agnostic one
    rng = np.random.default_rng(12)
    pairs = np.repeat(_boxes(rng, 6, 4096.0, 8.0, 16.0), 2, axis=0)
    cases.append(_case('two_classes_identical_boxes', pairs, np.linspace(0.9, 0.2, 12).astype(np.float32), np.tile([0, 1], 6), 1000, 100))
    return cases


CASES = make_cases()
