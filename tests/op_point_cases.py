"""Cases of the operating-point metrics (include/effdet_op_point.h), shared by tests/test_op_point_host.py and
tests/test_gpu_op_point.py: hand cases whose expected tables are literals, and seeded builders at the smallest shapes where the
kernels' loops loop.  A curves case is dict(name, C, dets [B, max_det, 6] fp32 or None, counts, gts, thresholds (None = the default
grid), iou, expect or None); a confusion case is dict(name, C, dets, counts, gts, conf, iou, expect or None).  Every image's rows are
score-descending, as effdet_finalize_dets writes them."""
import numpy as np

HIT, NEAR, OFF = 0.0, 2.0, 5.0                  # x shift of a 10 x 10 box against its GT cell: IoU 1, 2 / 3, 1 / 3


def _cell(i, shift=0.0):
    return [20.0 * i + shift, 0.0, 20.0 * i + 10.0 + shift, 10.0]


def _pack(images, max_det):
    """images: per image a list of rows (x1, y1, x2, y2, score, label) -> (dets [B, max_det, 6] fp32 with label -1 padding, counts)."""
    dets = np.zeros((len(images), max_det, 6), dtype=np.float32)
    dets[:, :, 5] = -1
    counts = np.zeros(len(images), dtype=np.int32)
    for b, rows in enumerate(images):
        rows = sorted(rows, key=lambda r: -np.float32(r[4]))          # stable: score-descending, ties in the given order
        counts[b] = len(rows)
        if rows:
            dets[b, :len(rows)] = np.asarray(rows, dtype=np.float64)
    return dets, counts


def device_gt(gts, C):
    """B arrays [g, 5] -> (boxes fp64 [B, G, 4], labels int32 [B, G]) with G >= 1, padding and labels that are no integer of [0, C) as
    -1: what evaluate.VOCMeanAP hands the kernels."""
    G = max([1] + [len(np.asarray(g).reshape(-1, 5)) for g in gts])
    boxes = np.zeros((len(gts), G, 4), dtype=np.float64)
    labels = np.full((len(gts), G), -1, dtype=np.int32)
    for b, g in enumerate(gts):
        g = np.asarray(g, dtype=np.float64).reshape(-1, 5)
        lab = g[:, 4]
        ok = (lab >= 0) & (lab < C) & (lab == np.floor(lab))
        boxes[b, :len(g)] = g[:, :4]
        labels[b, :len(g)] = np.where(ok, lab, -1).astype(np.int32)
    return boxes, labels


# ------------------------------------------------------------------------------------------------ curves
def _curves_hand():
    images = [[_cell(0) + [0.9, 0], _cell(0) + [0.8, 0], _cell(1) + [0.6, 1]],          # TP, duplicate (FP), TP
              [[50, 50, 60, 60, 0.4, 0], _cell(0) + [0.3, 0]]]                            # FP, TP
    gts = [np.array([_cell(0) + [0], _cell(1) + [1]], dtype=np.float64), np.array([_cell(0) + [0]], dtype=np.float64)]
    dets, counts = _pack(images, 4)
    expect = {
        'tp': [[2, 1, 1, 0], [1, 1, 0, 0]],
        'npred': [[4, 2, 1, 0], [1, 1, 0, 0]],
        'precision': [[0.5, 0.5, 1.0, 1.0], [1.0, 1.0, 1.0, 1.0]],
        'recall': [[1.0, 0.5, 0.5, 0.0], [1.0, 1.0, 0.0, 0.0]],
        'f1': [[0.6666666666666666, 0.5, 0.6666666666666666, 0.0], [1.0, 1.0, 0.0, 0.0]],
        'mean': [[0.75, 0.75, 1.0, 1.0], [1.0, 0.75, 0.25, 0.0], [0.8333333333333333, 0.75, 0.3333333333333333, 0.0]],
        'best': [[0.0, 0.5, 1.0, 0.6666666666666666], [0.0, 1.0, 1.0, 1.0], [0.0, 0.75, 1.0, 0.8333333333333333]],   # class 0: j = 0 ties j = 2
    }
    return dict(name='hand', C=2, dets=dets, counts=counts, gts=gts, thresholds=[0.25, 0.5, 0.85, 0.95], iou=0.5, expect=expect)


def _scene(rng, B, max_det, per_class, gt_classes, C, score_levels):
    """per_class[c] records of class c dealt over B images; every image has 8 GT cells labelled from gt_classes; a detection sits on a
    random cell (exactly, near or off it) or nowhere; scores are multiples of 1 / score_levels (ties within and across images)."""
    labels = np.concatenate([np.full(n, c) for c, n in enumerate(per_class)]).astype(np.int64)
    rng.shuffle(labels)
    parts = np.array_split(labels, B)
    assert max(len(p) for p in parts) <= max_det
    images, gts = [], []
    for part in parts:
        glab = rng.choice(gt_classes, 8)
        gts.append(np.array([_cell(i) + [glab[i]] for i in range(8)], dtype=np.float64))
        rows = []
        for c in part:
            i = rng.randint(0, 8)
            kind = rng.randint(0, 4)
            box = [300.0, 300.0, 320.0, 330.0] if kind == 3 else _cell(i, (HIT, NEAR, OFF)[kind])
            rows.append(box + [rng.randint(1, score_levels) / score_levels, c])
        images.append(rows)
    dets, counts = _pack(images, max_det)
    return dets, counts, gts


def _curves_chunks():
    rng = np.random.RandomState(11)
    # class 0: GT but no records; 1..5: the scan's carry (1, 255, 256, 257, 513 records); 6: records but no GT; 7: neither
    per_class = [0, 1, 255, 256, 257, 513, 40, 0]
    dets, counts, gts = _scene(rng, 6, 256, per_class, [0, 1, 2, 3, 4, 5], 8, 500)
    return dict(name='chunks', C=8, dets=dets, counts=counts, gts=gts, thresholds=[0.0, 0.1, 0.25, 0.5, 0.75, 0.9, 0.998], iou=0.5,
                expect=None, per_class=per_class)


def _curves_ties():
    rng = np.random.RandomState(12)
    # class 0 sorted: 200 records at 0.875, then a run of 120 at 0.5 (positions 200..319: across 256), then 50 at 0.125
    # (each score level aims at cells of its own, so that TPs and FPs mix inside the run on both sides of position 256)
    images = [[] for _ in range(16)]
    for score, n, cells in ((0.875, 200, (0, 1, 2)), (0.5, 120, (3, 4, 5)), (0.125, 50, (6, 7))):
        for q in range(n):
            i = cells[rng.randint(0, len(cells))]
            images[q % 16].append(_cell(i, (HIT, OFF)[rng.randint(0, 2)]) + [score, 0])
    for q in range(9):
        images[q % 16].append(_cell(8) + [0.5, 1])
    gts = [np.array([_cell(i) + [0 if i < 8 else 1] for i in range(9)], dtype=np.float64) for _ in range(16)]
    dets, counts = _pack(images, 32)
    below = float(np.nextafter(np.float32(0.5), np.float32(0.0)))
    return dict(name='ties', C=2, dets=dets, counts=counts, gts=gts, thresholds=[0.125, below, 0.5, 0.875], iou=0.5, expect=None,
                run=(200, 320))


def _curves_tiles():
    rng = np.random.RandomState(13)
    dets, counts, gts = _scene(rng, 3, 1024, [30, 25, 20], [0, 1, 2], 3, 64)
    return dict(name='tiles', C=3, dets=dets, counts=counts, gts=gts, thresholds=[0.05, 0.3, 0.5, 0.7, 0.95], iou=0.5, expect=None)


def _curves_extremes():
    rng = np.random.RandomState(14)
    dets, counts, gts = _scene(rng, 2, 64, [40, 30], [0, 1], 2, 2048)
    grid = ((np.arange(4096) - 1024) / 2048).astype(np.float32)    # -0.5 .. 1.4995 in exact steps: below and above every score, 0.0 too
    zero = [[_cell(0) + [0.5, 0], _cell(1) + [0.0, 0], _cell(2, OFF) + [0.0, 0]]]      # scores of +0.0 against the threshold 0.0
    zd, zc = _pack(zero, 4)
    zg = [np.array([_cell(0) + [0], _cell(1) + [0]], dtype=np.float64)]
    expect = {'tp': [[1]], 'npred': [[1]], 'precision': [[1.0]], 'recall': [[0.5]], 'f1': [[0.6666666666666666]],
              'mean': [[1.0], [0.5], [0.6666666666666666]], 'best': [[0.0, 1.0, 0.5, 0.6666666666666666]] * 2}
    return [dict(name='extremes_m4096', C=2, dets=dets, counts=counts, gts=gts, thresholds=grid, iou=0.5, expect=None),
            dict(name='extremes_m1', C=1, dets=zd, counts=zc, gts=zg, thresholds=[0.0], iou=0.5, expect=expect)]


def _curves_empty():
    M = 1001
    expect = {'tp': np.zeros((3, M), dtype=np.int32), 'npred': np.zeros((3, M), dtype=np.int32), 'precision': np.ones((3, M)),
              'recall': np.zeros((3, M)), 'f1': np.zeros((3, M)), 'mean': np.zeros((3, M)), 'best': [[-1.0, 0.0, 0.0, 0.0]] * 4}
    return dict(name='empty', C=3, dets=None, counts=None, gts=[], thresholds=None, iou=0.5, expect=expect)


CURVES_CASES = [_curves_hand(), _curves_chunks(), _curves_ties(), _curves_tiles()] + _curves_extremes() + [_curves_empty()]


# ------------------------------------------------------------------------------------------------ confusion
def _confusion_hand():
    # both predictions prefer object 0 (IoU 1.0 and 0.8); the loser's second candidate, object 1 (IoU 0.5), stays unmatched
    images = [[[0, 0, 10, 10, 0.9, 0], [0, 0, 10, 8, 0.8, 1]]]
    gts = [np.array([[0, 0, 10, 10, 0], [0, 0, 10, 16, 1]], dtype=np.float64)]
    dets, counts = _pack(images, 2)
    return dict(name='hand', C=2, dets=dets, counts=counts, gts=gts, conf=0.25, iou=0.45, expect=[[1, 0, 0], [0, 0, 1], [0, 1, 0]])


def _confusion_labels():
    images = [[_cell(0) + [0.9, 1], _cell(1, NEAR) + [0.8, 2], _cell(2) + [0.7, 0]]]
    gts = [np.array([_cell(0) + [0], _cell(1) + [2], _cell(2) + [1]], dtype=np.float64)]
    dets, counts = _pack(images, 3)
    return dict(name='labels', C=3, dets=dets, counts=counts, gts=gts, conf=0.25, iou=0.45,
                expect=[[0, 1, 0, 0], [1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 0]])


def _confusion_threshold():
    # image 0: IoU exactly 0.5 (100 / 200) against iou 0.5: no candidate; image 1: a score equal to conf is no prediction
    images = [[[0, 0, 10, 10, 0.9, 0]], [_cell(0) + [0.25, 1], _cell(1) + [0.5, 1]]]
    gts = [np.array([[0, 0, 10, 20, 0]], dtype=np.float64), np.array([_cell(0) + [1], _cell(1) + [1]], dtype=np.float64)]
    dets, counts = _pack(images, 2)
    return dict(name='threshold', C=2, dets=dets, counts=counts, gts=gts, conf=0.25, iou=0.5, expect=[[0, 0, 1], [0, 1, 0], [1, 1, 0]])


def _confusion_duplicates():
    # image 0: two identical GT boxes, the first row wins; image 1: two identical predictions, the lower row wins
    images = [[_cell(0) + [0.9, 2]], [_cell(3) + [0.6, 0], _cell(3) + [0.6, 1]]]
    gts = [np.array([_cell(0) + [0], _cell(0) + [1]], dtype=np.float64), np.array([_cell(3) + [2]], dtype=np.float64)]
    dets, counts = _pack(images, 2)
    return dict(name='duplicates', C=3, dets=dets, counts=counts, gts=gts, conf=0.25, iou=0.45,
                expect=[[0, 0, 1, 0], [0, 0, 0, 1], [1, 0, 0, 0], [0, 1, 0, 0]])


def _confusion_padded():
    # image 0: no predictions (counts 0) but objects; image 1: predictions, every GT row padding; image 2: labels out of range and
    # non-integer on both sides (rows past counts are never read: image 0's slots hold a row that would match)
    C = 2
    images = [[], [_cell(0) + [0.9, 0], _cell(1) + [0.8, 1]],
              [_cell(0) + [0.9, 2], _cell(1) + [0.8, -1], _cell(2) + [0.7, 0.5], _cell(3) + [0.6, 1]]]
    gts = [np.array([_cell(0) + [0], _cell(1) + [1]], dtype=np.float64), np.zeros((0, 5)),
           np.array([_cell(0) + [2], _cell(1) + [-1], _cell(2) + [0.5], _cell(3) + [0]], dtype=np.float64)]
    dets, counts = _pack(images, 4)
    dets[0, 0] = _cell(0) + [0.9, 0]
    return dict(name='padded', C=C, dets=dets, counts=counts, gts=gts, conf=0.25, iou=0.45, expect=[[0, 0, 1], [1, 0, 1], [1, 1, 0]])


def _boxes(rng, n):
    """n boxes on a coarse integer grid: small integers make equal IoUs (ties) common"""
    x = rng.randint(0, 12, n) * 4.0; y = rng.randint(0, 12, n) * 4.0
    return np.stack([x, y, x + rng.randint(2, 5, n) * 4.0, y + rng.randint(2, 5, n) * 4.0], 1)


def _confusion_seeded(name, seed, C, shapes, max_det):
    """shapes: per image (predictions, GT rows)"""
    rng = np.random.RandomState(seed)
    images, gts = [], []
    for P, Gn in shapes:
        g = _boxes(rng, Gn)
        gts.append(np.concatenate([g, rng.randint(0, C, (Gn, 1)).astype(np.float64)], 1))
        src = g[rng.randint(0, Gn, P)] if Gn else _boxes(rng, P)
        own = rng.rand(P) < 0.7
        bx = np.where(own[:, None], src + rng.randint(-1, 2, (P, 4)) * 4.0 * (rng.rand(P, 1) < 0.5), _boxes(rng, P))
        sc = rng.randint(1, 64, P) / 64.0                             # some at exactly conf = 0.25
        lab = rng.randint(0, C, P)
        images.append([list(bx[k]) + [sc[k], lab[k]] for k in range(P)])
    dets, counts = _pack(images, max_det)
    return dict(name=name, C=C, dets=dets, counts=counts, gts=gts, conf=0.25, iou=0.45, expect=None)


CONFUSION_CASES = [_confusion_hand(), _confusion_labels(), _confusion_threshold(), _confusion_duplicates(), _confusion_padded(),
                   _confusion_seeded('random', 21, 5, [(40, 12), (25, 30), (0, 5), (33, 0)], 48),
                   # more than 256 predictions in one image, more than 256 GT rows in another, and G = 2048 (the LDS limit)
                   _confusion_seeded('loops', 22, 4, [(300, 9), (60, 300), (40, 2048)], 320)]
