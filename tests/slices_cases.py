"""Seeded cases of the cross-tile merge (include/effdet_slices.h: effdet_slice_merge), shared by the CPU tier (tests/test_slices_host.py)
and the GPU tier (tests/test_gpu_slices.py).  A case: name, score [B][TPI][R] fp32, label int64, boxes [B][TPI][R][4] in each tile's own
frame, count [B][TPI] int32, table (ops.slice_plan's records), W, H, max_det and opts (the restatement's keyword arguments).

Rows past a list's count hold decoys scoring 0.999: a kernel that read them would emit them first."""
import numpy as np

F = np.float32
TILE = 128


def table5():
    """Four 128 x 128 tiles over a 200 x 230 image (rows at 0 and 72, columns at 0 and 102) and the whole image as a fifth view."""
    return [(0, 0, TILE, TILE, 1.0, 1.0), (0, 102, TILE, TILE, 1.0, 1.0), (72, 0, TILE, TILE, 1.0, 1.0), (72, 102, TILE, TILE, 1.0, 1.0),
            (0, 0, TILE, TILE, float(F(200.0 / 128.0)), float(F(230.0 / 128.0)))]


def grid_table(TPI, W=1024, H=1024):
    """TPI unit tiles at scattered origins of a W x H image."""
    return [(int((j * 37) % max(H - TILE, 1)), int((j * 101) % max(W - TILE, 1)), TILE, TILE, 1.0, 1.0) for j in range(TPI)]


def _lists(rng, B, TPI, R, counts, centres=12, labels=3, quant=None, spread=6.0, size=(16.0, 48.0)):
    """Clustered boxes: every row picks one of `centres` objects of the tile frame and jitters it, so lists overlap within and across
    tiles.  counts [B][TPI]; scores descending per list (ties kept where quant makes them)."""
    score = np.full((B, TPI, R), 0.999, dtype=F)
    label = np.zeros((B, TPI, R), dtype=np.int64)
    boxes = np.zeros((B, TPI, R, 4), dtype=F)
    boxes[..., 2:] = 32.0                                             # (decoys are proper boxes)
    cx, cy = rng.uniform(8, TILE - 8, centres), rng.uniform(8, TILE - 8, centres)
    cw, ch = rng.uniform(*size, centres), rng.uniform(*size, centres)
    cl = rng.integers(0, labels, centres)
    for b in range(B):
        for j in range(TPI):
            n = int(min(max(counts[b][j], 0), R))
            if n == 0:
                continue
            s = rng.uniform(0.05, 0.95, n)
            if quant:
                s = np.round(s * quant) / quant
            k = rng.integers(0, centres, n)
            x, y = cx[k] + rng.normal(0, spread, n), cy[k] + rng.normal(0, spread, n)
            w_, h_ = cw[k] * rng.uniform(0.6, 1.2, n), ch[k] * rng.uniform(0.6, 1.2, n)
            score[b, j, :n] = np.sort(s.astype(F))[::-1]
            label[b, j, :n] = np.where(rng.uniform(size=n) < 0.85, cl[k], rng.integers(0, labels, n))
            boxes[b, j, :n] = np.stack([x - w_ / 2, y - h_ / 2, x + w_ / 2, y + h_ / 2], 1).astype(F)
    return score, label, boxes, np.asarray(counts, dtype=np.int32).reshape(B, TPI)


def _case(name, lists, table, W, H, max_det, **opts):
    s, l, b, c = lists
    return dict(name=name, score=s, label=l, boxes=b, count=c, table=table, W=float(W), H=float(H), max_det=int(max_det), opts=opts)


def _build():
    cases = []
    rng = np.random.default_rng(20260)
    base = _lists(rng, 1, 5, 64, [[60, 61, 59, 62, 58]])
    for method in ('nms', 'nmm'):
        for metric in ('iou', 'ios'):
            for aware in (True, False):
                cases.append(_case('%s_%s_%s' % (method, metric, 'aware' if aware else 'agnostic'), base, table5(), 230, 200, 300,
                                   method=method, metric=metric, class_aware=aware, thr=0.4))
    # equal scores across tiles and within a tile: sixteen score values over 250 rows
    cases.append(_case('tied_scores', _lists(rng, 1, 5, 64, [[50] * 5], quant=16), table5(), 230, 200, 250, thr=0.5))
    # the chain in one tile: A (0.9) absorbs B (0.8); B would have absorbed C (0.7) -- IoU(B, C) = 42 / 72 -- but is dead; IoU(A, C) is
    # 35 / 107 and the grown hull is never matched against, so C is its own keeper.  D sits in another tile and overlaps nothing.
    s = np.zeros((1, 2, 4), dtype=F); l = np.zeros((1, 2, 4), dtype=np.int64); b = np.zeros((1, 2, 4, 4), dtype=F)
    s[0, 0, :3] = (0.9, 0.8, 0.7); b[0, 0, :3] = ((0, 0, 10, 10), (0, 0, 12, 6), (0, 0, 12, 3.5))
    s[0, 1, :1] = 0.6; b[0, 1, 0] = (0, 0, 8, 8)
    cases.append(_case('chain', (s, l, b, np.asarray([[3, 1]], dtype=np.int32)), [(0, 0, TILE, TILE, 1.0, 1.0), (40, 40, TILE, TILE, 1.0, 1.0)],
                       200, 200, 8, method='nmm', metric='iou', thr=0.5))
    # max_det cuts the pass mid-way
    cases.append(_case('max_det_cuts', base, table5(), 230, 200, 7, thr=0.4))
    # counts of 0, below 0 and above R; decoys past the counts
    cases.append(_case('counts_out_of_range', _lists(rng, 2, 5, 32, [[0, -3, 40, 32, 5], [1000, 0, 0, -1, 31]]), table5(), 230, 200, 100, thr=0.5))
    # NaN, +Inf and -Inf scores among the rows (a list is then no longer sorted: the order is the keys')
    bad = tuple(a.copy() for a in _lists(rng, 1, 5, 64, [[40] * 5]))
    bad[0][0, 0, 3], bad[0][0, 1, 0], bad[0][0, 2, 7], bad[0][0, 4, 39] = np.nan, np.inf, -np.inf, np.nan
    cases.append(_case('nonfinite_scores', bad, table5(), 230, 200, 200, thr=0.5))
    # rows that clip to nothing: beyond the right and bottom edge of the image from the last tiles, negative from the first, x2 < x1
    deg = tuple(a.copy() for a in _lists(rng, 1, 5, 64, [[40] * 5]))
    deg[2][0, 3, 0] = (130, 10, 150, 30); deg[2][0, 3, 1] = (10, 129, 30, 140); deg[2][0, 0, 2] = (-30, -30, -1, -1)
    deg[2][0, 1, 3] = (50, 10, 40, 30); deg[2][0, 2, 4] = (20, 20, 20, 40); deg[2][0, 4, 5] = (np.nan, 0, 10, 10)
    cases.append(_case('degenerate_boxes', deg, table5(), 230, 200, 200, thr=0.5))
    # skip_thr equal to a run of tied scores: >= keeps the run
    cases.append(_case('skip_thr_at_a_tie', _lists(rng, 1, 5, 64, [[50] * 5], quant=8), table5(), 230, 200, 250, thr=0.5, skip_thr=0.5))
    # three images: many survivors, none, one
    c3 = _lists(rng, 3, 5, 64, [[64, 64, 64, 64, 64], [0, 0, 0, 0, 0], [0, 0, 1, 0, 0]])
    cases.append(_case('batch3_one_empty', c3, table5(), 230, 200, 300, thr=0.5))
    # survivor counts around the wave and the workgroup size
    for n, TPI, R in ((1, 1, 8), (63, 3, 32), (65, 5, 16), (1025, 5, 256)):
        counts = [[min(R, n - j * R) if n - j * R > 0 else 0 for j in range(TPI)]]
        if n == 1025:
            counts = [[205] * 5]
        cases.append(_case('n%d' % n, _lists(rng, 1, TPI, R, counts, centres=40), grid_table(TPI) if TPI != 5 else table5(),
                           1024 if TPI != 5 else 230, 1024 if TPI != 5 else 200, n, thr=0.5))
    # the cap: 32 tiles of 256 rows, every row a survivor; max_det bounds the rounds
    cases.append(_case('n8192', _lists(rng, 1, 32, 256, [[256] * 32], centres=300, spread=3.0, size=(6.0, 20.0)), grid_table(32), 1024, 1024, 1000,
                       thr=0.5))
    # the cap's slots with a few survivors
    few = [[0] * 32]
    few[0][0], few[0][17], few[0][31] = 3, 1, 2
    cases.append(_case('n8192_few_alive', _lists(rng, 1, 32, 256, few), grid_table(32), 1024, 1024, 300, thr=0.5))
    return cases


CASES = _build()


def _model_images():
    import torch
    return torch.randn(2, 3, 600, 850, generator=torch.Generator().manual_seed(3))


# the model-level test (tests/test_gpu_slices_model.py) and its CPU fixture check: B = 2 of 600 x 850 (multiples of nothing), 3 x 5 tiles
# and the full view
MODEL_CASE = dict(images=_model_images, slice=(256, 256), overlap=(0.25, 0.25), tile_batch=8, top_n=200, max_det=300)
