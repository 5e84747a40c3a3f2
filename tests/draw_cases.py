"""Seeded cases of the device renderer (include/effdet_draw.h): frames, rows, counts, ids, scales, names, palette and options, built the
same way for the CPU tier (tests/test_draw_host.py: what the table reaches) and the GPU tier (tests/test_gpu_draw.py: exact bytes
against tests/draw_restated.py).  expected() paints a case once with the restatement and keeps the result."""
import numpy as np

from tests import draw_restated as R

TILE_W, TILE_H = 64, 16                                  # EFFDET_DRAW_TILE_W, _TILE_H (tests/test_draw_host.py holds them to the header)
ODD, EVEN, TILE = (37, 70), (64, 128), (TILE_H + 1, 2 * TILE_W + 3)      # W * 3 = 210 is no multiple of 4; partial tiles on both axes
NAMES = [b'aeroplane', b'bicycle', b'bird', b'boat', b'bottle', b'bus', b'car', b'cat']
PALETTE = np.array([[255, 0, 0], [0, 255, 0], [20, 20, 60], [250, 250, 210], [0, 102, 255], [223, 128, 255], [179, 255, 179]], dtype=np.uint8)
OPTS = dict(thickness=2, fill_alpha=0, label=True, show_score=True, show_id=False, text_scale=2, color_by='label')
nan, inf = float('nan'), float('inf')


def r(x1, y1, x2, y2, score=0.5, label=0.0):
    return [x1, y1, x2, y2, score, label]


def _build(seed, sizes, per_frame, counts=None, ids=None, scale=None, names=NAMES, S=6, K=None, mixed=False, tags=(), **opts):
    rng = np.random.RandomState(seed)
    B = len(sizes)
    assert mixed or len(set(sizes)) == 1                  # one [B, H, W, 3] block unless the case goes through (src, src_off, src_hw)
    K = max(1, max(len(p) for p in per_frame)) if K is None else K
    rows = np.zeros((B, K, S), dtype=np.float32)
    rows[:, :, 5] = -1.0                                  # padding rows as finalize_dets writes them
    for b, p in enumerate(per_frame):
        for k, row in enumerate(p[:K]):
            rows[b, k, :6] = row
            if S > 6:
                rows[b, k, 6:] = rng.uniform(0, 50, S - 6)
    o = dict(OPTS)
    o.update(opts)
    return dict(sizes=list(sizes), frames=[rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in sizes], rows=rows,
                counts=np.array([len(p) for p in per_frame] if counts is None else counts, dtype=np.int32),
                ids=None if ids is None else np.asarray(ids, dtype=np.int32).reshape(B, K),
                scale=None if scale is None else np.asarray(scale, dtype=np.float32).reshape(B, 2), names=names, palette=PALETTE,
                opts=o, mixed=mixed, max_hw=(max(h for h, _ in sizes), max(w for _, w in sizes)), tags=tuple(tags))


def _borders():
    rows = []
    for d in (-1, 0, 1):
        rows += [r(TILE_W + d, 3, TILE_W + 30 + d, 12, 0.9, 1), r(30, 5, TILE_W + d, 14, 0.8, 2), r(10, TILE_H + d, 40, TILE_H + 20 + d, 0.7, 3),
                 r(5, 2, 20, TILE_H + d, 0.6, 4), r(2 * TILE_W + d, 1, 2 * TILE_W + 2 + d, 9, 0.5, 5), r(100, TILE_H - 1 + d, 126, TILE_H + d, 0.4, 6)]
    return rows


def _pile(seed, n, S):
    rng = np.random.RandomState(seed)
    x, y = rng.randint(0, 40, n) + 0.5, rng.randint(0, 11, n) + 0.25
    return [r(x[i], y[i], x[i] + rng.randint(0, 20), y[i] + rng.randint(0, 5), rng.uniform(), rng.randint(0, 10)) for i in range(n)]


def _stack():
    return [r(5 + 6 * i, 4 + 3 * i, 45 + 6 * i, 24 + 3 * i, 0.3 + 0.1 * i, i) for i in range(5)] + [r(60, 10, 69, 36, 0.5, 6)]


BIG = 2 ** 31 - 1
CASES = {
    'borders_t1_tile': lambda: _build(1, [TILE], [_borders()], thickness=1, text_scale=1),
    'borders_t1_even': lambda: _build(1, [EVEN] * 2, [_borders(), _borders()[::-1]], thickness=1, text_scale=1),
    'borders_t2_tile': lambda: _build(2, [TILE], [_borders()], thickness=2, label=False),
    'borders_t2_even': lambda: _build(2, [EVEN], [_borders()], thickness=2, label=False),
    'outside': lambda: _build(3, [ODD], [[r(-30, -20, 10, 10, 0.9, 0), r(60, 30, 200, 100, 0.8, 1), r(-50, -50, -10, -10, 0.7, 2), r(100, 100, 120, 120, 0.6, 3),
                                          r(30, 20, 20, 25, 0.5, 4), r(25, 30, 45, 29, 0.5, 4), r(15, 15, 15, 15, 0.4, 5), r(40, 10, 40, 30, 0.3, 6),
                                          r(-1e9, 5, 1e9, 8, 0.2, 7), r(66, 28, 69, 36, 0.95, 0), r(2, 2, 30, 12, 0.85, 1)]],
                                 text_scale=1, tags=('outside', 'inside', 'shifted')),
    'thick16': lambda: _build(4, [EVEN], [[r(20, 20, 22, 22, 0.9, 0), r(50, 30, 90, 50, 0.8, 1), r(100, 8, 110, 40, 0.7, 2), r(120, 60, 127, 63, 0.6, 3)]],
                              thickness=16, text_scale=1),
    'thick5_small': lambda: _build(5, [ODD], [[r(10, 10, 11, 30, 0.9, 0), r(30, 5, 60, 8, 0.8, 1), r(40, 20, 44, 24, 0.7, 2), r(50, 28, 59, 36, 0.6, 3)]],
                                   thickness=5, label=False),
    't0_fill': lambda: _build(6, [ODD], [_stack()], thickness=0, fill_alpha=128, label=False),
    't0_label': lambda: _build(7, [ODD], [_stack()], thickness=0, text_scale=1),
    'nonfinite': lambda: _build(8, [ODD], [[r(nan, 5, 30, 20), r(5, 5, inf, 20), r(5, -inf, 30, 20), r(5, 5, 30, nan), r(8, 12, 40, 30, nan, 1), r(20, 14, 50, 33, inf, 2),
                                            r(30, 16, 60, 35, -inf, 3), r(1, 1, 60, 30, 0.9, -1.0), r(1, 1, 60, 30, 0.9, nan), r(3, 22, 20, 34, 0.5, 4)]], text_scale=1),
    'counts': lambda: _build(9, [ODD] * 4, [[r(5, 12, 30, 30, 0.9, 1), r(20, 15, 60, 35, 0.8, 2), r(40, 11, 66, 20, 0.7, 3)]] * 4, counts=[0, -3, 8, 2],
                             text_scale=1, tags=('count0',)),
    'alpha1': lambda: _build(10, [ODD], [_stack()], thickness=1, fill_alpha=1, text_scale=1),
    'alpha128': lambda: _build(11, [ODD], [_stack()], thickness=1, fill_alpha=128, text_scale=1),
    'alpha255': lambda: _build(12, [ODD], [_stack()], thickness=1, fill_alpha=255, label=False),
    'many100': lambda: _build(13, [ODD], [_pile(13, 100, 6)], thickness=1, fill_alpha=60, text_scale=1, tags=('over64',)),
    'pile1024': lambda: _build(14, [EVEN], [_pile(14, 1024, 8)], S=8, ids=np.random.RandomState(14).randint(1, 5000, 1024), thickness=1, fill_alpha=40,
                               text_scale=1, show_id=True, color_by='id', tags=('over256', 'empty')),
    'ids': lambda: _build(15, [EVEN], [[r(4, 12, 30, 20, 0.5, 0), r(40, 12, 60, 20, 0.6, 1), r(70, 12, 90, 20, 0.7, 2), r(4, 40, 30, 50, 0.8, 3),
                                        r(60, 40, 80, 50, 0.9, 4), r(100, 40, 110, 50, 0.9, 5)]], S=8, ids=[1, 9, 10, BIG, -5, 0], show_id=True,
                          color_by='id', text_scale=1),
    'ids_by_label': lambda: _build(16, [ODD], [[r(4, 12, 30, 20, 0.5, 0), r(20, 24, 60, 34, 0.6, 1)]], S=8, ids=[12, 345], show_id=True, show_score=False,
                                   text_scale=1),
    'pct': lambda: _build(17, [EVEN], [[r(2 + 40 * (i % 3), 10 + 18 * (i // 3), 30 + 40 * (i % 3), 16 + 18 * (i // 3), s, i % 8)
                                        for i, s in enumerate((0.0, 1.0, 0.004, 0.005, 0.995, 0.9949, -0.5, 7.0, 1e38))]], text_scale=1),
    'names': lambda: _build(18, [EVEN], [[r(2, 10, 20, 14, 0.11, 0), r(2, 24, 20, 28, 0.22, 1), r(2, 38, 20, 42, 0.33, 2), r(2, 52, 20, 56, 0.44, 3),
                                          r(70, 10, 90, 14, 0.55, 4), r(70, 24, 90, 28, 0.66, 5), r(70, 38, 90, 42, 0.77, 100000), r(70, 52, 90, 56, 0.88, 3e9),
                                          r(40, 30, 60, 34, 0.99, 1.9)]],
                            names=[b'0123456789abcdef', b'caf\xc3\xa9', b'', b'~tilde`', b'\x7f\x1f ok'], text_scale=1),
    'no_names': lambda: _build(19, [ODD], [[r(4, 12, 30, 20, 0.5, 0), r(20, 24, 60, 34, 0.6, 19)]], names=None, text_scale=1),
    'scale3': lambda: _build(20, [EVEN], [[r(4, 30, 60, 60, 0.87, 6), r(70, 5, 120, 40, 0.5, 7)]], text_scale=3),
    'scale8': lambda: _build(21, [EVEN], [[r(4, 2, 60, 60, 0.87, 6), r(90, 50, 120, 62, 0.5, 2)]], text_scale=8, tags=('inside', 'shifted')),
    'box_scale': lambda: _build(22, [ODD, ODD], [[r(10, 40, 80, 100, 0.9, 1), r(50.5, 20.3, 90.7, 60.9, 0.8, 2)]] * 2, scale=[[0.75, 0.3125], [1.0 / 3.0, 0.7]],
                                text_scale=1),
    'label_only': lambda: _build(23, [EVEN], [[r(70, 20, 90, 30, 0.9, 1)]], text_scale=1, tags=('label_only', 'one_row', 'empty')),
    'mixed': lambda: _build(24, [ODD, TILE, EVEN], [[r(5, 12, 30, 30, 0.9, 1), r(40, 11, 66, 20, 0.7, 3)], [r(60, 2, 100, 14, 0.5, 2), r(120, 12, 130, 16, 0.4, 0)],
                                                    [r(10, 20, 100, 50, 0.8, 5), r(64, 16, 127, 63, 0.6, 6), r(0, 0, 0, 0, 0.3, 7)]], S=8,
                            ids=[[3, 4, 0], [5, 6, 0], [7, 8, 9]], show_id=True, fill_alpha=90, text_scale=1, mixed=True),
    'mixed_default': lambda: _build(25, [EVEN, ODD, TILE], [[r(10, 20, 100, 50, 0.8, 5)], [r(5, 12, 30, 30, 0.9, 1)], [r(60, 2, 100, 14, 0.5, 2)]], mixed=True),
}
NAMES_OF_CASES = tuple(CASES)
_cache = {}


def case(name):
    if name not in _cache:
        _cache[name] = [CASES[name](), None]
    return _cache[name][0]


def paint_case(c, frames=None):
    """The restatement over every frame of c -> list of painted copies."""
    frames = c['frames'] if frames is None else frames
    return [R.paint(f.copy(), c['rows'][b], c['counts'][b], None if c['ids'] is None else c['ids'][b], None if c['scale'] is None else c['scale'][b],
                    c['names'], c['palette'], **c['opts']) for b, f in enumerate(frames)]


def expected(name):
    """The painted frames of a case, computed once and shared: do not write into them."""
    c = case(name)
    if _cache[name][1] is None:
        _cache[name][1] = paint_case(c)
        for f in _cache[name][1]:
            f.setflags(write=False)
    return _cache[name][1]


def tiles_touched(c, b):
    """The binning rule in plain Python: -> {(tile x, tile y): [(k, by box, by label), ...]} for frame b, over the tiles of its own H x W."""
    H, W = c['sizes'][b]
    ext = R.extents(c['rows'][b], c['counts'][b], W, None if c['ids'] is None else c['ids'][b], None if c['scale'] is None else c['scale'][b],
                    c['names'], **c['opts'])
    o = c['opts']
    out = {}
    for ty in range(-(-H // TILE_H)):
        for tx in range(-(-W // TILE_W)):
            x0, y0, x1, y1 = tx * TILE_W, ty * TILE_H, min(tx * TILE_W + TILE_W, W) - 1, min(ty * TILE_H + TILE_H, H) - 1

            def hits(q):
                return q is not None and q[0] <= x1 and q[2] >= x0 and q[1] <= y1 and q[3] >= y0
            out[(tx, ty)] = [(k, hits(box) and (o['thickness'] > 0 or o['fill_alpha'] > 0), hits(lab)) for k, box, lab, _, _ in ext if hits(box) or hits(lab)]
    return out
