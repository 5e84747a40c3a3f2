"""Seeded cases of the Mosaic / MixUp stage shared by tests/test_mosaic_host.py (CPU: every case reaches what it is tagged with) and
tests/test_gpu_mosaic.py (the kernels against tests/mosaic_restated.py).  TEST INFRASTRUCTURE ONLY.

A case: name, tags, S, fill, imgs (uint8 [h, w, 3] sources, 1 x 1 to 90 x 70), annots [B, M, 5] fp32 (-1 rows = padding), table
[B, len(MOSAIC_COLUMNS)] fp32, min_area, min_visibility.  Building the cases asserts that no box decision sits within 1e-9 relative
of its threshold, so the kept set is unambiguous in fp64 and no case is ever skipped for being too close."""
import numpy as np

from efficientdet.pytorch_amd.data import MOSAIC, MOSAIC_COLUMNS, check_mosaic_table
from tests import mosaic_restated as R


def _imgs(rng, sizes):
    return [rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in sizes]


def _row(on=1, cx=0, cy=0, src=(0, 0, 0, 0), side=(1, 1, 1, 1), mix=0, mix_src=0, lam=0.0):
    r = np.zeros(len(MOSAIC_COLUMNS), dtype=np.float32)
    r[MOSAIC['on']], r[MOSAIC['cx']], r[MOSAIC['cy']] = on, cx, cy
    r[MOSAIC['src0']:MOSAIC['src3'] + 1] = src
    r[MOSAIC['side0']:MOSAIC['side3'] + 1] = side
    r[MOSAIC['mix']], r[MOSAIC['mix_src']], r[MOSAIC['lam']] = mix, mix_src, lam
    return r


def _annots(lists):
    """per image a list of (x1, y1, x2, y2, label) -> [B, M, 5] fp32 with -1 rows after each image's own"""
    M = max(1, max(len(l) for l in lists))
    a = np.full((len(lists), M, 5), -1.0, dtype=np.float32)
    for b, l in enumerate(lists):
        if len(l):
            a[b, :len(l)] = np.asarray(l, dtype=np.float32)
    return a


def _random_boxes(rng, h, w, n):
    out = []
    for k in range(n):
        x1, y1 = rng.uniform(-0.2 * w, 0.9 * w), rng.uniform(-0.2 * h, 0.9 * h)
        out.append((x1, y1, x1 + rng.uniform(0.05 * w, 0.7 * w), y1 + rng.uniform(0.05 * h, 0.7 * h), float(k % 7)))
    return out


def _case(name, tags, S, imgs, annots, rows, fill=114, min_area=0.0, min_visibility=0.0):
    return dict(name=name, tags=tuple(tags), S=S, fill=fill, imgs=imgs, annots=_annots(annots), table=np.stack(rows).astype(np.float32),
                min_area=float(np.float32(min_area)), min_visibility=float(np.float32(min_visibility)))


def _build():
    rng = np.random.RandomState(20240517)
    C = []
    # --- pixels: one quadrant geometry at a time (B = 1, all four quadrants from the same source)
    im = _imgs(rng, [(20, 20)])
    C.append(_case('smaller_than_window', ['smaller', 'same_source', 'B1'], 32, im, [_random_boxes(rng, 20, 20, 3)],
                   [_row(cx=16, cy=16, side=(8, 8, 8, 8))]))
    im = _imgs(rng, [(40, 30)])
    C.append(_case('larger_than_window', ['larger', 'same_source', 'B1', 'odd_centre'], 32, im, [_random_boxes(rng, 40, 30, 3)],
                   [_row(cx=13, cy=19, side=(32, 32, 32, 32))]))
    im = _imgs(rng, [(24, 20)])
    C.append(_case('exact_copy', ['copy', 'B1'], 32, im, [_random_boxes(rng, 24, 20, 4)], [_row(cx=20, cy=24, side=(24, 24, 24, 24))]))
    im = _imgs(rng, [(5, 7), (1, 1), (3, 2)])
    C.append(_case('upscale_and_side_1', ['upscale', 'side1', 'B3', 'src_1x1'], 32, im,
                   [_random_boxes(rng, 5, 7, 2), [(0, 0, 1, 1, 2)], [(0.5, 0.5, 2, 3, 1)]],
                   [_row(cx=16, cy=16, src=(0, 1, 2, 0), side=(28, 32, 1, 1)),
                    _row(cx=8, cy=24, src=(1, 1, 2, 2), side=(1, 16, 9, 32)),
                    _row(cx=24, cy=8, src=(2, 0, 1, 0), side=(32, 7, 5, 20))]))
    # --- centres at 0, S, S/4, 3S/4: empty and full windows
    im = _imgs(rng, [(90, 70), (33, 64), (64, 17), (50, 50), (70, 90)])
    an = [_random_boxes(rng, h, w, n) for (h, w), n in zip([(90, 70), (33, 64), (64, 17), (50, 50), (70, 90)], (5, 2, 0, 4, 3))]
    C.append(_case('centres_at_the_borders', ['centre_0', 'centre_S', 'B5', 'no_boxes_source', 'padding_rows'], 64, im, an,
                   [_row(cx=0, cy=0, src=(0, 1, 2, 3), side=(64, 40, 33, 64)),
                    _row(cx=64, cy=64, src=(1, 2, 3, 4), side=(64, 64, 64, 64)),
                    _row(cx=0, cy=64, src=(2, 3, 4, 0), side=(50, 64, 32, 32)),
                    _row(cx=64, cy=0, src=(3, 4, 0, 1), side=(32, 32, 60, 32)),
                    _row(cx=64, cy=32, src=(4, 0, 1, 2), side=(64, 10, 47, 3))], min_visibility=0.25))
    C.append(_case('centres_at_quarters', ['centre_quarter', 'centre_three_quarters', 'pass_through_between', 'B5'], 64, im, an,
                   [_row(cx=16, cy=48, src=(0, 1, 2, 3), side=(40, 64, 33, 50)),
                    _row(on=0),
                    _row(cx=48, cy=16, src=(2, 2, 4, 0), side=(64, 31, 64, 20)),
                    _row(on=0, cx=99, cy=-5, src=(9, 9, 9, 9), side=(0, 0, 0, 0), mix_src=77, lam=3.0),     # ignored when off
                    _row(cx=16, cy=16, src=(4, 3, 2, 1), side=(17, 64, 64, 64))], min_area=4.0, min_visibility=0.1))
    # --- MixUp: lam 0, 1, 0.5 (half-up ties), 0.3; a partner equal to a quadrant source
    im = _imgs(rng, [(30, 45), (64, 64), (21, 13)])
    an = [_random_boxes(rng, 30, 45, 3), _random_boxes(rng, 64, 64, 2), _random_boxes(rng, 21, 13, 3)]
    for lam in (0.0, 1.0, 0.5, 0.3):
        C.append(_case('mixup_lam_%g' % lam, ['mix', 'lam_%g' % lam, 'partner_is_quadrant_source', 'B3'], 64, im, an,
                       [_row(cx=30, cy=35, src=(0, 1, 2, 1), side=(40, 64, 30, 50), mix=1, mix_src=1, lam=lam),
                        _row(on=0),
                        _row(cx=40, cy=21, src=(2, 0, 0, 1), side=(21, 45, 64, 33), mix=1, mix_src=2, lam=lam)], fill=7 if lam == 0.5 else 114))
    # --- boxes, hand-placed: sources of exactly 32 x 32 copied (side 32) around the centre (32, 32) of a 64 canvas, so source
    # coordinates map by a shift: TL + (0, 0), TR + (32, 0), BL + (0, 32), BR + (32, 32)
    im = _imgs(rng, [(32, 32), (32, 32)])
    an = [[(4, 4, 12, 12, 0),          # inside
           (0, 0, 32, 32, 1),          # exactly the window: on all four window edges
           (10, 10, 10, 20, 2),        # zero area
           (-9, 5, -1, 9, 3)],         # wholly outside the canvas in TL / BL, wholly outside the WINDOW (inside the canvas) in TR / BR
          [(8, 8, 24, 24, 4), (30, 2, 32, 6, 5)]]
    C.append(_case('boxes_by_hand', ['box_on_edge', 'box_outside', 'box_zero_area', 'padding_rows'], 64, im, an,
                   [_row(cx=32, cy=32, src=(0, 0, 1, 0), side=(32, 32, 32, 32)),
                    _row(cx=32, cy=32, src=(1, 1, 1, 1), side=(32, 32, 32, 32))]))
    # a box straddling the centre: source 0 is 40 x 40 copied (side 40) into TL with centre (32, 32): origin (-8, -8); the box
    # (30, 10, 50, 20) lands on x 22 .. 42 and the window keeps 22 .. 32: visibility 0.5; (34, 10, 50, 20) keeps 6 of 16: 0.375
    im = _imgs(rng, [(40, 40)])
    an = [[(30, 10, 50, 20, 0), (34, 10, 50, 20, 1), (24, 10, 44, 20, 2)]]
    for vis, tag in ((0.45, 'straddle_kept'), (0.55, 'straddle_dropped')):
        C.append(_case('box_' + tag, [tag, 'B1'], 64, im, an, [_row(cx=32, cy=32, side=(40, 40, 40, 40))], min_visibility=vis))
    # every row of all five sources kept: count == 5 M
    im = _imgs(rng, [(32, 32), (32, 32)])
    an = [[(2, 3, 20, 30, 0), (5, 5, 9, 9, 1), (1, 1, 31, 31, 2)], [(3, 2, 30, 20, 3), (8, 8, 16, 16, 4), (0.5, 0.5, 31.5, 31.5, 5)]]
    C.append(_case('all_rows_kept', ['count_5M', 'mix'], 64, im, an,
                   [_row(cx=32, cy=32, src=(0, 1, 1, 0), side=(32, 32, 32, 32), mix=1, mix_src=1, lam=0.5),
                    _row(cx=32, cy=32, src=(1, 0, 0, 1), side=(32, 32, 32, 32), mix=1, mix_src=0, lam=0.25)], min_visibility=0.9))
    # more rows than one round of the 64 lanes
    sizes = [(61, 47), (20, 70), (64, 64)]
    im = _imgs(rng, sizes)
    an = [_random_boxes(rng, h, w, n) for (h, w), n in zip(sizes, (150, 64, 65))]
    C.append(_case('many_boxes', ['more_than_64_rows', 'mix', 'B3'], 64, im, an,
                   [_row(cx=31, cy=33, src=(0, 1, 2, 0), side=(64, 50, 40, 64), mix=1, mix_src=2, lam=0.7),
                    _row(cx=20, cy=50, src=(1, 2, 0, 1), side=(33, 64, 64, 21)),
                    _row(on=0)], min_area=2.0, min_visibility=0.3))
    # a canvas side that is no multiple of 4: a row ends in a short run, and the stores are bytes
    sizes = [(17, 29), (40, 31)]
    im = _imgs(rng, sizes)
    an = [_random_boxes(rng, h, w, 3) for h, w in sizes]
    C.append(_case('side_not_multiple_of_4', ['S_mod_4'], 30, im, an,
                   [_row(cx=11, cy=17, src=(0, 1, 1, 0), side=(30, 22, 17, 9), mix=1, mix_src=1, lam=0.4),
                    _row(on=0)]))
    return C


def margins(case):
    """Per output image the restated details, after asserting that every decision is clear: a visibility ratio or a clipped area is
    further than 1e-9 relative from its threshold.  A clipped area of exactly 0 (a clamp collapsed the box) and a ratio of exactly 1
    (nothing was clamped) carry no rounding, so they are clear wherever the threshold lies."""
    hws = [im.shape[:2] for im in case['imgs']]
    out = []
    for b, row in enumerate(case['table']):
        kept, info = R.boxes(case['annots'], hws, row, case['S'], case['min_area'], case['min_visibility'], b, details=True)
        for q, area, clipped, _, _, _ in info:
            if area == 0.0:
                continue
            for v, thr, exact in ((clipped, case['min_area'], clipped == 0.0),
                                  (clipped / area, case['min_visibility'], clipped == 0.0 or clipped == area)):
                assert exact or abs(v - thr) > 1e-9 * max(abs(v), abs(thr)), (case['name'], b, q, v, thr)
        out.append((kept, info))
    return out


CASES = _build()
for _c in CASES:
    check_mosaic_table(_c['table'], len(_c['imgs']), _c['S'], np.array([im.shape[:2] for im in _c['imgs']]))
    margins(_c)
