"""Seeded cases of the affine / perspective warp shared by tests/test_affine_host.py (CPU: every case reaches what it is tagged with)
and tests/test_gpu_affine.py (the kernels against tests/affine_restated.py).  TEST INFRASTRUCTURE ONLY.

A case: name, tags, S, fill, imgs (uint8 [h, w, 3] sources, 1 x 1 to 200 x 150), annots [B, M, 5] fp32 (-1 rows = padding), table
[B, len(AFFINE_COLUMNS)] fp64, wh_thr, ar_thr, area_thr.  Building the cases asserts that no box decision sits within 1e-9 relative
of its threshold unless it sits exactly ON it (an exact small number on both sides, such as w2 == wh_thr == 2), so the kept set is
unambiguous in fp64 and no case is ever skipped for being too close."""
import math

import numpy as np

from efficientdet.pytorch_amd.data import AFFINE, AFFINE_COLUMNS, check_affine_table
from tests import affine_restated as R


def _imgs(rng, sizes):
    return [rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in sizes]


def _row(F=None, G=None, scale=None, on=1):
    """A table row from the forward matrix F (3 x 3, or 2 x 3 for an affine map); G defaults to inv(F) and may be given where an exact
    inverse is known; scale defaults to sqrt(|det F[:2, :2]|)."""
    r = np.zeros(len(AFFINE_COLUMNS), dtype=np.float64)
    r[AFFINE['on']] = on
    if F is None:
        return r
    F = np.asarray(F, dtype=np.float64)
    F = np.vstack([F, [0, 0, 1]]) if F.shape == (2, 3) else F
    if G is None:
        G = np.linalg.inv(F)
    G = np.asarray(G, dtype=np.float64)
    G = np.vstack([G, [0, 0, 1]]) if G.shape == (2, 3) else G
    r[AFFINE['f0']:AFFINE['f8'] + 1], r[AFFINE['g0']:AFFINE['g8'] + 1] = F.reshape(-1), G.reshape(-1)
    r[AFFINE['scale']] = math.sqrt(abs(F[0, 0] * F[1, 1] - F[0, 1] * F[1, 0])) if scale is None else scale
    return r


def shift(tx, ty):
    """Translation of the image by (tx, ty): exact F and G."""
    return _row([[1, 0, tx], [0, 1, ty]], [[1, 0, -tx], [0, 1, -ty]], 1.0)


def generic(rng, h, w, S, degrees=30.0, shear=10.0, scale=(0.5, 1.5), translate=0.1, perspective=0.0):
    """Rotation + shear + scale about the source centre, the composition of data.sample_affine_table restated with explicit draws."""
    C, P, Rm, Sh, T = (np.eye(3) for _ in range(5))
    C[0, 2], C[1, 2] = -w / 2, -h / 2
    P[2, 0], P[2, 1] = rng.uniform(-perspective, perspective, 2)
    a, k = math.radians(rng.uniform(-degrees, degrees)), rng.uniform(*scale) * S / max(h, w)
    Rm[:2, :2] = [[k * math.cos(a), k * math.sin(a)], [-k * math.sin(a), k * math.cos(a)]]
    Sh[0, 1], Sh[1, 0] = (math.tan(math.radians(v)) for v in rng.uniform(-shear, shear, 2))
    T[0, 2], T[1, 2] = rng.uniform(0.5 - translate, 0.5 + translate, 2) * S
    return _row(T @ Sh @ Rm @ P @ C, scale=k)


def _annots(lists):
    """per image a list of (x1, y1, x2, y2, label), None = a padding row in between -> [B, M, 5] fp32 with -1 rows after each image's own"""
    M = max(1, max(len(l) for l in lists))
    a = np.full((len(lists), M, 5), -1.0, dtype=np.float32)
    for b, l in enumerate(lists):
        for m, row in enumerate(l):
            if row is not None:
                a[b, m] = row
    return a


def _random_boxes(rng, h, w, n, holes=0):
    out = []
    for k in range(n):
        x1, y1 = rng.uniform(-0.2 * w, 0.9 * w), rng.uniform(-0.2 * h, 0.9 * h)
        out.append((x1, y1, x1 + rng.uniform(0.02 * w, 0.7 * w), y1 + rng.uniform(0.02 * h, 0.7 * h), float(k % 7)))
    for k in rng.permutation(n)[:holes]:
        out[k] = None
    return out


def _case(name, tags, S, imgs, annots, rows, fill=114, wh_thr=2.0, ar_thr=100.0, area_thr=0.1):
    return dict(name=name, tags=tuple(tags), S=S, fill=fill, imgs=imgs, annots=_annots(annots), table=np.stack(rows).astype(np.float64),
                wh_thr=float(wh_thr), ar_thr=float(ar_thr), area_thr=float(area_thr))


def _build():
    rng = np.random.RandomState(20241020)
    C = []
    few = lambda sizes: [_random_boxes(rng, h, w, 3) for h, w in sizes]                    # noqa: E731
    # --- exact matrices: the output is the source, moved
    sizes = [(32, 32)]
    C.append(_case('identity', ['identity', 'interior', 'B1'], 32, _imgs(rng, sizes), few(sizes), [shift(0, 0)]))
    sizes = [(32, 32), (20, 40), (32, 32)]
    C.append(_case('integer_translations', ['int_translation', 'all_fill_pixel', 'border_tap', 'B3'], 32, _imgs(rng, sizes), few(sizes),
                   [shift(3, -5), shift(-7, 2), shift(31, 31)]))
    C.append(_case('half_integer_translations', ['tie', 'B3'], 32, _imgs(rng, sizes), few(sizes),
                   [shift(2.5, 0), shift(0, -3.5), shift(1.5, 1.5)], fill=7))
    sizes = [(32, 32), (32, 20)]
    mirror = [[-1, 0, 31], [0, 1, 0]]                                  # x -> 31 - x on a 32-wide source, its own inverse
    swap = [[0, 1, 0], [1, 0, 0]]
    C.append(_case('mirror_and_transpose', ['mirror', 'transpose'], 32, _imgs(rng, sizes), few(sizes),
                   [_row(mirror, mirror, 1.0), _row(swap, swap, 1.0)]))
    sizes = [(16, 16), (64, 64)]
    C.append(_case('scale_2x_and_half', ['scale_2x', 'scale_half', 'tie'], 32, _imgs(rng, sizes), few(sizes),
                   [_row([[2, 0, 0], [0, 2, 0]], [[0.5, 0, 0], [0, 0.5, 0]], 2.0),
                    _row([[0.5, 0, 0], [0, 0.5, 0]], [[2, 0, 0], [0, 2, 0]], 0.5)]))
    # --- generic rotation + shear + scale over every source size, a pass-through in between, 150 rows of boxes per image
    sizes = [(90, 70), (200, 150), (1, 17), (1, 1), (64, 64)]
    rows = [generic(rng, h, w, 64) for h, w in sizes]
    rows[3] = _row(on=0)
    rows[3][1:] = (9.0, -1.0, 0.0, 0.0, 0.0, 7.0, 3.0, 0.0, 0.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0, -1.0, 0.0, -5.0, -3.0)   # ignored when off
    C.append(_case('generic', ['generic', 'interior', 'border_tap', 'all_fill_pixel', 'pass_through_between', 'larger_than_S', 'B5',
                               'more_than_64_rows', 'padding_between', 'src_1x1'], 64, _imgs(rng, sizes),
                   [_random_boxes(rng, h, w, 150, holes=20) for h, w in sizes], rows))
    sizes = [(90, 70)]
    C.append(_case('zoom_out', ['mostly_fill', 'B1'], 64, _imgs(rng, sizes), few(sizes),
                   [generic(rng, 90, 70, 64, degrees=45.0, shear=0.0, scale=(0.15, 0.15), translate=0.0)], fill=200))
    # --- zoom-in: all of the output inside one cell of four source pixels; on the 1 x 1 source the cell is the pixel and three fills
    sizes = [(90, 70), (1, 1), (1, 17)]
    C.append(_case('zoom_in', ['one_source_pixel', 'src_1x1', 'border_tap', 'B3'], 32, _imgs(rng, sizes), few(sizes),
                   [_row(np.linalg.inv([[0.01, 0, 5.2], [0, 0.01, 7.1], [0, 0, 1]]), [[0.01, 0, 5.2], [0, 0.01, 7.1]], 100.0),
                    _row(np.linalg.inv([[0.01, 0, -0.2], [0, 0.01, -0.2], [0, 0, 1]]), [[0.01, 0, -0.2], [0, 0.01, -0.2]], 100.0),
                    generic(rng, 1, 17, 32, degrees=80.0)]))
    # --- a perspective whose d = 0 line (x = 16) crosses the output: d > 0 left of it, exactly 0 on it, < 0 right of it
    sizes = [(90, 70)]
    G = np.array([[1.5, 0.1, 2.0], [0.2, 1.2, 3.0], [-1.0 / 16, 0.0, 1.0]])
    C.append(_case('perspective_d0', ['d_le_0', 'B1'], 32, _imgs(rng, sizes), few(sizes), [_row(np.linalg.inv(G), G, 0.7)]))
    sizes = [(90, 70), (64, 64)]
    C.append(_case('perspective_generic', ['perspective'], 64, _imgs(rng, sizes), few(sizes),
                   [generic(rng, h, w, 64, perspective=0.002) for h, w in sizes]))
    # --- coordinates exactly on -1, -0.5, 0, w - 1 and w (and the same along y with h = 1)
    sizes = [(1, 17), (1, 17)]
    C.append(_case('coordinates_on_the_edges', ['edges', 'border_tap'], 32, _imgs(rng, sizes), few(sizes), [shift(1, 1), shift(0.5, 0.5)], fill=255))
    # --- an output side that is no multiple of 4: a row ends in a short run, and the stores are bytes
    sizes = [(17, 29), (40, 31), (1, 1)]
    C.append(_case('side_not_multiple_of_4', ['S_mod_4', 'B3'], 30, _imgs(rng, sizes), few(sizes),
                   [generic(rng, 17, 29, 30), _row(on=0), generic(rng, 1, 1, 30, scale=(8.0, 9.0))]))
    # --- boxes by hand: a 64 x 64 source under the identity (scale 1), then under a perspective whose plane x = 32 cuts the boxes
    sizes = [(64, 64), (64, 64)]
    an = [[(4, 4, 12, 12, 0),            # inside: kept as it is
           (-20, 5, -4, 9, 1),           # outside: clipped to nothing
           (-6, 10, 10, 30, 2),          # straddles the border: 10 x 20 of 16 x 20 left, ratio 0.625
           None,
           (10, 10, 12, 30, 3),          # w2 == wh_thr exactly: dropped by that clause alone (ar = 10, ratio = 1)
           (10, 10, 12.5, 30, 4),        # just wider: kept
           (0, 0, 60, 5.5, 5),           # aspect ratio 10.9 < 12: kept
           (0, 0, 60, 4.5, 6),           # aspect ratio 13.3: dropped by that clause alone
           None,
           (-28, 10, 10, 30, 7),         # 10 of 38 wide left: ratio 0.263 > 0.25, kept
           (-32, 10, 10, 30, 8)],        # 10 of 42: ratio 0.238, dropped by that clause alone
          [(4, 4, 12, 12, 0),            # d = 0.875 and 0.625: kept
           None,
           (20, 4, 40, 12, 1),           # the corners at x = 40 have d = -0.25: behind the plane, dropped
           (20, 4, 32, 12, 2),           # the corners at x = 32 have d = 0: dropped
           (8, 20, 24, 28, 3)]]
    persp = [[1, 0, 0], [0, 1, 0], [-1.0 / 32, 0, 1]]
    C.append(_case('boxes_by_hand', ['box_kept', 'box_outside', 'box_straddle', 'drop_wh', 'drop_ar', 'drop_area', 'drop_behind',
                                     'padding_between'], 64, _imgs(rng, sizes), an,
                   [shift(0, 0), _row(persp, [[1, 0, 0], [0, 1, 0], [1.0 / 32, 0, 1]], 1.0)], wh_thr=2.0, ar_thr=12.0, area_thr=0.25))
    return C


def margins(case):
    """Per output image the restated (kept, details), after asserting that every decision of a row that is on is clear: each term of
    the filter is further than 1e-9 relative from its threshold, or exactly on it."""
    out = []
    for b, row in enumerate(case['table']):
        kept, info = R.boxes(case['annots'][b], case['imgs'][b].shape[:2], row, case['S'], case['wh_thr'], case['ar_thr'], case['area_thr'],
                             details=True)
        for i in info:
            if not i['ok']:
                continue
            for v, thr in ((i['w2'], case['wh_thr']), (i['h2'], case['wh_thr']), (i['ar'], case['ar_thr']), (i['ratio'], case['area_thr'])):
                assert v == thr or abs(v - thr) > 1e-9 * max(abs(v), abs(thr)), (case['name'], b, v, thr)
        out.append((kept, info))
    return out


CASES = _build()
for _c in CASES:
    check_affine_table(_c['table'], len(_c['imgs']), _c['S'])
    margins(_c)
