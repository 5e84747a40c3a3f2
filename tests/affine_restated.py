"""NumPy restatement of the affine / perspective warp (include/effdet_affine.h) at injected parameters: the specification the HIP
kernels of csrc/affine.hip are tested against.  TEST INFRASTRUCTURE ONLY.

Built on tests/augment_restated.py: LongestMaxSize's dimensions and resize (lms_dims, longest_max_size), the central pad (pad_centre)
and round-half-up (to_u8).  Where the kernel computes a run of pixels per thread and selects `fill` after clamped loads, this file
maps the whole output grid through G at once and gathers from a source padded with one ring of `fill`; the two must agree byte for
byte.  Boxes go through F in fp64 and through box_candidates' rule as the header states it."""
import numpy as np

from efficientdet.pytorch_amd.data import AFFINE
from tests import augment_restated as A


def mats(row):
    """-> (on, F [3, 3], G [3, 3], scale) of a table row, fp64."""
    r = np.asarray(row, dtype=np.float64)
    return (bool(r[AFFINE['on']]), r[AFFINE['f0']:AFFINE['f8'] + 1].reshape(3, 3), r[AFFINE['g0']:AFFINE['g8'] + 1].reshape(3, 3),
            float(r[AFFINE['scale']]))


def coords(G, S, h, w):
    """Source coordinates of the S x S output grid -> (u [S, S], v [S, S] fp64, inside [S, S] bool): the header's order of operations,
    every product and sum a separate fp64 rounding."""
    x = np.arange(S, dtype=np.float64)[None, :]
    y = np.arange(S, dtype=np.float64)[:, None]
    with np.errstate(all='ignore'):
        d = (G[2, 0] * x + G[2, 1] * y) + G[2, 2]
        u = ((G[0, 0] * x + G[0, 1] * y) + G[0, 2]) / d
        v = ((G[1, 0] * x + G[1, 1] * y) + G[1, 2]) / d
        inside = np.isfinite(d) & (d > 0) & np.isfinite(u) & np.isfinite(v) & (u > -1) & (u < w) & (v > -1) & (v < h)
    return u, v, inside


def warp(img, row, S, fill, details=False):
    """One output image: uint8 [S, S, 3].  img: the uint8 [h, w, 3] source; row: its table row.  details=True: also (inside, taps
    outside the source [S, S] of the inside pixels) for the tests that prove which branch a case reaches."""
    on, _, G, _ = mats(row)
    if not on:
        out = A.pad_centre(A.longest_max_size(img, S), S)
        return (out, None, None) if details else out
    h, w = img.shape[:2]
    u, v, inside = coords(G, S, h, w)
    u, v = np.where(inside, u, 0.0), np.where(inside, v, 0.0)
    x0, y0 = np.floor(u), np.floor(v)
    fx, fy = (u - x0).astype(np.float32)[..., None], (v - y0).astype(np.float32)[..., None]
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    ring = np.full((h + 2, w + 2, 3), fill, dtype=np.float32)         # the constant border: index i of the source is i + 1 here
    ring[1:-1, 1:-1] = img
    p00, p01, p10, p11 = ring[y0 + 1, x0 + 1], ring[y0 + 1, x0 + 2], ring[y0 + 2, x0 + 1], ring[y0 + 2, x0 + 2]
    top = p00 + fx * (p01 - p00)
    bot = p10 + fx * (p11 - p10)
    out = A.to_u8(top + fy * (bot - top))
    out[~inside] = fill
    if details:
        border = inside & ((x0 < 0) | (x0 + 1 >= w) | (y0 < 0) | (y0 + 1 >= h))
        return out, inside, border
    return out


def boxes(annot, hw, row, S, wh_thr, ar_thr, area_thr, details=False):
    """Boxes of one image -> [k, 5] fp32, the kept rows in input order.  annot: [n, 5] (label -1 rows are padding); hw: the source's
    (h, w).  details=True: also per candidate row a dict of the filter's terms."""
    on, F, _, scale = mats(row)
    a = np.asarray(annot, dtype=np.float32).reshape(-1, 5)
    a = a[a[:, 4] != -1]
    bx = a[:, :4].astype(np.float64)
    h, w = int(hw[0]), int(hw[1])
    if not on:
        rh, rw = A.lms_dims(h, w, S)
        ox, oy = (S - rw) // 2, (S - rh) // 2
        out = bx * np.array([rw / w, rh / h, rw / w, rh / h]) + np.array([ox, oy, ox, oy], dtype=np.float64)
        kept = np.concatenate([out.astype(np.float32), a[:, 4:5]], 1)
        return (kept, []) if details else kept
    cx = bx[:, [0, 2, 0, 2]]                                           # corners (x1, y1), (x2, y1), (x1, y2), (x2, y2)
    cy = bx[:, [1, 1, 3, 3]]
    with np.errstate(all='ignore'):
        d = (F[2, 0] * cx + F[2, 1] * cy) + F[2, 2]
        X = ((F[0, 0] * cx + F[0, 1] * cy) + F[0, 2]) / d
        Y = ((F[1, 0] * cx + F[1, 1] * cy) + F[1, 2]) / d
        ok = (np.isfinite(d) & (d > 0)).all(1)
        X, Y = np.where(ok[:, None], X, 0.0), np.where(ok[:, None], Y, 0.0)
        nb = np.stack([np.clip(X.min(1), 0, S), np.clip(Y.min(1), 0, S), np.clip(X.max(1), 0, S), np.clip(Y.max(1), 0, S)], 1)
        w2, h2 = nb[:, 2] - nb[:, 0], nb[:, 3] - nb[:, 1]
        w1, h1 = bx[:, 2] - bx[:, 0], bx[:, 3] - bx[:, 1]
        ar = np.maximum(w2 / (h2 + 1e-16), h2 / (w2 + 1e-16))
        ratio = w2 * h2 / (w1 * h1 * scale * scale + 1e-16)
        keep = ok & (w2 > wh_thr) & (h2 > wh_thr) & (ar < ar_thr) & (ratio > area_thr)
    kept = np.concatenate([nb[keep].astype(np.float32), a[keep, 4:5]], 1)
    if details:
        return kept, [dict(ok=bool(o), w2=float(p), h2=float(q), ar=float(r), ratio=float(s), box=tuple(n), kept=bool(k))
                      for o, p, q, r, s, n, k in zip(ok, w2, h2, ar, ratio, nb, keep)]
    return kept
