"""NumPy restatement of the Mosaic / MixUp stage (include/effdet_mosaic.h) at injected parameters: the specification the HIP kernels of
csrc/mosaic.hip are tested against.  TEST INFRASTRUCTURE ONLY.

Built on tests/augment_restated.py: its cv2.resize rule (resize_u8), LongestMaxSize's dimensions (lms_dims), the central pad
(pad_centre) and round-half-up (to_u8).  Where the kernel computes every canvas pixel from its quadrant's geometry, this file resizes
each source whole and pastes the part its window shows; the two must agree byte for byte.  Boxes go through the same geometry in fp64
and through filter_bboxes' rule as augment_restated.boxes states it."""
import numpy as np

from efficientdet.pytorch_amd.data import MOSAIC
from tests import augment_restated as A

SLOTS = ('TL', 'TR', 'BL', 'BR', 'partner')


def slot(hws, row, S, b, q):
    """Geometry of slot q (0..3 the quadrants, 4 the partner; q = 0 of a pass-through row is the image itself) of output image b ->
    (source index, rh, rw, ox, oy, (wx0, wx1, wy0, wy1))."""
    on = bool(row[MOSAIC['on']])
    if on and q < 4:
        s, side = int(row[MOSAIC['src0'] + q]), int(row[MOSAIC['side0'] + q])
        cx, cy = int(row[MOSAIC['cx']]), int(row[MOSAIC['cy']])
        rh, rw = A.lms_dims(int(hws[s][0]), int(hws[s][1]), side)
        right, bottom = q & 1, q & 2
        return (s, rh, rw, cx if right else cx - rw, cy if bottom else cy - rh,
                (cx if right else 0, S if right else cx, cy if bottom else 0, S if bottom else cy))
    s = int(row[MOSAIC['mix_src']]) if q == 4 else b
    rh, rw = A.lms_dims(int(hws[s][0]), int(hws[s][1]), S)
    return s, rh, rw, (S - rw) // 2, (S - rh) // 2, (0, S, 0, S)


def slots_of(row):
    on = bool(row[MOSAIC['on']])
    return ([0, 1, 2, 3] + ([4] if row[MOSAIC['mix']] else [])) if on else [0]


def _paste(canvas, img, ox, oy, win):
    """The part of img (placed with its top-left pixel at (ox, oy)) that the window shows."""
    rh, rw = img.shape[:2]
    xs, xe, ys, ye = max(ox, win[0]), min(ox + rw, win[1]), max(oy, win[2]), min(oy + rh, win[3])
    if xe > xs and ye > ys:
        canvas[ys:ye, xs:xe] = img[ys - oy:ye - oy, xs - ox:xe - ox]


def compose(imgs, row, S, fill, b):
    """Output image b: uint8 [S, S, 3].  imgs: the batch's uint8 [h, w, 3] sources; row: its table row."""
    hws = [im.shape[:2] for im in imgs]
    if not row[MOSAIC['on']]:
        return A.pad_centre(A.longest_max_size(imgs[b], S), S)
    canvas = np.full((S, S, 3), fill, dtype=np.uint8)
    for q in range(4):
        s, rh, rw, ox, oy, win = slot(hws, row, S, b, q)
        _paste(canvas, A.resize_u8(imgs[s], rw, rh), ox, oy, win)
    if row[MOSAIC['mix']]:
        s, rh, rw, ox, oy, win = slot(hws, row, S, b, 4)
        partner = np.full((S, S, 3), fill, dtype=np.uint8)
        _paste(partner, A.resize_u8(imgs[s], rw, rh), ox, oy, win)
        lam = np.float32(row[MOSAIC['lam']])
        canvas = A.to_u8(canvas.astype(np.float32) * lam + partner.astype(np.float32) * (np.float32(1) - lam))
    return canvas


def boxes(annots, hws, row, S, min_area, min_visibility, b, details=False):
    """Boxes of output image b -> [k, 5] fp32: the kept rows of TL, TR, BL, BR and the partner, each in input order.  annots: per
    source an [n, 5] array (label -1 rows are padding).  details=True: also (slot, unclipped area, clipped area, mapped box, window, kept) of
    every candidate row with a label."""
    out, info = [], []
    for q in slots_of(row):
        s, rh, rw, ox, oy, win = slot(hws, row, S, b, q)
        a = np.asarray(annots[s], dtype=np.float32).reshape(-1, 5)
        a = a[a[:, 4] != -1]
        h, w = int(hws[s][0]), int(hws[s][1])
        bx = a[:, :4].astype(np.float64) * np.array([rw / w, rh / h, rw / w, rh / h]) + np.array([ox, oy, ox, oy], dtype=np.float64)
        area = (bx[:, 2] - bx[:, 0]) * (bx[:, 3] - bx[:, 1])
        cb = np.stack([np.clip(bx[:, 0], win[0], win[1]), np.clip(bx[:, 1], win[2], win[3]),
                       np.clip(bx[:, 2], win[0], win[1]), np.clip(bx[:, 3], win[2], win[3])], 1)
        clipped = (cb[:, 2] - cb[:, 0]) * (cb[:, 3] - cb[:, 1])
        with np.errstate(divide='ignore', invalid='ignore'):
            keep = (area != 0) & ~(clipped / np.where(area != 0, area, 1) < min_visibility) & ~(clipped <= min_area)
        out.append(np.concatenate([cb[keep].astype(np.float32), a[keep, 4:5]], 1))
        info += [(q, float(u), float(c), tuple(x), win, bool(k)) for u, c, x, k in zip(area, clipped, bx, keep)]
    kept = np.concatenate(out, 0) if out else np.zeros((0, 5), dtype=np.float32)
    return (kept, info) if details else kept
