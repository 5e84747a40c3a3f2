"""The drawing rule of include/effdet_draw.h as a sequential painter in NumPy and Python integers: for every row in order its fill and
its outline, then for every row in order its label, each primitive painted as clipped rectangles over what is already there.  It is
deliberately not a gather (csrc/draw.hip resolves every pixel against a binned list instead).  The scale multiply and the percent are
np.float32 operations; the glyph bits come from the library's own font through effdet_draw_glyph (there is no second table)."""
import functools

import numpy as np

MAX_ROWS, NAME_MAX, MAX_THICKNESS, MAX_TEXT_SCALE, TEXT_MAX = 1024, 16, 16, 8, 32
LIM = 1 << 20
f32 = np.float32


@functools.lru_cache(maxsize=None)
def glyph(code):
    """The 40 bits of the glyph of `code` (bit (row r, column c) is 5r + 4 - c), from the library."""
    from efficientdet.pytorch_amd import build, _lib
    build.build(verbose=False)
    return int(_lib.require('effdet_draw_glyph').effdet_draw_glyph(int(code)))


def glyph_rows(code):
    """-> 8 strings of 5 characters, '#' for a set bit."""
    g = glyph(code)
    return [''.join('#' if (g >> (5 * r + 4 - c)) & 1 else '.' for c in range(5)) for r in range(8)]


def row_ints(row, sx=1.0, sy=1.0):
    """The header's "Coordinates": -> (X1, Y1, X2, Y2, L) or None for a skipped row."""
    with np.errstate(all='ignore'):
        v = [f32(row[0]) * f32(sx), f32(row[1]) * f32(sy), f32(row[2]) * f32(sx), f32(row[3]) * f32(sy)]
    lab = f32(row[5])
    if not all(np.isfinite(x) for x in v) or not lab >= 0:
        return None
    X1, Y1, X2, Y2 = (int(min(max(float(x), -LIM), LIM)) for x in v)               # int(): toward zero
    if X2 < X1 or Y2 < Y1:
        return None
    return X1, Y1, X2, Y2, int(min(float(lab), 2147483520.0))


def percent(score):
    score = f32(score)
    if not np.isfinite(score):
        return 0
    with np.errstate(all='ignore'):
        f = f32(f32(score * f32(100.0)) + f32(0.5))
    return 0 if f <= 0 else (100 if f >= 100 else int(f))


def label_text(row, L, rid, names, show_id, show_score):
    """-> the label's bytes."""
    out = b''
    if show_id:
        out += b'#%d ' % max(int(rid), 0)
    out += bytes(names[L]) if names is not None and L < len(names) else b'%d' % L
    if show_score:
        out += b' %d' % percent(row[4])
    assert len(out) <= TEXT_MAX
    return out


def label_rect(X1, Y1, n, W, t, s):
    """-> (Lx, Ly, width, height, moved inside, shifted left)."""
    o = t // 2
    width = 6 * s * n + s
    Lx, Ly = X1 - o, Y1 - o - 9 * s
    inside = Ly < 0
    if inside:
        Ly = Y1 - o + t
    shifted = Lx > W - width and Lx > 0
    Lx = max(min(Lx, W - width), 0)
    return Lx, Ly, width, 9 * s, inside, shifted


def _rect(frame, xa, ya, xb, yb, colour, alpha=255):
    """Paints the inclusive rectangle, clipped to the frame; alpha < 255 blends with what is there."""
    H, W = frame.shape[:2]
    xa, ya, xb, yb = max(xa, 0), max(ya, 0), min(xb, W - 1), min(yb, H - 1)
    if xb < xa or yb < ya:
        return
    c = np.asarray(colour, dtype=np.int64)
    if alpha == 255:
        frame[ya:yb + 1, xa:xb + 1] = c
    else:
        p = frame[ya:yb + 1, xa:xb + 1].astype(np.int64)
        frame[ya:yb + 1, xa:xb + 1] = (c * alpha + p * (255 - alpha) + 127) // 255


def colour_of(palette, key):
    return [int(v) for v in palette[int(key) % len(palette)]]                      # (Python's % is non-negative for a positive modulus)


def paint_box(frame, X1, Y1, X2, Y2, c, t, a):
    """The fill and then the outline of one row."""
    if a > 0:
        _rect(frame, X1, Y1, X2, Y2, c, a)
    if t > 0:
        o = t // 2
        ox1, oy1, ox2, oy2 = X1 - o, Y1 - o, X2 + o, Y2 + o
        hx1, hy1, hx2, hy2 = ox1 + t, oy1 + t, ox2 - t, oy2 - t
        if hx1 > hx2 or hy1 > hy2:
            _rect(frame, ox1, oy1, ox2, oy2, c)
        else:
            _rect(frame, ox1, oy1, ox2, hy1 - 1, c)                                # top, bottom, left, right strips around the hole
            _rect(frame, ox1, hy2 + 1, ox2, oy2, c)
            _rect(frame, ox1, hy1, hx1 - 1, hy2, c)
            _rect(frame, hx2 + 1, hy1, ox2, hy2, c)


def paint_label(frame, X1, Y1, text, c, t, s):
    W = frame.shape[1]
    Lx, Ly, width, height, _, _ = label_rect(X1, Y1, len(text), W, t, s)
    _rect(frame, Lx, Ly, Lx + width - 1, Ly + height - 1, c)
    ink = (0, 0, 0) if 299 * c[0] + 587 * c[1] + 114 * c[2] >= 128000 else (255, 255, 255)
    for j, ch in enumerate(text):
        g = glyph(ch if 0x20 <= ch <= 0x7E else ord('?'))
        x0, y0 = Lx + s + 6 * s * j, Ly + s
        for r in range(8):
            for col in range(5):
                if (g >> (5 * r + 4 - col)) & 1:
                    _rect(frame, x0 + col * s, y0 + r * s, x0 + col * s + s - 1, y0 + r * s + s - 1, ink)


def paint(frame, rows, count, ids=None, scale=None, names=None, palette=None, thickness=2, fill_alpha=0, label=True, show_score=True,
          show_id=False, text_scale=2, color_by='label'):
    """Paints one frame (uint8 [H, W, 3], in place and returned) with rows [K, S], its count, ids [K] and scale (sx, sy)."""
    K = len(rows)
    n = min(max(int(count), 0), K)
    sx, sy = (1.0, 1.0) if scale is None else scale
    todo = []
    for k in range(n):
        g = row_ints(rows[k], sx, sy)
        if g is not None:
            rid = int(ids[k]) if ids is not None else 0
            todo.append((k, g, rid, colour_of(palette, rid if color_by == 'id' else g[4])))
    for k, (X1, Y1, X2, Y2, L), rid, c in todo:
        paint_box(frame, X1, Y1, X2, Y2, c, thickness, fill_alpha)
    if label:
        for k, (X1, Y1, X2, Y2, L), rid, c in todo:
            paint_label(frame, X1, Y1, label_text(rows[k], L, rid, names, show_id, show_score), c, thickness, text_scale)
    return frame


def extents(rows, count, W, ids=None, scale=None, names=None, thickness=2, label=True, show_score=True, show_id=False, text_scale=2, **_):
    """The binning rule's input: per live row -> (k, outline rectangle, label rectangle or None, moved inside, shifted left), rectangles
    inclusive and unclipped."""
    out = []
    sx, sy = (1.0, 1.0) if scale is None else scale
    o = thickness // 2
    for k in range(min(max(int(count), 0), len(rows))):
        g = row_ints(rows[k], sx, sy)
        if g is None:
            continue
        X1, Y1, X2, Y2, L = g
        lab, inside, shifted = None, False, False
        if label:
            n = len(label_text(rows[k], L, int(ids[k]) if ids is not None else 0, names, show_id, show_score))
            Lx, Ly, w, h, inside, shifted = label_rect(X1, Y1, n, W, thickness, text_scale)
            lab = (Lx, Ly, Lx + w - 1, Ly + h - 1)
        out.append((k, (X1 - o, Y1 - o, X2 + o, Y2 + o), lab, inside, shifted))
    return out
