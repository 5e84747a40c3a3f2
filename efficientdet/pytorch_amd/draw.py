"""The device renderer's Python surface (csrc/draw.hip, include/effdet_draw.h holds the drawing rule): DrawOptions, draw_names,
draw_palette and draw_detections.  ``ops`` forwards these names (``ops.draw_detections`` and so on), ``evaluate.Annotator`` is the thin
wrapper over them."""
import numpy as np
import torch

from . import _lib as L
from .ops import _Options

DRAW_MAX_ROWS, DRAW_NAME_MAX, DRAW_MAX_THICKNESS, DRAW_MAX_TEXT_SCALE = L.DRAW_MAX_ROWS, L.DRAW_NAME_MAX, L.DRAW_MAX_THICKNESS, L.DRAW_MAX_TEXT_SCALE
DRAW_TILE_W, DRAW_TILE_H = L.DRAW_TILE_W, L.DRAW_TILE_H
_DRAW = ('effdet_draw_detections', 'effdet_draw_glyph')
DRAW_COLOR_BY = ('label', 'id')


def _whole(v, lo, hi):
    return not isinstance(v, bool) and isinstance(v, (int, np.integer)) and lo <= int(v) <= hi


class DrawOptions(_Options):
    """What draw_detections paints (include/effdet_draw.h): an outline of `thickness` pixels (0: none, at most 16) around every box, a
    translucent fill of the box with opacity fill_alpha / 255 (0: none), and with `label` a filled label holding the class name, with
    show_score the score in percent and with show_id '#' and the row's id in front; text_scale is the size of a font pixel (1..8; the
    font is 5 x 8); color_by: 'label' colours a row by its class, 'id' by its track id.  show_id and color_by='id' need ids."""

    def __init__(self, thickness=2, fill_alpha=0, label=True, show_score=True, show_id=False, text_scale=2, color_by='label'):
        if not _whole(thickness, 0, DRAW_MAX_THICKNESS):
            raise ValueError('DrawOptions: thickness must be a whole number in 0..%d, got %r' % (DRAW_MAX_THICKNESS, thickness))
        if not _whole(fill_alpha, 0, 255):
            raise ValueError('DrawOptions: fill_alpha must be a whole number in 0..255, got %r' % (fill_alpha,))
        if not _whole(text_scale, 1, DRAW_MAX_TEXT_SCALE):
            raise ValueError('DrawOptions: text_scale must be a whole number in 1..%d, got %r' % (DRAW_MAX_TEXT_SCALE, text_scale))
        if color_by not in DRAW_COLOR_BY:
            raise ValueError('DrawOptions: color_by must be one of %s, got %r' % (', '.join(map(repr, DRAW_COLOR_BY)), color_by))
        self.thickness, self.fill_alpha, self.text_scale, self.color_by = int(thickness), int(fill_alpha), int(text_scale), color_by
        self.label, self.show_score, self.show_id = bool(label), bool(show_score), bool(show_id)

    def key(self):
        return (self.thickness, self.fill_alpha, self.label, self.show_score, self.show_id, self.text_scale, self.color_by)

    def __repr__(self):
        return 'DrawOptions(thickness=%d, fill_alpha=%d, label=%r, show_score=%r, show_id=%r, text_scale=%d, color_by=%r)' % self.key()


class DrawNames:
    """The class names on the device as draw_detections reads them: bytes [n, 16] uint8 and lens [n] uint8 (None, None for n = 0)."""

    def __init__(self, bytes_, lens, n):
        self.bytes, self.lens, self.n = bytes_, lens, int(n)


def draw_names(names, device):
    """-> the DrawNames table of `names` (a sequence of str or bytes; str is encoded as UTF-8) on `device`: build it once and pass it to
    every draw_detections call.  A name longer than 16 bytes is refused; a byte outside 0x20..0x7E prints as '?'.  names=None or an
    empty sequence: the empty table, every label prints as its number."""
    raw = [] if names is None else [n.encode('utf-8') if isinstance(n, str) else bytes(n) for n in names]
    for n in raw:
        if len(n) > DRAW_NAME_MAX:
            raise ValueError('draw_names: %r is longer than %d bytes' % (n, DRAW_NAME_MAX))
    if not raw:
        return DrawNames(None, None, 0)
    table = np.zeros((len(raw), DRAW_NAME_MAX), dtype=np.uint8)
    for i, n in enumerate(raw):
        table[i, :len(n)] = np.frombuffer(n, dtype=np.uint8)
    lens = np.array([len(n) for n in raw], dtype=np.uint8)
    return DrawNames(torch.from_numpy(table).to(device), torch.from_numpy(lens).to(device), len(raw))


def draw_palette_host(n):
    """draw_palette's colours as a uint8 [n, 3] array on the host."""
    n = int(n)
    if n < 1:
        raise ValueError('draw_palette: n >= 1, got %d' % n)
    out = np.zeros((n, 3), dtype=np.uint8)
    for i in range(n):
        h = (i * 137) % 360                                # 137 and 360 are coprime: the first 360 hues are distinct
        up, down = (h % 60) * 255 // 60, 255 - (h % 60) * 255 // 60
        out[i] = ((255, up, 0), (down, 255, 0), (0, 255, up), (0, down, 255), (up, 0, 255), (255, 0, down))[h // 60]
    return out


def draw_palette(n, device):
    """-> the default palette, uint8 [n, 3] on `device`.  Colour i is the fully saturated, full-value HSV colour of hue
    (137 * i) mod 360 degrees, in integers: with f = hue mod 60, up = f * 255 // 60 and down = 255 - up, the sextant hue // 60 picks
    (255, up, 0), (down, 255, 0), (0, 255, up), (0, down, 255), (up, 0, 255), (255, 0, down).  Distinct for n <= 360."""
    return torch.from_numpy(draw_palette_host(n)).to(device)


_draw_defaults = {}                # device -> the default palette of calls without one


def draw_detections(frames, rows, counts, names=None, ids=None, box_scale=None, palette=None, options=None, inplace=False, max_hw=None):
    """Paints rows' boxes and labels into uint8 RGB frames on the device (include/effdet_draw.h holds the drawing rule; csrc/draw.hip).
    frames: a contiguous uint8 [B, H, W, 3] tensor, or decode_jpeg_batch's triple (src uint8, src_off [B] int64, src_hw [B, 2] int32)
    with max_hw=(Hmax, Wmax), no frame larger than that.  rows [B, K, S] fp32 (S >= 6: x1, y1, x2, y2, score, label, ...; K <= 1024)
    and counts [B] int32 as finalize_device or TrackedDetector.update return them; ids [B, K] int32 (update's) for show_id and
    color_by='id'; box_scale: [B, 2] fp32 on the device (sx, sy per frame, from the rows' pixels to the frame's) or one (sx, sy) pair
    for all frames; names: a draw_names table (or a sequence, tabled at every call); palette: uint8 [P, 3] on the device (None: 64
    colours of draw_palette).  -> the painted frames: a clone of `frames` (of src for the triple), or with inplace=True `frames` itself.

    One launch, nothing is read back, every refusal comes before the launch.  The call can be captured in a graph when it uploads
    nothing: names a draw_names table or None, palette a tensor (or the default after one eager call on that device), box_scale a
    tensor or None.  The options are launch arguments, so a captured call keeps the options it was captured with: capture again
    after changing them."""
    o = DrawOptions() if options is None else options
    if not isinstance(o, DrawOptions):
        raise TypeError('draw_detections: options must be a DrawOptions, not %r' % (o,))
    if isinstance(frames, (tuple, list)):
        if len(frames) != 3 or max_hw is None:
            raise ValueError('draw_detections: frames is a [B, H, W, 3] tensor or (src, src_off, src_hw) with max_hw=(Hmax, Wmax)')
        pix, off, hw = frames
        B, (Hmax, Wmax) = int(off.numel()), (int(v) for v in max_hw)
        assert pix.dtype == torch.uint8 and pix.is_contiguous() and pix.dim() == 1
        assert off.dtype == torch.int64 and off.is_contiguous() and off.device == pix.device
        assert hw.dtype == torch.int32 and hw.is_contiguous() and tuple(hw.shape) == (B, 2) and hw.device == pix.device
    else:
        if max_hw is not None:
            raise ValueError('draw_detections: max_hw goes with the (src, src_off, src_hw) form only')
        pix, off, hw = frames, None, None
        if pix.dim() != 4 or pix.shape[3] != 3:
            raise ValueError('draw_detections: frames must be [B, H, W, 3], got %s' % (tuple(pix.shape),))
        B, Hmax, Wmax = (int(v) for v in pix.shape[:3])
        assert pix.dtype == torch.uint8 and pix.is_contiguous()
    if B < 1 or not 1 <= Hmax <= L.DRAW_MAX_SIDE or not 1 <= Wmax <= L.DRAW_MAX_SIDE or B > L.DRAW_MAX_BATCH:
        raise ValueError('draw_detections: 1..%d frames of 1..%d pixels a side, got %d of %d x %d' % (L.DRAW_MAX_BATCH, L.DRAW_MAX_SIDE, B, Hmax, Wmax))
    dev = pix.device
    if rows.dim() != 3 or rows.shape[0] != B or rows.shape[2] < 6:
        raise ValueError('draw_detections: rows must be [%d, K, >= 6], got %s' % (B, tuple(rows.shape)))
    K, S = int(rows.shape[1]), int(rows.shape[2])
    if not 1 <= K <= DRAW_MAX_ROWS:
        raise ValueError('draw_detections: 1..%d rows per frame, got %d' % (DRAW_MAX_ROWS, K))
    assert rows.dtype == torch.float32 and rows.is_contiguous() and rows.device == dev
    assert counts.dtype == torch.int32 and counts.is_contiguous() and counts.numel() == B and counts.device == dev
    if ids is None and (o.show_id or o.color_by == 'id'):
        raise ValueError("draw_detections: show_id and color_by='id' need ids")
    if ids is not None:
        assert ids.dtype == torch.int32 and ids.is_contiguous() and tuple(ids.shape) == (B, K) and ids.device == dev
    if box_scale is not None and not torch.is_tensor(box_scale):
        sx, sy = (float(v) for v in box_scale)
        box_scale = torch.tensor([[sx, sy]] * B, dtype=torch.float32, device=dev)
    if box_scale is not None:
        assert box_scale.dtype == torch.float32 and box_scale.is_contiguous() and tuple(box_scale.shape) == (B, 2) and box_scale.device == dev
    if not isinstance(names, DrawNames):
        names = draw_names(names, dev)
    if names.n:
        assert names.bytes.device == dev and names.lens.device == dev
    if palette is None:
        if dev not in _draw_defaults:
            _draw_defaults[dev] = draw_palette(64, dev)
        palette = _draw_defaults[dev]
    if palette.dim() != 2 or palette.shape[0] < 1 or palette.shape[1] != 3:
        raise ValueError('draw_detections: palette must be [P >= 1, 3], got %s' % (tuple(palette.shape),))
    assert palette.dtype == torch.uint8 and palette.is_contiguous() and palette.device == dev
    lib = L.require(*_DRAW)
    if not inplace:
        pix = pix.clone()
    L.check(lib.effdet_draw_detections(L.ptr(pix), L.ptr(off), L.ptr(hw), B, Hmax, Wmax, L.ptr(rows), S, K, L.ptr(counts), L.ptr(ids),
                                       L.ptr(box_scale), L.ptr(names.bytes), L.ptr(names.lens), names.n, L.ptr(palette),
                                       int(palette.shape[0]), o.thickness, o.fill_alpha, int(o.label), int(o.show_score), int(o.show_id),
                                       o.text_scale, int(o.color_by == 'id'), L.stream_ptr()), 'effdet_draw_detections')
    return pix
