"""NumPy restatement of get_augumentation (datasets/augmentation.py:8-50) at injected parameters: the specification the HIP
chain of csrc/augment.hip is tested against.  TEST INFRASTRUCTURE ONLY.

The reference runs albumentations 0.4.x on OpenCV; neither is installed here, so this file restates the documented rules:
* resizes (LongestMaxSize, RandomResizedCrop, Resize) are cv2 INTER_LINEAR as oracle.pipeline_oracle.resize_bilinear restates
  it (half-pixel centres, edge clamp, fp32 blend), rounded half up to uint8.  cv2's own 8-bit path uses 11-bit fixed-point
  weights, which can differ by one grey level; that rule is not pinned here.
* RGB <-> HSV is cv2's uint8 rule: the 12-bit fixed-point forward conversion (H in [0, 180)) and the float inverse.
* RGB <-> LAB (CLAHE's colour space) is cv2's documented float formula (D65, sRGB gamma) in fp64, with L * 255 / 100 and
  a, b + 128 rounded half to even; cv2's 8-bit fixed-point LAB tables are not restated, so this can differ from cv2 by one level.
* CLAHE is cv2's algorithm (8 x 8 tiles, reflect-101 extension, clip + uniform redistribution + strided residual, fp32 LUT scale
  and bilinear blend between tile LUTs).
* LUT ops (brightness / contrast, gamma, RGB shift, HSV shifts) follow albumentations' uint8 LUTs; Normalize is its fp32 rule.
* boxes are pascal_voc pixels in fp64 through each geometric step, clipped and filtered at the end as filter_bboxes does.
"""
import numpy as np

from efficientdet.pytorch_amd.data import AUG, MEAN, STD
from oracle.pipeline_oracle import resize_bilinear


def to_u8(v):
    return np.clip(np.floor(v + np.float32(0.5)), 0, 255).astype(np.uint8)


def resize_u8(img, rw, rh):
    """cv2.resize(img, (rw, rh), INTER_LINEAR) on uint8, restated: float bilinear, round half up."""
    return to_u8(resize_bilinear(img, rw, rh))


def lms_dims(h, w, S):
    scale = S / max(h, w)
    return int(round(h * scale)), int(round(w * scale))


def longest_max_size(img, S):
    rh, rw = lms_dims(img.shape[0], img.shape[1], S)
    return img if (rh, rw) == img.shape[:2] else resize_u8(img, rw, rh)


def pad_centre(img, S):
    rh, rw = img.shape[:2]
    top, left = max(S - rh, 0) // 2, max(S - rw, 0) // 2
    out = np.zeros((max(S, rh), max(S, rw), 3), dtype=np.uint8)
    out[top:top + rh, left:left + rw] = img
    return out


def cv2_flip(img, code):
    if code != 0:
        img = img[:, ::-1]
    if code != 1:
        img = img[::-1]
    return img


# ------------------------------------------------------------------------------------------------ LUTs
def brightness_contrast_lut(alpha, beta):
    lut = np.arange(256).astype(np.float32) * np.float32(alpha)
    lut = lut + np.float32(float(np.float32(beta)) * 255.0)
    return np.clip(lut, 0, 255).astype(np.uint8)


def gamma_lut(gamma):
    return ((np.arange(256) * (1.0 / 255.0)) ** float(np.float32(gamma)) * 255.0).astype(np.uint8)


def rgb_shift_lut(shift):
    return np.clip(np.arange(256).astype(np.float32) + np.float32(shift), 0, 255).astype(np.uint8)


def hue_lut(shift):
    h = np.fmod(np.arange(256) + float(np.float32(shift)), 180.0)
    return np.where(h < 0, h + 180.0, h).astype(np.uint8)


def sat_val_lut(shift):
    return np.clip(np.arange(256) + float(np.float32(shift)), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ colour spaces
def rgb_to_hsv8(img):
    r, g, b = (img[..., c].astype(np.int64) for c in range(3))
    v = np.maximum(np.maximum(r, g), b)
    diff = v - np.minimum(np.minimum(r, g), b)
    sdiv = np.where(v > 0, np.rint((255 << 12) / np.maximum(v, 1)), 0).astype(np.int64)
    hdiv = np.where(diff > 0, np.rint((180 << 12) / (6.0 * np.maximum(diff, 1))), 0).astype(np.int64)
    s = (diff * sdiv + (1 << 11)) >> 12
    hh = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (hh * hdiv + (1 << 11)) >> 12
    return np.where(h < 0, h + 180, h), s, v


def hsv8_to_rgb8(h8, s8, v8):
    f = np.float32
    s = s8.astype(f) * (f(1) / f(255)); v = v8.astype(f) * (f(1) / f(255))
    h = np.fmod(h8.astype(f) * (f(6) / f(180)), f(6))
    sector = np.floor(h).astype(np.int64)
    h = h - sector.astype(f)
    bad = (sector < 0) | (sector >= 6)
    sector = np.where(bad, 0, sector); h = np.where(bad, f(0), h)
    tab = np.stack([v, v * (f(1) - s), v * (f(1) - s * h), v * (f(1) - s * (f(1) - h))], -1)
    sd = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])       # (b, g, r) per sector
    pick = lambda j: np.take_along_axis(tab, sd[sector][..., j:j + 1], -1)[..., 0]       # noqa: E731
    b, g, r = pick(0), pick(1), pick(2)
    grey = s == 0
    r = np.where(grey, v, r); g = np.where(grey, v, g); b = np.where(grey, v, b)
    return np.stack([sat_rint_u8(x * f(255)) for x in (r, g, b)], -1)


def hsv_shift(img, dh, ds, dv):
    h, s, v = rgb_to_hsv8(img)
    return hsv8_to_rgb8(hue_lut(dh)[h], sat_val_lut(ds)[s], sat_val_lut(dv)[v])


def sat_rint_u8(v):
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


LIN = np.where(np.arange(256) / 255.0 <= 0.04045, (np.arange(256) / 255.0) / 12.92,
               ((np.arange(256) / 255.0 + 0.055) / 1.055) ** 2.4)


def _lab_f(t):
    return np.where(t > 0.008856, np.cbrt(t), 7.787 * t + 16.0 / 116.0)


def rgb_to_lab8(img):
    R, G, B = (LIN[img[..., c]] for c in range(3))
    Y = 0.212671 * R + 0.715160 * G + 0.072169 * B
    X = (0.412453 * R + 0.357580 * G + 0.180423 * B) / 0.950456
    Z = (0.019334 * R + 0.119193 * G + 0.950227 * B) / 1.088754
    L = np.where(Y > 0.008856, 116.0 * np.cbrt(Y) - 16.0, 903.3 * Y)
    fx, fy, fz = _lab_f(X), _lab_f(Y), _lab_f(Z)
    return sat_rint_u8(L * (255.0 / 100.0)), sat_rint_u8(500.0 * (fx - fy) + 128.0), sat_rint_u8(200.0 * (fy - fz) + 128.0)


def _srgb8(x):
    x = np.clip(x, 0.0, 1.0)
    return sat_rint_u8(np.where(x <= 0.0031308, 12.92 * x, 1.055 * x ** (1.0 / 2.4) - 0.055) * 255.0)


def lab8_to_rgb8(L8, a8, b8):
    L = L8.astype(np.float64) * (100.0 / 255.0); a = a8.astype(np.float64) - 128.0; b = b8.astype(np.float64) - 128.0
    low = L <= 0.008856 * 903.3
    fy = np.where(low, 7.787 * (L / 903.3) + 16.0 / 116.0, (L + 16.0) / 116.0)
    Y = np.where(low, L / 903.3, fy * fy * fy)
    th = 7.787 * 0.008856 + 16.0 / 116.0
    fx = fy + a / 500.0; fz = fy - b / 200.0
    fx = np.where(fx > th, fx * fx * fx, (fx - 16.0 / 116.0) / 7.787)
    fz = np.where(fz > th, fz * fz * fz, (fz - 16.0 / 116.0) / 7.787)
    X = fx * 0.950456; Z = fz * 1.088754
    return np.stack([_srgb8(3.240479 * X - 1.53715 * Y - 0.498535 * Z), _srgb8(-0.969256 * X + 1.875991 * Y + 0.041556 * Z),
                     _srgb8(0.055648 * X - 0.204043 * Y + 1.057311 * Z)], -1)


# ------------------------------------------------------------------------------------------------ CLAHE
def clahe_tile_lut(hist, clip, area):
    """One tile: clip at max(int(clip * area / 256), 1), redistribute the excess uniformly, spread the residual at a stride of
    max(256 // residual, 1) from bin 0, then LUT = saturate_cast<uchar>(cdf * (255.f / area))."""
    h = np.asarray(hist, dtype=np.int64).copy()
    limit = max(int(float(np.float32(clip)) * area / 256), 1)
    clipped = int(np.maximum(h - limit, 0).sum())
    h = np.minimum(h, limit)
    batch = clipped // 256
    residual = clipped - batch * 256
    h += batch
    if residual:
        h[np.arange(0, 256, max(256 // residual, 1))[:residual]] += 1
    return sat_rint_u8(np.cumsum(h).astype(np.float32) * (np.float32(255) / np.float32(area)))


def clahe_luts(L, clip):
    """-> (luts [8, 8, 256] uint8, tile height, tile width).  An image whose sides are not both multiples of 8 is first extended at
    the bottom and right by 8 - side % 8 (8 when the side is a multiple) with reflect-101, as cv2 does."""
    H, W = L.shape
    ext = L
    if H % 8 or W % 8:
        ext = np.pad(L, ((0, 8 - H % 8), (0, 8 - W % 8)), mode='reflect')
    th, tw = ext.shape[0] // 8, ext.shape[1] // 8
    luts = np.zeros((8, 8, 256), dtype=np.uint8)
    for ty in range(8):
        for tx in range(8):
            tile = ext[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw]
            luts[ty, tx] = clahe_tile_lut(np.bincount(tile.ravel(), minlength=256), clip, th * tw)
    return luts, th, tw


def clahe_apply(L, luts, th, tw):
    f = np.float32

    def axis(n, t):
        tf = np.arange(n).astype(f) * (f(1) / f(t)) - f(0.5)
        t1 = np.floor(tf).astype(np.int64)
        a = tf - t1.astype(f)
        return np.maximum(t1, 0), np.minimum(t1 + 1, 7), a, f(1) - a
    y1, y2, ya, ya1 = axis(L.shape[0], th)
    x1, x2, xa, xa1 = axis(L.shape[1], tw)
    Y1, Y2, X1, X2 = y1[:, None], y2[:, None], x1[None, :], x2[None, :]
    g = lambda ty, tx: luts[ty, tx, L].astype(f)                                          # noqa: E731
    res = (g(Y1, X1) * xa1[None, :] + g(Y1, X2) * xa[None, :]) * ya1[:, None] + \
          (g(Y2, X1) * xa1[None, :] + g(Y2, X2) * xa[None, :]) * ya[:, None]
    return sat_rint_u8(res)


def clahe_rgb(img, clip):
    """albumentations CLAHE on RGB: cv2's CLAHE on the L channel of uint8 LAB, then back to RGB."""
    L, a, b = rgb_to_lab8(img)
    luts, th, tw = clahe_luts(L, clip)
    return lab8_to_rgb8(clahe_apply(L, luts, th, tw), a, b)


# ------------------------------------------------------------------------------------------------ chains
def normalize(img):
    m = np.asarray(MEAN, dtype=np.float32) * np.float32(255)
    inv = np.reciprocal(np.asarray(STD, dtype=np.float32) * np.float32(255), dtype=np.float32)
    return (img.astype(np.float32) - m) * inv


def train_stages(img, row, S):
    """One image through the 'train' chain with table row `row` -> dict of uint8 stages 'a' (LongestMaxSize + pad), 'b'
    (crop / Flip / Transpose / colour), 'L' (CLAHE's input L, zeros when CLAHE is off), 'final' (after the last flips) and the
    normalised fp32 'out' [S, S, 3]."""
    r = lambda n: row[AUG[n]]                                                             # noqa: E731
    a = pad_centre(longest_max_size(img, S), S)
    x = a
    if r('rrc'):
        y0, x0, h, w = (int(r(n)) for n in ('crop_y', 'crop_x', 'crop_h', 'crop_w'))
        x = resize_u8(x[y0:y0 + h, x0:x0 + w], S, S)
    if r('flip'):
        x = cv2_flip(x, int(r('flip_code')))
    if r('transpose'):
        x = x.transpose(1, 0, 2)
    color, shift = int(r('color')), int(r('shift'))
    if color == 1:
        x = brightness_contrast_lut(r('alpha'), r('beta'))[x]
    elif color == 2:
        x = gamma_lut(r('gamma'))[x]
    if shift == 1:
        x = np.stack([rgb_shift_lut(r(n))[x[..., c]] for c, n in enumerate(('r_shift', 'g_shift', 'b_shift'))], -1)
    elif shift == 2:
        x = hsv_shift(x, r('hue_shift'), r('sat_shift'), r('val_shift'))
    b = np.ascontiguousarray(x)
    L = np.zeros(b.shape[:2], dtype=np.uint8)
    if r('clahe'):
        L = rgb_to_lab8(b)[0]
        x = clahe_rgb(b, r('clip_limit'))
    if r('hflip'):
        x = x[:, ::-1]
    if r('vflip'):
        x = x[::-1]
    final = np.ascontiguousarray(x)
    return {'a': a, 'b': b, 'L': L, 'final': final, 'out': normalize(final)}


def valid_stages(img, H, W):
    u = resize_u8(img, W, H)
    return {'a': u, 'final': u, 'out': normalize(u)}


def _flip_x(bx, S):
    return np.stack([S - bx[:, 2], bx[:, 1], S - bx[:, 0], bx[:, 3]], 1)


def _flip_y(bx, S):
    return np.stack([bx[:, 0], S - bx[:, 3], bx[:, 2], S - bx[:, 1]], 1)


def boxes(annot, hw, row, H, W, min_area=0.0, min_visibility=0.0):
    """pascal_voc boxes [n, 5] of one image through the chain's geometry (row None: the stretch resize to H x W), clipped to
    the output and filtered (unclipped area 0, clipped / unclipped < min_visibility, clipped area <= min_area) -> [k, 5] fp32,
    kept rows in input order."""
    a = np.asarray(annot, dtype=np.float32).reshape(-1, 5)
    a = a[a[:, 4] != -1]
    h, w = hw
    bx = a[:, :4].astype(np.float64)
    if row is None:
        bx = bx * np.array([W / w, H / h, W / w, H / h])
    else:
        S = H
        r = lambda n: row[AUG[n]]                                                         # noqa: E731
        rh, rw = lms_dims(h, w, S)
        f = np.array([rw / w, rh / h, rw / w, rh / h])
        bx = bx * f + np.array([(S - rw) // 2, (S - rh) // 2, (S - rw) // 2, (S - rh) // 2], dtype=np.float64)
        if r('rrc'):
            y0, x0, ch, cw = (int(r(n)) for n in ('crop_y', 'crop_x', 'crop_h', 'crop_w'))
            bx = (bx - np.array([x0, y0, x0, y0])) * np.array([S / cw, S / ch, S / cw, S / ch])
        if r('flip'):
            code = int(r('flip_code'))
            if code != 0:
                bx = _flip_x(bx, S)
            if code != 1:
                bx = _flip_y(bx, S)
        if r('transpose'):
            bx = bx[:, [1, 0, 3, 2]]
        if r('hflip'):
            bx = _flip_x(bx, S)
        if r('vflip'):
            bx = _flip_y(bx, S)
    area = (bx[:, 2] - bx[:, 0]) * (bx[:, 3] - bx[:, 1])
    cb = np.stack([np.clip(bx[:, 0], 0, W), np.clip(bx[:, 1], 0, H), np.clip(bx[:, 2], 0, W), np.clip(bx[:, 3], 0, H)], 1)
    clipped = (cb[:, 2] - cb[:, 0]) * (cb[:, 3] - cb[:, 1])
    with np.errstate(divide='ignore', invalid='ignore'):
        keep = (area != 0) & ~(clipped / np.where(area != 0, area, 1) < min_visibility) & ~(clipped <= min_area)
    return np.concatenate([cb[keep].astype(np.float32), a[keep, 4:5]], 1)
