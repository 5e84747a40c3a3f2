"""CPU tier of the device-side get_augumentation: the NumPy restatement (tests/augment_restated.py) on hand-derived cases, and the
host sampler of data.DeviceAugmentation (statistics, ranges, reproducibility).  No GPU."""
import numpy as np
import pytest

from efficientdet.pytorch_amd import data as D
from tests import augment_restated as R


def row(**kw):
    r = np.zeros(len(D.AUG_COLUMNS), dtype=np.float32)
    for k, v in kw.items():
        r[D.AUG[k]] = v
    return r


def test_lut_entries():
    g = R.gamma_lut(2.0)                               # (i / 255) ** 2 * 255, truncated
    assert (g[0], g[128], g[255]) == (0, 64, 255)      # 128 ** 2 / 255 = 64.25
    bc = R.brightness_contrast_lut(1.0, 0.1)           # i + 25.5, clipped, truncated
    assert (bc[0], bc[100], bc[250]) == (25, 125, 255)
    bc = R.brightness_contrast_lut(1.5, 0.0)
    assert (bc[100], bc[200]) == (150, 255)
    bc = R.brightness_contrast_lut(0.5, -0.2)          # i / 2 - 51
    assert (bc[50], bc[103], bc[255]) == (0, 0, 76)
    s = R.rgb_shift_lut(-10.5)
    assert (s[5], s[100], s[255]) == (0, 89, 244)
    h = R.hue_lut(-3.5)                                # mod 180
    assert (h[0], h[10], h[179]) == (176, 6, 175)
    assert (R.sat_val_lut(20)[250], R.sat_val_lut(-20)[10]) == (255, 0)


def test_hsv_of_greys_and_primaries():
    px = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [7, 7, 7], [200, 200, 200], [255, 255, 0]], np.uint8)
    h, s, v = R.rgb_to_hsv8(px)
    assert h.tolist() == [0, 60, 120, 0, 0, 30] and s.tolist() == [255, 255, 255, 0, 0, 255] and v.tolist() == [255, 255, 255, 7, 200, 255]
    assert (R.hsv8_to_rgb8(h, s, v) == px).all()        # exact round trip for these
    assert (R.hsv_shift(px, 0, 0, 0) == px).all()
    out = R.hsv_shift(px[3:5], 0, 0, 20)                  # a value shift keeps greys grey
    assert out.tolist() == [[27, 27, 27], [220, 220, 220]]


def test_clahe_of_a_constant_image():
    # 64 x 64 of L = 100: 8 x 8 tiles of area 64, clip max(int(2 * 64 / 256), 1) = 1 -> 63 excess, batch 0, residual 63 at
    # stride 256 // 63 = 4 (bins 0, 4, ..., 248).  cdf[100] = 26 residual ones + 1 clipped = 27 -> rint(27 * 255 / 64) = 108.
    L = np.full((64, 64), 100, np.uint8)
    luts, th, tw = R.clahe_luts(L, 2.0)
    assert (th, tw) == (8, 8) and (luts[:, :, 100] == 108).all()
    assert (R.clahe_apply(L, luts, th, tw) == 108).all()


def test_clahe_one_tile_with_a_known_histogram():
    # area 256, bin 10: 200, bin 20: 56; clip 4 -> limit 4, excess 196 + 52 = 248 -> batch 0, residual 248 at stride 1:
    # bins 0..247 + 1.  cdf[0] = 1, cdf[10] = 11 - 1 + 5 = 15, cdf[20] = 29, cdf[255] = 256.
    hist = np.zeros(256, np.int64); hist[10] = 200; hist[20] = 56
    lut = R.clahe_tile_lut(hist, 4.0, 256)
    assert (lut[0], lut[9], lut[10], lut[20], lut[247], lut[255]) == (1, 10, 15, 29, 255, 255)
    # a histogram under the limit is a plain equalisation: 256 px spread evenly -> rint((i + 1) * 255 / 256), half to even:
    # i = 127 gives 127.5 -> 128, i = 126 gives 126.50390625 -> 127
    flat = R.clahe_tile_lut(np.ones(256, np.int64), 4.0, 256)
    assert (flat[0], flat[126], flat[127], flat[255]) == (1, 127, 128, 255)
    # redistribution batch: 1024 px in one bin, limit 4 * 1024 / 256 = 16 -> excess 1008 = 3 * 256 + 240
    h = np.zeros(256, np.int64); h[0] = 1024
    lut = R.clahe_tile_lut(h, 4.0, 1024)
    assert lut[0] == np.rint(np.float32(16 + 3 + 1) * np.float32(255 / 1024))


def test_clahe_reflect101_extension():
    rng = np.random.RandomState(3)
    L = rng.randint(0, 256, (20, 20)).astype(np.uint8)           # 20 % 8 = 4: extended to 24, tiles of 3
    luts, th, tw = R.clahe_luts(L, 3.0)
    assert (th, tw) == (3, 3)
    ext = np.pad(L, ((0, 4), (0, 4)), mode='reflect')
    assert ext[20, 0] == L[18, 0] and ext[23, 23] == L[15, 15]
    last = ext[21:24, 21:24]
    assert (luts[7, 7] == R.clahe_tile_lut(np.bincount(last.ravel(), minlength=256), 3.0, 9)).all()


def test_box_steps():
    S = 100
    ann = np.array([[10, 20, 30, 60, 3]], np.float32)
    hw = (100, 100)
    assert np.allclose(R.boxes(ann, hw, row(), S, S), [[10, 20, 30, 60, 3]])
    assert np.allclose(R.boxes(ann, hw, row(hflip=1), S, S), [[70, 20, 90, 60, 3]])
    assert np.allclose(R.boxes(ann, hw, row(vflip=1), S, S), [[10, 40, 30, 80, 3]])
    assert np.allclose(R.boxes(ann, hw, row(flip=1, flip_code=-1), S, S), [[70, 40, 90, 80, 3]])
    assert np.allclose(R.boxes(ann, hw, row(flip=1, flip_code=0), S, S), [[10, 40, 30, 80, 3]])
    assert np.allclose(R.boxes(ann, hw, row(transpose=1), S, S), [[20, 10, 60, 30, 3]])
    # LongestMaxSize: 50 x 200 -> 25 x 100 (x0.5), padded to the middle rows: top = 37
    assert np.allclose(R.boxes(np.array([[0, 0, 200, 50, 1]]), (50, 200), row(), S, S), [[0, 37, 100, 62, 1]])
    # crop (y 10, x 0, 50 x 50) -> x2 scale: (10, 20, 30, 60) -> (20, 20, 60, 100)
    assert np.allclose(R.boxes(ann, hw, row(rrc=1, crop_y=10, crop_x=0, crop_h=50, crop_w=50), S, S), [[20, 20, 60, 100, 3]])
    # clipped: crop (y 50, x 0, 50 x 50): y (20, 60) -> (-60, 20) clipped to (0, 20): 1/4 visible
    crop = row(rrc=1, crop_y=50, crop_x=0, crop_h=50, crop_w=50)
    assert np.allclose(R.boxes(ann, hw, crop, S, S), [[20, 0, 60, 20, 3]])
    assert len(R.boxes(ann, hw, crop, S, S, min_visibility=0.3)) == 0
    assert len(R.boxes(ann, hw, crop, S, S, min_visibility=0.25)) == 1
    assert len(R.boxes(ann, hw, crop, S, S, min_area=800)) == 0 and len(R.boxes(ann, hw, crop, S, S, min_area=799)) == 1
    # dropped: outside the crop; kept rows keep their order; padding rows ignored
    many = np.array([[60, 60, 70, 70, 1], [10, 20, 30, 60, 2], [-1, -1, -1, -1, -1], [0, 90, 10, 100, 4]], np.float32)
    got = R.boxes(many, hw, row(rrc=1, crop_y=0, crop_x=0, crop_h=50, crop_w=50), S, S)
    assert got[:, 4].tolist() == [2]
    got = R.boxes(many, hw, row(hflip=1), S, S)
    assert got[:, 4].tolist() == [1, 2, 4]
    # stretch resize ('valid'): per-axis scales
    assert np.allclose(R.boxes(np.array([[10, 20, 30, 40, 3]]), (50, 200), None, 100, 400), [[20, 40, 60, 80, 3]])


def test_sampler_statistics():
    N, S = 20000, 512
    t = D.sample_augment_table(np.random.RandomState(0), N, S)
    c = lambda n: t[:, D.AUG[n]]                                              # noqa: E731
    tol = 4 * np.sqrt(0.25 / N)
    assert abs(c('rrc').mean() - 0.3) < tol
    assert abs(c('clahe').mean() - 0.8) < tol
    for n in ('flip', 'transpose', 'hflip', 'vflip'):
        assert abs(c(n).mean() - 0.5) < tol, n
    for n in ('color', 'shift'):
        for code in (1, 2, 3):
            assert abs((c(n) == code).mean() - 1 / 6) < tol, (n, code)
        assert abs((c(n) == 0).mean() - 0.5) < tol
    on = c('rrc') == 1
    y, x, h, w = (c(n)[on] for n in ('crop_y', 'crop_x', 'crop_h', 'crop_w'))
    assert (h >= 1).all() and (w >= 1).all() and (y >= 0).all() and (x >= 0).all() and (y + h <= S).all() and (x + w <= S).all()
    assert (h == np.round(h)).all() and (w == np.round(w)).all()
    assert ((h * w) >= 0.08 * S * S * 0.9).all()
    assert set(np.unique(c('flip_code')[c('flip') == 1])) == {-1, 0, 1}
    bc, gm = c('color') == 1, c('color') == 2
    assert (np.abs(c('alpha')[bc] - 1) <= 0.4).all() and (np.abs(c('beta')[bc]) <= 0.5).all()
    assert (c('gamma')[gm] >= 0.5).all() and (c('gamma')[gm] <= 1.5).all()
    rgb, hsv = c('shift') == 1, c('shift') == 2
    assert (np.abs(c('r_shift')[rgb]) <= 20).all() and (np.abs(c('g_shift')[rgb]) <= 15).all() and (np.abs(c('b_shift')[rgb]) <= 15).all()
    assert (np.abs(c('hue_shift')[hsv]) <= 5).all() and (np.abs(c('sat_shift')[hsv]) <= 5).all() and (np.abs(c('val_shift')[hsv]) <= 20).all()
    cl = c('clahe') == 1
    assert (c('clip_limit')[cl] >= 1).all() and (c('clip_limit')[cl] <= 4).all()
    assert (c('clip_limit')[~cl] == 0).all() and (c('alpha')[~bc] == 0).all()


def test_sampler_is_reproducible():
    a = D.sample_augment_table(np.random.RandomState(7), 64, 512)
    b = D.sample_augment_table(np.random.RandomState(7), 64, 512)
    c = D.sample_augment_table(np.random.RandomState(8), 64, 512)
    assert (a == b).all() and not (a == c).all()


def test_table_check():
    good = np.stack([row(rrc=1, crop_y=10, crop_x=0, crop_h=50, crop_w=502), row(flip=1, flip_code=-1)])
    assert D.check_augment_table(good, 2, 512).dtype == np.float32
    with pytest.raises(ValueError):
        D.check_augment_table(good, 3, 512)
    with pytest.raises(ValueError):
        D.check_augment_table(np.stack([row(rrc=1, crop_y=10, crop_x=20, crop_h=50, crop_w=500), row()]), 2, 512)
    with pytest.raises(ValueError):
        D.check_augment_table(np.stack([row(rrc=1, crop_y=0, crop_x=0, crop_h=50.5, crop_w=50), row()]), 2, 512)
    with pytest.raises(ValueError):
        D.check_augment_table(np.stack([row(flip=1, flip_code=2), row()]), 2, 512)


def test_phase_arguments():
    with pytest.raises(ValueError):
        D.DeviceAugmentation('train', width=512, height=256, device='cpu')
    with pytest.raises(ValueError):
        D.DeviceAugmentation('eval', device='cpu')


def test_restatement_against_albumentations():
    """Where albumentations and cv2 import: the restatement at injected parameters against the real transforms.  Exact for the
    LUT and index-permutation ops; within one level where cv2's fixed-point conversions differ from the restated formulas."""
    A = pytest.importorskip('albumentations')
    pytest.importorskip('cv2')
    F = A.augmentations.functional
    rng = np.random.RandomState(0)
    img = rng.randint(0, 256, (64, 64, 3)).astype(np.uint8)
    assert (F.brightness_contrast_adjust(img, 1.2, 0.1, True) == R.brightness_contrast_lut(1.2, 0.1)[img]).all()
    assert (F.gamma_transform(img, 1.3) == R.gamma_lut(1.3)[img]).all()
    assert (F.transpose(img) == img.transpose(1, 0, 2)).all()
    for code in (-1, 0, 1):
        assert (F.random_flip(img, code) == R.cv2_flip(img, code)).all()
    assert np.abs(F.shift_hsv(img, 3, -2, 10).astype(int) - R.hsv_shift(img, 3, -2, 10).astype(int)).max() <= 1
    assert np.abs(F.clahe(img, 2.0, (8, 8)).astype(int) - R.clahe_rgb(img, 2.0).astype(int)).max() <= 2
    assert np.abs(F.resize(img, 40, 50).astype(int) - R.resize_u8(img, 50, 40).astype(int)).max() <= 1
