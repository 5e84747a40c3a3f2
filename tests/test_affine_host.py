"""CPU tier of the affine / perspective warp: the NumPy restatement (tests/affine_restated.py) against results derived without its
sampler (slicing, padding, integer arithmetic, boxes by hand), the binding's table and columns against include/effdet_affine.h, the
options' validation, every refusal of check_affine_table, the table sampler, the host-side EINVAL returns, and every case of
tests/affine_cases.py reaching what it is tagged with."""
import math
import os
import re

import numpy as np
import pytest

from efficientdet.pytorch_amd import data
from efficientdet.pytorch_amd.data import AFFINE, AFFINE_COLUMNS
from tests import augment_restated as A
from tests import affine_restated as R
from tests.affine_cases import CASES, _row, margins, shift

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BY_NAME = {c['name']: c for c in CASES}


def _shifted(img, tx, ty, S, fill):
    """img moved by the integers (tx, ty) on an S x S canvas of `fill`, by slicing."""
    h, w = img.shape[:2]
    out = np.full((S, S, 3), fill, dtype=np.uint8)
    xs, xe, ys, ye = max(tx, 0), min(tx + w, S), max(ty, 0), min(ty + h, S)
    if xe > xs and ye > ys:
        out[ys:ye, xs:xe] = img[ys - ty:ye - ty, xs - tx:xe - tx]
    return out


def test_identity_translations_mirror_and_transpose_by_slicing():
    c = BY_NAME['identity']
    assert np.array_equal(R.warp(c['imgs'][0], c['table'][0], 32, 114), c['imgs'][0])
    c = BY_NAME['integer_translations']
    for b, (tx, ty) in enumerate(((3, -5), (-7, 2), (31, 31))):
        assert np.array_equal(R.warp(c['imgs'][b], c['table'][b], 32, c['fill']), _shifted(c['imgs'][b], tx, ty, 32, c['fill'])), b
    c = BY_NAME['mirror_and_transpose']
    assert np.array_equal(R.warp(c['imgs'][0], c['table'][0], 32, 114), c['imgs'][0][:, ::-1])
    assert np.array_equal(R.warp(c['imgs'][1], c['table'][1], 32, 114), _shifted(c['imgs'][1].transpose(1, 0, 2), 0, 0, 32, 114))
    # a larger source under the identity is cropped at the top-left corner; a smaller one is padded with fill, not zeros
    big = np.random.RandomState(1).randint(0, 256, (50, 40, 3)).astype(np.uint8)
    assert np.array_equal(R.warp(big, shift(0, 0), 32, 9), big[:32, :32])
    assert np.array_equal(R.warp(big[:5, :7], shift(0, 0), 32, 9), _shifted(big[:5, :7], 0, 0, 32, 9))


def test_half_pixel_ties_round_up_by_integer_arithmetic():
    # a shift by 2.5 along x: output x samples u = x - 2.5, the mean of the pixels x - 3 and x - 2 (fill outside), rounded half up
    c = BY_NAME['half_integer_translations']
    img, fill = c['imgs'][0].astype(np.int64), c['fill']
    ring = np.full((32, 32 + 4, 3), fill, dtype=np.int64); ring[:, 3:35] = img[:, :32]          # ring[:, k] = source x = k - 3
    want = (ring[:, 0:32] + ring[:, 1:33] + 1) // 2
    got = R.warp(c['imgs'][0], c['table'][0], 32, fill)
    assert np.array_equal(got, want) and ((ring[:, 0:32] + ring[:, 1:33]) % 2 == 1).any()
    # the 2x scale: u = x / 2.  Even (x, y) copy; one odd coordinate is the half-up mean of two neighbours; both odd, of four
    c = BY_NAME['scale_2x_and_half']
    src = np.full((17, 17, 3), c['fill'], dtype=np.int64); src[:16, :16] = c['imgs'][0]
    a, b_, c_, d = src[:16, :16], src[:16, 1:17], src[1:17, :16], src[1:17, 1:17]
    want = np.zeros((32, 32, 3), dtype=np.int64)
    want[0::2, 0::2], want[0::2, 1::2], want[1::2, 0::2], want[1::2, 1::2] = a, (a + b_ + 1) // 2, (a + c_ + 1) // 2, (a + b_ + c_ + d + 2) // 4
    assert np.array_equal(R.warp(c['imgs'][0], c['table'][0], 32, c['fill']), want)
    # the 1/2 scale: u = 2 x lands on pixel centres, so it is a decimation
    assert np.array_equal(R.warp(c['imgs'][1], c['table'][1], 32, c['fill']), c['imgs'][1][::2, ::2])


def test_pass_through_is_the_chains_own_stage_a():
    rng = np.random.RandomState(3)
    off = _row(on=0)
    for h, w in ((90, 70), (5, 7), (64, 64), (1, 1), (17, 64), (200, 150)):
        img = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        want = A.train_stages(img, np.zeros(len(data.AUG_COLUMNS), dtype=np.float32), 64)['a']
        assert np.array_equal(R.warp(img, off, 64, 114), want)
        bx = np.array([[0, 0, w, h, 3], [-1, -1, -1, -1, -1], [0.25, 0.5, 0.75, 1, 0]], dtype=np.float32)   # inside: the chain clips nothing
        got = R.boxes(bx, (h, w), off, 64, 1e9, 0.0, 1e9)             # a pass-through row is not filtered, whatever the thresholds
        assert np.array_equal(got, A.boxes(bx, (h, w), np.zeros(len(data.AUG_COLUMNS), dtype=np.float32), 64, 64))


def test_boxes_by_hand():
    c = BY_NAME['boxes_by_hand']
    kw = dict(S=64, wh_thr=2.0, ar_thr=12.0, area_thr=0.25)
    got = R.boxes(c['annots'][0], (64, 64), c['table'][0], **kw)
    assert got.tolist() == [[4, 4, 12, 12, 0], [0, 10, 10, 30, 2], [10, 10, 12.5, 30, 4], [0, 0, 60, 5.5, 5], [0, 10, 10, 30, 7]]
    # each dropped row falls to one threshold: relax that one alone and the row comes back
    assert [r[4] for r in R.boxes(c['annots'][0], (64, 64), c['table'][0], 64, 1.5, 12.0, 0.25).tolist()] == [0, 2, 3, 4, 5, 7]
    assert [r[4] for r in R.boxes(c['annots'][0], (64, 64), c['table'][0], 64, 2.0, 14.0, 0.25).tolist()] == [0, 2, 4, 5, 6, 7]
    assert [r[4] for r in R.boxes(c['annots'][0], (64, 64), c['table'][0], 64, 2.0, 12.0, 0.2).tolist()] == [0, 2, 4, 5, 7, 8]
    # the perspective row: X = x / (1 - x / 32), Y = y / (1 - x / 32).  (4, 4, 12, 12): d = 0.875 at x = 4 and 0.625 at x = 12
    got = R.boxes(c['annots'][1], (64, 64), c['table'][1], **kw)
    want = [[4 / 0.875, 4 / 0.875, 12 / 0.625, 12 / 0.625, 0], [8 / 0.75, 20 / 0.75, 64, 64, 3]]
    assert got.shape == (2, 5) and np.array_equal(got, np.asarray(want, dtype=np.float32))
    # a scale column of 1.9 divides every area ratio by 3.61: the whole boxes (1 / 3.61 = 0.277) stay, the clipped ones (0.625 and
    # 0.263 at scale 1) fall below 0.25; at 2 the whole boxes sit on 0.25 exactly and `>` drops them too
    row = c['table'][0].copy(); row[AFFINE['scale']] = 1.9
    assert [r[4] for r in R.boxes(c['annots'][0], (64, 64), row, **kw).tolist()] == [0, 4, 5]
    row[AFFINE['scale']] = 2.0
    assert len(R.boxes(c['annots'][0], (64, 64), row, **kw)) == 0
    # under a general matrix the new box is the bounding box of the four corners: a rotation by 90 degrees about the origin plus a
    # shift by 40, (x, y) -> (40 - y, x), takes (2, 4, 10, 20) to (20, 2, 36, 10)
    rot = _row([[0, -1, 40], [1, 0, 0]], [[0, 1, 0], [-1, 0, 40]], 1.0)
    assert R.boxes([[2, 4, 10, 20, 6]], (64, 64), rot, 64, 2.0, 100.0, 0.1).tolist() == [[20, 2, 36, 10, 6]]


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'effdet_affine.h')).read(), flags=re.S)


def test_signatures_and_columns_match_the_header():
    """_lib.AFFINE_SIGNATURES against the prototypes of include/effdet_affine.h (names, return kind, parameter kinds in order), the
    column enum against AFFINE_COLUMNS, and the built library exports and binds both entry points."""
    from efficientdet.pytorch_amd import build, _lib, ops
    h = _header()
    scalar = {'int': 'i', 'long long': 'q', 'float': 'f', 'double': 'd', 'effdet_stream_t': 'p'}
    protos = {}
    for r, name, params in re.findall(r'^([a-z][a-z ]*?\*?)\s*\b(effdet_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', h, flags=re.M):
        kinds = ['p' if '*' in p else scalar[' '.join(p.split()).rsplit(' ', 1)[0]] for p in params.split(',')]
        assert name not in protos, name
        protos[name] = ({'int': 'i', 'long long': 'q'}[' '.join(r.split())], kinds)
    assert sorted(protos) == ['effdet_affine_boxes', 'effdet_affine_warp']
    others = [getattr(_lib, n) for n in dir(_lib) if n.endswith('SIGNATURES') and n != 'AFFINE_SIGNATURES']
    assert len(others) >= 12 and sorted(_lib.AFFINE_SIGNATURES) == sorted(protos) and not any(set(protos) & set(t) for t in others)
    build.build(verbose=False)
    L = _lib.require(*protos)
    for name, (r, kinds) in protos.items():
        sig = _lib.AFFINE_SIGNATURES[name]
        assert sig[1] == ':' and sig[0] == r, (name, sig, r)
        assert list(sig[2:].replace('s', 'p')) == kinds, (name, sig, ''.join(kinds))
        assert sig.endswith('s') and 'effdet_stream_t stream' in re.search(name + r'\s*\(([^)]*)\)', h).group(1)
        f = getattr(L, name)
        assert f.restype is _lib._CTYPE[sig[0]] and list(f.argtypes) == [_lib._CTYPE[c] for c in sig[2:]], name
    P = int(re.search(r'#define\s+EFFDET_AFFINE_P\s+(\d+)', h).group(1))
    enum = [e.strip() for e in re.search(r'enum\s*\{(.*?)\}', h, flags=re.S).group(1).split(',')]
    assert enum[0] == 'EFFDET_AFFINE_ON = 0' and all('=' not in e for e in enum[1:])
    names = [e.split('=')[0].strip()[len('EFFDET_AFFINE_'):].lower() for e in enum]
    assert tuple(names) == AFFINE_COLUMNS and P == len(AFFINE_COLUMNS) == ops.AFFINE_P == 20 and AFFINE == {n: i for i, n in enumerate(names)}
    assert '-ffp-contract=off' in build.PER_FILE['affine.hip']     # separately rounded fp64 products and fp32 blends: no FMA contraction
    # the generation and the first header's table did not move
    assert _lib.ABI_VERSION == 11 and not set(protos) & set(_lib.SIGNATURES)
    doc = open(os.path.join(ROOT, 'include', 'effdet_affine.h')).read()
    for phrase in ('on == 0, pass-through', 'pixel centres', 'constant border', 'round half up', 'box_candidates', 'left to right'):
        assert phrase in doc, phrase


def test_einval_returns_launch_nothing():
    """The refusals of both entry points are decided on the host, before any launch: they return on a machine without a device."""
    from efficientdet.pytorch_amd import build, _lib
    build.build(verbose=False)
    L = _lib.require('effdet_affine_warp', 'effdet_affine_boxes')
    buf = np.zeros(4096, dtype=np.uint8)
    p = buf.ctypes.data
    for B, S, fill in ((0, 32, 114), (-1, 32, 114), (2, 7, 114), (2, 0, 114), (2, 32, -1), (2, 32, 256), (65536, 32, 114), (1, 1 << 16, 114),
                       (1, 32769, 0)):
        assert L.effdet_affine_warp(p, p, p, p, B, S, fill, p, None) == -1, (B, S, fill)
    for B, S, M in ((0, 32, 4), (2, 7, 4), (2, 32, 0), (2, 32, -3), (65536, 32, 4), (2, 1 << 16, 4)):
        assert L.effdet_affine_boxes(p, p, B, S, p, M, 2.0, 100.0, 0.1, p, p, None) == -1, (B, S, M)
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert L.effdet_affine_warp(*args, 2, 32, 114, p, None) == -1
    assert L.effdet_affine_warp(p, p, p, p, 2, 32, 114, None, None) == -1
    for k in range(5):
        a = [p] * 5; a[k] = None
        assert L.effdet_affine_boxes(a[0], a[1], 2, 32, a[2], 4, 2.0, 100.0, 0.1, a[3], a[4], None) == -1, k
    assert not buf.any()


def test_options_validate_their_arguments():
    o = data.AffineOptions()
    assert o.key() == (1.0, 0.0, 0.1, (0.5, 1.5), 0.0, 0.0, 114, 2.0, 100.0, 0.1, 1)
    assert o == data.AffineOptions() and hash(o) == hash(data.AffineOptions()) and o != data.AffineOptions(fill=0)
    assert o != data.AffineOptions(canvas=2) and 'canvas=1' in repr(o) and 'area_thr=0.1' in repr(o)
    for bad in (dict(p=-0.1), dict(p=1.5), dict(p=float('nan')), dict(degrees=-1), dict(degrees=181), dict(degrees=float('nan')),
                dict(translate=-0.1), dict(translate=0.6), dict(scale=(0.0, 1.0)), dict(scale=(1.5, 0.5)), dict(scale=(0.5,)),
                dict(scale=(0.5, float('inf'))), dict(shear=90), dict(shear=-1), dict(perspective=-0.001), dict(perspective=float('inf')),
                dict(fill=-1), dict(fill=256), dict(fill=1.5), dict(fill=True), dict(wh_thr=-1), dict(ar_thr=0), dict(area_thr=-0.1),
                dict(area_thr=float('nan')), dict(canvas=0), dict(canvas=3), dict(canvas=True), dict(canvas=1.5)):
        with pytest.raises(ValueError):
            data.AffineOptions(**bad)
    for phase in ('valid', 'test'):
        with pytest.raises(ValueError, match="'train'"):
            data.DeviceAugmentation(phase=phase, affine=o, device='cpu')
    with pytest.raises(TypeError):
        data.DeviceAugmentation(phase='train', affine=True, device='cpu')
    with pytest.raises(ValueError, match='needs mosaic'):
        data.DeviceAugmentation(phase='train', affine=data.AffineOptions(canvas=2), device='cpu')
    aug = data.DeviceAugmentation(phase='train', width=64, height=64, device='cpu', mosaic=data.MosaicOptions(), affine=data.AffineOptions(canvas=2))
    assert aug.affine.canvas == 2
    one = [{'img': np.zeros((4, 4, 3), dtype=np.uint8), 'annot': np.zeros((0, 5))}]
    aug.mosaic = None                                                                      # set after construction: refused at the call
    with pytest.raises(ValueError, match='needs mosaic'):
        aug(one)
    aug = data.DeviceAugmentation(phase='train', width=64, height=64, device='cpu')
    assert aug.affine is None
    with pytest.raises(ValueError, match='no affine options'):
        aug(one, affine_table=np.zeros((1, 20)))
    aug = data.DeviceAugmentation(phase='valid', width=64, height=64, device='cpu')
    aug.affine = o
    with pytest.raises(ValueError, match="'train'"):
        aug(one)


def test_every_refusal_of_check_affine_table():
    B, S = 3, 32
    rng = np.random.RandomState(4)
    from tests.affine_cases import generic
    good = np.stack([generic(rng, 90, 70, S, perspective=0.001), _row(on=0), shift(2.5, -3)])
    out = data.check_affine_table(good, B, S)
    assert out.dtype == np.float64 and np.array_equal(out, good)
    assert np.array_equal(data.check_affine_table(good.tolist(), B, S), good)

    def refused(row, col, value, match):
        t = good.copy()
        t[row, AFFINE[col]] = value
        with pytest.raises(ValueError, match=r'row %d.*%s' % (row, match)):
            data.check_affine_table(t, B, S)
    with pytest.raises(ValueError, match='must be'):
        data.check_affine_table(good[:2], B, S)
    with pytest.raises(ValueError, match='must be'):
        data.check_affine_table(good[:, :19], B, S)
    refused(0, 'on', 2, '0 or 1'); refused(2, 'on', 0.5, '0 or 1'); refused(1, 'on', np.nan, '0 or 1'); refused(1, 'on', -1, '0 or 1')
    refused(0, 'f3', np.nan, 'finite'); refused(2, 'g8', np.inf, 'finite'); refused(0, 'scale', -np.inf, 'finite')
    refused(0, 'scale', 0.0, 'not positive'); refused(2, 'scale', -1.0, 'not positive')
    refused(0, 'g2', good[0, AFFINE['g2']] + 1e-6, 'not the inverse'); refused(2, 'f0', 1.0 + 1e-8, 'not the inverse')
    refused(2, 'g8', 2.0, 'not the inverse')
    t = good.copy(); t[2, AFFINE['g2']] += 1e-11                                           # inside the bound
    assert data.check_affine_table(t, B, S) is not None
    # a row that is off may hold anything else
    t = good.copy(); t[1, 1:] = np.nan
    assert data.check_affine_table(t, B, S) is not None


def test_sampler_ranges_inverse_and_scale_column():
    B, S, n = 8, 64, 250
    hw = np.array([[90, 70], [200, 150], [1, 17], [1, 1], [64, 64], [33, 64], [64, 17], [500, 375]])
    o = data.AffineOptions(p=0.7, degrees=25.0, translate=0.2, scale=(0.5, 1.5), shear=8.0, perspective=0.001)
    rng = np.random.RandomState(11)
    t = np.concatenate([data.sample_affine_table(rng, B, S, hw, o) for _ in range(n)])
    assert t.shape == (B * n, len(AFFINE_COLUMNS)) and t.dtype == np.float64
    on = t[:, AFFINE['on']] == 1
    assert set(np.unique(t[:, AFFINE['on']])) == {0.0, 1.0} and not t[~on].any()           # nothing is drawn for a row that is off
    assert abs(on.mean() - 0.7) < 5 * np.sqrt(0.7 * 0.3 / len(t))
    assert data.check_affine_table(t[:B], B, S) is not None
    longest = np.tile(hw.max(1), n).astype(np.float64)
    F = t[:, AFFINE['f0']:AFFINE['f8'] + 1].reshape(-1, 3, 3)
    G = t[:, AFFINE['g0']:AFFINE['g8'] + 1].reshape(-1, 3, 3)
    err = np.abs(F[on] @ G[on] - np.eye(3)).sum(2).max()
    assert err <= 1e-9, err
    # the scale column is s * S / max(h, w) with s in the range
    s = t[on, AFFINE['scale']] * longest[on] / S
    assert s.min() >= 0.5 and s.max() <= 1.5 and s.min() < 0.55 and s.max() > 1.45
    # undo the composition: F . inv(C) = T . Sh . R . P has the translation in its last column and the perspective terms in its last row
    for i in np.flatnonzero(on)[:400]:
        h, w = np.tile(hw, (n, 1))[i]
        Ci = np.array([[1, 0, w / 2], [0, 1, h / 2], [0, 0, 1.0]])
        K = F[i] @ Ci
        assert 0.3 * S - 1e-9 <= K[0, 2] <= 0.7 * S + 1e-9 and 0.3 * S - 1e-9 <= K[1, 2] <= 0.7 * S + 1e-9
        assert abs(K[2, 0]) <= 0.001 + 1e-12 and abs(K[2, 1]) <= 0.001 + 1e-12 and abs(K[2, 2] - 1) < 1e-12
        A2 = K[:2, :2] - np.outer(K[:2, 2], K[2, :2])                  # Sh . R: the perspective row's share of the translation removed
        k = t[i, AFFINE['scale']]
        # det(Sh . R) = k^2 (1 - tan(a) tan(b)), shears within 8 degrees
        assert (1 - math.tan(math.radians(8)) ** 2) - 1e-9 <= np.linalg.det(A2) / k ** 2 <= (1 + math.tan(math.radians(8)) ** 2) + 1e-9
    # defaults: no rotation, shear or perspective, so F is a scale and a translation about the centre
    d = data.sample_affine_table(np.random.RandomState(2), B, S, hw, data.AffineOptions())
    assert (d[:, AFFINE['on']] == 1).all() and not d[:, [AFFINE['f1'], AFFINE['f3'], AFFINE['f6'], AFFINE['f7']]].any()
    assert np.array_equal(d[:, AFFINE['f0']], d[:, AFFINE['scale']]) and np.array_equal(d[:, AFFINE['f4']], d[:, AFFINE['scale']])
    # the same seed gives the same table; p = 0 gives all rows off and draws one number per image
    a = data.sample_affine_table(np.random.RandomState(5), B, S, hw, o)
    assert np.array_equal(a, data.sample_affine_table(np.random.RandomState(5), B, S, hw, o))
    r1, r2 = np.random.RandomState(5), np.random.RandomState(5)
    z = data.sample_affine_table(r1, B, S, hw, data.AffineOptions(p=0.0))
    r2.rand(B)
    assert not z.any() and r1.rand() == r2.rand()
    with pytest.raises(ValueError, match='source sizes'):
        data.sample_affine_table(np.random.RandomState(5), B, S, hw[:3], o)


# ------------------------------------------------------------------------------------------------ the cases reach their tags
def _pixels(c):
    """per row that is on: (b, u, v, inside, border taps, d)"""
    for b, row in enumerate(c['table']):
        on, _, G, _ = R.mats(row)
        if on:
            h, w = c['imgs'][b].shape[:2]
            u, v, inside = R.coords(G, c['S'], h, w)
            _, _, border = R.warp(c['imgs'][b], row, c['S'], c['fill'], details=True)
            x, y = np.meshgrid(np.arange(c['S'], dtype=np.float64), np.arange(c['S'], dtype=np.float64))
            with np.errstate(all='ignore'):
                d = (G[2, 0] * x + G[2, 1] * y) + G[2, 2]
            yield b, u, v, inside, border, d, (h, w)


def _infos(c):
    return [i for _, info in margins(c) for i in info]


def _clauses(c, i):
    return (i['ok'], i['w2'] > c['wh_thr'] and i['h2'] > c['wh_thr'], i['ar'] < c['ar_thr'], i['ratio'] > c['area_thr'])


def _on_rows(c):
    return [r for r in c['table'] if r[AFFINE['on']]]


def _tie(c):
    for b, row in enumerate(c['table']):
        if row[AFFINE['on']]:
            h, w = c['imgs'][b].shape[:2]
            u, v, inside = R.coords(R.mats(row)[2], c['S'], h, w)
            if (inside & ((u - np.floor(u) == 0.5) | (v - np.floor(v) == 0.5))).any():
                return True
    return False


def _edges(c):
    seen = set()
    for b, u, v, inside, border, d, (h, w) in _pixels(c):
        for val, name in ((-1.0, '-1'), (-0.5, '-0.5'), (0.0, '0'), (w - 1.0, 'w-1'), (float(w), 'w')):
            if (u == val).any():
                seen.add(name)
                assert not inside[u == val].any() if name in ('-1', 'w') else inside[(u == val) & (v > -1) & (v < h)].all()
    return seen == {'-1', '-0.5', '0', 'w-1', 'w'}


TAGS = {
    'identity': lambda c: np.array_equal(c['table'][0][1:10].reshape(3, 3), np.eye(3)) and c['imgs'][0].shape[:2] == (c['S'], c['S']),
    'interior': lambda c: any((inside & ~border).any() for _, _, _, inside, border, _, _ in _pixels(c)),
    'border_tap': lambda c: any(border.any() for _, _, _, _, border, _, _ in _pixels(c)),
    'all_fill_pixel': lambda c: any((~inside).any() for _, _, _, inside, _, _, _ in _pixels(c)),
    'd_le_0': lambda c: any((d == 0).any() and (d < 0).any() and (d > 0).any() and inside.any() for _, _, _, inside, _, d, _ in _pixels(c)),
    'int_translation': lambda c: all(np.array_equal(r[1:10].reshape(3, 3)[:, :2], np.eye(3)[:, :2]) and r[3] == round(r[3]) and r[6] == round(r[6])
                                     for r in c['table']),
    'tie': _tie,
    'mirror': lambda c: c['table'][0][AFFINE['g0']] == -1,
    'transpose': lambda c: any(r[AFFINE['g0']] == 0 and r[AFFINE['g1']] == 1 and r[AFFINE['g3']] == 1 and r[AFFINE['g4']] == 0 for r in c['table']),
    'scale_2x': lambda c: any(r[AFFINE['f0']] == 2 and r[AFFINE['g0']] == 0.5 for r in c['table']),
    'scale_half': lambda c: any(r[AFFINE['f0']] == 0.5 and r[AFFINE['g0']] == 2 for r in c['table']),
    'generic': lambda c: all(r[AFFINE['f1']] != 0 and r[AFFINE['f3']] != 0 and abs(r[AFFINE['f1']]) != abs(r[AFFINE['f3']]) for r in _on_rows(c)),
    'perspective': lambda c: all(r[AFFINE['f6']] != 0 and r[AFFINE['f7']] != 0 for r in _on_rows(c)),
    'mostly_fill': lambda c: all(inside.mean() < 0.1 and inside.any() for _, _, _, inside, _, _, _ in _pixels(c)),
    'one_source_pixel': lambda c: any(inside.all() and len(np.unique(np.floor(u))) == 1 and len(np.unique(np.floor(v))) == 1
                                      for _, u, v, inside, _, _, _ in _pixels(c)),
    'src_1x1': lambda c: any(im.shape[:2] == (1, 1) for im in c['imgs']),
    'larger_than_S': lambda c: any(min(im.shape[:2]) > c['S'] and r[AFFINE['on']] for im, r in zip(c['imgs'], c['table'])),
    'pass_through_between': lambda c: any(c['table'][b - 1][0] and not c['table'][b][0] and c['table'][b + 1][0] for b in range(1, len(c['table']) - 1)),
    'edges': _edges,
    'S_mod_4': lambda c: c['S'] % 4 != 0,
    'B1': lambda c: len(c['imgs']) == 1, 'B3': lambda c: len(c['imgs']) == 3, 'B5': lambda c: len(c['imgs']) == 5,
    'more_than_64_rows': lambda c: c['annots'].shape[1] == 150 and min(len(k) for k, _ in margins(c)) > 64,
    'padding_between': lambda c: any((a[:int(np.flatnonzero(a[:, 4] != -1).max()), 4] == -1).any() for a in c['annots']),
    'box_kept': lambda c: any(all(_clauses(c, i)) and i['kept'] for i in _infos(c)),
    'box_outside': lambda c: any(i['ok'] and i['w2'] == 0 and not i['kept'] for i in _infos(c)),
    'box_straddle': lambda c: any(i['kept'] and i['box'][0] == 0 and 0.1 < i['ratio'] < 0.9 for i in _infos(c)),
    'drop_wh': lambda c: any(_clauses(c, i) == (True, False, True, True) and c['wh_thr'] in (i['w2'], i['h2']) for i in _infos(c)),
    'drop_ar': lambda c: any(_clauses(c, i) == (True, True, False, True) for i in _infos(c))
    and any(all(_clauses(c, i)) and i['ar'] > 0.9 * c['ar_thr'] for i in _infos(c)),
    'drop_area': lambda c: any(_clauses(c, i) == (True, True, True, False) for i in _infos(c))
    and any(all(_clauses(c, i)) and i['ratio'] < 1.1 * c['area_thr'] for i in _infos(c)),
    'drop_behind': lambda c: sum(not i['ok'] and not i['kept'] for i in _infos(c)) >= 2,
}
REQUIRED = set(TAGS)


def test_every_case_reaches_what_it_is_tagged_with():
    seen = set()
    for c in CASES:
        assert c['S'] in (30, 32, 64) and all(1 <= im.shape[0] <= 200 and 1 <= im.shape[1] <= 150 for im in c['imgs'])
        assert c['table'].dtype == np.float64 and c['annots'].dtype == np.float32 and len(c['imgs']) == len(c['table']) == len(c['annots'])
        for tag in c['tags']:
            assert TAGS[tag](c), (c['name'], tag)
            seen.add(tag)
    assert seen == REQUIRED, REQUIRED - seen
    assert {c['S'] for c in CASES} == {30, 32, 64}
    sizes = {im.shape[:2] for c in CASES for im in c['imgs']}
    assert {(1, 1), (1, 17), (90, 70), (200, 150)} <= sizes and any(3 * w % 4 for _, w in sizes)
    assert len(BY_NAME) == len(CASES)
