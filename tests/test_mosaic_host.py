"""CPU tier of the Mosaic / MixUp stage: the NumPy restatement (tests/mosaic_restated.py) on hand-derived arrays, the table sampler's
ranges and frequencies, every refusal of check_mosaic_table, the options' validation, the binding's table and columns against
include/effdet_mosaic.h, the host-side EINVAL returns, and every case of tests/mosaic_cases.py reaching what it is tagged with."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from efficientdet.pytorch_amd import data
from efficientdet.pytorch_amd.data import MOSAIC, MOSAIC_COLUMNS
from tests import augment_restated as A
from tests import mosaic_restated as R
from tests.mosaic_cases import CASES, _row, margins

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BY_NAME = {c['name']: c for c in CASES}


def _flat(h, w, colour):
    return np.broadcast_to(np.asarray(colour, dtype=np.uint8), (h, w, 3)).copy()


def test_four_flat_sources_of_window_size_give_four_rectangles():
    # S = 32, centre (12, 20): windows TL 12 x 20, TR 20 x 20, BL 12 x 12, BR 20 x 12 (w x h); every source has its window's size and
    # side = its longest side, so nothing is resized, nothing cropped and no fill shows
    imgs = [_flat(20, 12, (10, 20, 30)), _flat(20, 20, (40, 50, 60)), _flat(12, 12, (70, 80, 90)), _flat(12, 20, (100, 110, 120))]
    out = R.compose(imgs, _row(cx=12, cy=20, src=(0, 1, 2, 3), side=(20, 20, 12, 20)), 32, 255, 0)
    want = np.zeros((32, 32, 3), dtype=np.uint8)
    want[:20, :12], want[:20, 12:], want[20:, :12], want[20:, 12:] = (10, 20, 30), (40, 50, 60), (70, 80, 90), (100, 110, 120)
    assert np.array_equal(out, want)


def test_a_2x2_source_upscaled_to_4x4_by_hand():
    # half-pixel centres: output o samples s = (o + 0.5) / 2 - 0.5 = -0.25, 0.25, 0.75, 1.25 -> weights of the second tap 0 (clamped),
    # 0.25, 0.75, 1 (clamped).  Source [[0, 100], [200, 40]]: rows 0 and 3 are [0, 25, 75, 100] and [200, 160, 80, 40]; rows 1 and 2
    # blend them at 0.25 and 0.75: [50, 58.75, 76.25, 85] and [150, 126.25, 78.75, 55], rounded half up
    src = np.repeat(np.array([[0, 100], [200, 40]], dtype=np.uint8)[:, :, None], 3, 2)
    out = R.compose([src], _row(cx=4, cy=4, side=(4, 1, 1, 1)), 8, 9, 0)
    assert out[:4, :4, 0].tolist() == [[0, 25, 75, 100], [50, 59, 76, 85], [150, 126, 79, 55], [200, 160, 80, 40]]
    assert np.array_equal(out[:4, :4, 0], out[:4, :4, 2])
    # TR, BL and BR hold the 1 x 1 resize of the same source at the corner next to the centre, the rest is fill
    one = A.resize_u8(src, 1, 1)[0, 0, 0]
    assert out[3, 4, 0] == one and out[4, 3, 0] == one and out[4, 4, 0] == one
    rest = out.copy(); rest[:4, :4] = 9; rest[3, 4] = rest[4, 3] = rest[4, 4] = 9
    assert (rest == 9).all()
    # MixUp by hand: m = 101, p = 100 at lam 0.5 -> 100.5 -> 101 (half up); 100 and 101 at lam 0.25 -> 25 + 75.75 = 100.75 -> 101
    m, p = _flat(8, 8, (101, 100, 0)), _flat(8, 8, (100, 101, 255))
    for lam, want in ((0.5, (101, 101, 128)), (0.25, (100, 101, 191)), (1.0, (101, 100, 0)), (0.0, (100, 101, 255))):
        out = R.compose([m, p], _row(cx=8, cy=8, src=(0, 0, 0, 0), side=(8, 8, 8, 8), mix=1, mix_src=1, lam=lam), 8, 0, 0)
        assert (out == np.asarray(want, dtype=np.uint8)).all(), (lam, out[0, 0])


def test_pass_through_is_the_chains_own_stage_a():
    rng = np.random.RandomState(3)
    for h, w in ((90, 70), (5, 7), (64, 64), (1, 1), (17, 64)):
        img = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        want = A.pad_centre(A.longest_max_size(img, 64), 64)
        row = np.zeros(len(MOSAIC_COLUMNS), dtype=np.float32)
        assert np.array_equal(R.compose([img], row, 64, 114, 0), want)
        assert np.array_equal(want, A.train_stages(img, np.zeros(len(data.AUG_COLUMNS), dtype=np.float32), 64)['a'])
        bx = np.array([[1, 2, w, h, 3]], dtype=np.float32)
        got = R.boxes([bx], [(h, w)], row, 64, 0.0, 0.0, 0)
        assert np.array_equal(got, A.boxes(bx, (h, w), np.zeros(len(data.AUG_COLUMNS), dtype=np.float32), 64, 64))


def test_boxes_by_hand():
    c = BY_NAME['boxes_by_hand']
    hws = [im.shape[:2] for im in c['imgs']]
    # sources are copied, so a box moves by its quadrant's shift; TL (0, 0), TR (32, 0), BL (0, 32), BR (32, 32).  Row 0 shows source
    # 0 in TL, TR and BR and source 1 in BL; the zero-area row and the row left of the source never survive
    got = R.boxes(c['annots'], hws, c['table'][0], 64, 0.0, 0.0, 0)
    assert got.tolist() == [[4, 4, 12, 12, 0], [0, 0, 32, 32, 1], [36, 4, 44, 12, 0], [32, 0, 64, 32, 1], [8, 40, 24, 56, 4],
                            [30, 34, 32, 38, 5], [36, 36, 44, 44, 0], [32, 32, 64, 64, 1]]
    # the quadrant clip: 40 x 40 copies around (32, 32), TL origin (-8, -8), BL origin (-8, 32).  (30, 10, 50, 20) -> x 22 .. 42, cut at
    # 32: visibility 0.5; (34, ...) -> 26 .. 42: 0.375; (24, ...) -> 16 .. 36: 0.8.  In TR and BR (origin x = 32) the three show 0.1,
    # nothing and 0.4 of themselves
    c = BY_NAME['box_straddle_kept']
    got = R.boxes(c['annots'], [(40, 40)], c['table'][0], 64, 0.0, c['min_visibility'], 0)
    assert got.tolist() == [[22, 2, 32, 12, 0], [16, 2, 32, 12, 2], [22, 42, 32, 52, 0], [16, 42, 32, 52, 2]]
    c = BY_NAME['box_straddle_dropped']
    got = R.boxes(c['annots'], [(40, 40)], c['table'][0], 64, 0.0, c['min_visibility'], 0)
    assert got.tolist() == [[16, 2, 32, 12, 2], [16, 42, 32, 52, 2]]
    # with a low threshold the sliver that TR shows of the first box survives, clipped to TR's window (32 .. 64)
    assert R.boxes(c['annots'], [(40, 40)], c['table'][0], 64, 0.0, 0.05, 0).tolist()[3] == [62, 2, 64, 12, 0]
    # min_area is compared with the clipped area, and equality drops: (62 .. 64) x (2 .. 12) = 20
    assert len(R.boxes(c['annots'], [(40, 40)], c['table'][0], 64, 20.0, 0.05, 0)) == len(R.boxes(c['annots'], [(40, 40)], c['table'][0], 64, 19.5, 0.05, 0)) - 2
    # the partner's boxes follow the quadrants', scaled by LongestMaxSize(S) and centred: 32 x 32 -> 64 x 64 doubles them
    c = BY_NAME['all_rows_kept']
    got = R.boxes(c['annots'], [(32, 32)] * 2, c['table'][0], 64, 0.0, 0.9, 0)
    assert len(got) == 15 and got[12:].tolist() == [[6, 4, 60, 40, 3], [16, 16, 32, 32, 4], [1, 1, 63, 63, 5]]


def test_sampler_ranges_and_frequencies():
    B, S, n = 8, 64, 1250
    o = data.MosaicOptions(p=0.7, centre=(0.25, 0.75), scale=(0.5, 1.0), mixup_p=0.4, mixup_alpha=8.0)
    rng = np.random.RandomState(11)
    t = np.concatenate([data.sample_mosaic_table(rng, B, S, o) for _ in range(n)])
    assert t.shape == (B * n, len(MOSAIC_COLUMNS)) and t.dtype == np.float32 and B * n == 10 ** 4
    col = lambda name: t[:, MOSAIC[name]]                                                  # noqa: E731
    on, mix = col('on') == 1, col('mix') == 1
    assert set(np.unique(col('on'))) == {0.0, 1.0} and set(np.unique(col('mix'))) == {0.0, 1.0}
    assert np.array_equal(col('src0'), np.tile(np.arange(B), n)) and not (mix & ~on).any()
    assert np.array_equal(data.check_mosaic_table(t[:B], B, S, np.full((B, 2), 50)), t[:B])
    # five standard deviations of a Bernoulli frequency over the draws that reach it
    sd = lambda p, k: 5 * np.sqrt(p * (1 - p) / k)                                        # noqa: E731
    assert abs(on.mean() - 0.7) < sd(0.7, len(t)) and abs(mix[on].mean() - 0.4) < sd(0.4, on.sum())
    ints = t[:, :MOSAIC['lam']]
    assert np.array_equal(ints, np.round(ints))
    off = t[~on]
    assert not off[:, [i for i in range(len(MOSAIC_COLUMNS)) if i != MOSAIC['src0']]].any()           # nothing is drawn for a row that is off
    for name in ('cx', 'cy'):
        v = col(name)[on]
        assert v.min() == 16 and v.max() == 48 and len(np.unique(v)) == 33
        assert abs((v == 16).mean() - 1 / 33) < sd(1 / 33, on.sum())
    for q in range(1, 4):
        v = col('src%d' % q)[on]
        assert v.min() == 0 and v.max() == B - 1
        assert all(abs((v == s).mean() - 1 / B) < sd(1 / B, on.sum()) for s in range(B))
    for q in range(4):
        v = col('side%d' % q)[on]
        assert v.min() == 32 and v.max() == 64 and abs(v.mean() - 48) < 0.5
    v = col('mix_src')[mix]
    assert v.min() == 0 and v.max() == B - 1 and all(abs((v == s).mean() - 1 / B) < sd(1 / B, mix.sum()) for s in range(B))
    lam = col('lam')[mix]
    # Beta(8, 8): mean 1 / 2, variance 1 / (4 * 17)
    assert lam.min() > 0 and lam.max() < 1 and abs(lam.mean() - 0.5) < 5 * np.sqrt(1 / 68 / mix.sum()) and abs(lam.var() - 1 / 68) < 2e-3
    assert not col('lam')[~mix].any() and not col('mix_src')[~mix].any()
    # the same seed gives the same table; p = 0 draws nothing but the identity
    a = data.sample_mosaic_table(np.random.RandomState(5), 4, 32, o)
    assert np.array_equal(a, data.sample_mosaic_table(np.random.RandomState(5), 4, 32, o))
    z = data.sample_mosaic_table(np.random.RandomState(5), 4, 32, data.MosaicOptions(p=0.0))
    assert not z[:, MOSAIC['on']].any() and z[:, MOSAIC['src0']].tolist() == [0, 1, 2, 3]
    # a side never rounds below 1 or above S, a degenerate centre range is one value
    e = data.sample_mosaic_table(np.random.RandomState(5), 64, 8, data.MosaicOptions(centre=(0.5, 0.5), scale=(0.01, 0.02)))
    assert (e[:, MOSAIC['side0']:MOSAIC['side3'] + 1] == 1).all() and (e[:, MOSAIC['cx']] == 4).all() and (e[:, MOSAIC['cy']] == 4).all()


def test_options_validate_their_arguments():
    o = data.MosaicOptions()
    assert o.key() == (1.0, (0.25, 0.75), (0.5, 1.0), 114, 0.0, 8.0) and o == data.MosaicOptions() and hash(o) == hash(data.MosaicOptions())
    assert o != data.MosaicOptions(fill=0) and 'mixup_alpha=8.0' in repr(o)
    for bad in (dict(p=-0.1), dict(p=1.5), dict(p=float('nan')), dict(centre=(0.5, 0.4)), dict(centre=(-0.1, 0.5)), dict(centre=(0.2, 1.1)),
                dict(centre=(0.5,)), dict(scale=(0.0, 1.0)), dict(scale=(0.5, 1.5)), dict(scale=(0.8, 0.5)), dict(fill=-1), dict(fill=256),
                dict(fill=1.5), dict(fill=True), dict(mixup_p=2.0), dict(mixup_alpha=0.0), dict(mixup_alpha=float('inf'))):
        with pytest.raises(ValueError):
            data.MosaicOptions(**bad)
    with pytest.raises(ValueError):
        data.DeviceAugmentation(phase='valid', mosaic=o, device='cpu')
    with pytest.raises(ValueError):
        data.DeviceAugmentation(phase='test', mosaic=o, device='cpu')
    with pytest.raises(TypeError):
        data.DeviceAugmentation(phase='train', mosaic=True, device='cpu')
    aug = data.DeviceAugmentation(phase='train', width=64, height=64, device='cpu')
    assert aug.mosaic is None
    with pytest.raises(ValueError, match='no mosaic options'):
        aug([{'img': np.zeros((4, 4, 3), dtype=np.uint8), 'annot': np.zeros((0, 5))}], mosaic_table=np.zeros((1, 14), dtype=np.float32))
    aug = data.DeviceAugmentation(phase='valid', width=64, height=64, device='cpu')
    aug.mosaic = o                                                                         # set after construction: refused at the call
    with pytest.raises(ValueError, match="'train'"):
        aug([{'img': np.zeros((4, 4, 3), dtype=np.uint8), 'annot': np.zeros((0, 5))}])


def test_every_refusal_of_check_mosaic_table():
    B, S = 3, 32
    hw = np.array([[20, 30], [90, 70], [64, 2]])
    good = np.stack([_row(cx=0, cy=32, src=(0, 1, 1, 0), side=(32, 1, 32, 5), mix=1, mix_src=1, lam=1.0), _row(on=0),
                     _row(cx=7, cy=9, src=(1, 0, 1, 0), side=(9, 9, 9, 9))])
    assert data.check_mosaic_table(good, B, S, hw).dtype == np.float32
    assert np.array_equal(data.check_mosaic_table(good.astype(np.float64).tolist(), B, S, hw), good)

    def refused(row, col, value, match, b=0):
        t = good.copy()
        t[row, MOSAIC[col]] = value
        with pytest.raises(ValueError, match=r'row %d.*%s' % (row, match)):
            data.check_mosaic_table(t, B, S, hw)
    with pytest.raises(ValueError, match='must be'):
        data.check_mosaic_table(good[:2], B, S, hw)
    with pytest.raises(ValueError, match='must be'):
        data.check_mosaic_table(good[:, :13], B, S, hw)
    with pytest.raises(ValueError, match='source sizes'):
        data.check_mosaic_table(good, B, S, hw[:2])
    refused(0, 'on', 2, '0 or 1'); refused(0, 'on', 0.5, '0 or 1'); refused(2, 'mix', -1, '0 or 1'); refused(1, 'on', np.nan, '0 or 1')
    refused(1, 'mix', 1, 'mix needs on')
    refused(0, 'cx', 3.5, 'integer'); refused(2, 'side2', 8.25, 'integer'); refused(0, 'src1', np.inf, 'integer'); refused(2, 'mix_src', 0.5, 'integer')
    refused(0, 'cx', -1, 'centre'); refused(0, 'cy', S + 1, 'centre')
    refused(0, 'src0', -1, 'outside the batch'); refused(2, 'src3', B, 'outside the batch'); refused(0, 'mix_src', B, 'outside the batch')
    refused(0, 'side0', 0, r'outside \[1, 32\]'); refused(2, 'side1', S + 1, r'outside \[1, 32\]')
    refused(0, 'lam', -0.01, 'lam'); refused(0, 'lam', 1.5, 'lam'); refused(0, 'lam', np.nan, 'lam')
    # a resized side that rounds to 0: 64 x 2 at side 9 is 9 x 0 and at side 5 it is 5 x 0; at S = 32 it is 32 x 1
    refused(2, 'src0', 2, 'resizes to 0'); refused(0, 'src3', 2, 'resizes to 0')
    t = good.copy(); t[0, MOSAIC['mix_src']] = 2
    assert data.check_mosaic_table(t, B, S, hw) is not None
    with pytest.raises(ValueError, match='row 1.*resizes to 0'):                           # a pass-through, as for the chain itself
        data.check_mosaic_table(np.stack([_row(on=0)] * 3), B, S, np.array([[20, 30], [90, 1], [64, 2]]))
    with pytest.raises(ValueError, match='row 0.*partner 2.*resizes to 0'):
        data.check_mosaic_table(np.stack([t[0], _row(on=0), _row(on=0)]), B, S, np.array([[20, 30], [90, 70], [70, 1]]))
    # a row that is off may hold anything else
    t = good.copy(); t[1] = _row(on=0, cx=99, cy=-5, src=(9, 9, 9, 9), side=(0, 0, 0, 0), mix_src=77, lam=3.0)
    assert np.array_equal(data.check_mosaic_table(t, B, S, hw), t)


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'effdet_mosaic.h')).read(), flags=re.S)


def test_signatures_and_columns_match_the_header():
    """_lib.MOSAIC_SIGNATURES against the prototypes of include/effdet_mosaic.h (names, return kind, parameter kinds in order), the
    column enum against MOSAIC_COLUMNS, and the built library exports and binds both entry points."""
    from efficientdet.pytorch_amd import build, _lib, ops
    h = _header()
    scalar = {'int': 'i', 'long long': 'q', 'float': 'f', 'double': 'd', 'effdet_stream_t': 'p'}
    protos = {}
    for r, name, params in re.findall(r'^([a-z][a-z ]*?\*?)\s*\b(effdet_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', h, flags=re.M):
        kinds = ['p' if '*' in p else scalar[' '.join(p.split()).rsplit(' ', 1)[0]] for p in params.split(',')]
        assert name not in protos, name
        protos[name] = ({'int': 'i', 'long long': 'q'}[' '.join(r.split())], kinds)
    assert sorted(protos) == ['effdet_mosaic_boxes', 'effdet_mosaic_compose']
    others = [getattr(_lib, n) for n in dir(_lib) if n.endswith('SIGNATURES') and n != 'MOSAIC_SIGNATURES']
    assert len(others) >= 11 and sorted(_lib.MOSAIC_SIGNATURES) == sorted(protos) and not any(set(protos) & set(t) for t in others)
    build.build(verbose=False)
    L = _lib.require(*protos)
    for name, (r, kinds) in protos.items():
        sig = _lib.MOSAIC_SIGNATURES[name]
        assert sig[1] == ':' and sig[0] == r, (name, sig, r)
        assert list(sig[2:].replace('s', 'p')) == kinds, (name, sig, ''.join(kinds))
        assert sig.endswith('s') and 'effdet_stream_t stream' in re.search(name + r'\s*\(([^)]*)\)', h).group(1)
        f = getattr(L, name)
        assert f.restype is _lib._CTYPE[sig[0]] and list(f.argtypes) == [_lib._CTYPE[c] for c in sig[2:]], name
    P = int(re.search(r'#define\s+EFFDET_MOSAIC_P\s+(\d+)', h).group(1))
    enum = [e.strip() for e in re.search(r'enum\s*\{(.*?)\}', h, flags=re.S).group(1).split(',')]
    assert enum[0] == 'EFFDET_MOSAIC_ON = 0' and all('=' not in e for e in enum[1:])
    names = [e.split('=')[0].strip()[len('EFFDET_MOSAIC_'):].lower() for e in enum]
    assert tuple(names) == MOSAIC_COLUMNS and P == len(MOSAIC_COLUMNS) == ops.MOSAIC_P and MOSAIC == {n: i for i, n in enumerate(names)}
    assert '-ffp-contract=off' in build.PER_FILE['mosaic.hip']     # separately rounded products, fp64 box steps: no FMA contraction
    # the semantics are stated where the issue put them
    doc = open(os.path.join(ROOT, 'include', 'effdet_mosaic.h')).read()
    for phrase in ('on == 0, pass-through', 'QUADRANT WINDOW', 'round half up', 'indices into THIS batch', 'min_visibility'):
        assert phrase in doc, phrase


def test_einval_returns_launch_nothing():
    """The refusals of both entry points are decided on the host, before any launch: they return on a machine without a device."""
    from efficientdet.pytorch_amd import build, _lib
    build.build(verbose=False)
    L = _lib.require('effdet_mosaic_compose', 'effdet_mosaic_boxes')
    buf = np.zeros(4096, dtype=np.uint8)
    p = buf.ctypes.data
    for B, S, fill in ((0, 32, 114), (-1, 32, 114), (2, 7, 114), (2, 0, 114), (2, 32, -1), (2, 32, 256), (65536, 32, 114), (1, 1 << 16, 114)):
        assert L.effdet_mosaic_compose(p, p, p, p, B, S, fill, p, None) == -1, (B, S, fill)
    for B, S, M, M_out in ((0, 32, 4, 20), (2, 7, 4, 20), (2, 32, 4, 19), (2, 32, 4, 0), (2, 32, 0, 20), (2, 32, 1 << 30, 1 << 30)):
        assert L.effdet_mosaic_boxes(p, p, B, S, p, M, 0.0, 0.0, p, M_out, p, None) == -1, (B, S, M, M_out)
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert L.effdet_mosaic_compose(*args, 2, 32, 114, p, None) == -1
    assert L.effdet_mosaic_compose(p, p, p, p, 2, 32, 114, None, None) == -1
    assert L.effdet_mosaic_boxes(p, p, 2, 32, p, 4, 0.0, 0.0, None, 20, p, None) == -1
    assert L.effdet_mosaic_boxes(p, p, 2, 32, p, 4, 0.0, 0.0, p, 20, None, None) == -1
    assert C.sizeof(C.c_float) == 4 and not buf.any()


# ------------------------------------------------------------------------------------------------ the cases reach their tags
def _slots(c):
    hws = [im.shape[:2] for im in c['imgs']]
    for b, row in enumerate(c['table']):
        if row[MOSAIC['on']]:
            for q in range(4):
                s, rh, rw, ox, oy, win = R.slot(hws, row, c['S'], b, q)
                yield b, q, s, hws[s], (rh, rw), (ox, oy), win, int(row[MOSAIC['side0'] + q])


def _on_rows(c):
    return [r for r in c['table'] if r[MOSAIC['on']]]


def _mix_rows(c):
    return [r for r in c['table'] if r[MOSAIC['mix']]]


def _candidates(c):
    return [(b, i) for b, (_, info) in enumerate(margins(c)) for i in info]


def _half_up_tie(c):
    for b, row in enumerate(c['table']):
        if row[MOSAIC['mix']]:
            m_row, p_row = row.copy(), row.copy()
            m_row[MOSAIC['lam']], p_row[MOSAIC['lam']] = 1.0, 0.0
            m = R.compose(c['imgs'], m_row, c['S'], c['fill'], b).astype(np.int64)
            p = R.compose(c['imgs'], p_row, c['S'], c['fill'], b).astype(np.int64)
            odd = (m + p) % 2 == 1
            if odd.any() and np.array_equal(R.compose(c['imgs'], row, c['S'], c['fill'], b)[odd], ((m + p + 1) // 2)[odd]):
                return True
    return False


def _straddles(c, kept):
    cx = c['table'][0][MOSAIC['cx']]
    return any(bx[0] < cx < bx[2] and 0 < clipped < area and k == kept and
               (kept or (clipped > c['min_area'] and clipped / area < c['min_visibility']))
               for _, (q, area, clipped, bx, win, k) in _candidates(c))


def _copy_shown(c):
    for b, q, s, hw, r, (ox, oy), win, side in _slots(c):
        if r == tuple(hw) and win[1] > win[0] and win[3] > win[2]:
            out = R.compose(c['imgs'], c['table'][b], c['S'], c['fill'], b)
            xs, xe, ys, ye = max(ox, win[0]), min(ox + r[1], win[1]), max(oy, win[2]), min(oy + r[0], win[3])
            if xe > xs and ye > ys and not c['table'][b][MOSAIC['mix']]:
                return np.array_equal(out[ys:ye, xs:xe], c['imgs'][s][ys - oy:ye - oy, xs - ox:xe - ox])
    return False


def _fill_on_two_sides(c):
    for b, q, s, hw, (rh, rw), (ox, oy), win, side in _slots(c):
        if 0 < rw < win[1] - win[0] and 0 < rh < win[3] - win[2]:
            out = R.compose(c['imgs'], c['table'][b], c['S'], c['fill'], b)
            region = out[win[2]:win[3], win[0]:win[1]]
            shown = region[oy - win[2]:oy - win[2] + rh, ox - win[0]:ox - win[0] + rw]
            return bool((region == c['fill']).all(-1).sum() == region.shape[0] * region.shape[1] - rh * rw
                        and np.array_equal(shown, A.resize_u8(c['imgs'][s], rw, rh)) and shown.shape[0] < region.shape[0] and shown.shape[1] < region.shape[1])
    return False


TAGS = {
    'smaller': _fill_on_two_sides,
    'larger': lambda c: any(rw > win[1] - win[0] > 0 or rh > win[3] - win[2] > 0 for _, _, _, _, (rh, rw), _, win, _ in _slots(c)),
    'copy': _copy_shown,
    'upscale': lambda c: any(rh > hw[0] and rw > hw[1] for _, _, _, hw, (rh, rw), _, _, _ in _slots(c)),
    'side1': lambda c: any(side == 1 for *_, side in _slots(c)),
    'src_1x1': lambda c: any(im.shape[:2] == (1, 1) for im in c['imgs']) and any(tuple(hw) == (1, 1) for _, _, _, hw, *_ in _slots(c)),
    'same_source': lambda c: any(len(set(r[MOSAIC['src0']:MOSAIC['src3'] + 1].tolist())) == 1 for r in _on_rows(c)),
    'B1': lambda c: len(c['imgs']) == 1, 'B3': lambda c: len(c['imgs']) == 3, 'B5': lambda c: len(c['imgs']) == 5,
    'centre_0': lambda c: any(r[MOSAIC['cx']] == 0 for r in _on_rows(c)) and any(r[MOSAIC['cy']] == 0 for r in _on_rows(c)),
    'centre_S': lambda c: any(r[MOSAIC['cx']] == c['S'] for r in _on_rows(c)) and any(r[MOSAIC['cy']] == c['S'] for r in _on_rows(c)),
    'centre_quarter': lambda c: any(r[MOSAIC['cx']] == c['S'] // 4 for r in _on_rows(c)) and any(r[MOSAIC['cy']] == c['S'] // 4 for r in _on_rows(c)),
    'centre_three_quarters': lambda c: any(r[MOSAIC['cx']] == 3 * c['S'] // 4 for r in _on_rows(c)) and any(r[MOSAIC['cy']] == 3 * c['S'] // 4 for r in _on_rows(c)),
    'odd_centre': lambda c: any(r[MOSAIC['cx']] % 2 == 1 and r[MOSAIC['cy']] % 2 == 1 for r in _on_rows(c)),
    'pass_through_between': lambda c: any(c['table'][b - 1][0] and not c['table'][b][0] and c['table'][b + 1][0] for b in range(1, len(c['table']) - 1)),
    'mix': lambda c: len(_mix_rows(c)) > 0,
    'lam_0': lambda c: all(r[MOSAIC['lam']] == 0 for r in _mix_rows(c)) and len(_mix_rows(c)) > 0,
    'lam_1': lambda c: all(r[MOSAIC['lam']] == 1 for r in _mix_rows(c)) and len(_mix_rows(c)) > 0,
    'lam_0.5': lambda c: all(r[MOSAIC['lam']] == 0.5 for r in _mix_rows(c)) and _half_up_tie(c),
    'lam_0.3': lambda c: all(r[MOSAIC['lam']] == np.float32(0.3) for r in _mix_rows(c)) and len(_mix_rows(c)) > 0,
    'partner_is_quadrant_source': lambda c: any(r[MOSAIC['mix_src']] in r[MOSAIC['src0']:MOSAIC['src3'] + 1] for r in _mix_rows(c)),
    'box_on_edge': lambda c: any(k and bx[0] == win[0] and bx[2] == win[1] and bx[1] == win[2] and bx[3] == win[3]
                                 for _, (q, area, clipped, bx, win, k) in _candidates(c)),
    'box_outside': lambda c: any(area > 0 and clipped == 0 and (bx[2] <= win[0] or bx[0] >= win[1]) and 0 <= bx[0] and bx[2] <= c['S']
                                 for _, (q, area, clipped, bx, win, k) in _candidates(c))
    and any(area > 0 and clipped == 0 and bx[2] < 0 for _, (q, area, clipped, bx, win, k) in _candidates(c)),
    'box_zero_area': lambda c: any(area == 0 and not k for _, (q, area, clipped, bx, win, k) in _candidates(c)),
    'straddle_kept': lambda c: _straddles(c, True),
    'straddle_dropped': lambda c: _straddles(c, False),
    'padding_rows': lambda c: any((c['annots'][s][:, 4] == -1).any() and (c['annots'][s][:, 4] != -1).any() and q < 3 for _, q, s, *_ in _slots(c)),
    'no_boxes_source': lambda c: any((c['annots'][s][:, 4] == -1).all() for _, _, s, *_ in _slots(c)),
    'count_5M': lambda c: all(len(kept) == 5 * c['annots'].shape[1] for kept, _ in margins(c)),
    'more_than_64_rows': lambda c: c['annots'].shape[1] > 128 and max(len(kept) for kept, _ in margins(c)) > 128,
    'S_mod_4': lambda c: c['S'] % 4 != 0,
}
REQUIRED = set(TAGS)


def test_every_case_reaches_what_it_is_tagged_with():
    seen = set()
    for c in CASES:
        assert c['S'] in (30, 32, 64) and all(1 <= im.shape[0] <= 90 and 1 <= im.shape[1] <= 90 for im in c['imgs'])
        for tag in c['tags']:
            assert TAGS[tag](c), (c['name'], tag)
            seen.add(tag)
    assert seen == REQUIRED, REQUIRED - seen
    assert {c['S'] for c in CASES} >= {32, 64}
    sizes = {im.shape[:2] for c in CASES for im in c['imgs']}
    assert (1, 1) in sizes and (90, 70) in sizes
    assert len(BY_NAME) == len(CASES)
