"""CPU tier of the device renderer (include/effdet_draw.h, csrc/draw.hip, ops.draw_detections, evaluate.Annotator): the binding's table
and constants against the header, the refusals the entry point decides on the host, the font, the identities of the sequential
restatement (tests/draw_restated.py) and what the cases of tests/draw_cases.py reach, by a plain-Python statement of the binning rule."""
import os
import re

import numpy as np
import pytest

from tests import draw_restated as R
from tests import draw_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'effdet_draw.h')).read(), flags=re.S)


def _prototypes():
    scalar = {'int': 'i', 'long long': 'q', 'float': 'f', 'double': 'd', 'effdet_stream_t': 'p'}
    protos = {}
    for r, name, params in re.findall(r'^([a-z][a-z ]*?\*?)\s*\b(effdet_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', _header(), flags=re.M):
        kinds = ['p' if '*' in p else scalar[' '.join(p.split()).rsplit(' ', 1)[0]] for p in params.split(',')]
        assert name not in protos, name
        protos[name] = ({'int': 'i', 'long long': 'q', 'unsigned long long': 'Q'}[' '.join(r.split())], kinds)
    return protos


def _macro(name):
    return int(re.search(r'#define\s+EFFDET_DRAW_%s\s+(\d+)' % name, _header()).group(1))


# ------------------------------------------------------------------------------------------------ the binding
def test_signatures_match_the_header():
    from efficientdet.pytorch_amd import build, _lib
    protos = _prototypes()
    assert sorted(protos) == ['effdet_draw_detections', 'effdet_draw_glyph']
    others = [getattr(_lib, n) for n in dir(_lib) if n.endswith('SIGNATURES') and n != 'DRAW_SIGNATURES']
    assert sorted(_lib.DRAW_SIGNATURES) == sorted(protos) and len(others) >= 18 and not any(set(protos) & set(t) for t in others)
    build.build(verbose=False)
    L = _lib.require(*protos)
    for name, (r, kinds) in protos.items():
        sig = _lib.DRAW_SIGNATURES[name]
        assert sig[1] == ':' and sig[0] == r and list(sig[2:].replace('s', 'p')) == kinds, (name, sig, r, kinds)
        f = getattr(L, name)
        assert f.restype is _lib._CTYPE[sig[0]] and list(f.argtypes) == [_lib._CTYPE[c] for c in sig[2:]], name
    assert len(_lib.DRAW_SIGNATURES['effdet_draw_detections']) - 2 == 25 and _lib.DRAW_SIGNATURES['effdet_draw_detections'][-1] == 's'


def test_macros_match_the_constants():
    from efficientdet.pytorch_amd import _lib, ops
    want = dict(MAX_ROWS=1024, NAME_MAX=16, MAX_THICKNESS=16, MAX_TEXT_SCALE=8)
    for macro, value in want.items():
        assert _macro(macro) == value == getattr(_lib, 'DRAW_' + macro) == getattr(ops, 'DRAW_' + macro) == getattr(R, macro), macro
    assert _macro('TEXT_MAX') == _lib.DRAW_TEXT_MAX == R.TEXT_MAX == 1 + 10 + 1 + 16 + 1 + 3
    assert (_macro('TILE_W'), _macro('TILE_H')) == (_lib.DRAW_TILE_W, _lib.DRAW_TILE_H) == (ops.DRAW_TILE_W, ops.DRAW_TILE_H) == (C.TILE_W, C.TILE_H)
    assert _macro('TILE_W') == 64                                                  # a wave of 64 lanes owns a tile row
    assert _macro('MAX_SIDE') == _lib.DRAW_MAX_SIDE == R.LIM == 1 << 20 and _macro('MAX_BATCH') == _lib.DRAW_MAX_BATCH == 65535


def test_the_build_flag_the_generation_and_the_older_headers():
    from efficientdet.pytorch_amd import build, _lib
    import efficientdet.pytorch_amd as pkg
    assert '-ffp-contract=off' in build.PER_FILE['draw.hip'] and _lib.ABI_VERSION == 11
    for h in sorted(os.listdir(os.path.join(ROOT, 'include'))):
        if h != 'effdet_draw.h':
            assert 'effdet_draw' not in open(os.path.join(ROOT, 'include', h)).read(), h    # additive: no older header declares them
    assert 'effdet_draw_detections' not in _lib.SIGNATURES and pkg.DrawOptions is __import__('efficientdet.pytorch_amd.ops', fromlist=['x']).DrawOptions
    src = re.sub(r'//.*', '', open(os.path.join(ROOT, 'efficientdet', 'pytorch_amd', 'csrc', 'draw.hip')).read())
    assert 'atomic' not in src.lower() and 'asm' not in src                         # no atomics, plain C++


def test_refusals_are_decided_on_the_host_and_launch_nothing():
    from efficientdet.pytorch_amd import build, _lib
    build.build(verbose=False)
    L = _lib.require(*_lib.DRAW_SIGNATURES)
    buf = np.zeros(1 << 16, dtype=np.uint8)
    p = buf.ctypes.data

    def draw(**kw):
        a = dict(pix=p, off=None, hw=None, B=2, H=8, W=8, rows=p, S=6, K=4, counts=p, ids=None, scale=None, names=p, lens=p, n=3, pal=p, P=4,
                 t=2, a=0, label=1, score=1, sid=0, s=2, by=0)
        a.update(kw)
        return L.effdet_draw_detections(a['pix'], a['off'], a['hw'], a['B'], a['H'], a['W'], a['rows'], a['S'], a['K'], a['counts'], a['ids'], a['scale'],
                                        a['names'], a['lens'], a['n'], a['pal'], a['P'], a['t'], a['a'], a['label'], a['score'], a['sid'], a['s'],
                                        a['by'], None)
    for kw in (dict(K=1025), dict(t=17), dict(s=9), dict(H=(1 << 20) + 1), dict(W=(1 << 20) + 1), dict(B=65536)):
        assert draw(**kw) == -3, kw
    for kw in (dict(pix=None), dict(rows=None), dict(counts=None), dict(pal=None), dict(B=0), dict(K=0), dict(H=0), dict(W=0), dict(B=-1), dict(S=5),
               dict(S=0), dict(P=0), dict(sid=1), dict(by=1), dict(sid=1, label=0), dict(n=-1), dict(names=None), dict(lens=None), dict(t=-1),
               dict(a=-1), dict(a=256), dict(s=0), dict(pix=None, K=1025), dict(P=0, t=17)):
        assert draw(**kw) == -1, kw
    assert not buf.any()


def test_the_options_and_the_tables():
    from efficientdet.pytorch_amd import ops
    from efficientdet.pytorch_amd.evaluate import Annotator
    o = ops.DrawOptions()
    assert o.key() == (2, 0, True, True, False, 2, 'label') and o == ops.DrawOptions(thickness=2) and o != ops.DrawOptions(thickness=1)
    assert eval(repr(ops.DrawOptions(3, 128, False, False, True, 8, 'id')), {'DrawOptions': ops.DrawOptions}).key() == (3, 128, False, False, True, 8, 'id')
    for bad in (dict(thickness=-1), dict(thickness=17), dict(thickness=1.5), dict(fill_alpha=-1), dict(fill_alpha=256), dict(fill_alpha=0.5),
                dict(text_scale=0), dict(text_scale=9), dict(text_scale=True), dict(color_by='track'), dict(color_by=None)):
        with pytest.raises(ValueError):
            ops.DrawOptions(**bad)
    t = ops.draw_names(['a', b'0123456789abcdef', 'café'], 'cpu')
    assert t.n == 3 and tuple(t.bytes.shape) == (3, 16) and t.lens.tolist() == [1, 16, 5] and bytes(t.bytes[2, :5].tolist()) == b'caf\xc3\xa9'
    assert ops.draw_names(None, 'cpu').n == 0 and ops.draw_names([], 'cpu').bytes is None
    with pytest.raises(ValueError):
        ops.draw_names(['0123456789abcdefg'], 'cpu')
    with pytest.raises(ValueError):
        Annotator(['a-name-of-17-bytes'])
    with pytest.raises(TypeError):
        Annotator(['a'], options=dict(thickness=1))
    pal = ops.draw_palette_host(360)
    assert pal.dtype == np.uint8 and len({tuple(c) for c in pal}) == 360 and (pal.max(axis=1) == 255).all() and (pal.min(axis=1) == 0).all()
    assert tuple(pal[0]) == (255, 0, 0) and tuple(pal[1]) == (0, 255, 17 * 255 // 60) and np.array_equal(ops.draw_palette(5, 'cpu').numpy(), pal[:5])
    with pytest.raises(ValueError):
        ops.draw_palette(0, 'cpu')


# ------------------------------------------------------------------------------------------------ the font
def test_the_font():
    g = {c: R.glyph(c) for c in range(0x20, 0x7F)}
    assert len(g) == 95 and g[0x20] == 0 and all(0 < v < 1 << 40 for c, v in g.items() if c != 0x20)      # 8 rows of 5 columns, nothing beyond
    assert len(set(g.values())) == 95                                                                    # pairwise distinct
    for c in (0, 0x1F, 0x7F, 0xFF, -1, 1000):
        assert R.glyph(c) == g[ord('?')]
    row = lambda c, r: (g[ord(c)] >> (5 * r)) & 31
    for c in '0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ':
        assert row(c, 0) and row(c, 6) and not row(c, 7), c                                               # cap height: rows 0..6
    for c in 'abcdefghijklmnopqrstuvwxyz':
        assert row(c, 6) and bool(row(c, 7)) == (c in 'gjpqy') and bool(row(c, 0)) == (c in 'bdfhijklt'), c
    assert R.glyph_rows(ord('L')) == ['#....'] * 6 + ['#####', '.....']                                   # bit 4 of a row is the leftmost column
    assert R.glyph_rows(ord('7'))[0] == '#####' and R.glyph_rows(ord('7'))[1] == '....#'


def _blank(h=40, w=90, v=7):
    return np.full((h, w, 3), v, dtype=np.uint8)


def test_a_rendered_label():
    text = b'#12 person 87'
    f = R.paint(_blank(20, 90), np.array([[2, 12, 80, 18, 0.87, 0]], dtype=np.float32), 1, ids=[12], names=[b'person'], palette=C.PALETTE[3:4],
                thickness=0, show_id=True, text_scale=1)
    assert R.label_text([0, 0, 0, 0, 0.87, 0], 0, 12, [b'person'], True, True) == text
    lab = f[3:12, 2:2 + 6 * len(text) + 1]
    ink = (lab == 0).all(axis=2)
    assert ((lab == C.PALETTE[3]).all(axis=2) | ink).all() and not ink[0].any() and not ink[:, 0].any()   # a margin of one scale unit
    assert ink.sum() == sum(bin(R.glyph(ch)).count('1') for ch in text)
    assert (f[:3] == 7).all() and (f[12:] == 7).all() and (f[:, 2 + 6 * len(text) + 1:] == 7).all()


# ------------------------------------------------------------------------------------------------ the restatement's own identities
def test_restatement_identities():
    rows = np.array([[5, 12, 30, 30, 0.9, 1], [50, 14, 80, 35, 0.8, 2]], dtype=np.float32)
    kw = dict(palette=C.PALETTE, names=C.NAMES)
    a = R.paint(_blank(), rows, 2, thickness=0, fill_alpha=255, label=False, **kw)
    solid = _blank()
    solid[12:31, 5:31], solid[14:36, 50:81] = C.PALETTE[1], C.PALETTE[2]
    assert np.array_equal(a, solid)                                                # alpha 255 is a solid fill
    assert np.array_equal(R.paint(_blank(), rows, 2, thickness=0, fill_alpha=0, label=False, **kw), _blank())     # nothing to paint
    assert np.array_equal(R.paint(_blank(), rows, 0, **kw), _blank()) and np.array_equal(R.paint(_blank(), rows, -4, **kw), _blank())
    o = dict(thickness=3, fill_alpha=100, label=False)
    assert np.array_equal(R.paint(_blank(), rows, 2, **o, **kw), R.paint(_blank(), rows[::-1], 2, **o, **kw))      # disjoint: order is free
    over = np.array([[5, 12, 50, 30, 0.9, 1], [30, 14, 80, 35, 0.8, 2]], dtype=np.float32)
    assert not np.array_equal(R.paint(_blank(), over, 2, **o, **kw), R.paint(_blank(), over[::-1], 2, **o, **kw))  # overlapping: it is not
    one = R.paint(_blank(), over[:1], 1, thickness=0, fill_alpha=128, label=False, **kw)
    assert tuple(one[20, 20]) == tuple((int(c) * 128 + 7 * 127 + 127) // 255 for c in C.PALETTE[1])
    # the outline: thickness 2 around [10, 20] x [12, 18] covers [9, 21] x [11, 19] without [11, 19] x [13, 17]
    f = R.paint(_blank(), np.array([[10, 12, 20, 18, 0.5, 0]], dtype=np.float32), 1, thickness=2, label=False, **kw)
    m = (f == C.PALETTE[0]).all(axis=2)
    want = np.zeros_like(m)
    want[11:20, 9:22] = True
    want[13:18, 11:20] = False
    assert np.array_equal(m, want)
    assert R.row_ints([1.9, -1.9, 5.5, 3.2, 0, 0]) == (1, -1, 5, 3, 0) and R.row_ints([0, 0, 1e9, 4, 0, 3e9]) == (0, 0, 1 << 20, 4, 2147483520)
    assert R.row_ints([5, 0, 4, 4, 0, 0]) is None and R.row_ints([0, 0, 4, 4, 0, -1]) is None and R.row_ints([0, 0, 4, 4, 0, float('nan')]) is None
    assert [R.percent(s) for s in (0.0, 1.0, 0.004, 0.005, 0.995, 0.9949, -0.5, 7.0, float('nan'), float('inf'), 0.87)] == [0, 100, 0, 1, 100, 99, 0, 100, 0, 0, 87]


# ------------------------------------------------------------------------------------------------ what the cases reach
def test_the_case_table_reaches_every_path():
    seen = set()
    for name in C.NAMES_OF_CASES:
        c = C.case(name)
        assert c['rows'].shape[1] <= R.MAX_ROWS and c['rows'].shape[2] in (6, 8)
        for b, (H, W) in enumerate(c['sizes']):
            tiles = C.tiles_touched(c, b)
            lens = [len(v) for v in tiles.values()]
            got = set()
            if 0 in lens:
                got.add('empty')
            if 1 in lens:
                got.add('one_row')
            if max(lens) > 64:
                got.add('over64')
            if max(lens) > 256:
                got.add('over256')
            if any(lab and not box for v in tiles.values() for _, box, lab in v):
                got.add('label_only')
            ext = R.extents(c['rows'][b], c['counts'][b], W, None if c['ids'] is None else c['ids'][b], None if c['scale'] is None else c['scale'][b],
                            c['names'], **c['opts'])
            if any(inside for *_, inside, _ in ext if c['opts']['label']):
                got.add('inside')
            if any(shifted for *_, shifted in ext if c['opts']['label']):
                got.add('shifted')
            if any(q[2] < 0 or q[3] < 0 or q[0] >= W or q[1] >= H for _, q, _, _, _ in ext):
                got.add('outside')
            if c['counts'][b] == 0:
                got.add('count0')
            seen |= got
            assert set(c['tags']) <= got or len(c['sizes']) > 1, (name, c['tags'], got)
    assert seen >= {'empty', 'one_row', 'over64', 'over256', 'label_only', 'inside', 'shifted', 'outside', 'count0'}
    sizes = {s for n in C.NAMES_OF_CASES for s in C.case(n)['sizes']}
    assert sizes == {(37, 70), (64, 128), (C.TILE_H + 1, 2 * C.TILE_W + 3)} and (70 * 3) % 4 != 0
    mixed = C.case('mixed')
    assert mixed['mixed'] and len(mixed['sizes']) == 3 and mixed['max_hw'] == (64, 131) and any(h < 64 and w < 131 for h, w in mixed['sizes'])
    assert {C.case(n)['opts']['text_scale'] for n in C.NAMES_OF_CASES} >= {1, 2, 3, 8}
    assert {C.case(n)['opts']['thickness'] for n in C.NAMES_OF_CASES} >= {0, 1, 2, 5, 16}
    assert {C.case(n)['opts']['fill_alpha'] for n in C.NAMES_OF_CASES} >= {0, 1, 128, 255}
    assert {C.case(n)['opts']['color_by'] for n in C.NAMES_OF_CASES} == {'label', 'id'}
    assert C.case('pile1024')['rows'].shape[1:] == (1024, 8) and len(C.tiles_touched(C.case('pile1024'), 0)[(0, 0)]) > 1000
