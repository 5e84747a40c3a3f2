"""CPU tier of sliced inference: the NumPy restatement (tests/slices_restated.py) on hand-derived cases whose every number is exact, the
properties of the tile plan over a sweep, what the seeded cases claim to cover, the options' validation, the binding's table and structs
against include/effdet_slices.h, the host-side refusals of both entry points, and the fixture conditions of the model-level GPU test
(which need only the oracle and the restatement at that test's sizes)."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import slices_restated as R
from tests.slices_cases import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BY_NAME = {c['name']: c for c in CASES}
UNIT = [(0, 0, 128, 128, 1.0, 1.0)]


def _one(rows, table=None, **kw):
    """rows: per tile [(x1, y1, x2, y2, score, label)] -> the Run of one image of 200 x 200."""
    TPI, n = len(rows), max(len(r) for r in rows)
    s = np.zeros((TPI, n), dtype=np.float32); l = np.zeros((TPI, n), dtype=np.int64); b = np.zeros((TPI, n, 4), dtype=np.float32)
    for j, r in enumerate(rows):
        a = np.asarray(r, dtype=np.float64).reshape(-1, 6)
        s[j, :len(a)], l[j, :len(a)], b[j, :len(a)] = a[:, 4], a[:, 5], a[:, :4]
    return R.merge(s, l, b, [len(r) for r in rows], table or UNIT * TPI, 200.0, 200.0, **kw)


def test_worked_examples_by_hand():
    # a box truncated at a tile edge: tile 1 starts at x = 60 and sees (60, 0, 100, 40) of the object (0, 0, 100, 40) that tile 0 sees whole.
    # IoU = 1600 / 4000 = 0.4 does not match at 0.5; IoS = 1600 / 1600 = 1 does, and the hull is the full box
    two = [[(0, 0, 100, 40, 0.75, 1)], [(0, 0, 40, 40, 0.5, 1)]]
    tab = [(0, 0, 128, 128, 1.0, 1.0), (0, 60, 128, 128, 1.0, 1.0)]
    r = _one(two, tab, metric='iou')
    assert r.keepers == [(0, 0), (1, 0)] and r.boxes.tolist() == [[0, 0, 100, 40], [60, 0, 100, 40]] and r.score.tolist() == [0.75, 0.5]
    r = _one(two, tab, metric='ios')
    assert r.keepers == [(0, 0)] and r.absorbed == [[(1, 0)]] and r.boxes.tolist() == [[0, 0, 100, 40]] and r.label.tolist() == [1]
    # the test is >: IoS exactly at the threshold (0.5: (0, 0, 40, 40) against (20, 0, 60, 40)) does not match
    assert len(_one([[(0, 0, 40, 40, 0.75, 1), (20, 0, 60, 40, 0.5, 1)]], thr=0.5).keepers) == 2
    assert len(_one([[(0, 0, 40, 40, 0.75, 1), (20, 0, 60, 40, 0.5, 1)]], thr=0.25).keepers) == 1
    # NMM grows the keeper's box, NMS emits it as it is; score and label are the keeper's either way
    pair = [[(0, 0, 40, 40, 0.75, 2), (20, 0, 60, 40, 0.5, 2)]]
    assert _one(pair, thr=0.25, method='nmm').boxes.tolist() == [[0, 0, 60, 40]] and _one(pair, thr=0.25, method='nms').boxes.tolist() == [[0, 0, 40, 40]]
    # the chain: A absorbs B (IoU 60 / 112); B would have absorbed C (42 / 72) but is dead; IoU(A, C) = 35 / 107: C is its own keeper
    c = BY_NAME['chain']
    r = R.merge(c['score'][0], c['label'][0], c['boxes'][0], c['count'][0], c['table'], c['W'], c['H'], max_det=c['max_det'], **c['opts'])
    assert r.keepers == [(0, 0), (0, 2), (1, 0)] and r.absorbed == [[(0, 1)], [], []]
    assert r.boxes.tolist() == [[0, 0, 12, 10], [0, 0, 12, 3.5], [40, 40, 48, 48]] and r.own.tolist()[0] == [0, 0, 10, 10]
    # matching is against the keeper's OWN box: A (0,0,10,10) takes B (4,0,20,10) at IoU 60 / 200 = 0.3 > 0.25 and its hull becomes
    # (0,0,20,10), which C (11,0,20,10) overlaps by 90 / 200 = 0.45 -- but IoU(A, C) = 0, so C stays
    r = _one([[(0, 0, 10, 10, 0.75, 0), (4, 0, 20, 10, 0.5, 0), (11, 0, 20, 10, 0.25, 0)]], metric='iou', thr=0.25)
    assert r.keepers == [(0, 0), (0, 2)] and r.boxes.tolist() == [[0, 0, 20, 10], [11, 0, 20, 10]]
    # a tie is broken by tile, then by row: all four score 0.5 and do not overlap
    r = _one([[(0, 0, 8, 8, 0.5, 0), (10, 0, 18, 8, 0.5, 0)], [(20, 0, 28, 8, 0.5, 0), (30, 0, 38, 8, 0.5, 0)]])
    assert r.keepers == [(0, 0), (0, 1), (1, 0), (1, 1)]
    r = _one([[(0, 0, 8, 8, 0.25, 0)], [(0, 0, 8, 7, 0.5, 0), (0, 0, 8, 6, 0.25, 0)]], method='nms')      # the tied 0.25s: tile 0 first, both dead
    assert r.keepers == [(1, 0)] and r.absorbed == [[(0, 0), (1, 1)]]
    # class-aware: identical boxes of two labels are two keepers; class-agnostic: one
    same = [[(0, 0, 8, 8, 0.75, 1)], [(0, 0, 8, 8, 0.5, 2)]]
    assert len(_one(same, class_aware=True).keepers) == 2 and _one(same, class_aware=False).label.tolist() == [1]
    # the multipliers and the clip: (10, 10, 50, 60) of a view with mx = 2, my = 3 is (20, 30, 100, 180); a 200 x 200 image clips x' = 240
    r = _one([[(10, 10, 50, 60, 0.5, 0), (60, 0, 120, 10, 0.25, 0)]], [(0, 0, 128, 128, 3.0, 2.0)])
    assert r.boxes.tolist() == [[20, 30, 100, 180], [120, 0, 200, 30]]
    # count, skip_thr, NaN / Inf scores, labels outside [0, 65536) and boxes that clip to nothing
    rows = [[(0, 0, 8, 8, 0.75, 0), (20, 0, 28, 8, 0.5, 0), (40, 0, 48, 8, 0.25, 0)]]
    assert len(_one(rows, skip_thr=0.5).keepers) == 2 and len(_one(rows, max_det=1).keepers) == 1
    s, l, b = np.asarray([[0.75, 0.5, 0.25]], np.float32), np.zeros((1, 3), np.int64), np.asarray([[r_[:4] for r_ in rows[0]]], np.float32)
    assert len(R.merge(s, l, b, [2], UNIT, 200, 200).keepers) == 2 and len(R.merge(s, l, b, [-1], UNIT, 200, 200).keepers) == 0
    assert len(R.merge(s, l, b, [7], UNIT, 200, 200).keepers) == 3
    bad = [[(0, 0, 8, 8, np.nan, 0), (20, 0, 28, 8, np.inf, 0), (40, 0, 48, 8, 0.5, 65536), (60, 0, 68, 8, 0.5, -1), (300, 0, 308, 8, 0.5, 0),
            (80, 0, 80, 8, 0.5, 0), (100, 0, 108, 8, 0.25, 65535)]]
    assert _one(bad).keepers == [(0, 6)]
    assert _one([[]]).keepers == [] and _one([[]]).boxes.shape == (0, 4)


def test_the_key_orders_scores_descending():
    s = np.asarray([0.5, -0.0, 0.0, 1.0, -1.0, 2.0 ** 127, 2.0 ** -149], dtype=np.float32)
    assert s[np.argsort(R.score_key(s), kind='stable')].tolist() == [2.0 ** 127, 1.0, 0.5, 2.0 ** -149, 0.0, -0.0, -1.0]
    assert str(s[np.argsort(R.score_key(s), kind='stable')][4:6]) == '[ 0. -0.]' and not (R.score_key(s) == 0xffffffff).any()


@pytest.mark.parametrize('s', [128, 256, 512])
def test_plan_properties(s):
    from efficientdet.pytorch_amd import ops
    n = 0
    for ratio in (0.0, 0.1, 0.2, 0.25, 0.5, 0.77, 0.9):
        o = int(math.floor(ratio * s))
        step = s - o
        for L in sorted({s, s + 1, s + step - 1, s + step, s + step + 1, 2 * s, 3 * s - 1, 600, 850, 1999, 3000} - set(range(s))):
            pos = R.positions(L, s, ratio)
            assert pos == ops._slice_positions(L, s, ratio, 'width')
            assert len(pos) == -(-(L - s) // step) + 1                                       # ceil((L - s) / step) + 1
            assert pos[0] == 0 and pos[-1] == L - s and all(0 <= p and p + s <= L for p in pos) and pos == sorted(set(pos))
            covered = np.zeros(L, dtype=bool)
            for p in pos:
                covered[p:p + s] = True
            assert covered.all()
            gaps = [b - a for a, b in zip(pos, pos[1:])]
            assert all(g == step for g in gaps[:-1]) and all(0 < g <= step for g in gaps[-1:])    # overlap >= o, more into the last position
            n += 1
    assert n >= 40
    with pytest.raises(ValueError):
        R.positions(s - 1, s, 0.2)


def test_slice_plan_is_the_restated_plan():
    from efficientdet.pytorch_amd import ops
    o = ops.SliceOptions(slice=(256, 256), overlap=(0.25, 0.25), tile_batch=8, merge=ops.SliceMergeOptions(top_n=200, max_det=300))
    p = ops.slice_plan(600, 850, o)
    assert p == R.plan(600, 850, (256, 256), (0.25, 0.25)) and len(p) == 16
    assert [r[0] for r in p[:15:5]] == [0, 192, 344] and [r[1] for r in p[:5]] == [0, 192, 384, 576, 594]
    assert p[-1] == (0, 0, 256, 256, float(np.float32(600 / 256)), float(np.float32(850 / 256))) and all(r[4:] == (1.0, 1.0) for r in p[:-1])
    assert ops.slice_plan(256, 256, o) == [(0, 0, 256, 256, 1.0, 1.0)]                      # one tile, no full view
    q = ops.slice_plan(300, 256, ops.SliceOptions(slice=(256, 128), overlap=(0.0, 0.5), full_view=False))
    assert q == R.plan(300, 256, (256, 128), (0.0, 0.5), False) and [(r[0], r[1]) for r in q] == [(0, 0), (0, 64), (0, 128), (44, 0), (44, 64), (44, 128)]
    with pytest.raises(ValueError, match='height 200 is smaller than the slice height 256'):
        ops.slice_plan(200, 850, o)
    with pytest.raises(ValueError, match='width 255 is smaller than the slice width 256'):
        ops.slice_plan(600, 255, o)
    with pytest.raises(ValueError, match=r'41 \* 200 exceeds 8192'):                        # 5 x 8 tiles and the full view
        ops.slice_plan(1024, 1600, o)
    assert len(ops.slice_plan(1024, 1600, ops.SliceOptions(slice=(256, 256), overlap=(0.25, 0.25), full_view=False,
                                                           merge=ops.SliceMergeOptions(top_n=200)))) == 40
    with pytest.raises(TypeError):
        ops.slice_plan(600, 850, None)


def test_the_slicer_restatement_clamps_and_pads():
    src = np.arange(2 * 5 * 7 * 3, dtype=np.float32).reshape(2, 5, 7, 3)
    tab = [(1, 2, 3, 4, 1.0, 1.0), (-2, 5, 3, 4, 1.0, 1.0)]
    out = R.slice_images(src, tab, 1, 3, 4)
    assert out.shape == (2, 3, 4, 4) and not out[..., 3].any()
    assert np.array_equal(out[1, :, :, :3], src[1, 1:4, 2:6])                                 # flat tile 2 = image 1, tile 0
    assert np.array_equal(out[0, 0, :, :3], src[0, 0, [5, 6, 6, 6]]) and np.array_equal(out[0, 2, 0, :3], src[0, 0, 5])   # rows -2..0 -> 0, columns 5..8 -> 5, 6, 6, 6


def test_the_cases_cover_what_they_claim():
    def runs(c):
        return R.merge_batch(c['score'], c['label'], c['boxes'], c['count'], c['table'], c['W'], c['H'], c['max_det'], **c['opts'])[4]

    def survivors(c, b=0):
        return len(R.candidates(c['score'][b], c['label'][b], c['boxes'][b], c['count'][b], c['table'], c['W'], c['H'], c['opts'].get('skip_thr', 0.0))[1])
    combos = [c for c in CASES if re.fullmatch(r'(nms|nmm)_(iou|ios)_(aware|agnostic)', c['name'])]
    assert len(combos) == 8 and survivors(combos[0]) == 300
    kept = {c['name']: len(runs(c)[0].keepers) for c in combos}
    assert len(set(kept.values())) >= 3 and kept['nmm_ios_agnostic'] < kept['nmm_iou_aware'], kept      # the options tell the runs apart
    for c in combos:
        r = runs(c)[0]
        assert any(a for a in r.absorbed) and (c['opts']['method'] == 'nmm') == (not np.array_equal(r.boxes, r.own))
        assert any(t != k[0] for k, a in zip(r.keepers, r.absorbed) for t, _ in a)                      # a death across two tiles
    assert any(m != 1.0 for m in BY_NAME['nmm_ios_aware']['table'][-1][4:])                             # mx, my != 1 on the last tile
    c = BY_NAME['tied_scores']
    s = R.candidates(c['score'][0], c['label'][0], c['boxes'][0], c['count'][0], c['table'], c['W'], c['H'], 0.0)
    assert len(set(s[1].tolist())) <= 17 and list(zip((-s[1]).tolist(), s[3].tolist(), s[4].tolist())) == sorted(zip((-s[1]).tolist(), s[3].tolist(), s[4].tolist()))
    c = BY_NAME['max_det_cuts']
    assert len(runs(c)[0].keepers) == 7 < kept['nmm_ios_aware']
    c = BY_NAME['counts_out_of_range']
    assert c['count'].min() < 0 and c['count'].max() > c['score'].shape[2] and (c['count'] == 0).any()
    for b, r in enumerate(runs(c)):
        rows = np.minimum(np.maximum(c['count'][b], 0), 32)
        assert all(row < rows[t] for t, row in r.keepers + [x for a in r.absorbed for x in a]) and 0.999 not in r.score.tolist()
    c = BY_NAME['nonfinite_scores']
    assert survivors(c) == 200 - 4 and np.isfinite(runs(c)[0].score).all()
    assert survivors(BY_NAME['degenerate_boxes']) == 200 - 6
    c = BY_NAME['skip_thr_at_a_tie']
    s = c['score'][0][:, :50]
    assert (s == 0.5).sum() >= 10 and survivors(c) == (s >= 0.5).sum() and runs(c)[0].score.min() == 0.5
    c = BY_NAME['batch3_one_empty']
    assert survivors(c, 0) >= 300 and [survivors(c, b) for b in (1, 2)] == [0, 1] and [len(r.keepers) > 0 for r in runs(c)] == [True, False, True]
    for n in (1, 63, 65, 1025):
        assert survivors(BY_NAME['n%d' % n]) == n
    c = BY_NAME['n8192']
    assert c['score'].shape[1:] == (32, 256) and survivors(c) == 8192 and len(runs(c)[0].keepers) == c['max_det'] == 1000
    c = BY_NAME['n8192_few_alive']
    assert c['score'].shape[1:] == (32, 256) and survivors(c) == 6


def test_options_validate_their_arguments():
    from efficientdet.pytorch_amd import ops
    import efficientdet.pytorch_amd as pkg
    assert pkg.SliceOptions is ops.SliceOptions and pkg.SliceMergeOptions is ops.SliceMergeOptions and pkg.SlicedDetector is pkg.evaluate.SlicedDetector
    m = ops.SliceMergeOptions()
    assert m.key() == ('nmm', 'ios', 0.5, True, 0.0, 256, 300) and m == ops.SliceMergeOptions('nmm', 'ios', 0.5, True, 0.0, 256, 300)
    assert m != ops.SliceMergeOptions(method='nms') and m != None and hash(m) == hash(ops.SliceMergeOptions())   # noqa: E711
    assert repr(m) == "SliceMergeOptions(method='nmm', metric='ios', thr=0.5, class_aware=True, skip_thr=0.0, top_n=256, max_det=300)"
    for bad in (dict(method='wbf'), dict(metric='giou'), dict(thr=-0.1), dict(thr=1.5), dict(thr=float('nan')), dict(skip_thr=-1.0),
                dict(skip_thr=float('nan')), dict(skip_thr=float('inf')), dict(top_n=0), dict(top_n=8193), dict(max_det=0), dict(max_det=8193)):
        with pytest.raises(ValueError):
            ops.SliceMergeOptions(**bad)
    o = ops.SliceOptions()
    assert o.key() == ((512, 512), (0.2, 0.2), True, 32, m.key()) and o == ops.SliceOptions([512, 512], [0.2, 0.2], True, 32, ops.SliceMergeOptions())
    assert o != ops.SliceOptions(tile_batch=8) and o != ops.SliceOptions(merge=ops.SliceMergeOptions(thr=0.6)) and hash(o) == hash(ops.SliceOptions())
    assert repr(o) == 'SliceOptions(slice=(512, 512), overlap=(0.2, 0.2), full_view=True, tile_batch=32, merge=%r)' % m
    for bad in (dict(slice=(500, 512)), dict(slice=(512, 0)), dict(slice=(512,)), dict(slice=(256.5, 256)), dict(slice=512), dict(overlap=(0.95, 0.2)),
                dict(overlap=(0.2, -0.1)), dict(overlap=(0.2, float('nan'))), dict(overlap=(0.2,)), dict(tile_batch=0)):
        with pytest.raises(ValueError):
            ops.SliceOptions(**bad)
    with pytest.raises(TypeError):
        ops.SliceOptions(merge='nmm')


def test_sliced_detector_validates_without_a_device():
    import torch
    from efficientdet.pytorch_amd import EfficientDet, SlicedDetector, SliceOptions, evaluate
    m = EfficientDet(3, is_training=False)
    d = SlicedDetector(m)
    assert d.options == SliceOptions() and d.num_classes == 3 and next(d.parameters()) is next(m.parameters()) and d.eval() is d and d.train(False) is d
    e = SlicedDetector(evaluate.EnsembleDetector([m, m]), SliceOptions(slice=(256, 256)))
    assert e.num_classes == 3 and torch.is_tensor(next(e.parameters()))
    with pytest.raises(TypeError):
        SlicedDetector(m, options='nmm')
    with pytest.raises(TypeError):
        SlicedDetector(object())
    with pytest.raises(ValueError, match='height 200 is smaller'):                          # the plan comes first: nothing touches a device
        SlicedDetector(m, SliceOptions(slice=(256, 256))).detections(torch.zeros(1, 3, 200, 850), 200, 850)


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'effdet_slices.h')).read(), flags=re.S)


def test_signatures_and_structs_match_the_header(tmp_path):
    from efficientdet.pytorch_amd import build, _lib
    h = _header()
    scalar = {'int': 'i', 'long long': 'q', 'float': 'f', 'effdet_stream_t': 'p'}
    protos = {}
    for r, name, params in re.findall(r'^([a-z][a-z ]*?\*?)\s*\b(effdet_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', h, flags=re.M):
        kinds = ['p' if '*' in p else scalar[' '.join(p.split()).rsplit(' ', 1)[0]] for p in params.split(',')]
        assert name not in protos, name
        protos[name] = ({'int': 'i', 'long long': 'q'}[' '.join(r.split())], kinds)
    assert sorted(protos) == ['effdet_slice_images', 'effdet_slice_merge', 'effdet_slice_merge_workspace_bytes']
    others = [getattr(_lib, n) for n in dir(_lib) if n.endswith('SIGNATURES') and n != 'SLICES_SIGNATURES']
    assert sorted(_lib.SLICES_SIGNATURES) == sorted(protos) and len(others) >= 14 and not any(set(protos) & set(t) for t in others)
    build.build(verbose=False)
    L = _lib.require(*protos)
    for name, (r, kinds) in protos.items():
        sig = _lib.SLICES_SIGNATURES[name]
        assert sig[1] == ':' and sig[0] == r and list(sig[2:].replace('s', 'p')) == kinds, (name, sig, r, kinds)
        f = getattr(L, name)
        assert f.restype is _lib._CTYPE[sig[0]] and list(f.argtypes) == [_lib._CTYPE[c] for c in sig[2:]], name
    assert (_lib.SLICE_MAX_TILES, _lib.SLICE_MAX_IN) == tuple(int(re.search(r'#define\s+EFFDET_SLICE_%s\s+(\d+)' % k, h).group(1)) for k in ('MAX_TILES', 'MAX_IN'))
    assert (_lib.SLICE_MAX_IN, R.MAX_IN, R.MAX_TILES) == (8192, 8192, 1024)
    assert re.search(r'enum\s*\{\s*EFFDET_SLICE_NMS = 0,\s*EFFDET_SLICE_NMM = 1\s*\}', h) and re.search(r'enum\s*\{\s*EFFDET_SLICE_IOU = 0,\s*EFFDET_SLICE_IOS = 1\s*\}', h)
    assert (_lib.SLICE_NMS, _lib.SLICE_NMM, _lib.SLICE_IOU, _lib.SLICE_IOS) == (0, 1, 0, 1)
    assert '-ffp-contract=off' in build.PER_FILE['slices.hip'] and _lib.ABI_VERSION == 11 and not set(protos) & set(_lib.SIGNATURES)
    src = open(os.path.join(ROOT, 'efficientdet', 'pytorch_amd', 'csrc', 'slices.hip')).read()
    assert '#include "radix_sort.h"' in src and 'rs_sort(' in src and 'rs_score_key(' in src and 'EFFDET_SET_MAX_LDS(' in src    # the shared sort, not another
    structs = {'effdet_slice_tile_t': _lib.SliceTile, 'effdet_slice_images_t': _lib.SliceImages, 'effdet_slice_merge_t': _lib.SliceMerge}
    names = {}
    for cname, cls in structs.items():
        body = re.search(r'typedef struct \{((?:(?!typedef).)*?)\}\s*%s;' % cname, h, flags=re.S).group(1)
        fields = []
        for decl in [d.strip() for d in body.split(';') if d.strip()]:
            typ, rest = re.match(r'(const [a-z_ ]+\*|[a-z_ ]+\*|int|float|long long)\s*(.*)$', decl).groups()
            ct = C.c_void_p if '*' in typ else {'int': C.c_int, 'float': C.c_float, 'long long': C.c_longlong}[typ]
            fields += [(n.strip(), ct) for n in rest.split(',')]
        assert fields == list(cls._fields_), (cname, fields)
        names[cname] = [n for n, _ in fields]
    if shutil.which('gcc') is None:
        return
    src = tmp_path / 'h.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "effdet_slices.h"\nint main(void){' +
                   ''.join('printf("%%zu ", sizeof(%s));' % c + ''.join('printf("%%zu ", offsetof(%s, %s));' % (c, n) for n in names[c]) for c in structs) +
                   'return 0;}\n')
    subprocess.run(['gcc', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(tmp_path / 'h')], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / 'h')], check=True, capture_output=True, text=True).stdout.split()]
    want = []
    for c, cls in structs.items():
        want += [C.sizeof(cls)] + [getattr(cls, n).offset for n in names[c]]
    assert got == want and C.sizeof(_lib.SliceTile) == 16


def test_refusals_are_decided_on_the_host_and_launch_nothing():
    from efficientdet.pytorch_amd import build, _lib
    build.build(verbose=False)
    L = _lib.require('effdet_slice_images', 'effdet_slice_merge', 'effdet_slice_merge_workspace_bytes')
    buf = np.zeros(8192, dtype=np.uint8)
    p = buf.ctypes.data + (-buf.ctypes.data) % 16

    def img(**kw):
        d = _lib.SliceImages()
        d.src, d.dst, d.tiles, d.src_layout, d.dtype, d.B, d.H, d.W, d.C, d.T, d.t0, d.t1, d.h, d.w, d.src_ld, d.src_bstride = p, p, p, 1, 0, 2, 8, 8, 4, 3, 0, 6, 4, 4, 4, 256
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    f = L.effdet_slice_images
    assert f(None, None) == -1
    for kw in (dict(src=None), dict(dst=None), dict(tiles=None), dict(dst=p + 8), dict(tiles=p + 4)):
        assert f(C.byref(img(**kw)), None) == -1, kw
    for kw in (dict(src_layout=2), dict(dtype=2), dict(src_layout=0, dtype=1), dict(B=0), dict(B=65536), dict(H=0), dict(W=32769), dict(h=0), dict(w=32769),
               dict(T=0), dict(t0=-1), dict(t0=6), dict(t1=7), dict(t0=3, t1=3), dict(B=65535, T=65535), dict(B=400, T=400, t0=0, t1=65536),
               dict(C=2), dict(src_ld=3), dict(src_bstride=-1)):
        assert f(C.byref(img(**kw)), None) == -3, kw

    def mrg(**kw):
        d = _lib.SliceMerge()
        for n in ('score', 'label', 'boxes', 'count', 'tiles', 'out_score', 'out_label', 'out_boxes', 'out_count'):
            setattr(d, n, p)
        d.B, d.TPI, d.R, d.method, d.metric, d.class_aware, d.max_det, d.W, d.H, d.thr, d.skip_thr = 1, 4, 8, 1, 1, 1, 8, 100.0, 100.0, 0.5, 0.0
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    g, wsb = L.effdet_slice_merge, L.effdet_slice_merge_workspace_bytes
    need = wsb(1, 4, 8)
    assert need > 0 and wsb(1, 32, 256) > need and wsb(0, 4, 8) == 0 and wsb(1, 1025, 1) == 0 and wsb(1, 32, 257) == 0 and wsb(1, 4, 0) == 0
    assert g(None, p, need, None) == -1 and g(C.byref(mrg()), None, need, None) == -1 and g(C.byref(mrg()), p, need - 1, None) == -1
    for kw in (dict(B=0), dict(score=None), dict(label=None), dict(boxes=None), dict(count=None), dict(tiles=None), dict(out_score=None),
               dict(out_label=None), dict(out_boxes=None), dict(out_count=None), dict(boxes=p + 8), dict(out_boxes=p + 4), dict(tiles=p + 8), dict(label=p + 4)):
        assert g(C.byref(mrg(**kw)), p, need, None) == -1, kw
    big = 1 << 40                                                      # (the size is checked after the options: never reached)
    for kw in (dict(TPI=0), dict(TPI=1025, R=1), dict(R=0), dict(TPI=32, R=257), dict(TPI=1, R=8193), dict(max_det=0), dict(max_det=33), dict(method=2),
               dict(method=-1), dict(metric=2), dict(metric=-1), dict(thr=1.5), dict(thr=-0.1), dict(thr=float('nan')), dict(skip_thr=float('nan')),
               dict(W=0.0), dict(H=-1.0), dict(W=float('inf')), dict(H=float('nan'))):
        assert g(C.byref(mrg(**kw)), p, big, None) == -3, kw
    assert not buf.any()


def test_the_model_test_fixture_conditions_hold_on_the_oracle():
    """tests/test_gpu_slices_model.py asserts of its fixture that every list has 0 < count <= 200 and that in both images the restated
    merge has a death across two tiles and a hull larger than its keeper.  The same on the CPU: the oracle's D0 on the same seeded
    images and tiles (the full view through torch's bilinear interpolate), the top 1000 scores through its greedy NMS, 200 kept."""
    import torch
    from oracle import effdet_oracle as O
    from tests.slices_cases import MODEL_CASE as M
    sd = O.make_state_dict('efficientdet-d0', 20, seed=0)
    img = M['images']()
    Hh, Ww = img.shape[2:]
    h, w = M['slice']
    table = R.plan(Hh, Ww, M['slice'], M['overlap'])
    assert (Hh, Ww) == (600, 850) and len(table) == 16 and len(table) * M['top_n'] == 3200 <= R.MAX_IN
    with torch.no_grad():
        for b in range(2):
            S = np.zeros((16, 200), np.float32); Lb = np.zeros((16, 200), np.int64); Bx = np.zeros((16, 200, 4), np.float32); cnt = np.zeros(16, np.int32)
            for j, (y0, x0, _, _, _, _) in enumerate(table):
                x = img[b:b + 1, :, y0:y0 + h, x0:x0 + w] if j < 15 else torch.nn.functional.interpolate(img[b:b + 1], size=(h, w), mode='bilinear', align_corners=False)
                cls, reg, anc = O.forward_raw(sd, 'efficientdet-d0', 20, x)
                boxes = O.decode_clip(anc, reg, h, w)[0]
                sc, lab = cls[0].max(dim=1)
                top = torch.argsort(-sc, stable=True)[:1000]
                top = top[sc[top] > 0.01]
                keep = top[O.nms_greedy(boxes[top], sc[top], 0.5)[:200]]
                n = len(keep)
                S[j, :n], Lb[j, :n], Bx[j, :n], cnt[j] = sc[keep].numpy(), lab[keep].numpy(), boxes[keep].numpy(), n
            assert 0 < cnt.min() and cnt.max() <= 200
            r = R.merge(S, Lb, Bx, cnt, table, float(Ww), float(Hh), max_det=300)
            assert any(t != k[0] for k, a in zip(r.keepers, r.absorbed) for t, _ in a)
            assert ((r.boxes[:, 2] - r.boxes[:, 0]) * (r.boxes[:, 3] - r.boxes[:, 1]) > (r.own[:, 2] - r.own[:, 0]) * (r.own[:, 3] - r.own[:, 1])).any()
