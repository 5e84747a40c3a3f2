"""CPU tier: the NumPy restatement of the weighted boxes fusion (tests/wbf_restated.py) on hand-derived cases whose every number is
exact, fp32 against its float64 twin on the seeded cases, the single-view identity, the options' validation and the binding's table
and struct against include/effdet_wbf.h."""
import functools
import os
import re

import numpy as np
import pytest

from tests import wbf_restated as R
from tests.wbf_cases import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BY_NAME = {c['name']: c for c in CASES}
MARGIN = 1e-4


def _view(rows):
    """[(x1, y1, x2, y2, score, label)] -> one image's view."""
    a = np.asarray(rows, dtype=np.float64).reshape(-1, 6)
    return a[:, 4].astype(np.float32), a[:, 5].astype(np.int64), a[:, :4].astype(np.float32), len(a)


def _image_views(case, b):
    return [(s[b], l[b], bx[b], int(n[b])) for s, l, bx, n in case['views']]


def _opts(case):
    return R.Opts(case['iou_thr'], case['skip_thr'], case['top_n'])


@functools.lru_cache(maxsize=None)
def _runs(name, b):
    c = BY_NAME[name]
    args = (_image_views(c, b), c['weights'], c['flips'], c['muls'], _opts(c))
    return R.run_f32(*args), R.run_f64(*args)


@pytest.mark.parametrize('run', [R.run_f32, R.run_f64])
def test_worked_examples_by_hand(run):
    # the header's example: IoU((0,0,8,8), (0,0,8,6)) = 48 / 64 = 0.75 > 0.55 -> one cluster, box (0.75 * 8 + 0.25 * 6) / 1 = 7.5
    r = run([_view([(0, 0, 8, 8, 0.75, 1)]), _view([(0, 0, 8, 6, 0.25, 1)])])
    s, l, b = R.emit(r, 'avg')
    assert r.clusters == [[(0, 0), (1, 0)]] and s.tolist() == [0.5] and l.tolist() == [1] and b.tolist() == [[0, 0, 8, 7.5]]
    assert R.emit(r, 'max')[0].tolist() == [0.75]
    # another label: two clusters, each seen by one of two views -> halved under avg, untouched under max, boxes as they came
    r = run([_view([(0, 0, 8, 8, 0.75, 1)]), _view([(0, 0, 8, 6, 0.25, 2)])])
    s, l, b = R.emit(r, 'avg')
    assert s.tolist() == [0.375, 0.125] and l.tolist() == [1, 2] and b.tolist() == [[0, 0, 8, 8], [0, 0, 8, 6]]
    assert R.emit(r, 'max')[0].tolist() == [0.75, 0.25]
    # IoU exactly at the threshold (0.75) does not join: the test is >
    r = run([_view([(0, 0, 8, 8, 0.75, 1)]), _view([(0, 0, 8, 6, 0.25, 1)])], o=R.Opts(0.75))
    assert len(r.clusters) == 2
    # weights 2 and 1: conf 1.0 and 0.5, box y2 = (1.0 * 8 + 0.5 * 5) / 1.5 = 7, avg = (1.5 / 2) * 2 / 3 = 0.5, max = 1.0 / 2
    r = run([_view([(0, 0, 8, 8, 0.5, 0)]), _view([(0, 0, 8, 5, 0.5, 0)])], weights=[2.0, 1.0])
    assert R.emit(r, 'avg')[0].tolist() == [0.5] and R.emit(r, 'max')[0].tolist() == [0.5] and R.emit(r, 'avg')[2].tolist() == [[0, 0, 8, 7]]
    # three members from two views: cnt = 3 is clamped to V = 2: ((0.5 + 0.25 + 0.25) / 3) * 2 / 2 = 1 / 3
    r = run([_view([(0, 0, 8, 8, 0.5, 0), (0, 0, 8, 8, 0.25, 0)]), _view([(0, 0, 8, 8, 0.25, 0)])])
    assert r.clusters == [[(0, 0), (0, 1), (1, 0)]]
    assert R.emit(r, 'avg')[0][0] == r.T(1.0) / r.T(3.0) * r.T(2.0) / r.T(2.0) and R.emit(r, 'avg')[2].tolist() == [[0, 0, 8, 8]]
    # flip about 16 then x 2: (10, 0, 14, 4) -> (2, 0, 6, 4) -> (4, 0, 12, 8); view 0's (4, 0, 12, 8) is the same box
    r = run([_view([(4, 0, 12, 8, 0.5, 0)]), _view([(10, 0, 14, 4, 0.5, 0)])], flips=[None, 16.0], muls=[1.0, 2.0])
    assert r.clusters == [[(0, 0), (1, 0)]] and r.boxes.tolist() == [[4, 0, 12, 8]] and R.emit(r, 'avg')[0].tolist() == [0.5]
    # matching sees the CURRENT fused box: after (0,0,8,8) and (0,0,8,4) at equal conf fuse to (0,0,8,6) (IoU 0.5), the candidate
    # (0,0,8,3.5) has IoU 3.5 / 6 = 0.583 with the fused box but only 0.4375 with the founder: iou_thr 0.45 tells them apart
    r = run([_view([(0, 0, 8, 8, 0.5, 0), (0, 0, 8, 4, 0.5, 0), (0, 0, 8, 3.5, 0.25, 0)])], o=R.Opts(0.45))
    assert r.clusters == [[(0, 0), (0, 1), (0, 2)]] and r.boxes.tolist() == [[0, 0, 8, 5.5]]
    r = run([_view([(0, 0, 8, 8, 0.5, 0), (0, 0, 8, 3.5, 0.25, 0)])], o=R.Opts(0.45))
    assert len(r.clusters) == 2
    # count and top_n cut a view before the merge; skip_thr, NaN and degenerate rows drop out
    v = _view([(0, 0, 8, 8, 0.5, 0), (20, 0, 28, 8, 0.25, 0), (40, 0, 48, 8, 0.125, 0)])
    assert len(run([v], o=R.Opts(0.55, 0.0, 2)).clusters) == 2 and len(run([v[:3] + (1,)]).clusters) == 1
    assert len(run([v], o=R.Opts(0.55, 0.25)).clusters) == 2
    v = _view([(0, 0, 8, 8, np.nan, 0), (20, 0, 20, 8, 0.5, 0), (40, 8, 48, 0, 0.5, 0), (60, 0, 68, 8, 0.25, 0)])
    assert run([v]).clusters == [[(0, 3)]]
    # the tie of the seeded case: both IoUs are 128 / 640, the lower cluster index wins
    c = BY_NAME['mirror_symmetric_tie']
    r = run(_image_views(c, 0), o=_opts(c))
    assert len(r.clusters) == 101 and r.clusters[0] == [(0, 0), (0, 101)] and r.clusters[100] == [(0, 100)] and r.margin == 0.0
    # nothing in: nothing out
    assert run([_view([])]).clusters == [] and len(R.emit(run([_view([])]))[0]) == 0


def test_order_is_conf_then_view_then_row():
    c = BY_NAME['equal_conf_across_views']
    _, conf, _, v, r = R.candidates(_image_views(c, 0), c['weights'], c['flips'], c['muls'], _opts(c), np.float32)
    key = list(zip((-conf).tolist(), v.tolist(), r.tolist()))
    assert key == sorted(key) and len(set(conf.tolist())) <= 16 < len(conf)
    c = BY_NAME['count_exceeds_top_n']
    _, _, _, v, r = R.candidates(_image_views(c, 0), c['weights'], c['flips'], c['muls'], _opts(c), np.float32)
    assert (v == 0).sum() == 50 and r[v == 0].max() == 49 and (v == 1).sum() == 30          # cut per view, before the merge


def test_the_cases_cover_what_they_claim():
    assert sorted(c['n'] for c in CASES if re.fullmatch(r'n\d+', c['name'])) == [0, 1, 2, 63, 64, 65, 1023, 1024, 1025]
    assert BY_NAME['n4096_v4']['n'] == 4096 and sorted({len(c['views']) for c in CASES}) == [1, 2, 3, 4, 8]
    r = _runs('all_singletons_1100', 0)[0]
    assert len(r.clusters) == 1100 and all(len(m) == 1 for m in r.clusters)
    assert len(_runs('n4096_v4', 0)[0].clusters) > 2048                                       # a thread owns a third cluster
    r = _runs('one_cluster_of_300_identical', 0)[0]
    assert max(len(m) for m in r.clusters) == 300
    r = _runs('identical_boxes_different_labels', 0)[0]
    assert len(r.clusters) == 160 and all(len(m) == 2 for m in r.clusters)
    c = BY_NAME['batch3_one_empty']
    assert len(c['views'][0][3]) == 3 and _runs('batch3_one_empty', 1)[0].clusters == []
    assert len({v[0].shape[1] for v in BY_NAME['flip_mul_unequal_A']['views']}) == 3
    # the decoy rows past a view's count score 0.999 and are never members
    for c in CASES:
        for b in range(len(c['views'][0][3])):
            for members in _runs(c['name'], b)[0].clusters:
                assert all(r < min(int(c['views'][v][3][b]), c['top_n']) for v, r in members)


def test_float32_against_the_float64_twin():
    """Same membership wherever every decision of the float64 run is further than 1e-4 from iou_thr and from the runner-up; fused boxes
    and both scores within 1e-5 relative there.  At least 90 % of the seeded cases must qualify, or the comparison says nothing."""
    ok = 0
    for c in CASES:
        clear = True
        for b in range(len(c['views'][0][3])):
            r32, r64 = _runs(c['name'], b)
            if not r64.margin > MARGIN:
                clear = False
                continue
            assert r32.clusters == r64.clusters, (c['name'], b)
            for got, want in ((r32.boxes, r64.boxes), (r32.avg, r64.avg), (r32.max, r64.max)):
                np.testing.assert_allclose(got, want, rtol=1e-5, atol=0, err_msg=c['name'])
            assert np.array_equal(r32.label, r64.label)
        ok += clear
    print('%d of %d cases clear the %.0e margin' % (ok, len(CASES), MARGIN))
    assert ok >= 0.9 * len(CASES), (ok, len(CASES))


@pytest.mark.parametrize('name', ['all_singletons_1100', 'v1_n300'])
def test_single_view_identity(name):
    """One view whose rows overlap no more than iou_thr (iou_thr = 1 when they do): the output is the input, bit for bit."""
    c = BY_NAME[name]
    s, l, b, n = _image_views(c, 0)[0]
    n = int(n)
    o = R.Opts(0.55 if name == 'all_singletons_1100' else 1.0, 0.0, 1000)
    for w, conf_type in ((1.0, 'avg'), (1.0, 'max'), (0.7, 'max')):
        r = R.run_f32([(s, l, b, n)], weights=[w], o=o)
        es, el, eb = R.emit(r, conf_type)
        if w == 1.0:
            assert np.array_equal(es.view(np.uint32), s[:n].view(np.uint32))
        assert np.array_equal(el, l[:n]) and np.array_equal(eb.view(np.uint32), b[:n].view(np.uint32))


def test_options_validate_their_arguments():
    from efficientdet.pytorch_amd import ops
    o = ops.WBFOptions(0.6, 0.1, 'max', 500)
    assert o.key() == (0.6, 0.1, 'max', 500) and o == ops.WBFOptions(0.6, 0.1, 'max', 500) and o != ops.WBFOptions() and o != None   # noqa: E711
    assert hash(o) == hash(ops.WBFOptions(0.6, 0.1, 'max', 500)) and repr(o) == "WBFOptions(iou_thr=0.6, skip_box_thr=0.1, conf_type='max', top_n=500)"
    assert ops.WBFOptions().key() == (0.55, 0.0, 'avg', 1000)
    for bad in (dict(iou_thr=-0.1), dict(iou_thr=1.5), dict(iou_thr=float('nan')), dict(skip_box_thr=-1.0), dict(skip_box_thr=float('nan')),
                dict(conf_type='box_and_model_avg'), dict(top_n=0), dict(top_n=4097)):
        with pytest.raises(ValueError):
            ops.WBFOptions(**bad)
    t = ops.TTAOptions()
    assert t.hflip and t.weights is None and t.fusion == ops.WBFOptions() and t.num_views == 2 and t == ops.TTAOptions(True)
    assert t != ops.TTAOptions(False) and t != ops.TTAOptions(weights=(1, 2)) and ops.TTAOptions(weights=[1, 2]) == ops.TTAOptions(weights=(1.0, 2.0))
    assert hash(t) == hash(ops.TTAOptions()) and 'hflip=True' in repr(t)
    for bad in (dict(weights=(1.0,)), dict(weights=(1.0, 0.0)), dict(weights=(1.0, float('inf'))), dict(hflip=False, weights=(1.0, 1.0)),
                dict(fusion=ops.WBFOptions(top_n=2049))):
        with pytest.raises(ValueError):
            ops.TTAOptions(**bad)
    with pytest.raises(TypeError):
        ops.TTAOptions(fusion='avg')
    assert ops.TTAOptions(hflip=False, fusion=ops.WBFOptions(top_n=4096)).num_views == 1


def test_set_tta_and_ensemble_validate_without_a_device():
    import torch
    from efficientdet.pytorch_amd import EfficientDet, evaluate, ops
    m = EfficientDet(3, is_training=False)
    assert m.tta_options is None and m.set_tta(ops.TTAOptions()) is m and m.tta_options == ops.TTAOptions()
    assert m.set_tta(None).tta_options is None
    with pytest.raises(TypeError):
        m.set_tta(True)
    del m.tta_options                                                      # a model pickled before the option existed
    assert getattr(m, 'tta_options', None) is None
    e = evaluate.EnsembleDetector([m, m], weights=(2, 1))
    assert e.num_classes == 3 and e.weights == (2.0, 1.0) and next(e.parameters()) is next(m.parameters())
    for bad in (dict(models=[]), dict(models=[m] * 9), dict(models=[m, EfficientDet(4, is_training=False)]), dict(models=[m, m], weights=(1,)),
                dict(models=[m, m], fusion=ops.WBFOptions(top_n=4096))):
        with pytest.raises(ValueError):
            evaluate.EnsembleDetector(**bad)
    assert torch.is_tensor(next(e.parameters()))


def test_signatures_and_struct_match_the_header(tmp_path):
    """_lib.WBF_SIGNATURES against the prototypes of include/effdet_wbf.h (names, return kind, parameter kinds in order), the built library
    exports and binds them, and _lib.Wbf has the size and field offsets gcc gives effdet_wbf_t."""
    import ctypes as C
    import shutil
    import subprocess
    from efficientdet.pytorch_amd import build, _lib
    h = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'effdet_wbf.h')).read(), flags=re.S)
    scalar = {'int': 'i', 'long long': 'q', 'float': 'f', 'effdet_stream_t': 'p'}
    protos = {}
    for r, name, params in re.findall(r'^([a-z][a-z ]*?\*?)\s*\b(effdet_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', h, flags=re.M):
        kinds = ['p' if '*' in p else scalar[' '.join(p.split()).rsplit(' ', 1)[0]] for p in params.split(',')]
        assert name not in protos, name
        protos[name] = ({'int': 'i', 'long long': 'q'}[' '.join(r.split())], kinds)
    assert sorted(protos) == ['effdet_wbf', 'effdet_wbf_workspace_bytes']
    all_others = [_lib.SIGNATURES, _lib.ADDED_SIGNATURES, _lib.EMA_SIGNATURES, _lib.PLAN_SIGNATURES, _lib.LIVE_SIGNATURES,
                  _lib.BOX_LOSS_SIGNATURES, _lib.LOSS_OPTS_SIGNATURES, _lib.ATSS_SIGNATURES, _lib.CONV_PLAN_SIGNATURES]
    assert sorted(_lib.WBF_SIGNATURES) == sorted(protos) and not any(set(protos) & set(t) for t in all_others)
    build.build(verbose=False)
    L = _lib.require(*protos)
    for name, (r, kinds) in protos.items():
        sig = _lib.WBF_SIGNATURES[name]
        assert sig[1] == ':' and sig[0] == r, (name, sig, r)
        assert list(sig[2:].replace('s', 'p')) == kinds, (name, sig, ''.join(kinds))
        f = getattr(L, name)
        assert f.restype is _lib._CTYPE[sig[0]] and list(f.argtypes) == [_lib._CTYPE[c] for c in sig[2:]], name
    assert (_lib.WBF_MAX_VIEWS, _lib.WBF_MAX_IN) == tuple(int(re.search(r'#define\s+EFFDET_WBF_%s\s+(\d+)' % k, h).group(1)) for k in ('MAX_VIEWS', 'MAX_IN'))
    if shutil.which('gcc') is None:
        return
    fields = [n for n, _ in _lib.Wbf._fields_]
    assert fields == re.findall(r'\b(\w+)(?:\[EFFDET_WBF_MAX_VIEWS\])?\s*[;,]', re.search(r'typedef struct \{(.*?)\} effdet_wbf_t;', h, flags=re.S).group(1))
    src = tmp_path / 'h.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "effdet_wbf.h"\nint main(void){printf("%zu", sizeof(effdet_wbf_t));' +
                   ''.join('printf(" %%zu", offsetof(effdet_wbf_t, %s));' % n for n in fields) +
                   'return EFFDET_WBF_AVG == 0 && EFFDET_WBF_MAX == 1 ? 0 : 1;}\n')
    subprocess.run(['gcc', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(tmp_path / 'h')], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / 'h')], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(_lib.Wbf)] + [getattr(_lib.Wbf, n).offset for n in fields]


def test_against_the_published_implementation():
    """ensemble_boxes.weighted_boxes_fusion on a case with clear margins.  It works in normalised coordinates, divides a singleton's
    (conf * x) / conf and orders ties its own way: boxes within 1e-6 absolute (normalised), matched by label and score."""
    eb = pytest.importorskip('ensemble_boxes')
    c = BY_NAME['v3']
    views = _image_views(c, 0)
    assert _runs('v3', 0)[1].margin > MARGIN
    for conf_type in ('avg', 'max'):
        s, l, b = R.emit(_runs('v3', 0)[0], conf_type)
        pb, ps, pl = eb.weighted_boxes_fusion([(v[2][:v[3]] / 512.0).clip(0, 1).tolist() for v in views], [v[0][:v[3]].tolist() for v in views],
                                              [v[1][:v[3]].tolist() for v in views], weights=c['weights'], iou_thr=c['iou_thr'],
                                              skip_box_thr=c['skip_thr'], conf_type=conf_type)
        assert len(ps) == len(s)
        mine = sorted(zip(l.tolist(), s.tolist(), (b / 512.0).tolist()))
        theirs = sorted(zip([int(x) for x in pl], [float(x) for x in ps], np.asarray(pb).tolist()))
        for (l0, s0, b0), (l1, s1, b1) in zip(mine, theirs):
            assert l0 == l1 and abs(s0 - s1) <= 1e-6 and np.abs(np.asarray(b0) - np.asarray(b1)).max() <= 1e-6
