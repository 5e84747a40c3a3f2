"""CPU tier of the operating-point metrics (include/effdet_op_point.h, csrc/op_point.hip, evaluate.OperatingPoint): the NumPy
restatement (tests/op_point_restated.py) on the hand cases' literals, the prefix property the header claims (the counts at a threshold
are those of a full VOC re-evaluation over the detections above it), the confusion rule against an independent formulation written the
way Ultralytics writes it, what the cases claim to cover, the threshold validator, the binding's table against the header, and the
refusals both entry points decide on the host."""
import os
import re

import numpy as np
import pytest

from tests import op_point_restated as R
from tests.op_point_cases import CONFUSION_CASES, CURVES_CASES, device_gt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = {c['name']: c for c in CURVES_CASES}
CONFUSION = {c['name']: c for c in CONFUSION_CASES}
TABLES = ('tp', 'npred', 'precision', 'recall', 'f1', 'mean', 'best')


def _records(case):
    if case['dets'] is None:
        C = case['C']
        return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint8), np.zeros(C, dtype=np.int32)
    return R.voc_records(case['dets'], case['counts'], case['gts'], case['C'], case['iou'])


def _restated_curves(case):
    key, tp, gt_count = _records(case)
    return R.curves(key, tp, gt_count, case['C'], R.check_thresholds(case['thresholds']))


# ------------------------------------------------------------------------------------------------ literals
@pytest.mark.parametrize('name', [c['name'] for c in CURVES_CASES if c['expect'] is not None])
def test_the_restated_curves_reproduce_the_literals(name):
    case = CURVES[name]
    got = _restated_curves(case)
    for k in TABLES:
        want = np.asarray(case['expect'][k], dtype=got[k].dtype)
        assert got[k].shape == want.shape and np.array_equal(got[k], want), (name, k, got[k], want)


@pytest.mark.parametrize('name', [c['name'] for c in CONFUSION_CASES if c['expect'] is not None])
def test_the_restated_confusion_reproduces_the_literals(name):
    case = CONFUSION[name]
    got = R.confusion(case['dets'], case['counts'], case['gts'], case['C'], case['conf'], case['iou'])
    assert got.dtype == np.int64 and np.array_equal(got, np.asarray(case['expect'], dtype=np.int64)), (name, got)


def test_the_hand_case_differs_from_greedy_one_to_one_matching():
    """Greedy one-to-one matching would hand the loser its second candidate (IoU 0.5 > 0.45 with object 1): [1][1], not [1][C] + [C][1]."""
    case = CONFUSION['hand']
    d, g = case['dets'][0], case['gts'][0]
    ious = np.array([R.iou_row(d[k, :4], g[:, :4]) for k in range(2)])
    assert np.array_equal(ious, [[1.0, 0.625], [0.8, 0.5]]) and case['expect'][1][1] == 0 and case['expect'][1][2] == 1 and case['expect'][2][1] == 1


# ------------------------------------------------------------------------------------------------ the prefix property
def _voc_counts(rows, gts, C, iou):
    """The reference's evaluate restated per image and class (detections in row order, np.argmax, a taken set) -> (tp [C], fp [C])."""
    tp, fp = np.zeros(C, dtype=np.int64), np.zeros(C, dtype=np.int64)
    for d, g in zip(rows, gts):
        g = np.asarray(g, dtype=np.float64).reshape(-1, 5)
        for c in range(C):
            dc, gc = d[d[:, 5] == c], g[g[:, 4] == c, :4]
            taken = set()
            for r in dc:
                if len(gc) == 0:
                    fp[c] += 1
                    continue
                ov = R.iou_row(r[:4], gc)
                a = int(np.argmax(ov))
                if ov[a] >= iou and a not in taken:
                    taken.add(a); tp[c] += 1
                else:
                    fp[c] += 1
    return tp, fp


@pytest.mark.parametrize('name', [c['name'] for c in CURVES_CASES if c['dets'] is not None])
def test_counts_equal_a_full_reevaluation_above_each_threshold(name):
    case = CURVES[name]
    C, th = case['C'], R.check_thresholds(case['thresholds'])
    got = _restated_curves(case)
    rows = [case['dets'][b, :case['counts'][b]] for b in range(len(case['counts']))]
    assert all(np.all(np.diff(r[:, 4]) <= 0) for r in rows)                      # the precondition: score-descending rows
    seen = {}
    for j, t in enumerate(th):
        masks = [r[:, 4] > t for r in rows]
        k = b''.join(m.tobytes() for m in masks)
        if k not in seen:                                                        # (many thresholds select the same detections)
            seen[k] = _voc_counts([r[m] for r, m in zip(rows, masks)], case['gts'], C, case['iou'])
        tp, fp = seen[k]
        assert np.array_equal(got['tp'][:, j], tp) and np.array_equal(got['npred'][:, j] - got['tp'][:, j], fp), (name, j, t)
    assert len(seen) > 1 or len(th) == 1


# ------------------------------------------------------------------------------------------------ confusion: independent formulation
def _process_batch(d, n, g, C, conf, iou_thres):
    """Ultralytics' ConfusionMatrix.process_batch for one image: candidate list in (object, prediction) order, stable sort by IoU
    descending, first occurrence per prediction, sort again, first occurrence per object."""
    m = np.zeros((C + 1, C + 1), dtype=np.int64)
    d = d[:n]
    ok = (d[:, 5] >= 0) & (d[:, 5] < C) & (d[:, 5] == np.floor(d[:, 5])) & (d[:, 4] > np.float32(conf))
    d = d[ok]
    g = np.asarray(g, dtype=np.float64).reshape(-1, 5)
    g = g[(g[:, 4] >= 0) & (g[:, 4] < C) & (g[:, 4] == np.floor(g[:, 4]))]
    dc, gc = d[:, 5].astype(np.int64), g[:, 4].astype(np.int64)
    iou = np.array([R.iou_row(r[:4], g[:, :4]) for r in d]).reshape(len(d), len(g)).T          # [objects, predictions]
    x = np.nonzero(iou > iou_thres)
    matches = np.stack([x[0], x[1], iou[x[0], x[1]]], 1) if len(x[0]) else np.zeros((0, 3))
    if len(matches) > 1:
        matches = matches[np.argsort(-matches[:, 2], kind='stable')]
        matches = matches[np.unique(matches[:, 1], return_index=True)[1]]
        matches = matches[np.argsort(-matches[:, 2], kind='stable')]
        matches = matches[np.unique(matches[:, 0], return_index=True)[1]]
    m0, m1 = matches[:, 0].astype(np.int64), matches[:, 1].astype(np.int64)
    for i, c in enumerate(gc):
        hit = np.nonzero(m0 == i)[0]
        if len(hit) == 1:
            m[dc[m1[hit[0]]], c] += 1
        else:
            m[C, c] += 1
    for i, c in enumerate(dc):
        if not np.any(m1 == i):
            m[c, C] += 1
    return m


@pytest.mark.parametrize('name', [c['name'] for c in CONFUSION_CASES])
def test_the_restated_confusion_equals_the_process_batch_formulation(name):
    case = CONFUSION[name]
    C = case['C']
    got = R.confusion(case['dets'], case['counts'], case['gts'], C, case['conf'], case['iou'])
    want = sum(_process_batch(case['dets'][b], case['counts'][b], case['gts'][b], C, case['conf'], case['iou']) for b in range(len(case['gts'])))
    assert np.array_equal(got, want), (name, got, want)
    # column c sums to the class's objects, row r to its predictions
    _, labels = device_gt(case['gts'], C)
    objects = np.bincount(labels[labels >= 0], minlength=C)
    preds = np.zeros(C, dtype=np.int64)
    for b in range(len(case['gts'])):
        for r in case['dets'][b, :case['counts'][b]]:
            if 0 <= r[5] < C and r[5] == np.floor(r[5]) and r[4] > np.float32(case['conf']):
                preds[int(r[5])] += 1
    assert np.array_equal(got[:, :C].sum(0), objects) and np.array_equal(got[:C].sum(1), preds) and got[C, C] == 0


# ------------------------------------------------------------------------------------------------ coverage
def test_the_cases_reach_the_edges_they_are_tagged_with():
    names = [c['name'] for c in CURVES_CASES]
    assert names == ['hand', 'chunks', 'ties', 'tiles', 'extremes_m4096', 'extremes_m1', 'empty']
    hand = CURVES['hand']
    assert hand['C'] == 2 and len(hand['gts']) == 2 and int(hand['counts'].sum()) == 5 and len(hand['thresholds']) == 4
    # chunks: segment lengths around the 256-record chunk, a class with records and no GT, one with GT and no records
    ch = CURVES['chunks']
    key, tp, gt_count = _records(ch)
    lengths = np.bincount((key >> np.uint64(32)).astype(np.int64), minlength=ch['C'] + 1)[:ch['C']]
    assert list(lengths) == [0, 1, 255, 256, 257, 513, 40, 0]
    assert gt_count[0] > 0 and gt_count[6] == 0 and gt_count[7] == 0 and all(gt_count[1:6] > 0)
    assert all(tp[(key >> np.uint64(32)) == c].sum() > 0 for c in (2, 3, 4, 5))
    # ties: a run of equal scores across position 256 of the class's sorted segment; a threshold on it and one just below
    ti = CURVES['ties']
    key, tp, _ = _records(ti)
    low = np.sort(key[(key >> np.uint64(32)) == 0] & np.uint64(0xffffffff))
    k5 = np.uint64(R.score_key(np.float32(0.5))[0])
    run = np.nonzero(low == k5)[0]
    assert (run[0], run[-1] + 1) == ti['run'] and run[0] < 256 < run[-1]
    th = R.check_thresholds(ti['thresholds'])
    assert th[2] == np.float32(0.5) and th[1] == np.nextafter(np.float32(0.5), np.float32(0)) and th[1] < th[2]
    got = _restated_curves(ti)
    assert got['npred'][0, 2] == 200 and got['npred'][0, 1] == 320                # none of the run at 0.5, all of it just below
    seg_tp = tp[np.argsort(key, kind='stable')][:370]
    assert 0 < seg_tp[200:320].sum() < 120 and seg_tp[200:256].sum() > 0 and seg_tp[256:320].sum() > 0        # mixed TP / FP on both sides
    # tiles: more than one 2048-key tile of the sort, most of it empty slots
    tl = CURVES['tiles']
    key, _, _ = _records(tl)
    assert len(key) == 3 * 1024 > 2048 and tl['dets'].shape[1] == 1024
    assert np.count_nonzero((key >> np.uint64(32)) == tl['C']) > 2048 and np.count_nonzero((key >> np.uint64(32)) < tl['C']) == 75
    # extremes
    ex = CURVES['extremes_m4096']
    th = R.check_thresholds(ex['thresholds'])
    sc = ex['dets'][:, :, 4][ex['dets'][:, :, 5] >= 0]
    assert len(th) == 4096 and th[0] < sc.min() and th[-1] > sc.max() and np.any(th == 0) and np.isin(sc, th).all()
    got = _restated_curves(ex)
    assert got['npred'][:, 0].sum() == len(sc) and got['npred'][:, -1].sum() == 0
    e1 = CURVES['extremes_m1']
    assert len(e1['thresholds']) == 1 and e1['thresholds'][0] == 0.0 and np.count_nonzero(e1['dets'][0, :3, 4] == 0) == 2
    assert CURVES['empty']['dets'] is None and CURVES['empty']['thresholds'] is None
    # confusion
    lp = CONFUSION['loops']
    assert lp['counts'][0] > 256 and len(lp['gts'][1]) > 256 and len(lp['gts'][2]) == 2048 == R.MAX_GT
    pd = CONFUSION['padded']
    assert pd['counts'][0] == 0 and len(pd['gts'][0]) > 0 and len(pd['gts'][1]) == 0 and pd['counts'][1] > 0
    assert {2.0, -1.0, 0.5} <= set(pd['dets'][2, :, 5].tolist()) and {2.0, -1.0, 0.5} <= set(pd['gts'][2][:, 4].tolist())
    rn = CONFUSION['random']
    m = R.confusion(rn['dets'], rn['counts'], rn['gts'], rn['C'], rn['conf'], rn['iou'])
    assert np.trace(m[:rn['C'], :rn['C']]) > 0 and (m[:rn['C'], :rn['C']].sum() - np.trace(m[:rn['C'], :rn['C']])) > 0
    assert m[rn['C']].sum() > 0 and m[:, rn['C']].sum() > 0
    assert np.any(rn['dets'][:, :, 4] == np.float32(0.25))                         # scores exactly on conf


# ------------------------------------------------------------------------------------------------ the validator
def test_the_threshold_validator():
    from efficientdet.pytorch_amd import ops
    for f in (ops.op_thresholds, R.check_thresholds):
        d = f(None)
        assert d.dtype == np.float32 and np.array_equal(d, (np.arange(1001) / 1000).astype(np.float32))
        for bad in ([], [0.1, float('nan')], [0.1, float('inf')], [float('-inf'), 0.1], [0.5, 0.25], [0.25, 0.25],
                    np.linspace(0, 1, 4097), [[]]):
            with pytest.raises(ValueError):
                f(bad)
        t = f([-0.0, 0.5])
        assert t.dtype == np.float32 and not np.signbit(t[0]) and np.array_equal(t, np.array([0.0, 0.5], dtype=np.float32))
        assert len(f(np.linspace(0, 1, 4096))) == 4096 and len(f([0.3])) == 1
        src = np.array([-0.0, 1.0], dtype=np.float32)
        f(src)
        assert np.signbit(src[0])                                                  # the caller's array is left alone
    assert ops.OP_MAX_THRESHOLDS == R.MAX_THRESHOLDS == 4096 and ops.VOC_MAX_GT == R.MAX_GT


def test_the_meter_validates_without_a_device():
    from efficientdet.pytorch_amd.evaluate import OperatingPoint, evaluate_operating_point
    for kw in (dict(thresholds=[0.5, 0.1]), dict(thresholds=[]), dict(conf_threshold=float('nan')), dict(confusion_iou=float('nan'))):
        with pytest.raises(ValueError):
            OperatingPoint(3, device='cpu', **kw)
    with pytest.raises(ValueError):
        OperatingPoint(0, device='cpu')
    m = OperatingPoint(3, device='cpu')
    assert m.num_records == 0 and tuple(m._confusion.shape) == (4, 4) and len(m.thresholds) == 1001
    assert (m.iou_threshold, m.conf_threshold, m.confusion_iou) == (0.5, 0.25, 0.45)
    assert 'model.threshold' in evaluate_operating_point.__doc__ and 'score_threshold' in evaluate_operating_point.__doc__


# ------------------------------------------------------------------------------------------------ the binding
def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'effdet_op_point.h')).read(), flags=re.S)


def _prototypes():
    scalar = {'int': 'i', 'long long': 'q', 'float': 'f', 'double': 'd', 'effdet_stream_t': 'p'}
    protos = {}
    for r, name, params in re.findall(r'^([a-z][a-z ]*?\*?)\s*\b(effdet_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', _header(), flags=re.M):
        kinds = ['p' if '*' in p else scalar[' '.join(p.split()).rsplit(' ', 1)[0]] for p in params.split(',')]
        assert name not in protos, name
        protos[name] = ({'int': 'i', 'long long': 'q'}[' '.join(r.split())], kinds)
    return protos


def test_signatures_match_the_header():
    from efficientdet.pytorch_amd import build, _lib, ops
    protos = _prototypes()
    assert sorted(protos) == ['effdet_confusion_match', 'effdet_op_curves', 'effdet_op_curves_workspace_bytes']
    others = [getattr(_lib, n) for n in dir(_lib) if n.endswith('SIGNATURES') and n != 'OP_POINT_SIGNATURES']
    assert sorted(_lib.OP_POINT_SIGNATURES) == sorted(protos) and len(others) >= 15 and not any(set(protos) & set(t) for t in others)
    build.build(verbose=False)
    L = _lib.require(*protos)
    for name, (r, kinds) in protos.items():
        sig = _lib.OP_POINT_SIGNATURES[name]
        assert sig[1] == ':' and sig[0] == r and list(sig[2:].replace('s', 'p')) == kinds, (name, sig, r, kinds)
        f = getattr(L, name)
        assert f.restype is _lib._CTYPE[sig[0]] and list(f.argtypes) == [_lib._CTYPE[c] for c in sig[2:]], name
    assert _lib.OP_MAX_THRESHOLDS == int(re.search(r'#define\s+EFFDET_OP_MAX_THRESHOLDS\s+(\d+)', _header()).group(1)) == 4096
    assert '-ffp-contract=off' in build.PER_FILE['op_point.hip'] and _lib.ABI_VERSION == 11
    main = open(os.path.join(ROOT, 'include', 'effdet_hip.h')).read()
    assert not any(n in main for n in protos)                                      # additive: the main header does not know them
    src = open(os.path.join(ROOT, 'efficientdet', 'pytorch_amd', 'csrc', 'op_point.hip')).read()
    assert '#include "radix_sort.h"' in src and '#include "block_scan.h"' in src                  # the shared sort and scan, not others
    assert all(s in src for s in ('rs_sort(', 'rs_score_key(', 'rs_segment_bounds(', 'rs_init_kernel', 'block_scan_sum(', 'EFFDET_SET_MAX_LDS('))
    assert callable(ops.op_curves) and callable(ops.confusion_match)


def test_refusals_are_decided_on_the_host_and_launch_nothing():
    from efficientdet.pytorch_amd import build, _lib
    build.build(verbose=False)
    L = _lib.require(*_lib.OP_POINT_SIGNATURES)
    buf = np.zeros(1 << 20, dtype=np.uint8)
    p = buf.ctypes.data
    wsb = L.effdet_op_curves_workspace_bytes
    need = wsb(1000)
    assert need >= 1000 * 28 and wsb(0) > 0 and wsb(100000) > need and wsb(-1) == 0 and wsb(1 << 31) == 0
    assert need <= buf.size

    def curves(**kw):
        a = dict(key=p, tp_byte=p, N=1000, gt=p, C=3, th=p, M=5, ws=p, wsn=need, o1=p, o2=p, o3=p, o4=p, o5=p, o6=p, o7=p)
        a.update(kw)
        return L.effdet_op_curves(a['key'], a['tp_byte'], a['N'], a['gt'], a['C'], a['th'], a['M'], a['ws'], a['wsn'], a['o1'], a['o2'], a['o3'],
                                  a['o4'], a['o5'], a['o6'], a['o7'], None)
    for kw in (dict(M=0), dict(M=4097), dict(C=65536)):
        assert curves(**kw) == -3, kw
    for kw in (dict(key=None), dict(tp_byte=None), dict(gt=None), dict(th=None), dict(ws=None), dict(wsn=need - 1), dict(N=-1), dict(N=1 << 31),
               dict(C=0), dict(o1=None), dict(o2=None), dict(o3=None), dict(o4=None), dict(o5=None), dict(o6=None), dict(o7=None)):
        assert curves(**kw) == -1, kw

    def conf(**kw):
        a = dict(d=p, n=p, gb=p, gl=p, B=2, S=8, G=4, C=3, conf=0.25, iou=0.45, m=p)
        a.update(kw)
        return L.effdet_confusion_match(a['d'], a['n'], a['gb'], a['gl'], a['B'], a['S'], a['G'], a['C'], a['conf'], a['iou'], a['m'], None)
    assert conf(G=2049) == -3
    for kw in (dict(d=None), dict(n=None), dict(gb=None), dict(gl=None), dict(m=None), dict(B=0), dict(S=0), dict(G=0), dict(C=0), dict(C=65536),
               dict(conf=float('nan')), dict(iou=float('nan'))):
        assert conf(**kw) == -1, kw
    assert not buf.any()
