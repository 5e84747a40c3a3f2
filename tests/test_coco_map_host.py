"""CPU tier of the device COCO metric (csrc/coco_map.hip, evaluate.COCOMeanAP / evaluate_coco): the entry points are declared and
bound, the meter refuses bad arguments before any device work, summarize_lines reproduces COCOeval's format, and hand-derived
cases pin the NumPy restatement (tests/coco_eval_restated.py) that the GPU tier holds the device to.  Where pycocotools is
installed, the restatement is also compared with COCOeval itself."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import coco_eval_restated as R
from tests import coco_map_cases as CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = CASES.V


def test_coco_entry_points_are_declared_and_bound():
    from efficientdet.pytorch_amd import _lib, build, evaluate, ops
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'effdet_hip.h')).read(), flags=re.S)
    for name in ('effdet_coco_slots', 'effdet_coco_match', 'effdet_coco_accumulate', 'effdet_coco_accumulate_workspace_bytes'):
        assert re.search(r'\b%s\s*\(' % name, hdr), name
        assert name in _lib.SYMBOLS, name
    assert _lib.ABI_VERSION == 11 and re.search(r'EFFDET_ABI_VERSION\s+11\b', open(os.path.join(ROOT, 'include', 'effdet_hip.h')).read())
    assert '-ffp-contract=off' in build.PER_FILE['coco_map.hip']       # fp64 IoUs at exactly a threshold: no FMA contraction
    for f in (ops.coco_match, ops.coco_accumulate, evaluate.evaluate_coco, evaluate.summarize_lines):
        assert callable(f)
    L = _lib.lib()
    assert L.effdet_coco_accumulate_workspace_bytes.restype is ctypes.c_longlong
    assert L.effdet_coco_accumulate_workspace_bytes(ctypes.c_longlong(500000), 80) >= 500000 * 24
    assert L.effdet_coco_slots(49104, 80, 100) == 8000 and L.effdet_coco_slots(100, 80, 100) == 100


def test_stale_library_asks_for_a_rebuild(monkeypatch):
    from efficientdet.pytorch_amd import _lib, ops

    class Stale:                                                        # same ABI generation, built before the COCO entry points
        pass
    monkeypatch.setattr(_lib, '_lib', Stale())
    with pytest.raises(RuntimeError, match='rebuild'):
        ops.coco_slots(100, 80)


def test_thresholds_are_numpy_linspace():
    from efficientdet.pytorch_amd import evaluate as EV
    assert EV.COCO_IOU_THRS[8] == 0.8999999999999999 and np.array_equal(EV.COCO_IOU_THRS, R.IOU_THRS)
    assert np.array_equal(EV.COCO_REC_THRS, R.REC_THRS)
    assert sum(EV.COCO_REC_THRS[i] != i / 100 for i in range(101)) == 10
    assert EV.COCO_AREA_RNG.tolist() == R.AREA_RNG and EV.COCO_MAX_DETS == R.MAX_DETS


def test_coco_meter_rejects_bad_arguments():
    from efficientdet.pytorch_amd.evaluate import COCOMeanAP
    with pytest.raises(ValueError):
        COCOMeanAP(0, device='cpu')
    with pytest.raises(ValueError):
        COCOMeanAP(1025, device='cpu')
    m = COCOMeanAP(80, device='cpu')
    dets, counts = torch.zeros(2, 100, 6), torch.zeros(2, dtype=torch.int32)
    g = [np.zeros((0, 7))] * 2
    with pytest.raises(ValueError, match=r'\[n, 7\]'):
        m.add(dets, counts, [1, 2], [np.zeros((3, 5)), np.zeros((0, 7))])
    with pytest.raises(ValueError, match='ground-truth arrays'):
        m.add(dets, counts, [1, 2], [np.zeros((0, 7))])
    with pytest.raises(ValueError, match='at most'):
        m.add(dets, counts, [1, 2], [np.zeros((2049, 7)), np.zeros((0, 7))])
    with pytest.raises(ValueError, match='out of range'):
        m.add(dets, counts, [1, 2], [np.array([[0, 0, 1, 1, 80, 0, 1]]), np.zeros((0, 7))])
    with pytest.raises(ValueError, match='float64'):
        m.add(dets, counts, [1, 2], torch.zeros(2, 3, 7, dtype=torch.float32))
    with pytest.raises(ValueError, match=r'\[B, max_det, 6\]'):
        m.add(torch.zeros(2, 100, 5), counts, [1, 2], g)
    with pytest.raises(ValueError, match='image ids'):
        m.add(dets, counts, [1], g)
    with pytest.raises(ValueError, match=r'2\^31'):
        m.add(dets, counts, [-1, 2], g)
    with pytest.raises(ValueError, match='twice'):
        m.add(dets, counts, [4, 4], g)
    m._seen.add(7)                                                      # as if image 7 had been added
    with pytest.raises(ValueError, match='twice'):
        m.add(dets, counts, [7, 8], g)
    assert m.num_records == 0                                           # nothing was appended


def test_summarize_lines_format():
    from efficientdet.pytorch_amd.evaluate import summarize_lines
    lines = summarize_lines([0.1234, 0.5, 0.25, -1, 0.0, 1.0, 0.3, 0.4, 0.45, -1.0, 0.2, 0.6])
    assert len(lines) == 12
    assert lines[0] == ' Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 0.123'
    assert lines[1] == ' Average Precision  (AP) @[ IoU=0.50      | area=   all | maxDets=100 ] = 0.500'
    assert lines[2] == ' Average Precision  (AP) @[ IoU=0.75      | area=   all | maxDets=100 ] = 0.250'
    assert lines[3] == ' Average Precision  (AP) @[ IoU=0.50:0.95 | area= small | maxDets=100 ] = -1.000'
    assert lines[4] == ' Average Precision  (AP) @[ IoU=0.50:0.95 | area=medium | maxDets=100 ] = 0.000'
    assert lines[6] == ' Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=  1 ] = 0.300'
    assert lines[7] == ' Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets= 10 ] = 0.400'
    assert lines[11] == ' Average Recall     (AR) @[ IoU=0.50:0.95 | area= large | maxDets=100 ] = 0.600'


# ------------------------------------------------------------------------------------------------ hand-derived cases
# v = 1 / (1 + 2^-52) = 0.9999999999999998: the precision of one TP and no FP (the eps is added to the denominator).
# Stats are means over T x R (AP) or T (AR) entries; numpy's pairwise sums may round the last bit of a mean of equal values.
HAND = {
    # one GT [0,0,10,10] (area 100: small), one detection on it: matched at every t; all / small: precision v at every r,
    # recall 1; medium / large have no non-ignored GT: -1
    'perfect': [V, V, V, V, -1, -1, 1, 1, 1, 1, -1, -1],
    # [0,0,10,10] vs GT [0,0,6,10]: i = 60, u = 100 + 60 - 60 -> IoU 0.6 exactly: matched at t = 0.5, 0.55, 0.6 (3 of 10);
    # unmatched t: tp 0 fp 1 -> precision 0, recall 0.  AP = 3 v / 10, AP50 v, AP75 0, AR = 0.3
    'iou_0.6': [0.3 * V, V, 0, 0.3 * V, -1, -1, 0.3, 0.3, 0.3, 0.3, -1, -1],
    # IoU 90 / 100 = 0.9 >= iouThrs[8] = 0.8999999999999999: matched at 9 of 10 thresholds
    'iou_0.9': [0.9 * V, V, V, 0.9 * V, -1, -1, 0.9, 0.9, 0.9, 0.9, -1, -1],
    # GT areas exactly 32^2 (small AND medium) and 96^2 (medium AND large), each hit by a detection (0.9 on the small one).
    # all / medium: two TPs -> pr [v, 2 / (2 + eps) = 1.0], envelope 1.0 everywhere -> 1.0.  small: the 96^2 GT is ignored, the
    # second detection matches it (ignored) -> pr [v, v] -> v.  large: the 32^2 GT is ignored and sorted last; detection 1 matches
    # it (ignored), detection 2 matches the large GT and then BREAKS at the ignored one -> pr [0, v], envelope v.  AR@1: only the
    # 0.9 detection per (image, category) -> 1 of 2 GTs = 0.5
    'area_edges': [1, 1, 1, V, 1, V, 0.5, 1, 1, 1, 1, 1],
    # a crowd GT [0,0,100,100] absorbs three detections inside it (IoU = i / detection area = 1, every t; a crowd GT stays
    # matchable), all ignored; the fourth detection hits the one normal GT.  Sequence [ig, ig, ig, tp] -> rc [0,0,0,1],
    # pr [0,0,0,v], envelope v -> AP v.  AR@1 keeps only the first (ignored) detection: recall 0
    'crowd': [V, V, V, V, -1, -1, 0, 1, 1, 1, -1, -1],
    # GT a (normal) and GT b (crowd) on the same box.  Detection 1 matches a, then BREAKS at b (ignored) although b's IoU ties
    # (a tie would otherwise go to the later GT): TP.  Detection 2 skips a (taken), matches crowd b: ignored.  pr [v, v] -> v
    'ignored_break': [V, V, V, V, -1, -1, 1, 1, 1, 1, -1, -1],
    # images added as 3 then 2, equal scores: COCOeval ranks image 2 (FP) before image 3 (TP).  rc [0, 0.5], pr [0, 0.5],
    # envelope 0.5 up to recThrs[50] = 0.5, then 0 -> AP = 51 * 0.5 / 101 = 0.2524752475247525 (in add order it would be v)
    'ties_desc_ids': [25.5 / 101, 25.5 / 101, 25.5 / 101, 25.5 / 101, -1, -1, 0.5, 0.5, 0.5, 0.5, -1, -1],
    # 150 GTs, 150 detections each on one of them, scores descending: only the first 100 enter.  tp 1..100 of npig 150:
    # precision 1.0 (v at the first point, lifted by the envelope) up to recall 2/3: recThrs 0..0.66 -> 67 of 101 -> AP 67 / 101;
    # AR@1 = 1/150, AR@10 = 10/150, AR@100 = 100/150
    'rank_cut_150': [67 / 101, 67 / 101, 67 / 101, 67 / 101, -1, -1, 1 / 150, 10 / 150, 100 / 150, 100 / 150, -1, -1],
    # category 1 perfect (v), category 2 has a GT and no detection: precision 0, recall 0 (it counts) -> AP v / 2, AR 0.5
    'cat_without_dets': [V / 2, V / 2, V / 2, V / 2, -1, -1, 0.5, 0.5, 0.5, 0.5, -1, -1],
    # image 5 has a detection (0.95) and no GT: FP before image 1's TP (0.9): rc [0, 1], pr [0, 1 / (2 + eps) = 0.5] -> AP 0.5
    'img_without_gt': [0.5, 0.5, 0.5, 0.5, -1, -1, 1, 1, 1, 1, -1, -1],
}


@pytest.mark.parametrize('name', sorted(HAND))
def test_restatement_on_hand_derived_cases(name):
    gt, dt, ids, K = CASES.hand_cases()[name]
    stats, precision, recall = R.coco_eval(gt, dt, ids)
    assert precision.shape == (10, 101, K, 4, 3) and recall.shape == (10, K, 4, 3)
    np.testing.assert_allclose(stats, HAND[name], rtol=0, atol=1e-15)


def test_restatement_pins_exact_array_entries():
    """Entries the derivations above name, bit for bit."""
    c = CASES.hand_cases()
    _, p, r = R.coco_eval(*c['perfect'][:3])
    assert np.all(p[:, :, 0, :2, :] == V) and V == 0.9999999999999998 and np.all(p[:, :, 0, 2:, :] == -1)
    assert np.all(r[:, 0, :2, :] == 1.0) and np.all(r[:, 0, 2:, :] == -1)
    _, p, r = R.coco_eval(*c['iou_0.6'][:3])
    assert r[:, 0, 0, 2].tolist() == [1, 1, 1] + [0] * 7
    _, p, r = R.coco_eval(*c['iou_0.9'][:3])
    assert r[:, 0, 0, 2].tolist() == [1] * 9 + [0]
    _, p, r = R.coco_eval(*c['ties_desc_ids'][:3])
    assert np.all(p[:, :51, 0, 0, 2] == 0.5) and np.all(p[:, 51:, 0, 0, 2] == 0)
    _, p, r = R.coco_eval(*c['rank_cut_150'][:3])
    assert np.all(r[:, 0, 0, :] == [1 / 150, 10 / 150, 100 / 150])
    assert np.all(p[:, :67, 0, 0, 2] == 1.0) and np.all(p[:, 67:, 0, 0, 2] == 0)
    _, p, r = R.coco_eval(*c['cat_without_dets'][:3])
    assert np.all(p[:, :, 1, :2, :] == 0) and np.all(r[:, 1, :2, :] == 0)


# ------------------------------------------------------------------------------------------------ against pycocotools, where present
def _pycocotools(gt, dt, ids):
    pytest.importorskip('pycocotools')
    from pycocotools.coco import COCO
    from pycocotools.cocoeval import COCOeval
    import contextlib
    import io
    g = COCO()
    g.dataset = {'images': [{'id': i} for i in sorted(set(ids))], 'annotations': [dict(a) for a in gt['annotations']],
                 'categories': gt['categories']}
    with contextlib.redirect_stdout(io.StringIO()):
        g.createIndex()
        d = g.loadRes([dict(x) for x in dt]) if dt else COCO()
        e = COCOeval(g, d, 'bbox')
        e.params.imgIds = ids
        e.evaluate()
        e.accumulate()
        e.summarize()
    return e.stats, e.eval['precision'], e.eval['recall']


@pytest.mark.parametrize('name', sorted(HAND))
def test_restatement_equals_pycocotools_on_hand_cases(name):
    gt, dt, ids, _ = CASES.hand_cases()[name]
    want = _pycocotools(gt, dt, ids)
    got = R.coco_eval(gt, dt, ids)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    np.testing.assert_allclose(got[0], want[0], rtol=0, atol=1e-12)


def test_restatement_equals_pycocotools_on_a_random_set():
    gt, dt, ids, _ = CASES.random_case(n_img=40, K=12, max_rows=120, seed=3)
    want = _pycocotools(gt, dt, ids)
    got = R.coco_eval(gt, dt, ids)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    np.testing.assert_allclose(got[0], want[0], rtol=0, atol=1e-12)
