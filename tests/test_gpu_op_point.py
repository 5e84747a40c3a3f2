"""GPU tier of the operating-point metrics (csrc/op_point.hip; ops.op_curves / ops.confusion_match, evaluate.OperatingPoint /
evaluate_operating_point) against the NumPy restatement tests/op_point_restated.py on the cases of tests/op_point_cases.py.  Every
compared value is an integer or an fp64 produced by single uncontracted operations in a fixed order: every comparison is exact."""
import numpy as np
import pytest
import torch

from oracle import effdet_oracle as O
from tests import op_point_restated as R
from tests.op_point_cases import CONFUSION_CASES, CURVES_CASES, device_gt

pytestmark = pytest.mark.gpu

CURVES = {c['name']: c for c in CURVES_CASES}
CONFUSION = {c['name']: c for c in CONFUSION_CASES}
TABLES = ('tp', 'npred', 'precision', 'recall', 'f1', 'mean', 'best')
_RESTATED = {}


def _restated(case):
    """(key, tp byte, gt_count, curves) of a curves case, computed once and shared"""
    if case['name'] not in _RESTATED:
        if case['dets'] is None:
            rec = np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint8), np.zeros(case['C'], dtype=np.int32)
        else:
            rec = R.voc_records(case['dets'], case['counts'], case['gts'], case['C'], case['iou'])
        _RESTATED[case['name']] = rec + (R.curves(*rec, case['C'], R.check_thresholds(case['thresholds'])),)
    return _RESTATED[case['name']]


def _upload(case):
    boxes, labels = device_gt(case['gts'], case['C'])
    return (torch.from_numpy(case['dets']).cuda(), torch.from_numpy(case['counts']).cuda(), torch.from_numpy(boxes).cuda(),
            torch.from_numpy(labels).cuda())


def _device_records(case):
    from efficientdet.pytorch_amd import ops
    C = case['C']
    gt_count = torch.zeros(C, dtype=torch.int32, device='cuda')
    if case['dets'] is None:
        return torch.zeros(1, dtype=torch.int64, device='cuda'), torch.zeros(1, dtype=torch.uint8, device='cuda'), 0, gt_count
    dets, counts, boxes, labels = _upload(case)
    N = dets.shape[0] * dets.shape[1]
    key = torch.full((N,), -1, dtype=torch.int64, device='cuda'); tp = torch.full((N,), 255, dtype=torch.uint8, device='cuda')
    ops.voc_match(dets, counts, boxes, labels, C, case['iou'], key, tp, gt_count)
    return key, tp, N, gt_count


def _filled(C, M):
    """op_curves' outputs, every byte 0xFF"""
    return {'tp': torch.full((C, M), -1, dtype=torch.int32, device='cuda'), 'npred': torch.full((C, M), -1, dtype=torch.int32, device='cuda'),
            **{k: torch.full(s, -1, dtype=torch.int64, device='cuda').view(torch.float64)
               for k, s in (('precision', (C, M)), ('recall', (C, M)), ('f1', (C, M)), ('mean', (3, M)), ('best', (C + 1, 4)))}}


def _intact(out):
    return all(bool((t.view(torch.uint8) == 255).all()) for t in out.values())


# ------------------------------------------------------------------------------------------------ ops.op_curves
@pytest.mark.parametrize('name', [c['name'] for c in CURVES_CASES])
def test_curves_equal_the_restatement(name):
    from efficientdet.pytorch_amd import ops
    case = CURVES[name]
    C = case['C']
    wkey, wtp, wcount, want = _restated(case)
    key, tp, N, gt_count = _device_records(case)
    assert N == len(wkey) and np.array_equal(gt_count.cpu().numpy(), wcount)
    assert np.array_equal(key[:N].cpu().numpy().view(np.uint64), wkey) and np.array_equal(tp[:N].cpu().numpy(), wtp)
    M = len(R.check_thresholds(case['thresholds']))
    runs = []
    for _ in range(2):
        out = _filled(C, M)
        assert _intact(out)
        got = ops.op_curves(key, tp, N, gt_count, C, case['thresholds'], out=out)
        runs.append({k: got[k].cpu().numpy() for k in TABLES})
        assert np.array_equal(got['thresholds'].cpu().numpy(), R.check_thresholds(case['thresholds']))
    for k in TABLES:
        assert runs[0][k].dtype == want[k].dtype and np.array_equal(runs[0][k], want[k]), (name, k)
        assert runs[0][k].tobytes() == runs[1][k].tobytes(), (name, k)                         # two runs are bit-equal
    if case['expect'] is not None:
        for k in TABLES:
            assert np.array_equal(runs[0][k], np.asarray(case['expect'][k], dtype=want[k].dtype)), (name, k)
    fresh = ops.op_curves(key, tp, N, gt_count, C, case['thresholds'])                         # and with outputs of its own
    assert all(np.array_equal(fresh[k].cpu().numpy(), want[k]) for k in TABLES)


# ------------------------------------------------------------------------------------------------ ops.confusion_match
@pytest.mark.parametrize('name', [c['name'] for c in CONFUSION_CASES])
def test_confusion_equals_the_restatement(name):
    from efficientdet.pytorch_amd import ops
    case = CONFUSION[name]
    C = case['C']
    want = R.confusion(case['dets'], case['counts'], case['gts'], C, case['conf'], case['iou'])
    if case['expect'] is not None:
        assert np.array_equal(want, np.asarray(case['expect'], dtype=np.int64))
    dets, counts, boxes, labels = _upload(case)
    runs = []
    for _ in range(2):
        m = torch.zeros((C + 1, C + 1), dtype=torch.int64, device='cuda')
        ops.confusion_match(dets, counts, boxes, labels, C, case['conf'], case['iou'], m)
        runs.append(m.cpu().numpy())
    assert np.array_equal(runs[0], want), (name, runs[0], want)
    assert runs[0].tobytes() == runs[1].tobytes()
    # the call ADDS: a second call into a used matrix, and image by image, give the sums
    ops.confusion_match(dets, counts, boxes, labels, C, case['conf'], case['iou'], m)
    assert np.array_equal(m.cpu().numpy(), 2 * want)
    seed = torch.arange((C + 1) * (C + 1), dtype=torch.int64, device='cuda').reshape(C + 1, C + 1) << 33
    m = seed.clone()
    for b in range(dets.shape[0]):
        ops.confusion_match(dets[b:b + 1], counts[b:b + 1], boxes[b:b + 1], labels[b:b + 1], C, case['conf'], case['iou'], m)
    assert np.array_equal((m - seed).cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_outputs_alone():
    from efficientdet.pytorch_amd import _lib, ops
    L = _lib.require('effdet_op_curves', 'effdet_op_curves_workspace_bytes', 'effdet_confusion_match')
    case = CURVES['hand']
    C = case['C']
    key, tp, N, gt_count = _device_records(case)
    ws = torch.empty(int(L.effdet_op_curves_workspace_bytes(N)), dtype=torch.uint8, device='cuda')
    th = torch.linspace(0, 1, 4097, device='cuda')
    out = _filled(C, 4097)
    p = _lib.ptr

    def call(M=4, gt=gt_count, tp_out=out['tp']):
        return L.effdet_op_curves(p(key), p(tp), N, p(gt), C, p(th), M, p(ws), ws.numel(), p(tp_out), p(out['npred']), p(out['precision']),
                                  p(out['recall']), p(out['f1']), p(out['mean']), p(out['best']), _lib.stream_ptr())
    assert call(M=4097) == -3 and call(M=0) == -3 and call(gt=None) == -1 and call(tp_out=None) == -1
    torch.cuda.synchronize()
    assert _intact(out)
    assert call() == 0                                                  # (the same arguments with M in range are served)
    torch.cuda.synchronize()
    assert not _intact(out)
    with pytest.raises(ValueError):
        ops.op_curves(key, tp, N, gt_count, C, np.linspace(0, 1, 4097))
    dets, counts, boxes, labels = _upload(CONFUSION['hand'])
    big_b = torch.zeros((1, 2049, 4), dtype=torch.float64, device='cuda'); big_l = torch.full((1, 2049), -1, dtype=torch.int32, device='cuda')
    m = torch.full((3, 3), -1, dtype=torch.int64, device='cuda')
    f = L.effdet_confusion_match
    assert f(p(dets), p(counts), p(big_b), p(big_l), 1, 2, 2049, 2, 0.25, 0.45, p(m), _lib.stream_ptr()) == -3
    assert f(p(dets), None, p(boxes), p(labels), 1, 2, 2, 2, 0.25, 0.45, p(m), _lib.stream_ptr()) == -1
    assert f(p(dets), p(counts), p(boxes), p(labels), 1, 2, 2, 2, 0.25, 0.45, None, _lib.stream_ptr()) == -1
    torch.cuda.synchronize()
    assert bool((m == -1).all())
    with pytest.raises(RuntimeError, match='EFFDET_EUNSUPPORTED'):
        ops.confusion_match(dets, counts, big_b, big_l, 2, 0.25, 0.45, m)
    assert bool((m == -1).all())


# ------------------------------------------------------------------------------------------------ the meter
def _check_result(got, want_curves, want_confusion, th, gt_count, C):
    for k in ('tp', 'npred', 'precision', 'recall', 'f1', 'mean'):
        assert got[k].dtype == want_curves[k].dtype and np.array_equal(got[k], want_curves[k]), k
    best = want_curves['best']
    assert np.array_equal(got['thresholds'], th) and got['thresholds'].dtype == np.float32
    assert got['num_annotations'].dtype == np.int64 and np.array_equal(got['num_annotations'], gt_count)
    assert sorted(got['per_class']) == [c for c in range(C) if gt_count[c] > 0]
    for c, row in got['per_class'].items():
        assert row == (float(th[int(best[c, 0])]), best[c, 1], best[c, 2], best[c, 3]), c
    j = int(best[C, 0])
    assert got['overall'] == ((float(th[j]), best[C, 1], best[C, 2], best[C, 3]) if j >= 0 else (None, 0.0, 0.0, 0.0))
    assert got['confusion'].dtype == np.int64 and np.array_equal(got['confusion'], want_confusion)
    assert sorted(got) == sorted(['thresholds', 'tp', 'npred', 'precision', 'recall', 'f1', 'mean', 'num_annotations', 'per_class', 'overall',
                                  'ap', 'mean_ap', 'confusion'])


def test_the_meter_over_two_batches_equals_the_restatement_over_the_union(monkeypatch):
    from efficientdet.pytorch_amd.evaluate import OperatingPoint, VOCMeanAP
    case = CURVES['chunks']
    C, th = case['C'], R.check_thresholds(case['thresholds'])
    _, _, wcount, want = _restated(case)
    monkeypatch.setattr(OperatingPoint, 'INITIAL_CAPACITY', 512)                # so that add also grows the buffers
    meter, voc = OperatingPoint(C, thresholds=case['thresholds']), VOCMeanAP(C)
    dets, counts = torch.from_numpy(case['dets']).cuda(), torch.from_numpy(case['counts']).cuda()
    for sl in (slice(0, 2), slice(2, 6)):
        meter.add(dets[sl], counts[sl], case['gts'][sl])
        voc.add(dets[sl], counts[sl], case['gts'][sl])
    got = meter.compute()
    assert meter.num_records == case['dets'].shape[0] * case['dets'].shape[1] > 512
    _check_result(got, want, R.confusion(case['dets'], case['counts'], case['gts'], C, 0.25, 0.45), th, wcount, C)
    mean, aps = voc.compute()
    assert got['ap'].dtype == np.float64 and [got['ap'][c] for c in range(C)] == [aps[c][0] for c in range(C)]
    assert type(got['mean_ap']) is np.float64 and got['mean_ap'] == mean and sum(got['ap'] > 0) >= 4
    again = meter.compute()                                                     # compute() does not consume the records
    assert all(np.array_equal(again[k], got[k]) for k in ('tp', 'npred', 'f1', 'mean', 'confusion', 'ap'))
    meter.reset()
    assert meter.num_records == 0 and not meter.compute()['confusion'].any()


def test_an_unused_meter_gives_the_empty_case():
    from efficientdet.pytorch_amd.evaluate import OperatingPoint
    case = CURVES['empty']
    C = case['C']
    got = OperatingPoint(C).compute()
    want = {k: np.asarray(v, dtype=np.int32 if k in ('tp', 'npred') else np.float64) for k, v in case['expect'].items()}
    _check_result(got, want, np.zeros((C + 1, C + 1), dtype=np.int64), R.check_thresholds(None), np.zeros(C, dtype=np.int64), C)
    assert got['per_class'] == {} and got['overall'] == (None, 0.0, 0.0, 0.0) and got['mean_ap'] == 0 and not got['ap'].any()


# ------------------------------------------------------------------------------------------------ evaluate_operating_point
class _Recorder:
    """The model as evaluate_operating_point sees it; keeps each forward's (cls, reg, anchors)."""
    def __init__(self, m):
        self.m, self.out = m, []
        self.threshold, self.iou_threshold = m.threshold, m.iou_threshold

    def eval(self): self.m.eval()
    def parameters(self): return self.m.parameters()

    def forward_raw(self, x):
        r = self.m.forward_raw(x)
        self.out.append((r, int(x.shape[2]), int(x.shape[3])))
        return r


class _Generator:
    def __init__(self, imgs, scales, anns, nc):
        self.imgs, self.scales, self.anns, self.nc = imgs, scales, anns, nc
    def __len__(self): return len(self.imgs)
    def __getitem__(self, i): return {'img': self.imgs[i], 'scale': self.scales[i]}
    def load_annotations(self, i): return self.anns[i].copy()
    def num_classes(self): return self.nc
    def label_to_name(self, l): return 'c%d' % l


def test_evaluate_operating_point_end_to_end(capsys):
    from efficientdet.pytorch_amd import EfficientDet, EFFICIENTDET
    from efficientdet.pytorch_amd import evaluate as EV
    net, nc = 'efficientdet-d0', 8
    c = EFFICIENTDET[net]
    m = EfficientDet(nc, network=net, W_bifpn=c['W_bifpn'], D_bifpn=c['D_bifpn'], D_class=c['D_class'], compute_dtype=torch.float32,
                     is_training=False, threshold=0.05)
    m.load_state_dict(O.make_state_dict(net, nc, seed=0))
    m = m.cuda()
    img, _ = O.synthetic_batch(6, 128, seed=4, num_classes=nc)
    imgs = [img[i].permute(1, 2, 0).contiguous() for i in range(6)]
    scales = [0.5, 1.25, 0.8, 1.0, 2.0, 0.37]
    rng = np.random.RandomState(5)
    anns = []
    for i in range(6):                             # GT partly placed on the model's own detections (random init: no TP otherwise)
        k = [4, 0, 7, 2, 5, 3][i]
        s_, l_, b_ = m.detect(imgs[i].permute(2, 0, 1)[None].cuda())[0]
        b_ = b_.cpu().numpy().astype(np.float64) / scales[i]; l_ = l_.cpu().numpy()
        pick = rng.choice(len(b_), k, replace=False) if k else np.zeros(0, dtype=np.int64)
        bx = b_[pick] + rng.normal(0, 1.0, (k, 4))
        lab = np.where(rng.rand(k) < 0.8, l_[pick], rng.randint(0, nc, k)).astype(np.float64)
        anns.append(np.concatenate([bx, lab[:, None]], 1) if k else np.zeros((0, 5)))
    rec = _Recorder(m)
    before = m.threshold
    conf = 0.06                                    # (a random-init model scores low: the default 0.25 would leave no prediction)
    got = EV.evaluate_operating_point(_Generator(imgs, scales, anns, nc), rec, batch_size=3, conf_threshold=conf)
    printed = capsys.readouterr().out.splitlines()
    assert m.threshold == before and rec.threshold == before and len(rec.out) == 2
    dets, counts = [], []
    first = 0
    for (cls, reg, anc), H, W in rec.out:                                      # finalize_device's own rows of the same outputs
        s, l, b, cnt = EV.postprocess(m, cls, reg, anc, H, W)
        B = int(cls.shape[0])
        d, n = EV.finalize_device(s, l, b, cnt, scales[first:first + B], score_threshold=0.05, max_detections=100)
        dets.append(d.cpu().numpy()); counts.append(n.cpu().numpy())
        first += B
    dets, counts = np.concatenate(dets), np.concatenate(counts)
    assert counts.sum() > 200
    th = R.check_thresholds(None)
    key, tp, gt_count = R.voc_records(dets, counts, anns, nc, 0.5)
    want = R.curves(key, tp, gt_count, nc, th)
    wconf = R.confusion(dets, counts, anns, nc, conf, 0.45)
    _check_result(got, want, wconf, th, gt_count, nc)
    assert tp.sum() > 0 and np.trace(wconf[:nc, :nc]) > 0 and wconf[:nc, nc].sum() > 0
    voc = EV.VOCMeanAP(nc)
    voc.add(torch.from_numpy(dets).cuda(), torch.from_numpy(counts).cuda(), anns)
    mean, aps = voc.compute()
    assert got['mean_ap'] == mean and [got['ap'][k] for k in range(nc)] == [aps[k][0] for k in range(nc)]
    j = int(want['best'][nc, 0])
    assert j >= 0 and got['overall'][0] == float(th[j])
    lines = ['c{}: annotations {} P {:.4f} R {:.4f} F1 {:.4f} best threshold {} AP {}'.format(
        k, int(gt_count[k]), want['precision'][k, j], want['recall'][k, j], want['f1'][k, j],
        float(th[int(want['best'][k, 0])]) if gt_count[k] > 0 else None, np.float64(aps[k][0])) for k in range(nc)]
    lines.append('overall: threshold {} P {:.4f} R {:.4f} F1 {:.4f} mAP {}'.format(float(th[j]), want['best'][nc, 1], want['best'][nc, 2],
                                                                                 want['best'][nc, 3], mean))
    at = printed.index('operating point:')
    assert printed[at + 1:] == lines
