"""GPU tier of the device COCO metric (csrc/coco_map.hip; evaluate.COCOMeanAP / evaluate_coco) against the NumPy restatement of
COCOeval (tests/coco_eval_restated.py): precision / recall bit for bit, the 12 stats within 1e-12."""
import numpy as np
import pytest
import torch

from oracle import effdet_oracle as O
from tests import coco_eval_restated as R
from tests import coco_map_cases as CASES

pytestmark = pytest.mark.gpu


def _pack(rows_list):
    """per-image [n, 6] rows -> (dets [B, M, 6] fp32 on the device, rows past the count: label -1; counts [B] int32)."""
    B = len(rows_list)
    M = max([1] + [len(r) for r in rows_list])
    dets = np.zeros((B, M, 6), dtype=np.float32)
    dets[:, :, 5] = -1
    counts = np.zeros(B, dtype=np.int32)
    for i, r in enumerate(rows_list):
        dets[i, :len(r)] = r
        counts[i] = len(r)
    return torch.from_numpy(dets).cuda(), torch.from_numpy(counts).cuda()


def _device(case, batch=None, order=None):
    from efficientdet.pytorch_amd.evaluate import COCOMeanAP
    gt, dt, ids, K = case
    dets, gts = CASES.per_image_rows(gt, dt, ids)
    idx = list(range(len(ids))) if order is None else list(order)
    batch = batch or len(idx)
    meter = COCOMeanAP(K)
    for s in range(0, len(idx), batch):
        sel = idx[s:s + batch]
        d, c = _pack([dets[i] for i in sel])
        meter.add(d, c, [ids[i] for i in sel], [gts[i] for i in sel])
    return meter


def _assert_equal(got, want):
    stats, arrays = got
    ws, wp, wr = want
    assert arrays['precision'].shape == wp.shape and arrays['recall'].shape == wr.shape
    assert np.array_equal(arrays['precision'], wp), np.argwhere(arrays['precision'] != wp)[:10]       # bit for bit
    assert np.array_equal(arrays['recall'], wr), np.argwhere(arrays['recall'] != wr)[:10]
    assert stats.dtype == np.float64 and stats.shape == (12,)
    np.testing.assert_allclose(stats, ws, rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------------ 1. hand-derived cases
@pytest.mark.parametrize('name', sorted(CASES.hand_cases()))
def test_hand_cases_vs_restatement(name):
    case = CASES.hand_cases()[name]
    got = _device(case).compute(full=True)
    _assert_equal(got, R.coco_eval(*case[:3]))


# ------------------------------------------------------------------------------------------------ 2. COCO-scale seeded sets
@pytest.mark.parametrize('seed', [1, 2])
def test_random_sets_vs_restatement(seed):
    case = CASES.random_case(n_img=300, K=80, max_rows=400, seed=seed)
    got = _device(case, batch=32).compute(full=True)
    want = R.coco_eval(*case[:3])
    _assert_equal(got, want)
    assert (want[1] > 0).sum() > 1000 and want[0][0] > 0.01                # a non-trivial set


# ------------------------------------------------------------------------------------------------ 3. invariance, determinism
def test_batching_order_invariance_and_determinism():
    case = CASES.random_case(n_img=120, K=80, max_rows=250, seed=7)
    ref_stats, ref_arr = _device(case, batch=32).compute(full=True)
    rng = np.random.RandomState(0)
    for batch, order in ((1, None), (7, None), (32, rng.permutation(120)), (32, None)):
        stats, arr = _device(case, batch=batch, order=order).compute(full=True)
        assert np.array_equal(stats, ref_stats), (batch, stats - ref_stats)
        assert np.array_equal(arr['precision'], ref_arr['precision']) and np.array_equal(arr['recall'], ref_arr['recall'])
    m = _device(case, batch=32)
    assert np.array_equal(m.compute(), m.compute())
    m.reset()
    assert m.num_records == 0 and np.all(m.compute() == -1)


# ------------------------------------------------------------------------------------------------ 4. evaluate_coco end to end
class _Recorder:
    def __init__(self, m):
        self.m, self.out, self.trained = m, [], False
        self.threshold, self.iou_threshold = m.threshold, m.iou_threshold

    def eval(self): self.m.eval()
    def train(self): self.trained = True
    def parameters(self): return self.m.parameters()

    def forward_raw(self, x):
        r = self.m.forward_raw(x)
        self.out.append((r, int(x.shape[2]), int(x.shape[3])))
        return r


class _Coco:
    """The pycocotools COCO methods evaluate_coco calls, over a dict."""
    def __init__(self, d):
        self.d = d

    def getCatIds(self): return [c['id'] for c in self.d['categories']]
    def getAnnIds(self, imgIds): return [a['id'] for a in self.d['annotations'] if a['image_id'] in imgIds]
    def loadAnns(self, ids): return [dict(a) for a in self.d['annotations'] if a['id'] in set(ids)]


class _Dataset:
    def __init__(self, imgs, scales, image_ids, coco, label_map):
        self.imgs, self.scales, self.image_ids, self.coco, self.label_map = imgs, scales, image_ids, coco, label_map
    def __len__(self): return len(self.imgs)
    def __getitem__(self, i): return {'img': self.imgs[i], 'scale': self.scales[i]}
    def label_to_coco_label(self, l): return self.label_map[l]


@pytest.mark.parametrize('batch_size', [1, 3])
def test_evaluate_coco_end_to_end_vs_host_path(batch_size, capsys):
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
    image_ids = [42, 7, 1000, 3, 99, 12]                                   # not sorted: COCOeval evaluates them in np.unique order
    label_map = {l: 10 + 3 * l for l in range(nc)}                        # coco category ids; the GT also uses id 95 (no label)
    rng = np.random.RandomState(5)
    anns, aid = [], 1
    for i in range(6):                             # GT partly placed on the model's own detections (random init: no TP otherwise)
        k = [4, 0, 7, 2, 5, 3][i]
        s_, l_, b_ = m.detect(imgs[i].permute(2, 0, 1)[None].cuda())[0]
        b_ = b_.cpu().numpy().astype(np.float64) / scales[i]; l_ = l_.cpu().numpy()
        pick = rng.choice(len(b_), k, replace=False) if k else np.zeros(0, dtype=np.int64)
        for j in pick:
            x1, y1, x2, y2 = b_[j] + rng.normal(0, 1.0, 4)
            lab = int(l_[j]) if rng.rand() < 0.8 else int(rng.randint(0, nc))
            cat = label_map[lab] if rng.rand() < 0.9 else 95
            w, h = max(x2 - x1, 0.5), max(y2 - y1, 0.5)
            anns.append({'id': aid, 'image_id': image_ids[i], 'category_id': cat, 'bbox': [x1, y1, w, h],
                         'iscrowd': int(rng.rand() < 0.15), 'area': w * h * rng.uniform(0.6, 1.0)})
            aid += 1
    gt = {'annotations': anns, 'categories': [{'id': label_map[l]} for l in range(nc)] + [{'id': 95}]}
    rec = _Recorder(m)
    got = EV.evaluate_coco(_Dataset(imgs, scales, image_ids, _Coco(gt), label_map), rec, batch_size=batch_size)
    printed = capsys.readouterr().out.splitlines()
    assert len(rec.out) == (6 if batch_size == 1 else 2) and rec.trained
    results, first = [], 0
    for (cls, reg, anc), H, W in rec.out:                                      # the existing host path on the same outputs
        s, l, b, cnt = EV.postprocess(m, cls, reg, anc, H, W)
        B = int(cls.shape[0])
        dets, counts = EV.finalize(s, l, b, cnt, scales[first:first + B], score_threshold=0.05, xywh=True)
        results += EV.coco_results(dets, counts, image_ids[first:first + B], label_to_coco_label=lambda v: label_map[v])
        first += B
    assert len(results) > 200
    want = R.coco_eval(gt, results, image_ids)
    np.testing.assert_allclose(got, want[0], rtol=0, atol=1e-12)
    assert printed[-12:] == EV.summarize_lines(want[0])
    assert got[1] > 0                                                          # some TPs at all


def test_evaluate_coco_without_detections_returns_none(capsys):
    from efficientdet.pytorch_amd import evaluate as EV

    class Empty(_Recorder):
        def forward_raw(self, x):
            cls, reg, anc = self.m.forward_raw(x)
            return torch.zeros_like(cls), reg, anc                             # every score 0: nothing passes the threshold
    from efficientdet.pytorch_amd import EfficientDet, EFFICIENTDET
    c = EFFICIENTDET['efficientdet-d0']
    m = EfficientDet(4, network='efficientdet-d0', W_bifpn=c['W_bifpn'], D_bifpn=c['D_bifpn'], D_class=c['D_class'],
                     compute_dtype=torch.float32, is_training=False, threshold=0.05)
    m.load_state_dict(O.make_state_dict('efficientdet-d0', 4, seed=0))
    m = m.cuda()
    img, _ = O.synthetic_batch(2, 128, seed=4, num_classes=4)
    gt = {'annotations': [{'id': 1, 'image_id': 5, 'category_id': 1, 'bbox': [0, 0, 9, 9], 'iscrowd': 0, 'area': 81.0}],
          'categories': [{'id': c} for c in range(4)]}
    ds = _Dataset([img[i].permute(1, 2, 0).contiguous() for i in range(2)], [1.0, 1.0], [5, 6], _Coco(gt), {l: l for l in range(4)})
    assert EV.evaluate_coco(ds, Empty(m)) is None
    assert 'Average Precision' not in capsys.readouterr().out


# ------------------------------------------------------------------------------------------------ 5. no host sync in add
def test_add_performs_no_device_to_host_transfer(monkeypatch):
    from efficientdet.pytorch_amd import evaluate as EV
    gt, dt, ids, K = CASES.random_case(n_img=24, K=80, max_rows=200, seed=11)
    dets, gts = CASES.per_image_rows(gt, dt, ids)
    d, c = _pack(dets)
    G = max(len(a) for a in gts)
    h = np.zeros((24, G, 7)); h[:, :, 4] = -1
    for i, a in enumerate(gts):
        h[i, :len(a)] = a
    dev_gt = torch.from_numpy(h).cuda()
    monkeypatch.setattr(EV.COCOMeanAP, 'INITIAL_CAPACITY', 256)                 # so that add also grows the buffer
    meter = EV.COCOMeanAP(K)
    torch.cuda.synchronize()

    def boom(*a, **k):
        raise AssertionError('device->host transfer inside COCOMeanAP.add')
    with monkeypatch.context() as mp:
        for name in ('item', 'cpu', 'tolist', 'numpy'):
            mp.setattr(torch.Tensor, name, boom)
        mp.setattr(torch.cuda, 'synchronize', boom)
        meter.add(d[:12], c[:12], ids[:12], gts[:12])
        meter.add(d[12:], c[12:], ids[12:], dev_gt[12:])
    assert meter.capacity > 256 and meter.num_records == 24 * d.shape[1]
    _assert_equal(meter.compute(full=True), R.coco_eval(gt, dt, ids))
