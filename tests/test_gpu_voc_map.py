"""GPU tier of the device VOC metric (csrc/voc_map.hip; evaluate.finalize_device / VOCMeanAP / evaluate_voc) against the reference's
evaluate (eval.py:165-257): the reference-source fixture tests/golden/voc_map.npz, and a test-local NumPy restatement of evaluate
whose score sort is STABLE (the documented tie rule; the reference's np.argsort is unstable for ties)."""
import os

import numpy as np
import pytest
import torch

from oracle import effdet_oracle as O

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ restatement of eval.py:165-257
def _overlap(a, b):
    """compute_overlap (eval.py:19-43), same fp64 operation order: a [N, 4], b [K, 4] -> [N, K]."""
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    iw = np.minimum(a[:, 2:3], b[:, 2]) - np.maximum(a[:, 0:1], b[:, 0])
    ih = np.minimum(a[:, 3:4], b[:, 3]) - np.maximum(a[:, 1:2], b[:, 1])
    iw = np.maximum(iw, 0)
    ih = np.maximum(ih, 0)
    ua = ((a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]))[:, None] + area - iw * ih
    ua = np.maximum(ua, np.finfo(float).eps)
    return iw * ih / ua


def _compute_ap(recall, precision):
    mrec = np.concatenate(([0.], recall, [1.]))
    mpre = np.concatenate(([0.], precision, [0.]))
    mpre = np.maximum.accumulate(mpre[::-1])[::-1]              # the envelope loop of eval.py:64-65 (max is exact)
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])


def restated_evaluate(rows, gts, num_classes, iou_threshold=0.5):
    """rows[i]: image i's detections [n, 6] (x1, y1, x2, y2, score, label; finalize's valid prefix, score order), gts[i]: [g, 5]
    -> (mean, {label: (ap, num_annotations)}, {label: (recall, precision)}) with a stable score sort."""
    C = num_classes
    scores, tps = [[] for _ in range(C)], [[] for _ in range(C)]
    nann = np.zeros(C)
    for d, g in zip(rows, gts):
        d = np.asarray(d, dtype=np.float64).reshape(-1, 6)
        g = np.asarray(g, dtype=np.float64).reshape(-1, 5)
        for c in range(C):
            nann[c] += int((g[:, 4] == c).sum())
        for c in np.unique(d[:, 5]).astype(np.int64):
            if not 0 <= c < C:
                continue
            dc = d[d[:, 5] == c]
            gc = g[g[:, 4] == c, :4]
            scores[c].append(dc[:, 4])
            tp = np.zeros(len(dc))
            if len(gc):
                ov = _overlap(dc[:, :4], gc)
                asg = np.argmax(ov, axis=1)
                ok = ov[np.arange(len(dc)), asg] >= iou_threshold
                taken = set()
                for k in range(len(dc)):
                    if ok[k] and asg[k] not in taken:
                        tp[k] = 1
                        taken.add(asg[k])
            tps[c].append(tp)
    aps, curves = {}, {}
    for c in range(C):
        if nann[c] == 0:
            aps[c] = 0, 0
            continue
        s = np.concatenate(scores[c]) if scores[c] else np.zeros(0)
        t = np.concatenate(tps[c]) if tps[c] else np.zeros(0)
        order = np.argsort(-s, kind='stable')
        tp = np.cumsum(t[order]); fp = np.cumsum(1 - t[order])
        recall = tp / float(nann[c])
        precision = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
        aps[c] = _compute_ap(recall, precision), float(nann[c])
        curves[c] = recall, precision
    return np.mean([aps[c][0] for c in range(C)]), aps, curves


def _assert_same_structure(got, want, C, tol):
    gm, ga = got
    wm, wa = want
    assert type(gm) is type(wm) is np.float64
    assert sorted(ga) == sorted(wa) == list(range(C))
    for c in range(C):
        assert type(ga[c][0]) is type(wa[c][0]) and type(ga[c][1]) is type(wa[c][1]), (c, ga[c], wa[c])
        assert ga[c][1] == wa[c][1], c
        assert abs(ga[c][0] - wa[c][0]) <= tol, (c, ga[c][0], wa[c][0])
    assert abs(gm - wm) <= tol


# ------------------------------------------------------------------------------------------------ fixture helpers
def _golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'voc_map.npz'), allow_pickle=False)


def _raw_batch(g, idx):
    """Replayed NMS output of images idx, padded: (scores, labels, boxes, count) on the device."""
    A = max([len(g[f'in{i}_scores']) for i in idx] + [1])
    B = len(idx)
    s = torch.zeros(B, A); l = torch.zeros(B, A, dtype=torch.int64); b = torch.zeros(B, A, 4); cnt = torch.zeros(B, dtype=torch.int32)
    for j, i in enumerate(idx):
        k = len(g[f'in{i}_scores']); cnt[j] = k
        if k:
            s[j, :k] = torch.from_numpy(g[f'in{i}_scores']); l[j, :k] = torch.from_numpy(g[f'in{i}_labels'])
            b[j, :k] = torch.from_numpy(g[f'in{i}_boxes'])
    return s.cuda(), l.cuda(), b.cuda(), cnt.cuda()


def _feed(g, meter, batches):
    from efficientdet.pytorch_amd import evaluate as EV
    thr, mx = float(g['score_threshold']), int(g['max_detections'])
    for idx in batches:
        s, l, b, cnt = _raw_batch(g, idx)
        dets, counts = EV.finalize_device(s, l, b, cnt, [float(g['scales'][i]) for i in idx], score_threshold=thr, max_detections=mx)
        meter.add(dets, counts, [g[f'gt{i}'] for i in idx])


# ------------------------------------------------------------------------------------------------ 1. reference-source fixture
def test_voc_map_vs_the_reference_source_golden(golden_dir):
    from efficientdet.pytorch_amd.evaluate import VOCMeanAP
    g = _golden(golden_dir)
    NC, n = int(g['num_classes']), len(g['scales'])
    meter = VOCMeanAP(NC, iou_threshold=float(g['iou_threshold']))
    _feed(g, meter, [list(range(i, min(n, i + 8))) for i in range(0, n, 8)])
    mean, aps, curves = meter.compute(curves=True)
    assert [aps[c][1] for c in range(NC)] == [0 if v == 0 else float(v) for v in g['num_annotations']]
    assert sorted(curves) == [int(c) for c in g['curve_classes']]
    for c in curves:
        r, p = curves[c]
        assert np.array_equal(r, g['recall%d' % c]) and np.array_equal(p, g['precision%d' % c]), c      # bit for bit
    for c in range(NC):
        assert abs(aps[c][0] - g['ap'][c]) <= 1e-12, (c, aps[c][0], g['ap'][c])
    assert aps[19] == (0, 0) and type(aps[0][0]) is np.float64 and type(aps[0][1]) is float
    assert type(mean) is np.float64 and abs(mean - g['mean_ap']) <= 1e-12


# ------------------------------------------------------------------------------------------------ 2. evaluate_voc end to end
class _Recorder:
    """The model as evaluate_voc sees it; keeps each forward's (cls, reg, anchors) so the host path scores the same outputs."""
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


@pytest.mark.parametrize('batch_size', [1, 3])
def test_evaluate_voc_end_to_end_vs_host_path(batch_size, capsys):
    from efficientdet.pytorch_amd import EfficientDet, EFFICIENTDET
    from efficientdet.pytorch_amd import evaluate as EV
    net, nc = 'efficientdet-d0', 8
    c = EFFICIENTDET[net]
    m = EfficientDet(nc, network=net, W_bifpn=c['W_bifpn'], D_bifpn=c['D_bifpn'], D_class=c['D_class'], compute_dtype=torch.float32,
                     is_training=False, threshold=0.05)
    m.load_state_dict(O.make_state_dict(net, nc, seed=0))
    m = m.cuda()
    img, _ = O.synthetic_batch(6, 128, seed=4, num_classes=nc)
    imgs = [img[i].permute(1, 2, 0).contiguous() for i in range(6)]                # HWC, as the reference's datasets yield them
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
    got = EV.evaluate_voc(_Generator(imgs, scales, anns, nc), rec, batch_size=batch_size)
    printed = capsys.readouterr().out
    assert 'mAP:' in printed and 'avg mAP: {}'.format(got[0]) in printed and 'c7: ' in printed
    assert len(rec.out) == (6 if batch_size == 1 else 2)
    rows, first = [], 0
    for (cls, reg, anc), H, W in rec.out:                                      # the existing host path on the same outputs
        s, l, b, cnt = EV.postprocess(m, cls, reg, anc, H, W)
        B = int(cls.shape[0])
        dets, counts = EV.finalize(s, l, b, cnt, scales[first:first + B], score_threshold=0.05, max_detections=100)
        rows += [dets[j, :int(counts[j])] for j in range(B)]
        first += B
    assert sum(len(r) for r in rows) > 200                                       # long lists
    want = restated_evaluate(rows, anns, nc)
    _assert_same_structure(got, want[:2], nc, 1e-12)
    assert any(0 < got[1][c][0] for c in range(nc))                             # some TPs at all


# ------------------------------------------------------------------------------------------------ 3. ties
def test_tied_scores_follow_insertion_order():
    """Equal scores of one class with mixed TP / FP across and within images: ranked by (image, slot), like a stable sort."""
    from efficientdet.pytorch_amd.evaluate import VOCMeanAP
    C, M = 3, 8
    dets = np.zeros((4, M, 6), dtype=np.float32); dets[:, :, 5] = -1
    counts = np.array([4, 3, 0, 5], dtype=np.int32)
    gts = [np.array([[0, 0, 10, 10, 0], [20, 20, 30, 30, 0], [0, 0, 10, 10, 1]], dtype=np.float64),
           np.array([[0, 0, 10, 10, 0]], dtype=np.float64), np.zeros((0, 5)),
           np.array([[5, 5, 15, 15, 0], [40, 40, 50, 50, 2]], dtype=np.float64)]
    hit, miss = [0, 0, 10, 10], [100, 100, 110, 110]
    dets[0, :4] = [hit + [0.75, 0], miss + [0.75, 0], [20, 20, 30, 30, 0.75, 0], hit + [0.5, 1]]
    dets[1, :3] = [miss + [0.75, 0], hit + [0.75, 0], hit + [0.75, 0]]                 # FP before TP before duplicate, all tied
    dets[3, :5] = [miss + [0.75, 0], [5, 5, 15, 15, 0.75, 0], miss + [0.5, 1], [40, 40, 50, 50, 0.5, 2], miss + [0.5, 2]]
    rows = [dets[i, :counts[i]] for i in range(4)]
    want = restated_evaluate(rows, gts, C)
    meter = VOCMeanAP(C)
    meter.add(torch.from_numpy(dets).cuda(), torch.from_numpy(counts).cuda(), gts)
    mean, aps, curves = meter.compute(curves=True)
    for c in range(C):
        assert aps[c] == want[1][c], (c, aps[c], want[1][c])
        assert np.array_equal(curves[c][0], want[2][c][0]) and np.array_equal(curves[c][1], want[2][c][1]), c
    assert mean == want[0]
    # a different (unstable) order of the tied class-0 rows gives another AP: the rule is observable here
    assert aps[0][0] != restated_evaluate([rows[1], rows[0], rows[2], rows[3]], [gts[1], gts[0], gts[2], gts[3]], C)[1][0][0]


# ------------------------------------------------------------------------------------------------ 4. batching invariance, determinism
def test_batching_invariance_and_determinism(golden_dir):
    from efficientdet.pytorch_amd.evaluate import VOCMeanAP
    g = _golden(golden_dir)
    NC, n = int(g['num_classes']), len(g['scales'])
    results = []
    for batches in ([list(range(n))], [list(range(i, i + 3)) for i in range(0, n, 3)], [[i] for i in range(n)], [list(range(n))]):
        meter = VOCMeanAP(NC)
        _feed(g, meter, batches)
        results.append(meter.compute(curves=True))
    mean0, aps0, cv0 = results[0]
    for mean, aps, cv in results[1:]:
        assert mean == mean0 and aps == aps0
        assert sorted(cv) == sorted(cv0) and all(np.array_equal(cv[c][0], cv0[c][0]) and np.array_equal(cv[c][1], cv0[c][1]) for c in cv)
    meter.reset()
    assert meter.num_records == 0 and meter.compute()[1] == {c: (0, 0) for c in range(NC)}


# ------------------------------------------------------------------------------------------------ 5. scale
def _synthetic(n_img, C, seed, slots=100):
    rng = np.random.RandomState(seed)
    ng = rng.randint(0, 9, n_img)
    gts, dets = [], np.zeros((n_img, slots, 6), dtype=np.float32)
    counts = rng.randint(0, slots + 1, n_img).astype(np.int32)
    counts[::7] = slots
    for i in range(n_img):
        x1 = rng.uniform(0, 400, ng[i]); y1 = rng.uniform(0, 400, ng[i])
        g = np.stack([x1, y1, x1 + rng.uniform(10, 200, ng[i]), y1 + rng.uniform(10, 200, ng[i]), rng.randint(0, C, ng[i])], 1) \
            if ng[i] else np.zeros((0, 5))
        gts.append(g)
        k = counts[i]
        gi = g[rng.randint(0, ng[i], k)] if ng[i] else np.zeros((k, 5))
        near = (rng.rand(k) < 0.6) & (ng[i] > 0)
        wh = np.concatenate([gi[:, 2:4] - gi[:, 0:2]] * 2, 1)
        bx = gi[:, :4] + rng.normal(0, 0.12, (k, 4)) * wh
        rnd = rng.uniform(0, 400, (k, 2))
        rb = np.concatenate([rnd, rnd + rng.uniform(5, 150, (k, 2))], 1)
        box = np.where(near[:, None], bx, rb)
        lab = np.where(near & (rng.rand(k) < 0.8), gi[:, 4], rng.randint(0, C, k))
        sc = np.sort(rng.randint(1, 20000, k).astype(np.float32) / np.float32(20000))[::-1]    # coarse: many ties across images
        dets[i, :k, :4], dets[i, :k, 4], dets[i, :k, 5] = box, sc, lab
    dets[:, :, 5][np.arange(slots)[None, :] >= counts[:, None]] = -1
    return dets, counts, gts


@pytest.mark.parametrize('n_img,C', [(4952, 20), (600, 80)])
def test_voc_scale_vs_restatement(n_img, C):
    from efficientdet.pytorch_amd.evaluate import VOCMeanAP
    dets, counts, gts = _synthetic(n_img, C, seed=C)
    meter = VOCMeanAP(C)
    dd, cd = torch.from_numpy(dets).cuda(), torch.from_numpy(counts).cuda()
    for i in range(0, n_img, 32):
        meter.add(dd[i:i + 32], cd[i:i + 32], gts[i:i + 32])
    assert meter.num_records == n_img * 100
    if n_img * 100 > VOCMeanAP.INITIAL_CAPACITY:
        assert meter.capacity >= meter.num_records > VOCMeanAP.INITIAL_CAPACITY       # the buffer grew past its first allocation
    got = meter.compute()
    want = restated_evaluate([dets[i, :counts[i]] for i in range(n_img)], gts, C)
    _assert_same_structure(got, want[:2], C, 1e-12)
    assert sum(1 for c in range(C) if got[1][c][0] > 0) >= C // 2


# ------------------------------------------------------------------------------------------------ 6. no host sync in add
def test_add_performs_no_device_to_host_transfer(monkeypatch, golden_dir):
    from efficientdet.pytorch_amd import evaluate as EV
    g = _golden(golden_dir)
    s, l, b, cnt = _raw_batch(g, list(range(12)))
    dets, counts = EV.finalize_device(s, l, b, cnt, [float(v) for v in g['scales'][:12]])
    gts = [g[f'gt{i}'] for i in range(12)]
    G = max(len(a) for a in gts)
    hb = np.zeros((12, G, 4)); hl = np.full((12, G), -1, dtype=np.int32)
    for i, a in enumerate(gts):
        hb[i, :len(a)] = a[:, :4]; hl[i, :len(a)] = a[:, 4]
    dev_gt = (torch.from_numpy(hb).cuda(), torch.from_numpy(hl).cuda())
    monkeypatch.setattr(EV.VOCMeanAP, 'INITIAL_CAPACITY', 256)                   # so that add also grows the buffer
    meter = EV.VOCMeanAP(int(g['num_classes']))
    torch.cuda.synchronize()

    def boom(*a, **k):
        raise AssertionError('device->host transfer inside VOCMeanAP.add')
    with monkeypatch.context() as mp:
        for name in ('item', 'cpu', 'tolist', 'numpy'):
            mp.setattr(torch.Tensor, name, boom)
        mp.setattr(torch.cuda, 'synchronize', boom)
        meter.add(dets, counts, gts)
        meter.add(dets, counts, dev_gt)
    assert meter.capacity > 256 and meter.num_records == 2 * 12 * 100
    mean, aps = meter.compute()
    ref = EV.VOCMeanAP(int(g['num_classes']))
    ref.add(dets, counts, gts); ref.add(dets, counts, gts)
    assert ref.compute()[1] == aps
