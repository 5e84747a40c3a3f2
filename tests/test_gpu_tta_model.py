"""GPU: test-time augmentation and ensembles at the model level (D0 @128, B = 2, seeded weights).

  * set_tta(None) and set_tta(TTAOptions(hflip=False)) equal the plain detection path bit for bit (forward_raw + evaluate.postprocess,
    which is what detect() did before TTA existed);
  * hflip=True: detect() equals the fp32 restatement (tests/wbf_restated.py) of the fusion applied to the two views' device outputs,
    the views obtained by forward_raw + evaluate.postprocess on the batch and on its mirror image;
  * evaluate.detections_batched and graph.GraphedDetect agree with detect() bit for bit; GraphedDetect refuses a changed set_tta;
  * an EnsembleDetector of the model with itself, weights (1, 1), returns the model's own boxes and scores within 1 ulp:
    score (s + s) / 2 * 2 / 2 is exact, box (s x + s x) / (2 s) rounds s x once and the quotient once.
"""
import numpy as np
import pytest
import torch

from oracle import effdet_oracle as O
from tests import wbf_restated as R

pytestmark = pytest.mark.gpu
S = 128


@pytest.fixture(scope='module')
def setup():
    from efficientdet.pytorch_amd import EfficientDet, EFFICIENTDET, evaluate
    net, nc = 'efficientdet-d0', 20
    c = EFFICIENTDET[net]
    m = EfficientDet(nc, network=net, W_bifpn=c['W_bifpn'], D_bifpn=c['D_bifpn'], D_class=c['D_class'], is_training=False,
                     compute_dtype=torch.float32)
    m.load_state_dict(O.make_state_dict(net, nc, seed=0)); m = m.cuda().eval()
    img, _ = O.synthetic_batch(2, S, seed=1, num_classes=nc)
    img = img.cuda()
    views = []
    with torch.no_grad():
        for x in (img, torch.flip(img, (3,))):
            cls, reg, anc = m.forward_raw(x)
            views.append(evaluate.postprocess(m, cls, reg, anc, S, S))
    counts = views[0][3].tolist()
    assert 0 < min(counts) and max(counts) <= 1000 and max(views[1][3].tolist()) <= 1000          # (nothing is cut by top_n = 1000)
    plain = [(views[0][0][i, :n], views[0][1][i, :n], views[0][2][i, :n]) for i, n in enumerate(counts)]
    return m, img, views, plain


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _all_same(got, want):
    return len(got) == len(want) and all(_same(g, w) for g, w in zip(got, want))


def test_no_tta_and_single_view_tta_are_the_plain_path(setup):
    from efficientdet.pytorch_amd import TTAOptions, evaluate
    from efficientdet.pytorch_amd.graph import GraphedDetect
    m, img, views, plain = setup
    assert m.tta_options is None and _all_same(m.detect(img), plain)
    try:
        assert m.set_tta(TTAOptions(hflip=False)) is m
        assert _all_same(m.detect(img), plain)
        assert _all_same(GraphedDetect(m, img)(), plain)
        out, oc = evaluate.detections_batched(m, img, [1.0, 1.0], score_threshold=0.0, max_detections=100)
        m.set_tta(None)
        ref, rc = evaluate.detections_batched(m, img, [1.0, 1.0], score_threshold=0.0, max_detections=100)
        assert np.array_equal(out, ref) and np.array_equal(oc, rc)
    finally:
        m.set_tta(None)
    assert _all_same(GraphedDetect(m, img)(), plain)


@pytest.mark.parametrize('conf_type,weights', [('avg', None), ('max', (2.0, 1.0))])
def test_hflip_tta_is_the_restated_fusion_of_the_two_views(setup, conf_type, weights):
    from efficientdet.pytorch_amd import TTAOptions, WBFOptions, evaluate
    from efficientdet.pytorch_amd.graph import GraphedDetect
    m, img, views, plain = setup
    host = [tuple(t.cpu().numpy() for t in v) for v in views]
    opt = TTAOptions(hflip=True, weights=weights, fusion=WBFOptions(conf_type=conf_type))
    try:
        m.set_tta(opt)
        dets = m.detect(img)
        assert len(dets) == 2
        for i, (s, l, b) in enumerate(dets):
            run = R.run_f32([(v[0][i], v[1][i], v[2][i], int(v[3][i])) for v in host], weights, [None, float(S)], None, R.Opts())
            rs, rl, rb = R.emit(run, conf_type)
            print('image %d: %d + %d rows -> %d clusters, the largest of %d' % (i, host[0][3][i], host[1][3][i], len(rs), max(len(c) for c in run.clusters)))
            assert 0 < len(rs) <= int(host[0][3][i]) + int(host[1][3][i])
            assert len(s) == len(rs) and np.array_equal(l.cpu().numpy(), rl)
            assert np.array_equal(s.cpu().numpy().view(np.uint32), rs.view(np.uint32))
            assert np.array_equal(b.cpu().numpy().view(np.uint32), rb.view(np.uint32))
        out, oc = evaluate.detections_batched(m, img, [1.0, 1.0], score_threshold=0.0, max_detections=100)
        assert oc.tolist() == [min(len(d[0]), 100) for d in dets]
        for i, n in enumerate(oc.tolist()):
            assert np.array_equal(out[i, :n, 4], dets[i][0][:n].cpu().numpy()) and np.array_equal(out[i, :n, :4], dets[i][2][:n].cpu().numpy())
            assert np.array_equal(out[i, :n, 5], dets[i][1][:n].cpu().numpy().astype(np.float32))
        gd = GraphedDetect(m, img)
        for _ in range(2):                                                          # the second replay too
            assert _all_same(gd(), dets)
        m.set_tta(None)
        with pytest.raises(RuntimeError, match='tta_options changed after capture'):
            gd()
        m.set_tta(TTAOptions(hflip=True, weights=weights, fusion=WBFOptions(conf_type=conf_type)))      # an equal object: the same configuration
        assert _all_same(gd(), dets)
    finally:
        m.set_tta(None)


def test_packed_images_flip(setup):
    from efficientdet.pytorch_amd import PackedImages, TTAOptions, ops
    m, img, views, plain = setup
    x = torch.zeros(2, S, S, 4, device='cuda')
    x[..., :3] = img.permute(0, 2, 3, 1)
    packed = PackedImages(ops.Map.of(x))
    try:
        m.set_tta(TTAOptions())
        assert _all_same(m.detect(packed), m.detect(img))
        arena = torch.zeros(2 * S * S * 4 + 64, device='cuda')
        with pytest.raises(TypeError, match='dense'):
            m.detect(PackedImages(ops.Map(arena, 2, S, S, 4, off=64)))
    finally:
        m.set_tta(None)


def _ulps(a, b):
    a, b = (np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64) for x in (a, b))
    return int(np.abs(a - b).max()) if a.size else 0


def test_ensemble_of_the_model_with_itself_returns_its_own_detections(setup):
    from efficientdet.pytorch_amd import evaluate
    m, img, views, plain = setup
    e = evaluate.EnsembleDetector([m, m], weights=(1, 1))
    dets = e.detect(img)
    worst_s = worst_b = 0
    for (s, l, b), (ps, pl, pb) in zip(dets, plain):
        # NMS left no same-label pair above its IoU threshold 0.5 < 0.55: every cluster is a detection and its twin, in score order
        assert len(s) == len(ps) and torch.equal(l, pl)
        worst_s = max(worst_s, _ulps(s.cpu().numpy(), ps.cpu().numpy())); worst_b = max(worst_b, _ulps(b.cpu().numpy(), pb.cpu().numpy()))
    print('ensemble of a model with itself: largest deviation %d ulp (scores), %d ulp (boxes); bound 1' % (worst_s, worst_b))
    assert worst_s <= 1 and worst_b <= 1
    out, oc = evaluate.detections_batched(e, img, [1.0, 1.0], score_threshold=0.0, max_detections=100)
    assert oc.tolist() == [min(len(d[0]), 100) for d in dets]
    for i, n in enumerate(oc.tolist()):
        assert np.array_equal(out[i, :n, 4], dets[i][0][:n].cpu().numpy())
