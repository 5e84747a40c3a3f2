"""GPU: multi-scale test-time augmentation and mixed-size ensembles at the model level (D0, 20 classes, B = 2, base 256 x 256, seeded
weights), in the manner of tests/test_gpu_tta_model.py.

The views are obtained independently of ops.model_detections: forward_raw + evaluate.postprocess on the batch, on torch.flip of it, on
ops.resample_images(batch, (128, 128)) and (384, 384) and on their mirrored forms, each decoded against its own size.  They are fused
on the host by the fp32 restatement of the fusion (tests/wbf_restated.run_f32) with the flips and multipliers of ops.tta_view_plan, and
detect() must equal that in labels, score bits and box bits.  detections_batched and GraphedDetect agree with detect(); scales=() is
today's hflip TTA; the parameter-preparation table settles; an ensemble with scales=(None, 0.5) is the restated fusion of the plain
view and the 128 x 128 view under the multipliers (1, 2).

The seeded weights score nearly every anchor above the model's threshold (the plain NMS keeps about 1350 boxes per image at 256 x 256
and 3200 at 384 x 384), so the model runs with set_nms(NMSOptions(max_det=MAX_DET)): every view then holds at most MAX_DET <= top_n rows
and the fusion cuts nothing, which the fixture asserts for all six views."""
import numpy as np
import pytest
import torch

from oracle import effdet_oracle as O
from tests import wbf_restated as R

pytestmark = pytest.mark.gpu
S = 256
SIZES = (S, S // 2, 3 * S // 2)              # the base and the scales 0.5 and 1.5
TOP_N = 600
MAX_DET = 300                                # rows per image and view (the model's own NMS option)


@pytest.fixture(scope='module')
def setup():
    from efficientdet.pytorch_amd import EfficientDet, EFFICIENTDET, NMSOptions, evaluate, ops
    net, nc = 'efficientdet-d0', 20
    c = EFFICIENTDET[net]
    m = EfficientDet(nc, network=net, W_bifpn=c['W_bifpn'], D_bifpn=c['D_bifpn'], D_class=c['D_class'], is_training=False,
                     compute_dtype=torch.float32)
    m.load_state_dict(O.make_state_dict(net, nc, seed=0)); m = m.cuda().eval()
    m.set_nms(NMSOptions(method='hard', pre_nms_top_n=1000, max_det=MAX_DET))
    img, _ = O.synthetic_batch(2, S, seed=1, num_classes=nc)
    img = img.cuda()
    views = {}                                                   # (size, flip) -> the view's device outputs on the host
    with torch.no_grad():
        for size in SIZES:
            for flip in (False, True):
                if size == S:
                    x = torch.flip(img, (3,)) if flip else img
                else:
                    x = ops.resample_images(img, (size, size), flip)
                cls, reg, anc = m.forward_raw(x)
                v = evaluate.postprocess(m, cls, reg, anc, size, size)
                views[(size, flip)] = tuple(t.cpu().numpy() for t in v)
    for k, v in views.items():
        print('view %s: counts %s' % (k, v[3].tolist()))
        assert 0 < v[3].min() and v[3].max() <= MAX_DET <= TOP_N, (k, v[3].tolist())         # nothing is cut by top_n
    return m, img, views


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _all_same(got, want):
    return len(got) == len(want) and all(_same(g, w) for g, w in zip(got, want))


def _restated(views, keys, i, weights, muls, top_n, conf_type='avg'):
    flips = [float(size) if flip else None for size, flip in keys]
    run = R.run_f32([(views[k][0][i], views[k][1][i], views[k][2][i], int(views[k][3][i])) for k in keys], weights, flips, muls, R.Opts(top_n=top_n))
    return R.emit(run, conf_type), run


def _assert_is_restated(dets, views, keys, weights, muls, top_n):
    assert len(dets) == 2
    for i, (s, l, b) in enumerate(dets):
        (rs, rl, rb), run = _restated(views, keys, i, weights, muls, top_n)
        rows = sum(int(views[k][3][i]) for k in keys)
        print('image %d: %d rows of %d views -> %d clusters, the largest of %d' % (i, rows, len(keys), len(rs), max(len(c) for c in run.clusters)))
        assert 0 < len(rs) <= rows and max(len(c) for c in run.clusters) > 1
        assert len(s) == len(rs) and np.array_equal(l.cpu().numpy(), rl)
        assert np.array_equal(s.cpu().numpy().view(np.uint32), rs.view(np.uint32))
        assert np.array_equal(b.cpu().numpy().view(np.uint32), rb.view(np.uint32))


def _plan_keys(plan):
    return [(hv, flip) for hv, _, flip, _, _ in plan]


def test_one_scale_without_flip_is_the_restated_fusion(setup):
    from efficientdet.pytorch_amd import TTAOptions, evaluate, ops
    m, img, views = setup
    opt = TTAOptions(hflip=False, scales=(0.5,))
    plan = ops.tta_view_plan(S, S, opt)
    assert _plan_keys(plan) == [(256, False), (128, False)] and [p[3] for p in plan] == [1.0, 2.0]
    try:
        m.set_tta(opt)
        dets = m.detect(img)
        _assert_is_restated(dets, views, _plan_keys(plan), None, [p[3] for p in plan], 1000)
        out, oc = evaluate.detections_batched(m, img, [1.0, 1.0], score_threshold=0.0, max_detections=100)
        assert oc.tolist() == [min(len(d[0]), 100) for d in dets]
        for i, n in enumerate(oc.tolist()):
            assert np.array_equal(out[i, :n, 4], dets[i][0][:n].cpu().numpy()) and np.array_equal(out[i, :n, :4], dets[i][2][:n].cpu().numpy())
            assert np.array_equal(out[i, :n, 5], dets[i][1][:n].cpu().numpy().astype(np.float32))
    finally:
        m.set_tta(None)


def test_six_views_are_the_restated_fusion_and_the_graph_agrees(setup):
    from efficientdet.pytorch_amd import TTAOptions, WBFOptions, evaluate, ops
    from efficientdet.pytorch_amd.graph import GraphedDetect
    m, img, views = setup
    opt = TTAOptions(hflip=True, scales=(0.5, 1.5), fusion=WBFOptions(top_n=TOP_N))
    plan = ops.tta_view_plan(S, S, opt)
    keys = _plan_keys(plan)
    assert keys == [(256, False), (256, True), (128, False), (128, True), (384, False), (384, True)]
    muls = [p[3] for p in plan]
    assert muls == [1.0, 1.0, 2.0, 2.0, float(np.float32(2.0 / 3.0)), float(np.float32(2.0 / 3.0))]
    try:
        m.set_tta(opt)
        dets = m.detect(img)
        _assert_is_restated(dets, views, keys, None, muls, TOP_N)
        out, oc = evaluate.detections_batched(m, img, [1.0, 1.0], score_threshold=0.0, max_detections=100)
        assert oc.tolist() == [min(len(d[0]), 100) for d in dets]
        for i, n in enumerate(oc.tolist()):
            assert np.array_equal(out[i, :n, 4], dets[i][0][:n].cpu().numpy()) and np.array_equal(out[i, :n, :4], dets[i][2][:n].cpu().numpy())
            assert np.array_equal(out[i, :n, 5], dets[i][1][:n].cpu().numpy().astype(np.float32))
        gd = GraphedDetect(m, img)
        for _ in range(2):                                                          # the second replay too
            assert _all_same(gd(), dets)
        m.set_tta(TTAOptions(hflip=True, scales=(0.5,), fusion=WBFOptions(top_n=TOP_N)))
        with pytest.raises(RuntimeError, match='tta_options changed after capture'):
            gd()
        m.set_tta(TTAOptions(hflip=True, scales=(1.5, 0.5), fusion=WBFOptions(top_n=TOP_N)))     # the order of the views is part of it
        with pytest.raises(RuntimeError, match='tta_options changed after capture'):
            gd()
        m.set_tta(TTAOptions(hflip=True, scales=[0.5, 1.5], fusion=WBFOptions(top_n=TOP_N)))     # an equal object: the same configuration
        assert _all_same(gd(), dets)
    finally:
        m.set_tta(None)


def test_weights_follow_the_view_order(setup):
    from efficientdet.pytorch_amd import TTAOptions, ops
    m, img, views = setup
    w = (1.0, 0.5, 2.0, 0.25)
    opt = TTAOptions(hflip=True, scales=(1.5,), weights=w)
    plan = ops.tta_view_plan(S, S, opt)
    assert [p[4] for p in plan] == list(w)
    try:
        m.set_tta(opt)
        _assert_is_restated(m.detect(img), views, _plan_keys(plan), w, [p[3] for p in plan], 1000)
    finally:
        m.set_tta(None)


def test_empty_scales_is_todays_hflip_tta_bit_for_bit(setup):
    from efficientdet.pytorch_amd import TTAOptions
    m, img, views = setup
    try:
        m.set_tta(TTAOptions(scales=()))
        dets = m.detect(img)
        _assert_is_restated(dets, views, [(256, False), (256, True)], None, None, 1000)      # muls None: no multiplier at all, as before
        m.set_tta(TTAOptions())
        assert _all_same(m.detect(img), dets)
    finally:
        m.set_tta(None)


def test_a_bad_scale_is_refused_before_any_launch(setup):
    from efficientdet.pytorch_amd import TTAOptions
    m, img, views = setup
    calls = []
    orig = m.forward_raw
    try:
        m.forward_raw = lambda x: calls.append(1) or orig(x)
        m.set_tta(TTAOptions(hflip=False, scales=(0.75,)))
        with pytest.raises(ValueError, match='H = 256, W = 256 at scale s = 0.75'):
            m.detect(img)
        assert not calls
    finally:
        del m.forward_raw
        m.set_tta(None)


def test_parameter_preparation_settles_under_multi_view_calls(setup):
    from efficientdet.pytorch_amd import TTAOptions, WBFOptions
    m, img, views = setup

    def jobs():
        return sum(len(p.jobs) for p in m._prep.values())
    try:
        m.set_tta(TTAOptions(hflip=True, scales=(0.5, 1.5), fusion=WBFOptions(top_n=TOP_N)))
        first = m.detect(img)
        m.detect(img)
        preps = {k: id(p) for k, p in m._prep.items()}
        n2 = jobs()
        assert n2 > 0
        m.detect(img)
        n3 = jobs()
        for _ in range(2):
            m.detect(img)
        last = m.detect(img)
        n6 = jobs()
        print('recorded jobs after calls 2, 3, 6: %d, %d, %d' % (n2, n3, n6))
        assert n3 == n2 and n6 == n2                            # neither reset (the count would drop) nor growing call after call
        assert {k: id(p) for k, p in m._prep.items()} == preps
        assert _all_same(last, first)
    finally:
        m.set_tta(None)


def test_ensemble_with_a_half_size_member(setup):
    from efficientdet.pytorch_amd import evaluate
    m, img, views = setup
    e = evaluate.EnsembleDetector([m, m], weights=(1, 1), scales=(None, 0.5))
    dets = e.detect(img)
    _assert_is_restated(dets, views, [(256, False), (128, False)], (1.0, 1.0), [1.0, 2.0], 1000)
    out, oc = evaluate.detections_batched(e, img, [1.0, 1.0], score_threshold=0.0, max_detections=100)
    assert oc.tolist() == [min(len(d[0]), 100) for d in dets]
    for i, n in enumerate(oc.tolist()):
        assert np.array_equal(out[i, :n, 4], dets[i][0][:n].cpu().numpy())
    with pytest.raises(ValueError, match='EnsembleDetector: H = 256, W = 256 at scale s = 0.75'):
        evaluate.EnsembleDetector([m, m], scales=(None, 0.75)).detect(img)
