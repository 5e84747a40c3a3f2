"""GPU: the rescoring NMS (effdet_soft_nms behind ops.soft_nms, EfficientDet.set_nms and the three detection paths).

  * hard and linear: idx, count and new_score equal the float32 restatement (tests/soft_nms_restated.py) BIT FOR BIT on every case;
  * hard, class-agnostic, uncapped: idx and count equal ops.nms -- the existing, separately tested greedy kernels -- exactly;
  * gaussian (sigma 0.3, 0.5): the validator replays the device's pick order in float64, tol = 2e-4 relative.  Why 2e-4: one rescoring
    carries about 1e-6 relative error (the IoU's few ulps amplified by d/d(iou) of iou^2 / sigma = 2 iou / sigma <= 6.7, plus expf and
    one multiply at a few ulps each); a candidate is rescored at most max_det = 100 times in these cases -> 1e-4; twice that.  Derived,
    not measured; the test prints the largest deviation per case (pytest -s) and DESIGN.md section 7 is where it is recorded;
  * the model level (D0 @128, B = 2) through model.set_nms, with nms_options=None shown unchanged against ops.nms + ops.gather_dets;
  * the C ABI's error codes for every out-of-limit argument, with nothing launched.
"""
import numpy as np
import pytest
import torch

from oracle import effdet_oracle as O
from tests import soft_nms_restated as R
from tests.soft_nms_cases import CASES

pytestmark = pytest.mark.gpu
TOL = 2e-4


def _opts(case, method, **kw):
    d = dict(threshold=case['threshold'], iou_threshold=case['iou_threshold'], method=method, sigma=0.5, class_aware=False,
             pre_nms_top_n=case['pre_nms_top_n'], max_det=case['max_det'])
    d.update(kw)
    return R.Opts(**d)


def _device_run(case, o):
    from efficientdet.pytorch_amd import ops
    boxes, score, label = (torch.from_numpy(case[k]).cuda() for k in ('boxes', 'score', 'label'))
    idx, new_score, count = ops.soft_nms(boxes, score, label, o.threshold, o.iou_threshold, o.method, o.sigma, o.class_aware,
                                         o.pre_nms_top_n, o.max_det)
    return idx.cpu().numpy(), new_score.cpu().numpy(), count.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize('aware', [False, True], ids=['agnostic', 'per_class'])
@pytest.mark.parametrize('method', ['hard', 'linear'])
@pytest.mark.parametrize('case', CASES, ids=lambda c: c['name'])
def test_hard_and_linear_equal_the_float32_restatement_bit_for_bit(case, method, aware):
    o = _opts(case, method, class_aware=aware)
    idx, new_score, count = _device_run(case, o)
    for b in range(case['boxes'].shape[0]):
        ridx, rs, n = R.run_f32(case['boxes'][b], case['score'][b], case['label'][b], o)
        assert int(count[b]) == n, (b, int(count[b]), n)
        assert np.array_equal(idx[b, :n], ridx), b
        assert np.array_equal(_bits(new_score[b, :n]), _bits(rs)), (b, np.abs(new_score[b, :n] - rs).max())
        assert not idx[b, n:].any() and not _bits(new_score[b, n:]).any()          # rows past the count: index 0, score +0
        assert np.all(new_score[b, :n][:-1] >= new_score[b, :n][1:])                # emitted scores never increase


@pytest.mark.parametrize('case', [c for c in CASES if c['n'] <= c['pre_nms_top_n']], ids=lambda c: c['name'])
def test_hard_class_agnostic_uncapped_equals_the_greedy_kernels(case):
    from efficientdet.pytorch_amd import ops
    o = _opts(case, 'hard', max_det=max(case['n'], 1))
    idx, new_score, count = _device_run(case, o)
    gidx, gcount = ops.nms(torch.from_numpy(case['boxes']).cuda(), torch.from_numpy(case['score']).cuda(), o.threshold, o.iou_threshold)
    gidx, gcount = gidx.cpu().numpy(), gcount.cpu().numpy()
    assert np.array_equal(count, gcount), (count, gcount)
    for b, n in enumerate(count.tolist()):
        assert np.array_equal(idx[b, :n], gidx[b, :n]), b
        assert np.array_equal(_bits(new_score[b, :n]), _bits(case['score'][b][idx[b, :n]]))      # hard: the scores are the input's


@pytest.mark.parametrize('aware', [False, True], ids=['agnostic', 'per_class'])
@pytest.mark.parametrize('sigma', [0.3, 0.5])
@pytest.mark.parametrize('case', CASES, ids=lambda c: c['name'])
def test_gaussian_passes_the_float64_validator(case, sigma, aware):
    o = _opts(case, 'gaussian', sigma=sigma, class_aware=aware)
    idx, new_score, count = _device_run(case, o)
    worst = 0.0
    for b in range(case['boxes'].shape[0]):
        n = int(count[b])
        worst = max(worst, R.check_run(case['boxes'][b], case['score'][b], case['label'][b], o, idx[b], new_score[b], n, TOL))
        assert not idx[b, n:].any() and not _bits(new_score[b, n:]).any()
        assert np.all(new_score[b, :n][:-1] >= new_score[b, :n][1:])
    print('gaussian %s sigma %.1f %s: largest relative deviation from float64 %.3g (bound %.3g)'
          % (case['name'], sigma, 'per_class' if aware else 'agnostic', worst, TOL))


def test_two_classes_on_identical_boxes():
    case = next(c for c in CASES if c['name'] == 'two_classes_identical_boxes')
    for method in ('hard', 'linear', 'gaussian'):
        _, s, count = _device_run(case, _opts(case, method, class_aware=True))
        assert int(count[0]) == 12 and np.array_equal(_bits(s[0, :12]), _bits(case['score'][0]))
    idx, _, count = _device_run(case, _opts(case, 'hard'))
    assert int(count[0]) == 6 and idx[0, :6].tolist() == [0, 2, 4, 6, 8, 10]


# ----------------------------------------------------------------------------- the C ABI's error codes
def test_out_of_limit_arguments_return_the_documented_codes_and_launch_nothing():
    from efficientdet.pytorch_amd import _lib as L
    lib = L.require('effdet_soft_nms', 'effdet_soft_nms_workspace_bytes')
    EINVAL, EUNSUPPORTED = -1, -3
    B, A = 2, 64
    boxes = torch.rand(B, A, 4, device='cuda'); score = torch.rand(B, A, device='cuda')
    label = torch.zeros(B, A, dtype=torch.int32, device='cuda')
    nbytes = int(lib.effdet_soft_nms_workspace_bytes(B, A, 100))
    assert nbytes > 0
    ws = torch.zeros(nbytes, dtype=torch.uint8, device='cuda')
    idx = torch.full((B, A), -7, dtype=torch.int32, device='cuda')
    ns = torch.full((B, A), -7.0, device='cuda')
    cnt = torch.full((B,), -7, dtype=torch.int32, device='cuda')
    good = dict(boxes=L.ptr(boxes), score=L.ptr(score), label=None, threshold=0.05, iou=0.5, method=1, sigma=0.5, aware=0, top_n=100,
                max_det=50, idx=L.ptr(idx), ns=L.ptr(ns), cnt=L.ptr(cnt), ws=L.ptr(ws), nbytes=nbytes, B=B, A=A)

    def call(**kw):
        a = dict(good); a.update(kw)
        return lib.effdet_soft_nms(a['boxes'], a['score'], a['label'], a['threshold'], a['iou'], a['method'], a['sigma'], a['aware'],
                                   a['top_n'], a['max_det'], a['idx'], a['ns'], a['cnt'], a['ws'], a['nbytes'], a['B'], a['A'],
                                   L.stream_ptr())
    for kw in (dict(top_n=0), dict(top_n=4097), dict(top_n=-1), dict(max_det=0), dict(max_det=101), dict(top_n=4096, max_det=4097),
               dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float('nan')), dict(method=3), dict(method=-1)):
        assert call(**kw) == EUNSUPPORTED, kw
    for kw in (dict(label=L.ptr(label)), dict(aware=1), dict(boxes=None), dict(score=None), dict(idx=None), dict(ns=None), dict(cnt=None),
               dict(ws=None), dict(nbytes=nbytes - 1), dict(B=0), dict(A=0)):
        assert call(**kw) == EINVAL, kw
    torch.cuda.synchronize()
    assert bool((idx == -7).all()) and bool((ns == -7.0).all()) and bool((cnt == -7).all())      # nothing was launched
    assert call() == 0 and call(label=L.ptr(label), aware=1) == 0 and call(top_n=4096, max_det=4096) == 0
    torch.cuda.synchronize()
    assert bool((cnt >= 0).all())


# ----------------------------------------------------------------------------- the model level
@pytest.fixture(scope='module')
def model_and_batch():
    from efficientdet.pytorch_amd import EfficientDet, EFFICIENTDET
    net, nc = 'efficientdet-d0', 20
    c = EFFICIENTDET[net]
    m = EfficientDet(nc, network=net, W_bifpn=c['W_bifpn'], D_bifpn=c['D_bifpn'], D_class=c['D_class'], is_training=False,
                     compute_dtype=torch.float32)
    m.load_state_dict(O.make_state_dict(net, nc, seed=0)); m = m.cuda().eval()
    img, _ = O.synthetic_batch(2, 128, seed=1, num_classes=nc)
    img = img.cuda()
    with torch.no_grad():
        cls, reg, anc = m.forward_raw(img)
    from efficientdet.pytorch_amd import ops
    decoded = ops.decode_score(anc, reg, cls, 128, 128)
    return m, img, (cls, reg, anc), decoded


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('options', [dict(method='gaussian', sigma=0.5, class_aware=True), dict(method='linear', pre_nms_top_n=64, max_det=20),
                                     dict(method='hard', class_aware=True, pre_nms_top_n=4096)], ids=lambda d: d['method'])
def test_model_paths_with_options(model_and_batch, options):
    from efficientdet.pytorch_amd import NMSOptions, evaluate, ops
    from efficientdet.pytorch_amd.graph import GraphedDetect
    m, img, (cls, reg, anc), (boxes, score, label) = model_and_batch
    opt = NMSOptions(**options)
    try:
        assert m.set_nms(opt) is m and m.nms_options is opt
        s, l, b, count = ops.model_nms(m, boxes, score, label)
        idx, ns, cnt = ops.soft_nms(boxes, score, label, m.threshold, m.iou_threshold, opt.method, opt.sigma, opt.class_aware,
                                    opt.pre_nms_top_n, opt.max_det)
        counts = count.tolist()
        assert counts == cnt.tolist() and min(counts) > 0 and max(counts) <= opt.max_det
        want = []
        for i, n in enumerate(counts):
            pick = idx[i, :n].long()
            assert torch.equal(s[i, :n], ns[i, :n]) and torch.equal(b[i, :n], boxes[i][pick]) and torch.equal(l[i, :n], label[i][pick].long())
            want.append((s[i, :n], l[i, :n], b[i, :n]))
        dets = m.detect(img)
        assert len(dets) == 2 and all(_same(d, w) for d, w in zip(dets, want))
        ps, pl, pb, pc = evaluate.postprocess(m, cls, reg, anc, 128, 128)
        assert torch.equal(pc, count) and all(_same((ps[i, :n], pl[i, :n], pb[i, :n]), want[i]) for i, n in enumerate(counts))
        out, oc = evaluate.detections_batched(m, img, [1.0, 1.0], score_threshold=0.0, max_detections=100)
        assert out.shape == (2, 100, 6) and oc.tolist() == counts
        for i, n in enumerate(counts):
            assert np.array_equal(out[i, :n, 4], want[i][0].cpu().numpy())
        gd = GraphedDetect(m, img)
        for _ in range(2):                                                          # the second replay too
            assert all(_same(d, w) for d, w in zip(gd(), want))
        m.set_nms(None)
        with pytest.raises(RuntimeError, match='nms_options changed after capture'):
            gd()
        m.set_nms(NMSOptions(**options))                                            # an equal object is the same configuration
        assert all(_same(d, w) for d, w in zip(gd(), want))
    finally:
        m.set_nms(None)
    with pytest.raises(TypeError):
        m.set_nms('gaussian')


def test_model_paths_without_options_are_todays(model_and_batch):
    from efficientdet.pytorch_amd import NMSOptions, evaluate, ops
    from efficientdet.pytorch_amd.graph import GraphedDetect
    m, img, (cls, reg, anc), (boxes, score, label) = model_and_batch
    assert m.nms_options is None
    idx, count = ops.nms(boxes, score, float(m.threshold), float(m.iou_threshold))
    s, l, b = ops.gather_dets(boxes, score, label, idx, count)
    counts = count.tolist()
    assert min(counts) > 0
    want = [(s[i, :n], l[i, :n], b[i, :n]) for i, n in enumerate(counts)]
    got = ops.model_nms(m, boxes, score, label)
    assert torch.equal(got[3], count) and all(_same((got[0][i, :n], got[1][i, :n], got[2][i, :n]), want[i]) for i, n in enumerate(counts))
    assert all(_same(d, w) for d, w in zip(m.detect(img), want))
    ps, pl, pb, pc = evaluate.postprocess(m, cls, reg, anc, 128, 128)
    assert torch.equal(pc, count) and all(_same((ps[i, :n], pl[i, :n], pb[i, :n]), want[i]) for i, n in enumerate(counts))
    gd = GraphedDetect(m, img)
    assert all(_same(d, w) for d, w in zip(gd(), want))
    m.set_nms(NMSOptions('linear'))
    try:
        with pytest.raises(RuntimeError, match='nms_options changed after capture'):
            gd()
    finally:
        m.set_nms(None)
    assert all(_same(d, w) for d, w in zip(gd(), want))
