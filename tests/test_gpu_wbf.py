"""GPU: the weighted boxes fusion (effdet_wbf behind ops.fuse_detections).

  * on every seeded case and both conf types, count, labels and the BIT PATTERNS of scores and boxes equal the float32 restatement
    (tests/wbf_restated.py): the kernel's file is built without FMA contraction and every operation is an IEEE one;
  * rows past the count are zero, emitted scores never increase;
  * the C ABI's error codes for every out-of-limit argument, with nothing launched.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import wbf_restated as R
from tests.wbf_cases import CASES

pytestmark = pytest.mark.gpu
BY_NAME = {c['name']: c for c in CASES}


@functools.lru_cache(maxsize=None)
def _reference(name):
    """The fp32 restatement of every image of a case, once for both conf types (the clustering does not depend on the type)."""
    c = BY_NAME[name]
    o = R.Opts(c['iou_thr'], c['skip_thr'], c['top_n'])
    return [R.run_f32([(s[b], l[b], bx[b], int(n[b])) for s, l, bx, n in c['views']], c['weights'], c['flips'], c['muls'], o)
            for b in range(len(c['views'][0][3]))]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize('conf_type', ['avg', 'max'])
@pytest.mark.parametrize('case', CASES, ids=lambda c: c['name'])
def test_fusion_equals_the_float32_restatement_bit_for_bit(case, conf_type):
    from efficientdet.pytorch_amd import ops
    views = [tuple(torch.from_numpy(a).cuda() for a in v) for v in case['views']]
    opt = ops.WBFOptions(case['iou_thr'], case['skip_thr'], conf_type, case['top_n'])
    s, l, b, count = (t.cpu().numpy() for t in ops.fuse_detections(views, case['weights'], case['flips'], case['muls'], opt))
    B, N = len(case['views'][0][3]), len(views) * case['top_n']
    assert s.shape == (B, N) and l.shape == (B, N) and b.shape == (B, N, 4) and count.shape == (B,) and l.dtype == np.int64
    for i, run in enumerate(_reference(case['name'])):
        rs, rl, rb = R.emit(run, conf_type)
        n = len(rs)
        assert int(count[i]) == n, (i, int(count[i]), n)
        assert np.array_equal(l[i, :n], rl), i
        assert np.array_equal(_bits(s[i, :n]), _bits(rs)), (i, np.abs(s[i, :n] - rs).max())
        assert np.array_equal(_bits(b[i, :n]), _bits(rb)), (i, np.abs(b[i, :n] - rb).max())
        assert not _bits(s[i, n:]).any() and not l[i, n:].any() and not _bits(b[i, n:]).any()      # rows past the count: zeros
        assert np.all(s[i, :n][:-1] >= s[i, :n][1:])                                               # emitted scores never increase


def test_out_of_limit_arguments_return_the_documented_codes_and_launch_nothing():
    from efficientdet.pytorch_amd import _lib as L
    lib = L.require('effdet_wbf', 'effdet_wbf_workspace_bytes')
    EINVAL, EUNSUPPORTED = -1, -3
    B, A, V, top_n = 2, 64, 2, 32
    score = [torch.rand(B, A, device='cuda') for _ in range(V)]
    label = [torch.zeros(B, A, dtype=torch.int64, device='cuda') for _ in range(V)]
    boxes = [torch.rand(B, A, 4, device='cuda') + torch.tensor([0.0, 0.0, 1.0, 1.0], device='cuda') for _ in range(V)]
    count = [torch.full((B,), A, dtype=torch.int32, device='cuda') for _ in range(V)]
    N = 8 * 512                                                             # room for the largest valid call below
    os_ = torch.full((B, N), -7.0, device='cuda'); ol = torch.full((B, N), -7, dtype=torch.int64, device='cuda')
    ob = torch.full((B, N, 4), -7.0, device='cuda'); oc = torch.full((B,), -7, dtype=torch.int32, device='cuda')
    nbytes = int(lib.effdet_wbf_workspace_bytes(B, V, top_n))
    assert nbytes >= 0
    ws = torch.zeros(max(nbytes, 1), dtype=torch.uint8, device='cuda')

    def call(views=V, nb=nbytes, **kw):
        d = L.Wbf()
        for v in range(min(views, 8)):
            u = v % V
            d.score[v], d.label[v], d.boxes[v], d.count[v], d.A[v] = L.ptr(score[u]), L.ptr(label[u]), L.ptr(boxes[u]), L.ptr(count[u]), A
            d.weight[v], d.mul[v], d.flip[v], d.width[v] = 1.0, 1.0, 0, 0.0
        d.V, d.B, d.top_n, d.conf_type, d.iou_thr, d.skip_thr = views, B, top_n, 0, 0.55, 0.0
        d.out_score, d.out_label, d.out_boxes, d.out_count = L.ptr(os_), L.ptr(ol), L.ptr(ob), L.ptr(oc)
        for k, val in kw.items():
            if isinstance(val, tuple):
                getattr(d, k)[val[0]] = val[1]
            else:
                setattr(d, k, val)
        return lib.effdet_wbf(C.byref(d), L.ptr(ws), nb, L.stream_ptr())
    nan, inf = float('nan'), float('inf')
    for kw in (dict(views=0), dict(views=9), dict(top_n=0), dict(top_n=-1), dict(top_n=2049), dict(views=8, top_n=513), dict(conf_type=2),
               dict(conf_type=-1), dict(iou_thr=-0.5), dict(iou_thr=1.5), dict(iou_thr=nan), dict(skip_thr=nan), dict(weight=(1, 0.0)),
               dict(weight=(0, -1.0)), dict(weight=(1, nan)), dict(weight=(0, inf)), dict(mul=(1, 0.0)), dict(mul=(0, nan)), dict(mul=(1, inf)),
               dict(flip=(1, 1), width=(1, inf)), dict(flip=(0, 1), width=(0, nan))):
        assert call(**kw) == EUNSUPPORTED, kw
    for kw in (dict(score=(1, None)), dict(label=(0, None)), dict(boxes=(1, None)), dict(count=(0, None)), dict(A=(1, 0)),
               dict(boxes=(0, L.ptr(boxes[0]) + 4)), dict(out_score=None), dict(out_label=None), dict(out_boxes=None), dict(out_count=None),
               dict(out_boxes=L.ptr(ob) + 8), dict(B=0), dict(nb=-1)):
        assert call(**kw) == EINVAL, kw
    assert lib.effdet_wbf(None, L.ptr(ws), nbytes, L.stream_ptr()) == EINVAL
    torch.cuda.synchronize()
    assert bool((os_ == -7.0).all()) and bool((ol == -7).all()) and bool((ob == -7.0).all()) and bool((oc == -7).all())      # nothing was launched
    assert call() == 0 and call(views=8, top_n=512) == 0 and call(views=1, top_n=4096, conf_type=1) == 0
    assert call(flip=(1, 1), width=(1, 512.0), mul=(0, 2.0), weight=(1, 0.5), skip_thr=inf) == 0
    torch.cuda.synchronize()
    assert bool((oc >= 0).all())


def test_python_wrapper_refuses_bad_views():
    from efficientdet.pytorch_amd import ops
    s = torch.rand(1, 8, device='cuda'); l = torch.zeros(1, 8, dtype=torch.int64, device='cuda')
    b = torch.rand(1, 8, 4, device='cuda'); c = torch.full((1,), 8, dtype=torch.int32, device='cuda')
    v = (s, l, b, c)
    for bad in (dict(views=[]), dict(views=[v] * 9), dict(views=[v, v], weights=[1.0]), dict(views=[v], weights=[0.0]), dict(views=[v], muls=[0.0]),
                dict(views=[v, v], flips=[None]), dict(views=[v] * 5, options=ops.WBFOptions(top_n=1000)), dict(views=[(s, l, b[:, :4], c[:0])])):
        with pytest.raises(ValueError):
            ops.fuse_detections(**bad)
    with pytest.raises(TypeError):
        ops.fuse_detections([(s, l.int(), b, c)])
