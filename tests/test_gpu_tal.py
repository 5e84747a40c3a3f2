"""GPU parity of the task-aligned matcher (include/effdet_tal.h, csrc/loss.hip) on the cases of tests/tal_cases.py.

Metrics: ops.loss_tal_metrics against the float64 restatement (tests/tal_restated.py); the yardstick is the float32 NumPy evaluation of
the same lines, and the device's largest error may be METRIC_FACTOR = 4 times the yardstick's largest (the transcendentals differ by a
few ulp, and beta multiplies log2's error).  `pytest -s` prints the ratio per case.
Selection: exact.  The keys in the workspace carry the metrics plane's bits; the integer-only restatement, fed the device's own planes,
reproduces the keys, the codes of all B A anchors and num_pos; and the codes equal the float64 restatement's on every case
(tests/test_tal_host.py proves the gap condition that makes this a fair demand).
Aligned target: bit for bit the float32 evaluation of (m umax) / (mmax + 1e-9f) from the device's bits; without it q is
include/effdet_quality_loss.h's on the matcher's codes, under tests/test_gpu_quality_loss.py's rule for q.
Downstream: losses, d(logit), d(reg) against the restatements run on the device's codes and targets, with the rules of
tests/test_gpu_atss.py / tests/test_gpu_quality_loss.py (assert_close at 2e-4; FACTOR times the float32 run's deviation from float64).
Layouts, determinism and the garbage workspace are bit for bit."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import loss_cases as LC
from tests import loss_options_restated as R
from tests import quality_loss_restated as QR
from tests import tal_cases as TC
from tests import tal_restated as TR
from tests.gpu_util import assert_close
from tests.test_gpu_atss import FACTOR, GS, _same_values
from tests.test_gpu_quality_loss import FACTOR as Q_FACTOR

pytestmark = pytest.mark.gpu

METRIC_FACTOR = 4.0
EINVAL = -1
QUALITY = {'focal': None, 'qfl': dict(kind='qfl'), 'vfl': dict(kind='vfl')}
BOXES = {'smooth_l1': None, 'giou': ('giou', 2.0)}
DOWNSTREAM = [(name, qn, bn) for name in ('s128_nc4', 'n70') for qn in QUALITY for bn in BOXES] + \
    [('s128_nc80', 'qfl', 'giou'), ('dup', 'vfl', 'smooth_l1'), ('bad_label', 'focal', 'giou')]


@functools.lru_cache(maxsize=None)
def _device_case(name):
    c = TC.get(name)
    return tuple(c[k].cuda() for k in ('cls', 'reg', 'anc', 'ann'))


def _matcher(name, **kw):
    from efficientdet.pytorch_amd import ops
    return ops.TaskAlignedOptions(**dict(TC.get(name)['tal'], **kw))


def _qopt(qn):
    from efficientdet.pytorch_amd import ops
    return None if QUALITY[qn] is None else ops.QualityLossOptions(**QUALITY[qn])


def _box(bn):
    from efficientdet.pytorch_amd import ops
    return None if BOXES[bn] is None else ops.BoxLossOptions(*BOXES[bn])


def _gs(a=GS[0], b=GS[1]):
    return torch.tensor([a, b], dtype=torch.float32).cuda()


def _al(n):
    return (n + 255) // 256 * 256


def _codes(ws, B, A):
    return ws[:B * A * 4].view(torch.int32).reshape(B, A).cpu().long()


def _num_pos(ws, B, A):
    off = _al(4 * B * A)
    return ws[off:off + B * 128].view(torch.int32).reshape(B, 32)[:, 2].cpu().long()


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _ratio(got, f32, ref):
    return float((got.double().cpu() - ref).abs().max()), float((f32.double() - ref).abs().max())


@functools.lru_cache(maxsize=None)
def _forward(name, qn='qfl', bn='smooth_l1', aligned=True):
    """One forward call of the case -> (losses, ws, codes, device m plane, device u plane); shared, read-only."""
    from efficientdet.pytorch_amd import ops
    cls, reg, anc, ann = _device_case(name)
    B, A, _ = cls.shape
    m = _matcher(name, aligned_target=aligned)
    losses, ws = ops.loss_opts_fwd(cls, reg, anc, ann, box=_box(bn), matcher=m, quality=_qopt(qn))
    dm, du = ops.loss_tal_metrics(cls, reg, anc, ann, m)
    return losses, ws, _codes(ws, B, A), dm, du


@pytest.mark.parametrize('name', sorted(TC.CASES))
def test_metrics_against_float64(name):
    c = TC.get(name)
    _, _, _, dm, du = _forward(name)
    ref_m, ref_u = TC.reference(name)['m'], TC.reference(name)['u']
    m32, u32 = TR.metrics(c, c['tal'], np.float32)
    for what, got, f32, ref in (('m', dm, m32, ref_m), ('u', du, u32, ref_u)):
        got = got.cpu().numpy()
        assert got.shape == ref.shape and np.isfinite(got).all()
        err, yard = float(np.abs(got.astype(np.float64) - ref).max()), float(np.abs(f32.astype(np.float64) - ref).max())
        print('\n%s %s: max %.3g device err %.3g yardstick %.3g ratio %.2f' % (name, what, float(ref.max()), err, yard, err / max(yard, 1e-300)))
        assert err <= METRIC_FACTOR * yard, (name, what, err, yard)
        assert np.array_equal(got != 0, f32 != 0)                                            # exact 0 off the inside set, on pad / bad-label rows
    assert float(du.min()) >= 0.0 and float(du.max()) <= 1.0


@pytest.mark.parametrize('name', sorted(TC.CASES))
def test_selection_codes_and_aligned_target_exactly(name):
    from efficientdet.pytorch_amd import ops
    c, ref = TC.get(name), TC.reference(name)
    cls, reg, anc, ann = _device_case(name)
    B, A, nc = cls.shape
    N = ann.shape[1]
    topk = c['tal']['topk']
    losses, ws, codes, dm, du = _forward(name)
    keys, mm = ops.loss_tal_candidates(ws, B, A, N)
    keys, mm = keys.cpu().numpy().view(np.uint64), mm.cpu().numpy()
    q = ops.loss_quality_targets(ws, B, A, N, matcher=_matcher(name)).cpu().numpy()
    mb, ub = _u32(dm), _u32(du)
    for b in range(B):
        rows = TR.valid_rows(c, b)
        if not rows:
            assert bool((codes[b] == LC.CODE_IGN).all()) and int((keys[b] != TR.NO_KEY).sum()) == 0 and not q[b].any() and not mm[b].any()
            continue
        want_keys, want_codes = TR.assign_bits(mb[b], ub[b], rows, topk)
        for n in range(N):
            got = [int(k) for k in keys[b, n]]
            w = want_keys.get(n, [])
            assert got == w + [TR.NO_KEY] * (TR.MAX_TOPK - len(w)), (name, b, n)             # rank order, count-padded with the no-key value
            for k in w:
                assert (~(k >> 32)) & 0xFFFFFFFF == int(mb[b, n, k & 0xFFFFFFFF])           # the key carries the metrics plane's bits
            assert [k & 0xFFFFFFFF for k in w] == ref['winners'].get((b, n), []), (name, b, n)
        assert np.array_equal(codes[b].numpy(), want_codes), name                           # all A anchors, from the device's own bits
        want_q, want_mm = TR.target(mb[b], ub[b], want_codes, want_keys)
        assert np.array_equal(q[b].view(np.uint32), want_q.view(np.uint32)), name            # bit for bit; +0.0 elsewhere
        for n in range(N):
            assert tuple(mm[b, n].tolist()) == tuple(float(v) for v in want_mm.get(n, (0.0, 0.0))), (name, b, n)
    assert torch.equal(codes, ref['codes']), torch.nonzero(codes != ref['codes'])[:4].tolist()      # end to end: the float64 codes
    assert torch.equal(_num_pos(ws, B, A), ref['num_pos'])
    if name == 'hand':
        assert {int(a): int(codes[0, a]) for a in torch.nonzero(codes[0] >= 0).reshape(-1)} == TC.HAND_CODES
        assert {int(a): float(q[0, a]) for a in np.nonzero(q[0])[0]} == TC.HAND_Q


@pytest.mark.parametrize('name', ['s128_nc4', 'nested', 'few'])
def test_without_the_aligned_target_q_is_the_quality_losss(name):
    from efficientdet.pytorch_amd import ops
    c = TC.get(name)
    cls, reg, anc, ann = _device_case(name)
    B, A, _ = cls.shape
    N = ann.shape[1]
    _, ws1, codes1, _, _ = _forward(name)
    losses, ws, codes, _, _ = _forward(name, aligned=False)
    assert torch.equal(codes, codes1)                                                        # the assignment does not depend on it
    q = ops.loss_quality_targets(ws, B, A, N, matcher=_matcher(name)).cpu()
    ref, f32 = QR.quality(c, codes, torch.float64), QR.quality(c, codes, torch.float32)
    err, yard = _ratio(q, f32, ref)
    print('\n%s: q err %.3g yardstick %.3g ratio %.2f' % (name, err, yard, err / max(yard, 1e-300)))
    assert yard > 0.0 and err <= Q_FACTOR * yard
    assert int(_bits(q)[codes < 0].abs().max()) == 0 and torch.equal(q == 0, ref == 0)
    _, mm = ops.loss_tal_candidates(ws, B, A, N)
    assert not bool(mm.any())                                                                # no target pass ran
    q1 = ops.loss_quality_targets(ws1, B, A, N, matcher=_matcher(name)).cpu()
    assert not torch.equal(q1, q) and torch.equal(q1 == 0, q == 0)


@pytest.mark.parametrize('run', DOWNSTREAM, ids=lambda r: '%s-%s-%s' % r)
def test_losses_and_gradients_on_the_device_codes_and_targets(run):
    from efficientdet.pytorch_amd import ops
    name, qn, bn = run
    c = TC.get(name)
    cls, reg, anc, ann = _device_case(name)
    B, A, nc = cls.shape
    N = ann.shape[1]
    m, quality, box = _matcher(name), _qopt(qn), _box(bn)
    losses, ws, codes, _, _ = _forward(name, qn, bn)
    q = ops.loss_quality_targets(ws, B, A, N, matcher=m).cpu() if quality is not None else None
    qo = None if quality is None else QR.options(**QUALITY[qn])
    ref = TR.downstream(c, codes, q, R.options(), qo, BOXES[bn], GS, torch.float64)
    f32 = TR.downstream(c, codes, q, R.options(), qo, BOXES[bn], GS, torch.float32)
    assert_close(losses.cpu(), ref['losses'], 2e-4, '%s %s %s losses' % run)
    dcls = ops.loss_opts_bwd_cls(cls, ann, _gs(), ws, torch.float32, None, matcher=m, quality=quality)
    dreg = ops.loss_opts_bwd_reg(reg, anc, ann, _gs(), ws, torch.float32, box=box, matcher=m, quality=quality)
    err_c, yard_c = _ratio(dcls, f32['dlogit'], ref['dlogit'])
    err_r, yard_r = _ratio(dreg, f32['dreg'], ref['dreg'])
    print('\n%s %s %s: losses %.9g %.9g (float64 %.9g %.9g) num_pos %s | dlogit err %.3g yardstick %.3g ratio %.2f | dreg err %.3g '
          'yardstick %.3g ratio %.2f' % (name, qn, bn, float(losses[0]), float(losses[1]), float(ref['losses'][0]), float(ref['losses'][1]),
                                         ref['num_pos'].tolist(), err_c, yard_c, err_c / max(yard_c, 1e-300), err_r, yard_r,
                                         err_r / max(yard_r, 1e-300)))
    assert yard_c > 0.0 and err_c <= FACTOR * yard_c, (run, 'dlogit', err_c, yard_c)
    assert err_r <= FACTOR * yard_r, (run, 'dreg', err_r, yard_r)
    assert int(_bits(dreg.cpu())[codes < 0].abs().max()) == 0                                # exact +0.0 away from the positives
    assert bool(torch.isfinite(dcls).all())
    # the one-pass training call: the same codes, targets and losses[1]; d(logit) at an upstream gradient of one; d(reg) from its workspace
    dld = LC.dld_for(nc)
    l2, ws2, dpix = ops.loss_opts_fwd_grad(cls, reg, anc, ann, torch.float32, dld, box=box, matcher=m, quality=quality)
    assert torch.equal(ws2[:B * A * 4], ws[:B * A * 4]) and torch.equal(_bits(l2[1:2]), _bits(losses[1:2]))
    assert_close(l2.cpu(), ref['losses'], 2e-4, '%s %s %s fwd_grad losses' % run)
    one = ops.loss_opts_bwd_cls(cls, ann, _gs(1.0, 1.0), ws, torch.float32, None, matcher=m, quality=quality)
    assert torch.equal(_bits(dpix[:, :, :9 * nc].reshape(B, A, nc)), _bits(one)) and int(_bits(dpix[:, :, 9 * nc:]).abs().max()) == 0
    assert torch.equal(_bits(ops.loss_opts_bwd_reg(reg, anc, ann, _gs(), ws2, torch.float32, box=box, matcher=m, quality=quality)), _bits(dreg))
    if quality is not None:
        assert torch.equal(_bits(ops.loss_quality_targets(ws2, B, A, N, matcher=m)), _bits(q.cuda()))


@pytest.mark.parametrize('name', ['n70', 's128_nc80'])
def test_output_layouts(name):
    from efficientdet.pytorch_amd import ops
    cls, reg, anc, ann = _device_case(name)
    B, A, nc = cls.shape
    kw = dict(matcher=_matcher(name), quality=_qopt('qfl'), box=_box('giou'))
    bkw = dict(matcher=kw['matcher'], quality=kw['quality'])
    dld = LC.dld_for(nc)
    _, ws, pix = ops.loss_opts_fwd_grad(cls, reg, anc, ann, torch.float32, dld, **kw)
    _, _, pix_bf16 = ops.loss_opts_fwd_grad(cls, reg, anc, ann, torch.bfloat16, dld, **kw)
    _, _, split = ops.loss_opts_fwd_grad(cls, reg, anc, ann, torch.float32, dld, split=True, **kw)
    one = _gs(1.0, 1.0)
    bwd_cls = functools.partial(ops.loss_opts_bwd_cls, cls, ann, loss=None, **bkw)
    rows = bwd_cls(one, ws, torch.float32)
    _same_values(rows, pix, pix_bf16, bwd_cls(one, ws, torch.bfloat16), split, B, A, nc, dld)
    assert float(rows.abs().max()) > 0.0
    fn = functools.partial(ops.loss_opts_bwd_reg, reg, anc, ann, _gs(), ws, box=kw['box'], **bkw)
    rows = fn(torch.float32)
    _same_values(rows, fn(torch.float32, reg_ld=64), fn(torch.bfloat16, reg_ld=64), fn(torch.bfloat16), fn(torch.float32, reg_ld=64, split=True),
                 B, A, 4, 64)
    assert float(rows.abs().max()) > 0.0


def _raw(name, ws, losses, tal=None, quality='qfl', low_quality=0, null=False, dpix=None, nbytes=None):
    from efficientdet.pytorch_amd import _lib as L
    cls, reg, anc, ann = _device_case(name)
    B, A, nc = cls.shape
    N = ann.shape[1]
    t = L.Tal(**dict(dict(topk=13, alpha=1.0, beta=6.0, aligned_target=1), **(tal or {})))
    d = R.DEFAULTS
    o = L.LossOpts(d['alpha'], d['gamma'], d['label_smoothing'], d['beta'], d['reg_weight'], d['pos_iou'], d['neg_iou'], low_quality, 0, 1.0)
    q = None if quality is None else ctypes.byref(L.QualityLoss(**dict(dict(kind=1, beta=2.0, alpha=0.75, gamma=2.0), **(quality if isinstance(quality, dict) else {}))))
    lib = L.require('effdet_loss_tal_fwd', 'effdet_loss_tal_fwd_grad')
    at = None if null else ctypes.byref(t)
    nbytes = ws.numel() if nbytes is None else nbytes
    if dpix is None:
        return lib.effdet_loss_tal_fwd(L.ptr(cls), L.ptr(reg), L.ptr(anc), L.ptr(ann), L.ptr(losses), L.ptr(ws), nbytes, B, A, nc, N,
                                       ctypes.byref(o), at, q, L.stream_ptr())
    return lib.effdet_loss_tal_fwd_grad(L.ptr(cls), L.ptr(reg), L.ptr(anc), L.ptr(ann), L.ptr(losses), L.ptr(ws), nbytes, L.ptr(dpix),
                                        dpix.shape[2], L.F32, B, A, nc, N, ctypes.byref(o), at, q, L.stream_ptr())


def _views(ws, B, A, N):
    from efficientdet.pytorch_amd import ops
    m = ops.TaskAlignedOptions()
    keys, mm = ops.loss_tal_candidates(ws, B, A, N)
    return [ws[:B * A * 4].view(torch.int32), _num_pos(ws, B, A), ops.loss_quality_targets(ws, B, A, N, matcher=m), keys, mm]


@pytest.mark.parametrize('name', ['n70', 's128_nc4'])
def test_two_runs_and_a_garbage_workspace_are_bitwise_equal(name):
    from efficientdet.pytorch_amd import ops
    cls, reg, anc, ann = _device_case(name)
    B, A, nc = cls.shape
    N = ann.shape[1]
    kw = dict(matcher=_matcher(name), quality=_qopt('qfl'))
    runs = []
    for _ in range(2):
        losses, ws, dpix = ops.loss_opts_fwd_grad(cls, reg, anc, ann, torch.float32, LC.dld_for(nc), **kw)
        runs.append([losses.clone(), dpix, ops.loss_opts_bwd_reg(reg, anc, ann, _gs(), ws, torch.float32, **kw)] +
                    [v.clone() for v in _views(ws, B, A, N)])
    for a, b in zip(*runs):
        assert torch.equal(a, b) if a.dtype in (torch.int32, torch.int64) else torch.equal(_bits(a), _bits(b))
    ws = torch.full((ws.numel(),), 0xFF, dtype=torch.uint8, device=cls.device)
    losses = torch.empty(2, device=cls.device)
    dpix = torch.empty_like(runs[0][1])
    assert TC.get(name)['tal'] == TR.DEFAULTS and _raw(name, ws, losses, dpix=dpix) == 0
    dreg = ops.loss_opts_bwd_reg(reg, anc, ann, _gs(), ws, torch.float32, **kw)
    for a, b in zip(runs[0], [losses, dpix, dreg] + _views(ws, B, A, N)):
        assert torch.equal(a, b) if a.dtype in (torch.int32, torch.int64) else torch.equal(_bits(a), _bits(b))


def test_error_codes_and_nothing_enqueued():
    from efficientdet.pytorch_amd import _lib as L
    name = 's128_nc4'
    cls, reg, anc, ann = _device_case(name)
    B, A, nc = cls.shape
    N = ann.shape[1]
    t = L.Tal(13, 1.0, 6.0, 1)
    lib = L.require('effdet_loss_tal_workspace_bytes', 'effdet_loss_tal_metrics')
    nbytes = int(lib.effdet_loss_tal_workspace_bytes(B, A, nc, N, ctypes.byref(t)))
    assert nbytes > int(lib.effdet_loss_quality_workspace_bytes(B, A, nc, N, None))
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=cls.device)
    losses = torch.full((2,), 7.0, device=cls.device)
    dpix = torch.full((B, A // 9, LC.dld_for(nc)), 7.0, device=cls.device)
    out = torch.full((2, B, N, A), 7.0, device=cls.device)
    nan = float('nan')
    bad = [dict(tal=dict(topk=0)), dict(tal=dict(topk=17)), dict(tal=dict(alpha=nan)), dict(tal=dict(beta=nan)), dict(tal=dict(alpha=4.5)),
           dict(tal=dict(beta=-1.0)), dict(tal=dict(aligned_target=2)), dict(null=True), dict(low_quality=1), dict(quality=dict(kind=3)),
           dict(quality=dict(beta=nan)), dict(nbytes=nbytes - 1), dict(nbytes=int(lib.effdet_loss_quality_workspace_bytes(B, A, nc, N, None)))]
    for kw in bad:
        for quality in ((kw['quality'],) if 'quality' in kw else ('qfl', None)):
            k = dict(kw, quality=quality)
            assert _raw(name, ws, losses, **k) == EINVAL, k
            assert _raw(name, ws, losses, dpix=dpix, **k) == EINVAL, k
    for kw in (dict(topk=0), dict(topk=17), dict(alpha=nan)):
        tt = L.Tal(**dict(dict(topk=13, alpha=1.0, beta=6.0, aligned_target=1), **kw))
        assert lib.effdet_loss_tal_metrics(L.ptr(cls), L.ptr(reg), L.ptr(anc), L.ptr(ann), L.ptr(out), B, A, nc, N, ctypes.byref(tt),
                                           L.stream_ptr()) == EINVAL
    assert lib.effdet_loss_tal_metrics(L.ptr(cls), L.ptr(reg), L.ptr(anc), L.ptr(ann), L.ptr(out), B, A, nc, N, None, L.stream_ptr()) == EINVAL
    torch.cuda.synchronize()
    assert bool((losses == 7.0).all()) and bool((dpix == 7.0).all()) and bool((out == 7.0).all()) and int(ws.max()) == 0      # no kernel ran
    assert _raw(name, ws, losses, dpix=dpix) == 0
    torch.cuda.synchronize()
    assert not bool((losses == 7.0).any()) and not bool((dpix == 7.0).any())
    assert torch.equal(_codes(ws, B, A), TC.reference(name)['codes'])
