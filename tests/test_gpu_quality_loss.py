"""GPU parity of the IoU-aware class losses (include/effdet_quality_loss.h, csrc/loss.hip) on the runs of tests/quality_loss_cases.py
against the float64 restatement (tests/quality_loss_restated.py).

Assignment, num_pos, losses[1], d(reg): torch.equal to the same call without the quality loss (the same options struct through the
effdet_loss_opts_* / effdet_loss_atss_* kernels), d(reg) in its three layouts; the codes also equal the restatement's.
q: the rule tests/test_gpu_box_loss.py applies to the same IoU expression -- the device may deviate from float64 by FACTOR = 8 times the
largest deviation of the float32 evaluation of the same restatement.
losses[0]: the rule of tests/test_gpu_loss_options.py, assert_close at 2e-4.
d(logit): that file's gradient rule with its FACTOR and upstream gradients GS = (0.7, 1.3), on the fp32 outputs (flat, pixel-major with
the padded pitch 64 for 36 channels, and the one-pass kernel's); the bf16 and split outputs are those values rounded, bit for bit.
Nothing is excluded from a comparison (tests/test_quality_loss_host.py proves the margins).  `pytest -s` prints the achieved figures."""
import ctypes
import functools

import pytest
import torch

from tests import loss_cases as LC
from tests import quality_loss_cases as QC
from tests.gpu_util import assert_close

pytestmark = pytest.mark.gpu

FACTOR = 8.0
GS = QC.GS
EINVAL = -1


@functools.lru_cache(maxsize=None)
def _device_case(name):
    c = QC.get(name)
    return tuple(c[k].cuda() for k in ('cls', 'reg', 'anc', 'ann'))


def _kw(name, on, box):
    """The Python options of a run -> (keyword arguments of the forward calls, of the d(reg) call, of the class backward)."""
    from efficientdet.pytorch_amd import ops
    c = QC.get(name)
    loss = ops.LossOptions(**QC.OPTS[on]) if QC.OPTS[on] else None
    bx = None if box is None else ops.BoxLossOptions(*box)
    if QC.is_atss(c):
        m = ops.ATSSOptions(c['topk'])
        return dict(loss=loss, box=bx, matcher=m, levels=[b - a for a, b in zip(c['level_start'][:-1], c['level_start'][1:])]), \
            dict(loss=loss, box=bx, matcher=m), dict(matcher=m)
    return dict(loss=loss, box=bx), dict(loss=loss, box=bx), dict()


def _qopt(qn):
    from efficientdet.pytorch_amd import ops
    return ops.QualityLossOptions(**QC.QUALITY[qn])


def _gs(a=GS[0], b=GS[1]):
    return torch.tensor([a, b], dtype=torch.float32).cuda()


def _al(n):
    return (n + 255) // 256 * 256


def _codes(ws, B, A):
    return ws[:B * A * 4].view(torch.int32).reshape(B, A).cpu().long()


def _num_pos(ws, B, A):
    """stat[b][2] of the workspace: the integer count of positives."""
    off = _al(4 * B * A)
    return ws[off:off + B * 128].view(torch.int32).reshape(B, 32)[:, 2].cpu().long()


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _unpix(dpix, B, A, nc):
    return dpix[:, :, :9 * nc].reshape(B, A, nc)


def _split_halves(t):
    B, P, ld = t.shape
    h = t.contiguous().view(torch.bfloat16).reshape(B, P, ld // 32, 2, 32)
    return h[:, :, :, 0].reshape(B, P, ld), h[:, :, :, 1].reshape(B, P, ld)


def _ratio(got, f32, ref):
    return float((got.double().cpu() - ref).abs().max()), float((f32.double() - ref).abs().max())


def _plain_twin(name, on, box):
    """The same options WITHOUT the quality loss through the option kernels -> (losses, ws, d(reg) call).  Where the Python surface
    would take the reference's own entry points (no LossOptions, no matcher), the default VALUES go through effdet_loss_opts_* by
    hand: that is the call the quality path is the twin of."""
    from efficientdet.pytorch_amd import _lib as L, ops
    cls, reg, anc, ann = _device_case(name)
    fkw, rkw, _ = _kw(name, on, box)
    if fkw['loss'] is not None or 'matcher' in fkw:
        losses, ws = ops.loss_opts_fwd(cls, reg, anc, ann, **fkw)
        return losses, ws, lambda dtype, **kw: ops.loss_opts_bwd_reg(reg, anc, ann, _gs(), ws, dtype, **dict(rkw, **kw))
    lib = L.require('effdet_loss_opts_fwd', 'effdet_loss_opts_bwd_reg', 'effdet_loss_opts_workspace_bytes')
    B, A, nc = cls.shape
    N = ann.shape[1]
    d = ops.LossOptions()
    kind, weight = ops._box_loss_args(fkw['box']) or (0, 1.0)
    o = L.LossOpts(d.alpha, d.gamma, d.label_smoothing, d.beta, d.reg_weight, d.pos_iou, d.neg_iou, 0, kind, weight)
    nbytes = int(lib.effdet_loss_opts_workspace_bytes(B, A, nc, N))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=cls.device)
    losses = torch.empty(2, device=cls.device)
    assert lib.effdet_loss_opts_fwd(L.ptr(cls), L.ptr(reg), L.ptr(anc), L.ptr(ann), L.ptr(losses), L.ptr(ws), nbytes, B, A, nc, N,
                                    ctypes.byref(o), L.stream_ptr()) == 0

    def bwd_reg(dtype, reg_ld=0, split=False):
        out = torch.empty((B, A // 9, reg_ld) if reg_ld else (B, A, 4), dtype=dtype, device=cls.device)
        gs = _gs()
        assert lib.effdet_loss_opts_bwd_reg(L.ptr(reg), L.ptr(anc), L.ptr(ann), L.ptr(gs), L.ptr(ws), L.ptr(out), reg_ld,
                                            L.F32_SPLIT if split else L.dtype_code(dtype), B, A, N, ctypes.byref(o), L.stream_ptr()) == 0
        return out
    return losses, ws, bwd_reg


@pytest.mark.parametrize('run', QC.RUNS, ids=lambda r: '%s-%s-%s' % r[:3])
def test_assignment_box_term_targets_loss_and_gradient(run):
    from efficientdet.pytorch_amd import ops
    name, on, qn, box = run
    cls, reg, anc, ann = _device_case(name)
    B, A, nc = cls.shape
    N = ann.shape[1]
    ref, f32 = QC.reference(name, on, qn, box)
    fkw, rkw, ckw = _kw(name, on, box)
    q = _qopt(qn)
    losses, ws = ops.loss_opts_fwd(cls, reg, anc, ann, quality=q, **fkw)
    # ---- the assignment and the box term are the twin's, bit for bit
    codes = _codes(ws, B, A)
    assert torch.equal(codes, ref['codes']), torch.nonzero(codes != ref['codes'])[:4].tolist()
    pl, pws, p_bwd_reg = _plain_twin(name, on, box)
    assert torch.equal(ws[:B * A * 4], pws[:B * A * 4]) and torch.equal(_num_pos(ws, B, A), _num_pos(pws, B, A))
    assert torch.equal(_num_pos(ws, B, A), ref['num_pos'])
    assert torch.equal(_bits(losses[1:2]), _bits(pl[1:2])) and not torch.equal(_bits(losses[0:1]), _bits(pl[0:1]))
    layouts = [dict(), dict(reg_ld=64), dict(reg_ld=64, split=True)] if A % 9 == 0 else [dict()]
    for kw in layouts:
        got = ops.loss_opts_bwd_reg(reg, anc, ann, _gs(), ws, torch.float32, quality=q, **dict(rkw, **kw))
        assert torch.equal(_bits(got), _bits(p_bwd_reg(torch.float32, **kw))), kw
    # ---- q against float64
    qd = ops.loss_quality_targets(ws, B, A, N, matcher=fkw.get('matcher'))
    err_q, yard_q = _ratio(qd, f32['q'], ref['q'])
    assert int(_bits(qd.cpu())[ref['codes'] < 0].abs().max()) == 0                     # exact +0.0 off the positives
    assert torch.equal(qd.cpu() == 0, ref['q'] == 0)                                   # ... and the q == 0 positives are the restatement's
    assert float(qd.min()) >= 0.0 and float(qd.max()) <= 1.0
    # ---- losses
    assert_close(losses.cpu(), ref['losses'], 2e-4, '%s %s %s losses' % run[:3])
    # ---- d(logit), flat
    dcls = ops.loss_opts_bwd_cls(cls, ann, _gs(), ws, torch.float32, fkw['loss'], quality=q, **ckw)
    err_c, yard_c = _ratio(dcls, f32['dlogit'], ref['dlogit'])
    print('\n%s %s %s %s: losses %.9g %.9g (float64 %.9g %.9g) | q err %.3g yardstick %.3g ratio %.2f | dlogit max %.3g err %.3g yardstick '
          '%.3g ratio %.2f' % (name, on, qn, box, float(losses[0]), float(losses[1]), float(ref['losses'][0]), float(ref['losses'][1]),
                               err_q, yard_q, err_q / max(yard_q, 1e-300), float(ref['dlogit'].abs().max()), err_c, yard_c,
                               err_c / max(yard_c, 1e-300)))
    assert yard_q > 0.0 and err_q <= FACTOR * yard_q, (run, 'q', err_q, yard_q)
    assert yard_c > 0.0 and err_c <= FACTOR * yard_c, (run, 'dlogit', err_c, yard_c)
    got_c = dcls.cpu()
    assert bool(torch.isfinite(got_c).all())
    ign = ref['codes'] == LC.CODE_IGN
    if bool(ign.any()):
        assert int(_bits(got_c)[ign].abs().max()) == 0
    assert torch.equal(_bits(ops.loss_opts_bwd_cls(cls, ann, _gs(), ws, torch.bfloat16, fkw['loss'], quality=q, **ckw)), _bits(dcls.bfloat16()))
    if nc % 4:
        return
    # ---- pixel-major with the padded pitch: the class backward (F32, BF16) and the one-pass forward + gradient (F32, BF16, F32_SPLIT)
    dld = LC.dld_for(nc)
    assert dld == 64 and 9 * nc == 36
    want = torch.zeros(B, A // 9, dld, dtype=torch.float32, device=cls.device)
    want[:, :, :9 * nc] = dcls.reshape(B, A // 9, 9 * nc)
    pix = ops.loss_opts_bwd_cls(cls, ann, _gs(), ws, torch.float32, fkw['loss'], dld=dld, quality=q, **ckw)
    assert torch.equal(_bits(pix), _bits(want)) and int(_bits(pix[:, :, 9 * nc:]).abs().max()) == 0
    assert torch.equal(_bits(ops.loss_opts_bwd_cls(cls, ann, _gs(), ws, torch.bfloat16, fkw['loss'], dld=dld, quality=q, **ckw)),
                       _bits(want.bfloat16()))
    l2, ws2, one_pix = ops.loss_opts_fwd_grad(cls, reg, anc, ann, torch.float32, dld, quality=q, **fkw)
    assert torch.equal(ws2[:B * A * 4], ws[:B * A * 4]) and torch.equal(_bits(l2[1:2]), _bits(losses[1:2]))
    assert torch.equal(_bits(ops.loss_quality_targets(ws2, B, A, N)), _bits(qd))
    assert_close(l2.cpu(), ref['losses'], 2e-4, '%s %s %s fwd_grad losses' % run[:3])
    one = ops.loss_opts_bwd_cls(cls, ann, _gs(1.0, 1.0), ws, torch.float32, fkw['loss'], quality=q, **ckw)
    assert torch.equal(_bits(_unpix(one_pix, B, A, nc)), _bits(one)) and int(_bits(one_pix[:, :, 9 * nc:]).abs().max()) == 0
    err_1, yard_1 = _ratio(_unpix(one_pix, B, A, nc) * GS[0], f32['dlogit'], ref['dlogit'])      # fwd_grad, then the scaling
    assert err_1 <= FACTOR * yard_1, (run, 'fwd_grad dlogit', err_1, yard_1)
    _, _, bf_pix = ops.loss_opts_fwd_grad(cls, reg, anc, ann, torch.bfloat16, dld, quality=q, **fkw)
    _, _, split = ops.loss_opts_fwd_grad(cls, reg, anc, ann, torch.float32, dld, split=True, quality=q, **fkw)
    assert torch.equal(_bits(bf_pix), _bits(one_pix.bfloat16()))
    hi, lo = _split_halves(split)
    assert torch.equal(_bits(hi), _bits(one_pix.bfloat16())) and torch.equal(_bits(lo), _bits((one_pix - one_pix.bfloat16().float()).bfloat16()))
    assert torch.equal(_bits(ops.loss_opts_bwd_reg(reg, anc, ann, _gs(), ws2, torch.float32, quality=q, **rkw)),
                       _bits(p_bwd_reg(torch.float32)))


def test_the_edges_element_by_element():
    """tests/quality_loss_cases.edges on the device: q rounds to 1, q exactly 0 at a positive (the varifocal loss takes the negative
    branch), p == t exactly (loss term and gradient exactly 0 under QFL), the clamp ends, the dw cap."""
    from efficientdet.pytorch_amd import ops
    cls, reg, anc, ann = _device_case('edges')
    B, A, nc = cls.shape
    T, T_CAP, T_OFF = QC.T, QC.T_CAP, QC.T_OFF
    for qn in ('qfl', 'vfl'):
        ref, _ = QC.reference('edges', 'default', qn, None)
        _, ws = ops.loss_opts_fwd(cls, reg, anc, ann, quality=_qopt(qn))
        q = ops.loss_quality_targets(ws, B, A, ann.shape[1]).cpu()
        assert float(q[0, T]) == 1.0 and float(q[0, T_OFF]) == 0.0 and float(q[1, T]) == 0.5 and 0.0 < float(q[0, T_CAP]) < 1.0
        g = ops.loss_opts_bwd_cls(cls, ann, _gs(), ws, torch.float32, None, quality=_qopt(qn)).cpu()
        assert bool(torch.isfinite(g).all())
        assert float(g[0, T, 0]) == 0.0 and float(g[0, T, 1]) == 0.0 and float(g[0, T, 2]) != 0.0 and float(g[0, T, 3]) != 0.0     # outside / on the clamp
        assert float(g[0, T_CAP, 0]) != 0.0 and float(g[0, T_CAP, 1]) != 0.0 and float(g[0, T_CAP, 2]) == 0.0 and float(g[0, T_CAP, 3]) == 0.0
        assert torch.equal(g[0, T_OFF] != 0, ref['dlogit'][0, T_OFF] != 0) and float(g[0, T_OFF, 1]) > 0.0      # pushed DOWN: a negative's gradient
        if qn == 'qfl':
            assert float(g[1, T, 2]) == 0.0                                             # p == t: exactly 0, not 0 / 0
        assert int(_bits(g[2]).abs().max()) == 0                                        # the image without a valid row
        assert bool((g[3] > 0).all())                                                   # rows but no positive: every element a negative


@pytest.mark.parametrize('run', [('straddle_lq', 'lq', 'vfl15', ('ciou', 2.0)), ('atss_nested', 'huber', 'qfl', ('giou', 2.0))],
                         ids=lambda r: '%s-%s-%s' % r[:3])
def test_two_runs_are_bitwise_equal(run):
    from efficientdet.pytorch_amd import ops
    name, on, qn, box = run
    cls, reg, anc, ann = _device_case(name)
    B, A, nc = cls.shape
    fkw, rkw, ckw = _kw(name, on, box)
    q = _qopt(qn)
    runs = []
    for _ in range(2):
        losses, ws, dpix = ops.loss_opts_fwd_grad(cls, reg, anc, ann, torch.float32, LC.dld_for(nc), quality=q, **fkw)
        runs.append((losses.clone(), dpix, ops.loss_quality_targets(ws, B, A, ann.shape[1]).clone(),
                     ops.loss_opts_bwd_cls(cls, ann, _gs(), ws, torch.float32, fkw['loss'], quality=q, **ckw),
                     ops.loss_opts_bwd_reg(reg, anc, ann, _gs(), ws, torch.float32, quality=q, **rkw),
                     ws[:B * A * 4].view(torch.float32).clone()))
    for a, b in zip(*runs):
        assert torch.equal(_bits(a), _bits(b))


def test_non_finite_inputs():
    """nan_zero as in the existing kernels: an ignored anchor's gradient is p - p in every form.  A non-finite regression value at a
    positive anchor makes q NaN there and losses[0] non-finite; losses[1] and the other images' gradients do not change."""
    from efficientdet.pytorch_amd import ops
    cls, reg, anc, ann = _device_case('straddle_lq')
    B, A, nc = cls.shape
    fkw, _, _ = _kw('straddle_lq', 'lq', None)
    dld = LC.dld_for(nc)
    for qn in ('qfl', 'vfl'):
        q = _qopt(qn)
        bad = cls.clone()
        bad[1, 7, 2] = float('nan')                                                    # image 1 has no valid row: every anchor ignored
        bad[1, 200, 1] = float('inf')
        losses, ws, pix = ops.loss_opts_fwd_grad(bad, reg, anc, ann, torch.float32, dld, quality=q, **fkw)
        ref, _, pix0 = ops.loss_opts_fwd_grad(cls, reg, anc, ann, torch.float32, dld, quality=q, **fkw)
        assert torch.equal(_bits(losses), _bits(ref)) and bool(torch.isfinite(ref).all())
        for got in (_unpix(pix, B, A, nc), ops.loss_opts_bwd_cls(bad, ann, _gs(), ws, torch.float32, fkw['loss'], quality=q),
                    _unpix(ops.loss_opts_bwd_cls(bad, ann, _gs(), ws, torch.float32, fkw['loss'], dld=dld, quality=q), B, A, nc)):
            nan = torch.isnan(got)
            assert torch.nonzero(nan).tolist() == [[1, 7, 2], [1, 200, 1]]
            assert int(_bits(got[1])[~nan[1]].abs().max()) == 0
        assert torch.equal(_bits(pix[0]), _bits(pix0[0])) and torch.equal(_bits(pix[2]), _bits(pix0[2]))
        # a non-finite r at a positive anchor of image 0
        codes = _codes(ws, B, A)
        a = int(torch.nonzero(codes[0] >= 0)[0])
        for v, k in ((float('nan'), 0), (float('inf'), 2), (float('-inf'), 3)):
            r2 = reg.clone()
            r2[0, a, k] = v
            l2, ws2, pix2 = ops.loss_opts_fwd_grad(cls, r2, anc, ann, torch.float32, dld, quality=q, **fkw)
            qd = ops.loss_quality_targets(ws2, B, A, ann.shape[1])
            assert torch.nonzero(torch.isnan(qd)).tolist() == [[0, a]] and not bool(torch.isfinite(l2[0]))
            assert torch.equal(_bits(pix2[2]), _bits(pix0[2]))


def test_none_is_the_existing_calls_on_the_device():
    from efficientdet.pytorch_amd import ops
    cls, reg, anc, ann = _device_case('straddle')
    nc = cls.shape[2]
    lf, wsf = ops.focal_loss_fwd(cls, reg, anc, ann)
    l, ws = ops.loss_opts_fwd(cls, reg, anc, ann, quality=None)
    assert torch.equal(_bits(l), _bits(lf)) and ws.numel() == wsf.numel()
    lf2, _, df2 = ops.focal_loss_fwd_grad(cls, reg, anc, ann, torch.float32, LC.dld_for(nc))
    l2, _, d2 = ops.loss_opts_fwd_grad(cls, reg, anc, ann, torch.float32, LC.dld_for(nc), quality=None)
    assert torch.equal(_bits(l2), _bits(lf2)) and torch.equal(_bits(d2), _bits(df2))
    opt = ops.LossOptions(gamma=1.5)
    a, wa = ops.loss_opts_fwd(cls, reg, anc, ann, opt)
    b, wb = ops.loss_opts_fwd(cls, reg, anc, ann, opt, quality=None)
    assert torch.equal(_bits(a), _bits(b)) and wa.numel() == wb.numel()


def test_error_codes_and_nothing_enqueued():
    from efficientdet.pytorch_amd import _lib as L
    cls, reg, anc, ann = _device_case('straddle_lq')
    B, A, nc = cls.shape
    N = ann.shape[1]
    lib = L.require('effdet_loss_quality_fwd', 'effdet_loss_quality_fwd_grad', 'effdet_loss_quality_bwd_cls', 'effdet_loss_quality_workspace_bytes')
    nbytes = int(lib.effdet_loss_quality_workspace_bytes(B, A, nc, N, None))
    assert nbytes > int(lib.effdet_loss_opts_workspace_bytes(B, A, nc, N))
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=cls.device)
    losses = torch.full((2,), 7.0, device=cls.device)
    dld = LC.dld_for(nc)
    dpix = torch.full((B, A // 9, dld), 7.0, device=cls.device)
    gs = _gs()
    opts = L.LossOpts(0.25, 2.0, 0.0, 0.1, 50.0, 0.5, 0.4, 1, 0, 1.0)
    atss = L.Atss(9, 2)
    for i, v in enumerate([0, 252, 261]):
        atss.level_start[i] = v
    ref = lambda s: None if s is None else ctypes.byref(s)      # noqa: E731

    def fwd(q, o=opts, t=None, nb=nbytes, n=N):
        return lib.effdet_loss_quality_fwd(L.ptr(cls), L.ptr(reg), L.ptr(anc), L.ptr(ann), L.ptr(losses), L.ptr(ws), nb, B, A, nc, n,
                                           ref(o), ref(t), ref(q), L.stream_ptr())

    def fwd_grad(q, o=opts, t=None, ld=dld, dtype=L.F32):
        return lib.effdet_loss_quality_fwd_grad(L.ptr(cls), L.ptr(reg), L.ptr(anc), L.ptr(ann), L.ptr(losses), L.ptr(ws), nbytes, L.ptr(dpix),
                                                ld, dtype, B, A, nc, N, ref(o), ref(t), ref(q), L.stream_ptr())

    def bwd_cls(q, o=opts, ld=dld, dtype=L.F32, out=dpix):
        return lib.effdet_loss_quality_bwd_cls(L.ptr(cls), L.ptr(ann), L.ptr(gs), L.ptr(ws), L.ptr(out), ld, dtype, B, A, nc, N, ref(o),
                                               ref(q), L.stream_ptr())
    ok = dict(kind=1, beta=2.0, alpha=0.75, gamma=2.0)
    nan = float('nan')
    for kw in (dict(kind=0), dict(kind=3), dict(kind=-1), dict(beta=0.5), dict(beta=8.5), dict(beta=nan), dict(alpha=0.0), dict(alpha=1.5),
               dict(alpha=nan), dict(gamma=-0.5), dict(gamma=8.5), dict(gamma=nan)):
        for kind in (1, 2):
            q = L.QualityLoss(**dict(dict(ok, kind=kind), **kw))
            assert fwd(q) == EINVAL and fwd_grad(q) == EINVAL and bwd_cls(q) == EINVAL, kw
    assert fwd(None) == EINVAL and fwd_grad(None) == EINVAL and bwd_cls(None) == EINVAL
    good = L.QualityLoss(**ok)
    # the twins' conditions: the options struct, the matcher's, the workspace, the layouts
    bad_opts = L.LossOpts(0.25, 2.0, 0.0, 0.0, 50.0, 0.5, 0.4, 1, 0, 1.0)
    assert fwd(good, o=bad_opts) == EINVAL and fwd_grad(good, o=bad_opts) == EINVAL and bwd_cls(good, o=bad_opts) == EINVAL
    assert fwd(good, o=None) == EINVAL and fwd_grad(good, o=None) == EINVAL and bwd_cls(good, o=None) == EINVAL
    assert fwd(good, t=atss) == EINVAL                                                 # low_quality with ATSS
    short = L.Atss(9, 2)
    short.level_start[1], short.level_start[2] = 252, 260
    noq = L.LossOpts(0.25, 2.0, 0.0, 0.1, 50.0, 0.5, 0.4, 0, 0, 1.0)
    assert fwd(good, o=noq, t=short) == EINVAL and fwd_grad(good, o=noq, t=short) == EINVAL
    assert fwd(good, nb=nbytes - 1) == EINVAL and fwd(good, n=0) == EINVAL
    assert fwd(good, nb=int(lib.effdet_loss_opts_workspace_bytes(B, A, nc, N))) == EINVAL      # the options' workspace is too small
    assert fwd_grad(good, ld=0) == EINVAL and fwd_grad(good, ld=9 * nc - 4) == EINVAL and fwd_grad(good, dtype=7) == EINVAL
    assert fwd_grad(good, ld=dld + 4, dtype=L.F32_SPLIT) == EINVAL
    assert bwd_cls(good, ld=9 * nc - 4) == EINVAL and bwd_cls(good, dtype=L.F32_SPLIT) == EINVAL and bwd_cls(good, out=None) == EINVAL
    torch.cuda.synchronize()
    for t in (losses, dpix):
        assert bool((t == 7.0).all())                                                  # no kernel ran
    assert int(ws.max()) == 0
    # and the same buffers are written by a valid call, with either matcher
    assert fwd_grad(good) == 0 and bwd_cls(good) == 0
    torch.cuda.synchronize()
    assert not bool((losses == 7.0).any()) and not bool((dpix == 7.0).any())
    assert fwd(L.QualityLoss(**dict(ok, kind=2)), o=noq, t=atss) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(losses).all())
