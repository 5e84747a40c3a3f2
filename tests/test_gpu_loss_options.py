"""GPU parity of the loss-option kernels (include/effdet_loss_opts.h, csrc/loss.hip) on the runs of tests/loss_options_cases.py against
the float64 restatement (tests/loss_options_restated.py).

Assignment: the codes in the workspace equal the restatement's exactly on every run (tests/test_loss_options_host.py proves the margin
that makes this a fair demand, and pins the exact ties by hand).
Losses: the rule and tolerance tests/test_gpu_loss_edges.py applies to the default term, assert_close at 2e-4.
Gradients: the rule of tests/test_gpu_box_loss.py -- per run the SAME restatement is evaluated in float32 on the CPU, and the device may
deviate from float64 by FACTOR = 8 times that evaluation's largest deviation, for d(logit) and for d(reg).  The float32 restatement
spells the power exp2(gamma * log2 u) as the device does, so it carries the same amplification of the logarithm's rounding.  No
element is excluded.  `pytest -s` prints the achieved ratios.
Everything else -- layouts, scaling by powers of two, determinism, the default path -- is bit for bit."""
import ctypes
import functools

import pytest
import torch

from tests import loss_cases as LC
from tests import loss_options_cases as OC
from tests import loss_options_restated as R
from tests.gpu_util import assert_close

pytestmark = pytest.mark.gpu

FACTOR = 8.0
GS = (0.7, 1.3)                                     # upstream gradients of the two losses


@functools.lru_cache(maxsize=None)
def _reference(name, on, box=None):
    """-> (float64 run, float32 run) of the restatement with the upstream gradients GS; computed once, read-only."""
    c, o = OC.get(name), OC.opts(on)
    ref = R.run(c, o, box=box, gscale=GS, dtype=torch.float64)
    return ref, R.run(c, o, box=box, gscale=GS, dtype=torch.float32, codes=ref['codes'])


@functools.lru_cache(maxsize=None)
def _device_case(name):
    c = OC.get(name)
    return tuple(c[k].cuda() for k in ('cls', 'reg', 'anc', 'ann'))


def _opt(on, **kw):
    from efficientdet.pytorch_amd import ops
    return ops.LossOptions(**dict(OC.OPTS[on], **kw))


def _gs(a=GS[0], b=GS[1]):
    return torch.tensor([a, b], dtype=torch.float32).cuda()


def _codes(ws, B, A):
    """The per-anchor assignment code the forward pass left at the head of its workspace."""
    return ws[:B * A * 4].view(torch.int32).reshape(B, A).cpu().long()


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _unpix(dpix, B, A, nc):
    return dpix[:, :, :9 * nc].reshape(B, A, nc)


def _ratio(got, f32, ref):
    yard = float((f32.double() - ref).abs().max())
    err = float((got.double().cpu() - ref).abs().max())
    return err, yard


@pytest.mark.parametrize('run', OC.RUNS, ids=lambda r: '%s-%s' % r)
def test_assignment_losses_and_gradients_against_float64(run):
    from efficientdet.pytorch_amd import ops
    name, on = run
    cls, reg, anc, ann = _device_case(name)
    B, A, nc = cls.shape
    ref, f32 = _reference(name, on)
    opt = _opt(on)
    losses, ws = ops.loss_opts_fwd(cls, reg, anc, ann, opt)
    codes = _codes(ws, B, A)
    assert torch.equal(codes, ref['codes']), torch.nonzero(codes != ref['codes'])[:4].tolist()
    if opt.pos_iou == 0.5 and opt.neg_iou == LC_NEG and not opt.low_quality:      # the matcher of today's kernel, bit for bit
        _, ws0 = ops.focal_loss_fwd(cls, reg, anc, ann)
        assert torch.equal(ws[:B * A * 4], ws0[:B * A * 4])
    assert_close(losses.cpu(), ref['losses'], 2e-4, '%s %s losses' % run)
    dcls = ops.loss_opts_bwd_cls(cls, ann, _gs(), ws, torch.float32, opt)
    dreg = ops.loss_opts_bwd_reg(reg, anc, ann, _gs(), ws, torch.float32, loss=opt)
    err_c, yard_c = _ratio(dcls, f32['dlogit'], ref['dlogit'])
    err_r, yard_r = _ratio(dreg, f32['dreg'], ref['dreg'])
    print('\n%s %s: losses %.9g %.9g (float64 %.9g %.9g, ratio to the 2e-4 bound %.3g) | dlogit max %.3g err %.3g yardstick %.3g ratio %.2f '
          '| dreg max %.3g err %.3g yardstick %.3g ratio %.2f'
          % (name, on, float(losses[0]), float(losses[1]), float(ref['losses'][0]), float(ref['losses'][1]),
             float(((losses.cpu().double() - ref['losses']).abs() / (2e-4 * ref['losses'].abs().clamp(min=1e-2 * float(ref['losses'].abs().max())))).max()),
             float(ref['dlogit'].abs().max()), err_c, yard_c, err_c / max(yard_c, 1e-300),
             float(ref['dreg'].abs().max()), err_r, yard_r, err_r / max(yard_r, 1e-300)))
    assert yard_c > 0.0 and err_c <= FACTOR * yard_c, (run, 'dlogit', err_c, yard_c)
    # (a run whose positives all sit on the linear side with a representable scale has yardstick 0: the device must then be exact)
    assert err_r <= FACTOR * yard_r, (run, 'dreg', err_r, yard_r)
    # exact +0.0: d(reg) away from the positives, d(logit) at ignored anchors and in images without a valid row
    got_r, got_c = dreg.cpu(), dcls.cpu()
    assert int(_bits(got_r)[ref['codes'] < 0].abs().max()) == 0
    ign = ref['codes'] == LC.CODE_IGN
    if bool(ign.any()):
        assert int(_bits(got_c)[ign].abs().max()) == 0
    assert bool((got_c[~ign] != 0).all())                                              # every live element carries a gradient
    if int(ref['num_pos'].sum()) > 0:
        assert bool((got_r[ref['codes'] >= 0] != 0).any(dim=1).float().mean() > 0.9)
    # the training path: one pass over cls for losses and d(logit) at an upstream gradient of one, d(reg) from its workspace
    if nc % 4 == 0:
        dld = LC.dld_for(nc)
        l2, ws2, dpix = ops.loss_opts_fwd_grad(cls, reg, anc, ann, torch.float32, dld, loss=opt)
        assert torch.equal(_codes(ws2, B, A), codes)
        assert torch.equal(_bits(l2[1:2]), _bits(losses[1:2]))
        assert_close(l2.cpu(), ref['losses'], 2e-4, '%s %s fwd_grad losses' % run)
        assert int(_bits(dpix[:, :, 9 * nc:]).abs().max()) == 0
        one = ops.loss_opts_bwd_cls(cls, ann, _gs(1.0, 1.0), ws, torch.float32, opt)
        assert torch.equal(_bits(_unpix(dpix, B, A, nc)), _bits(one))
        assert torch.equal(_bits(ops.loss_opts_bwd_reg(reg, anc, ann, _gs(), ws2, torch.float32, loss=opt)), _bits(dreg))


LC_NEG = float(torch.tensor(0.4, dtype=torch.float32))


def _split_halves(t):
    """[B, P, ld] buffer in the split layout -> (hi, lo) as bf16 [B, P, ld]: every 32-channel group is [32 x hi | 32 x lo]."""
    B, P, ld = t.shape
    h = t.contiguous().view(torch.bfloat16).reshape(B, P, ld // 32, 2, 32)
    return h[:, :, :, 0].reshape(B, P, ld), h[:, :, :, 1].reshape(B, P, ld)


def _same_values(f32_rows, pix, pix_bf16, rows_bf16, split, B, A, per, ld):
    """How the layouts of one gradient relate to its fp32 row form [B][A][per]: pixel-major rows of pitch ld with +0.0 pads, bf16 = the
    fp32 value rounded to nearest even, split = [hi | lo] with hi = bf16(v), lo = bf16(v - hi)."""
    want = torch.zeros(B, A // 9, ld, dtype=torch.float32, device=f32_rows.device)
    want[:, :, :9 * per] = f32_rows.reshape(B, A // 9, 9 * per)
    assert torch.equal(_bits(pix), _bits(want))
    if rows_bf16 is not None:
        assert torch.equal(_bits(rows_bf16), _bits(f32_rows.bfloat16()))
    assert torch.equal(_bits(pix_bf16), _bits(want.bfloat16()))
    hi, lo = _split_halves(split)
    assert torch.equal(_bits(hi), _bits(want.bfloat16()))
    assert torch.equal(_bits(lo), _bits((want - want.bfloat16().float()).bfloat16()))


@pytest.mark.parametrize('run', [('straddle_lq', 'paper'), ('nc80', 'paper_nolq'), ('lq_ties', 'high_bands_lq')], ids=lambda r: '%s-%s' % r)
def test_output_layouts(run):
    from efficientdet.pytorch_amd import ops
    name, on = run
    cls, reg, anc, ann = _device_case(name)
    B, A, nc = cls.shape
    opt = _opt(on)
    dld = LC.dld_for(nc)
    # d(logit): the one-pass kernel's three element types against the [B][A][nc] fp32 form at an upstream gradient of one
    _, ws, pix = ops.loss_opts_fwd_grad(cls, reg, anc, ann, torch.float32, dld, loss=opt)
    _, _, pix_bf16 = ops.loss_opts_fwd_grad(cls, reg, anc, ann, torch.bfloat16, dld, loss=opt)
    _, _, split = ops.loss_opts_fwd_grad(cls, reg, anc, ann, torch.float32, dld, split=True, loss=opt)
    one = _gs(1.0, 1.0)
    rows = ops.loss_opts_bwd_cls(cls, ann, one, ws, torch.float32, opt)
    _same_values(rows, pix, pix_bf16, ops.loss_opts_bwd_cls(cls, ann, one, ws, torch.bfloat16, opt), split, B, A, nc, dld)
    assert float(rows.abs().max()) > 0.0
    # ... and bwd_cls's own pixel-major form, with an upstream gradient
    gs = _gs()
    rows = ops.loss_opts_bwd_cls(cls, ann, gs, ws, torch.float32, opt)
    want = torch.zeros(B, A // 9, dld, dtype=torch.float32, device=cls.device)
    want[:, :, :9 * nc] = rows.reshape(B, A // 9, 9 * nc)
    assert torch.equal(_bits(ops.loss_opts_bwd_cls(cls, ann, gs, ws, torch.float32, opt, dld=dld)), _bits(want))
    assert torch.equal(_bits(ops.loss_opts_bwd_cls(cls, ann, gs, ws, torch.bfloat16, opt, dld=dld)), _bits(want.bfloat16()))
    # d(reg): the three layouts of loss_bwd_reg_kernel
    fn = functools.partial(ops.loss_opts_bwd_reg, reg, anc, ann, gs, ws, loss=opt)
    rows = fn(torch.float32)
    _same_values(rows, fn(torch.float32, reg_ld=64), fn(torch.bfloat16, reg_ld=64), fn(torch.bfloat16), fn(torch.float32, reg_ld=64, split=True),
                 B, A, 4, 64)
    assert float(rows.abs().max()) > 0.0


def test_non_finite_probabilities_where_the_loss_does_not_reach():
    """nan_zero as in the existing kernels: an ignored anchor's gradient is p - p -- +0.0, or NaN for a NaN or inf p -- in every form."""
    from efficientdet.pytorch_amd import ops
    cls, reg, anc, ann = _device_case('straddle_lq')
    B, A, nc = cls.shape
    opt = _opt('paper')
    bad = cls.clone()
    bad[1, 7, 2] = float('nan')                                                        # image 1 has no valid row: every anchor ignored
    bad[1, 200, 1] = float('inf')
    dld = LC.dld_for(nc)
    losses, ws, pix = ops.loss_opts_fwd_grad(bad, reg, anc, ann, torch.float32, dld, loss=opt)
    ref, _, pix0 = ops.loss_opts_fwd_grad(cls, reg, anc, ann, torch.float32, dld, loss=opt)
    assert torch.equal(_bits(losses), _bits(ref))
    for got in (_unpix(pix, B, A, nc), ops.loss_opts_bwd_cls(bad, ann, _gs(), ws, torch.float32, opt),
                _unpix(ops.loss_opts_bwd_cls(bad, ann, _gs(), ws, torch.float32, opt, dld=dld), B, A, nc)):
        nan = torch.isnan(got)
        assert torch.nonzero(nan).tolist() == [[1, 7, 2], [1, 200, 1]]
        assert int(_bits(got[1])[~nan[1]].abs().max()) == 0
    assert torch.equal(_bits(pix[0]), _bits(pix0[0])) and torch.equal(_bits(pix[2]), _bits(pix0[2]))


@pytest.mark.parametrize('run', [('straddle_lq', 'paper'), ('s128_r05', 'bands')], ids=lambda r: '%s-%s' % r)
def test_reg_weight_and_upstream_gradients_scale_by_powers_of_two(run):
    from efficientdet.pytorch_amd import ops
    name, on = run
    cls, reg, anc, ann = _device_case(name)
    o1, o2, o0 = _opt(on, reg_weight=1.0), _opt(on, reg_weight=2.0), _opt(on, reg_weight=0.0)
    l1, ws = ops.loss_opts_fwd(cls, reg, anc, ann, o1)
    l2, ws2 = ops.loss_opts_fwd(cls, reg, anc, ann, o2)
    assert torch.equal(_bits(l2[1:2]), _bits(l1[1:2] * 2.0)) and torch.equal(_bits(l2[0:1]), _bits(l1[0:1])) and float(l1[1]) > 0.0
    g1 = ops.loss_opts_bwd_reg(reg, anc, ann, _gs(1.0, 1.0), ws, torch.float32, loss=o1)
    assert torch.equal(_bits(ops.loss_opts_bwd_reg(reg, anc, ann, _gs(1.0, 1.0), ws2, torch.float32, loss=o2)), _bits(g1 * 2.0))
    assert torch.equal(_bits(ops.loss_opts_bwd_reg(reg, anc, ann, _gs(1.0, 0.25), ws, torch.float32, loss=o1)), _bits(g1 * 0.25))
    assert torch.equal(_bits(ops.loss_opts_bwd_reg(reg, anc, ann, _gs(8.0, 0.5), ws, torch.float32, loss=o2)), _bits(g1))
    c1 = ops.loss_opts_bwd_cls(cls, ann, _gs(1.0, 1.0), ws, torch.float32, o1)
    assert torch.equal(_bits(ops.loss_opts_bwd_cls(cls, ann, _gs(4.0, 3.0), ws, torch.float32, o1)), _bits(c1 * 4.0))
    assert torch.equal(_bits(ops.loss_opts_bwd_cls(cls, ann, _gs(0.125, 1.0), ws2, torch.float32, o2)), _bits(c1 * 0.125))
    l0, ws0 = ops.loss_opts_fwd(cls, reg, anc, ann, o0)
    assert float(l0[1]) == 0.0 and torch.equal(_bits(l0[0:1]), _bits(l1[0:1]))
    assert int(_bits(ops.loss_opts_bwd_reg(reg, anc, ann, _gs(), ws0, torch.float32, loss=o0) + 0.0).abs().max()) == 0


@pytest.mark.parametrize('run', [('straddle_lq', 'paper'), ('nc80', 'paper_nolq')], ids=lambda r: '%s-%s' % r)
def test_two_runs_are_bitwise_equal(run):
    from efficientdet.pytorch_amd import ops
    name, on = run
    cls, reg, anc, ann = _device_case(name)
    nc = cls.shape[2]
    opt = _opt(on)
    runs = []
    for _ in range(2):
        losses, ws, dpix = ops.loss_opts_fwd_grad(cls, reg, anc, ann, torch.float32, LC.dld_for(nc), loss=opt)
        runs.append((losses.clone(), dpix, ops.loss_opts_bwd_reg(reg, anc, ann, _gs(), ws, torch.float32, loss=opt),
                     ws[:cls.shape[0] * cls.shape[1] * 4].view(torch.float32).clone()))
    for a, b in zip(*runs):
        assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize('kind', ['giou', 'ciou'])
def test_an_iou_box_term_runs_over_the_promoted_assignment(kind):
    """box_kind = giou / ciou with low_quality: the box-loss restatement evaluated on the promoted assignment; reg_weight does not
    apply, box_weight does."""
    from efficientdet.pytorch_amd import ops
    name, on = 'straddle_lq', 'paper'
    cls, reg, anc, ann = _device_case(name)
    B, A, nc = cls.shape
    box = ops.BoxLossOptions(kind, 2.0)
    ref, f32 = _reference(name, on, (kind, 2.0))
    opt = _opt(on)
    losses, ws = ops.loss_opts_fwd(cls, reg, anc, ann, opt, box)
    assert torch.equal(_codes(ws, B, A), ref['codes']) and int((ref['codes'][2] >= 0).sum()) == 1       # image 2 trains on its promoted anchor
    assert_close(losses.cpu(), ref['losses'], 2e-4, '%s losses' % kind)
    dreg = ops.loss_opts_bwd_reg(reg, anc, ann, _gs(), ws, torch.float32, loss=opt, box=box)
    err, yard = _ratio(dreg, f32['dreg'], ref['dreg'])
    print('\n%s over the promoted assignment: losses[1] %.9g (float64 %.9g) | dreg max %.3g err %.3g yardstick %.3g ratio %.2f'
          % (kind, float(losses[1]), float(ref['losses'][1]), float(ref['dreg'].abs().max()), err, yard, err / max(yard, 1e-300)))
    assert yard > 0.0 and err <= FACTOR * yard
    assert bool((dreg[2, OC.STRADDLE_SMALL] != 0).any()) and int(_bits(dreg.cpu())[ref['codes'] < 0].abs().max()) == 0
    # the class term is the smooth-L1 run's; the box term is the existing kernels' on this workspace, bit for bit
    plain, ws1 = ops.loss_opts_fwd(cls, reg, anc, ann, opt)
    assert torch.equal(_bits(plain[0:1]), _bits(losses[0:1])) and not torch.equal(_bits(plain[1:2]), _bits(losses[1:2]))
    assert torch.equal(_bits(ops.box_loss_bwd_reg(reg, anc, ann, _gs(), ws1, torch.float32, options=box)), _bits(dreg))
    l2, ws2, _ = ops.loss_opts_fwd_grad(cls, reg, anc, ann, torch.float32, LC.dld_for(nc), loss=opt, box=box)
    assert torch.equal(_bits(l2[1:2]), _bits(losses[1:2]))
    # reg_weight is the smooth-L1 term's alone
    l3, _ = ops.loss_opts_fwd(cls, reg, anc, ann, _opt(on, reg_weight=1.0), box)
    assert torch.equal(_bits(l3), _bits(losses))


@pytest.mark.parametrize('name', OC.DEFAULT_CASES)
def test_default_options_and_none_are_the_existing_calls(name):
    from efficientdet.pytorch_amd import ops
    cls, reg, anc, ann = _device_case(name)
    nc = cls.shape[2]
    dld = LC.dld_for(nc)
    lf, wsf = ops.focal_loss_fwd(cls, reg, anc, ann)
    lf2, wsf2, df2 = ops.focal_loss_fwd_grad(cls, reg, anc, ann, torch.float32, dld)
    for opt in (None, ops.LossOptions(), ops.LossOptions(beta=1.0 / 9.0, neg_iou=0.4, low_quality=False)):
        l, ws = ops.loss_opts_fwd(cls, reg, anc, ann, opt)
        assert torch.equal(_bits(l), _bits(lf)) and ws.numel() == wsf.numel()       # (the existing workspace: the existing call)
        l2, ws2, d2 = ops.loss_opts_fwd_grad(cls, reg, anc, ann, torch.float32, dld, loss=opt)
        assert torch.equal(_bits(l2), _bits(lf2)) and torch.equal(_bits(d2), _bits(df2)) and ws2.numel() == wsf2.numel()
        for kw in (dict(), dict(reg_ld=64), dict(reg_ld=64, split=True)):
            assert torch.equal(_bits(ops.loss_opts_bwd_reg(reg, anc, ann, _gs(), ws, torch.float32, loss=opt, **kw)),
                               _bits(ops.focal_loss_bwd_reg(reg, anc, ann, _gs(), wsf, torch.float32, **kw)))
        box = ops.BoxLossOptions('giou', 2.0)
        lb, wsb = ops.loss_opts_fwd(cls, reg, anc, ann, opt, box)
        assert torch.equal(_bits(lb), _bits(ops.box_loss_fwd(cls, reg, anc, ann, box)[0]))
    # the default VALUES through the new kernels are the same loss up to rounding (another spelling of the power and of the knee)
    from efficientdet.pytorch_amd import _lib as L
    lib = L.require('effdet_loss_opts_fwd', 'effdet_loss_opts_workspace_bytes')
    B, A, _ = cls.shape
    N = ann.shape[1]
    d = ops.LossOptions()
    o = L.LossOpts(d.alpha, d.gamma, d.label_smoothing, d.beta, d.reg_weight, d.pos_iou, d.neg_iou, 0, 0, 1.0)
    nbytes = int(lib.effdet_loss_opts_workspace_bytes(B, A, nc, N))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=cls.device)
    losses = torch.empty(2, device=cls.device)
    assert lib.effdet_loss_opts_fwd(L.ptr(cls), L.ptr(reg), L.ptr(anc), L.ptr(ann), L.ptr(losses), L.ptr(ws), nbytes, B, A, nc, N,
                                    ctypes.byref(o), L.stream_ptr()) == 0
    assert torch.equal(ws[:B * A * 4], wsf[:B * A * 4])
    assert_close(losses.cpu(), lf.cpu(), 1e-5, 'default values through the option kernels')


def test_error_codes_and_nothing_enqueued():
    from efficientdet.pytorch_amd import _lib as L
    cls, reg, anc, ann = _device_case('straddle_lq')
    B, A, nc = cls.shape
    N = ann.shape[1]
    lib = L.require('effdet_loss_opts_fwd', 'effdet_loss_opts_fwd_grad', 'effdet_loss_opts_bwd_cls', 'effdet_loss_opts_bwd_reg')
    nbytes = int(lib.effdet_loss_opts_workspace_bytes(B, A, nc, N))
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=cls.device)
    losses = torch.full((2,), 7.0, device=cls.device)
    dld = LC.dld_for(nc)
    dpix = torch.full((B, A // 9, dld), 7.0, device=cls.device)
    dreg = torch.full((B, A // 9, 64), 7.0, device=cls.device)
    gs = _gs()
    EINVAL = -1
    ok = dict(alpha=0.25, gamma=1.5, label_smoothing=0.0, beta=0.1, reg_weight=50.0, pos_iou=0.5, neg_iou=0.4, low_quality=1, box_kind=0,
              box_weight=1.0)

    def fwd(o, nb=nbytes, n=N):
        return lib.effdet_loss_opts_fwd(L.ptr(cls), L.ptr(reg), L.ptr(anc), L.ptr(ann), L.ptr(losses), L.ptr(ws), nb, B, A, nc, n,
                                        ctypes.byref(o) if o is not None else None, L.stream_ptr())

    def fwd_grad(o, ld=dld, dtype=L.F32):
        return lib.effdet_loss_opts_fwd_grad(L.ptr(cls), L.ptr(reg), L.ptr(anc), L.ptr(ann), L.ptr(losses), L.ptr(ws), nbytes, L.ptr(dpix), ld,
                                             dtype, B, A, nc, N, ctypes.byref(o) if o is not None else None, L.stream_ptr())

    def bwd_cls(o, ld=dld, dtype=L.F32, out=dpix):
        return lib.effdet_loss_opts_bwd_cls(L.ptr(cls), L.ptr(ann), L.ptr(gs), L.ptr(ws), L.ptr(out), ld, dtype, B, A, nc, N,
                                            ctypes.byref(o) if o is not None else None, L.stream_ptr())

    def bwd_reg(o, reg_ld=64, dtype=L.F32, a=A, out=dreg):
        return lib.effdet_loss_opts_bwd_reg(L.ptr(reg), L.ptr(anc), L.ptr(ann), L.ptr(gs), L.ptr(ws), L.ptr(out), reg_ld, dtype, B, a, N,
                                            ctypes.byref(o) if o is not None else None, L.stream_ptr())
    nan, inf = float('nan'), float('inf')
    for kw in (dict(alpha=0.0), dict(alpha=1.0), dict(alpha=nan), dict(gamma=-1.0), dict(gamma=8.5), dict(gamma=nan), dict(label_smoothing=1.0),
               dict(label_smoothing=nan), dict(beta=0.0), dict(beta=inf), dict(beta=nan), dict(reg_weight=-1.0), dict(reg_weight=nan),
               dict(pos_iou=0.3), dict(pos_iou=1.5), dict(neg_iou=-0.1), dict(neg_iou=nan), dict(low_quality=2), dict(box_kind=5),
               dict(box_kind=-1), dict(box_weight=-1.0), dict(box_weight=inf)):
        o = L.LossOpts(**dict(ok, **kw))
        assert fwd(o) == EINVAL and fwd_grad(o) == EINVAL and bwd_cls(o) == EINVAL and bwd_reg(o) == EINVAL, kw
    assert fwd(None) == EINVAL and fwd_grad(None) == EINVAL and bwd_cls(None) == EINVAL and bwd_reg(None) == EINVAL
    good = L.LossOpts(**ok)
    giou = L.LossOpts(**dict(ok, box_kind=2))
    # the twins' conditions
    assert fwd(good, nb=nbytes - 1) == EINVAL and fwd(good, n=0) == EINVAL
    assert fwd_grad(good, ld=0) == EINVAL and fwd_grad(good, ld=9 * nc - 4) == EINVAL and fwd_grad(good, ld=9 * nc + 2) == EINVAL
    assert fwd_grad(good, dtype=7) == EINVAL and fwd_grad(good, ld=dld + 4, dtype=L.F32_SPLIT) == EINVAL
    assert bwd_cls(good, ld=9 * nc - 4) == EINVAL and bwd_cls(good, dtype=L.F32_SPLIT) == EINVAL and bwd_cls(good, out=None) == EINVAL
    for o in (good, giou):
        assert bwd_reg(o, reg_ld=32) == EINVAL and bwd_reg(o, reg_ld=38) == EINVAL and bwd_reg(o, a=A + 1) == EINVAL
        assert bwd_reg(o, reg_ld=0, dtype=L.F32_SPLIT) == EINVAL and bwd_reg(o, reg_ld=48, dtype=L.F32_SPLIT) == EINVAL
        assert bwd_reg(o, dtype=7) == EINVAL and bwd_reg(o, out=None) == EINVAL
    torch.cuda.synchronize()
    for t in (losses, dpix, dreg):
        assert bool((t == 7.0).all())                                              # no kernel ran
    assert int(ws.max()) == 0
    # and the same buffers are written by a valid call
    assert fwd_grad(good) == 0 and bwd_reg(good) == 0
    torch.cuda.synchronize()
    assert not bool((losses == 7.0).any()) and not bool((dpix == 7.0).any()) and not bool((dreg == 7.0).any())
