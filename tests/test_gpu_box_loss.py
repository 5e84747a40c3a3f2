"""GPU parity of the IoU-family box loss kernels (include/effdet_box_loss.h, csrc/loss.hip) on the cases of tests/box_loss_cases.py
against the float64 restatement (tests/box_loss_restated.py).

Tolerance: not a fixed number.  Per case and kind the SAME restatement is evaluated in float32 on the CPU; the device may deviate from
float64 by FACTOR = 8 times that evaluation's largest deviation -- of the per-anchor loss for losses[1] (a weighted mean of per-anchor
losses: its error is at most the largest per-anchor one), of the gradient elements for d(reg).  The factor covers the device's other
operation order, fp contraction, the last bits of expf / atanf / the division, and the analytic gradient against autograd's chain.
tests/test_box_loss_host.py proves that no select of a non-tie case has operands closer than 1e-2 px and that the tie cases are exact
in both precisions, so no element is excluded.  `pytest -s` prints the achieved ratio per case."""
import functools

import pytest
import torch

from tests import box_loss_cases as BC
from tests import box_loss_restated as R
from tests import loss_cases as LC

pytestmark = pytest.mark.gpu

FACTOR = 8.0
CASE_NAMES = sorted(BC.CASES)


@functools.lru_cache(maxsize=None)
def _reference(name, kind):
    """-> (float64 run, float32 run) of the restatement with weight 1 and an upstream gradient of 1; computed once, read-only."""
    c = BC.get(name)
    return R.run(c, kind, dtype=torch.float64), R.run(c, kind, dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def _device_case(name):
    c = BC.get(name)
    return tuple(c[k].cuda() for k in ('cls', 'reg', 'anc', 'ann'))


def _opt(kind, weight=1.0):
    from efficientdet.pytorch_amd import ops
    return ops.BoxLossOptions(kind, weight)


def _gs(v=1.0):
    return torch.tensor([1.0, v], dtype=torch.float32).cuda()


def _codes(ws, B, A):
    """The per-anchor assignment code the forward pass left at the head of its workspace."""
    return ws[:B * A * 4].view(torch.int32).reshape(B, A).cpu().long()


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize('name', CASE_NAMES)
@pytest.mark.parametrize('kind', R.KINDS)
def test_loss_and_gradient_against_float64(kind, name):
    from efficientdet.pytorch_amd import ops
    cls, reg, anc, ann = _device_case(name)
    B, A, nc = cls.shape
    ref, f32 = _reference(name, kind)
    losses, ws = ops.box_loss_fwd(cls, reg, anc, ann, _opt(kind))
    dreg = ops.box_loss_bwd_reg(reg, anc, ann, _gs(), ws, torch.float32, options=_opt(kind))
    focal, _ = ops.focal_loss_fwd(cls, reg, anc, ann)
    assert torch.equal(_codes(ws, B, A), LC.oracle_states(BC.get(name), torch.float64))        # the assignment is not touched
    assert torch.equal(_bits(losses[0:1]), _bits(focal[0:1]))                                   # nor is the class term
    # losses[1]
    yard_l = float((f32['per_anchor'].double() - ref['per_anchor']).abs().max())
    err_l = abs(float(losses[1]) - ref['loss'])
    # d(reg)
    got = dreg.cpu()
    yard_g = float((f32['grad'].double() - ref['grad']).abs().max())
    err_g = float((got.double() - ref['grad']).abs().max())
    print('\n%s %s: loss %.9g (float64 %.9g) err %.3g yardstick %.3g ratio %.2f | grad max %.3g err %.3g yardstick %.3g ratio %.2f'
          % (name, kind, float(losses[1]), ref['loss'], err_l, yard_l, err_l / max(yard_l, 1e-300), float(ref['grad'].abs().max()),
             err_g, yard_g, err_g / max(yard_g, 1e-300)))
    assert yard_l > 0.0 and yard_g > 0.0
    assert err_l <= FACTOR * yard_l, (name, kind, 'loss', err_l, yard_l)
    assert err_g <= FACTOR * yard_g, (name, kind, 'grad', err_g, yard_g)
    # exact +0.0 in every row of an anchor that is not positive
    b, a, _ = ref['pos']
    nonpos = torch.ones(B, A, dtype=torch.bool); nonpos[b, a] = False
    assert int(_bits(got)[nonpos].abs().max()) == 0
    assert bool((got[b, a] != 0).any(dim=1).float().mean() > 0.9)                               # and the positives carry a gradient
    # the training path: the same box term after the one-pass class kernel, whose own outputs are the focal call's
    dld = LC.dld_for(nc)
    l2, ws2, dpix = ops.box_loss_fwd_grad(cls, reg, anc, ann, torch.float32, dld, options=_opt(kind))
    f2, _, fpix = ops.focal_loss_fwd_grad(cls, reg, anc, ann, torch.float32, dld)
    assert torch.equal(_bits(l2[1:2]), _bits(losses[1:2])) and torch.equal(_bits(l2[0:1]), _bits(f2[0:1])) and torch.equal(_bits(dpix), _bits(fpix))
    assert torch.equal(_bits(ops.box_loss_bwd_reg(reg, anc, ann, _gs(), ws2, torch.float32, options=_opt(kind))), _bits(dreg))


def _split_halves(t):
    """[B, P, ld] buffer in the split layout -> (hi, lo) as bf16 [B, P, ld]: every 32-channel group is [32 x hi | 32 x lo]."""
    B, P, ld = t.shape
    h = t.contiguous().view(torch.bfloat16).reshape(B, P, ld // 32, 2, 32)
    return h[:, :, :, 0].reshape(B, P, ld), h[:, :, :, 1].reshape(B, P, ld)


def _layout_relations(f32_rows, pix, pix_bf16, rows_bf16, split, B, A):
    """How the outputs of one d(reg) kernel relate to its fp32 [B][A][4] output; asserted on the smooth-L1 kernel (the control) and on
    the new one alike."""
    want = torch.zeros(B, A // 9, 64, dtype=torch.float32, device=f32_rows.device)
    want[:, :, :36] = f32_rows.reshape(B, A // 9, 36)
    assert torch.equal(_bits(pix), _bits(want))                                   # pixel-major rows, +0.0 in [36, 64), bit for bit
    assert torch.equal(_bits(rows_bf16), _bits(f32_rows.bfloat16()))              # bf16: the fp32 value rounded to nearest even
    assert torch.equal(_bits(pix_bf16), _bits(want.bfloat16()))
    hi, lo = _split_halves(split)
    assert torch.equal(_bits(hi), _bits(want.bfloat16()))                         # split: hi = bf16(v), lo = bf16(v - hi)
    assert torch.equal(_bits(lo), _bits((want - want.bfloat16().float()).bfloat16()))


@pytest.mark.parametrize('name', ['straddle', 's128_r20'])
@pytest.mark.parametrize('kind', R.KINDS)
def test_output_layouts(kind, name):
    from efficientdet.pytorch_amd import ops
    cls, reg, anc, ann = _device_case(name)
    B, A, _ = cls.shape
    _, ws = ops.box_loss_fwd(cls, reg, anc, ann, _opt(kind))
    gs = _gs(1.3)

    def outputs(fn, **kw):
        return (fn(reg, anc, ann, gs, ws, torch.float32, **kw), fn(reg, anc, ann, gs, ws, torch.float32, reg_ld=64, **kw),
                fn(reg, anc, ann, gs, ws, torch.bfloat16, reg_ld=64, **kw), fn(reg, anc, ann, gs, ws, torch.bfloat16, **kw),
                fn(reg, anc, ann, gs, ws, torch.float32, reg_ld=64, split=True, **kw))
    _layout_relations(*outputs(ops.focal_loss_bwd_reg), B, A)                      # the control: the existing kernel's three outputs
    out = outputs(ops.box_loss_bwd_reg, options=_opt(kind))
    _layout_relations(*out, B, A)
    assert float(out[0].abs().max()) > 0.0


@pytest.mark.parametrize('kind', R.KINDS)
def test_two_runs_are_bitwise_equal(kind):
    from efficientdet.pytorch_amd import ops
    cls, reg, anc, ann = _device_case('s128_r20')
    runs = []
    for _ in range(2):
        losses, ws = ops.box_loss_fwd(cls, reg, anc, ann, _opt(kind, 1.5))
        runs.append((losses.clone(), ops.box_loss_bwd_reg(reg, anc, ann, _gs(0.7), ws, torch.float32, options=_opt(kind, 1.5))))
    assert torch.equal(_bits(runs[0][0]), _bits(runs[1][0])) and torch.equal(_bits(runs[0][1]), _bits(runs[1][1]))


@pytest.mark.parametrize('kind', R.KINDS)
def test_weight_and_upstream_gradient_scale_by_powers_of_two(kind):
    from efficientdet.pytorch_amd import ops
    cls, reg, anc, ann = _device_case('straddle')
    l1, ws = ops.box_loss_fwd(cls, reg, anc, ann, _opt(kind, 1.0))
    g1 = ops.box_loss_bwd_reg(reg, anc, ann, _gs(1.0), ws, torch.float32, options=_opt(kind, 1.0))
    l4, ws4 = ops.box_loss_fwd(cls, reg, anc, ann, _opt(kind, 4.0))
    assert torch.equal(_bits(l4[1:2]), _bits(l1[1:2] * 4.0)) and torch.equal(_bits(l4[0:1]), _bits(l1[0:1]))
    assert torch.equal(_bits(ops.box_loss_bwd_reg(reg, anc, ann, _gs(1.0), ws4, torch.float32, options=_opt(kind, 4.0))), _bits(g1 * 4.0))
    assert torch.equal(_bits(ops.box_loss_bwd_reg(reg, anc, ann, _gs(0.25), ws, torch.float32, options=_opt(kind, 1.0))), _bits(g1 * 0.25))
    assert torch.equal(_bits(ops.box_loss_bwd_reg(reg, anc, ann, _gs(0.5), ws, torch.float32, options=_opt(kind, 8.0))), _bits(g1 * 4.0))
    l0, ws0 = ops.box_loss_fwd(cls, reg, anc, ann, _opt(kind, 0.0))
    assert float(l0[1]) == 0.0
    assert int(_bits(ops.box_loss_bwd_reg(reg, anc, ann, _gs(1.0), ws0, torch.float32, options=_opt(kind, 0.0)) + 0.0).abs().max()) == 0


def test_smooth_l1_through_the_option_is_the_existing_path():
    from efficientdet.pytorch_amd import ops
    cls, reg, anc, ann = _device_case('straddle')
    nc = cls.shape[2]
    for opt in (None, ops.BoxLossOptions(), ops.BoxLossOptions('smooth_l1', 1.0)):
        l, ws = ops.box_loss_fwd(cls, reg, anc, ann, opt)
        lf, wsf = ops.focal_loss_fwd(cls, reg, anc, ann)
        assert torch.equal(_bits(l), _bits(lf))
        for kw in (dict(), dict(reg_ld=64), dict(reg_ld=64, split=True)):
            assert torch.equal(_bits(ops.box_loss_bwd_reg(reg, anc, ann, _gs(1.3), ws, torch.float32, options=opt, **kw)),
                               _bits(ops.focal_loss_bwd_reg(reg, anc, ann, _gs(1.3), wsf, torch.float32, **kw)))
        l2, _, d2 = ops.box_loss_fwd_grad(cls, reg, anc, ann, torch.float32, LC.dld_for(nc), options=opt)
        lf2, _, df2 = ops.focal_loss_fwd_grad(cls, reg, anc, ann, torch.float32, LC.dld_for(nc))
        assert torch.equal(_bits(l2), _bits(lf2)) and torch.equal(_bits(d2), _bits(df2))
    # and an IoU kind is another loss
    assert float(ops.box_loss_fwd(cls, reg, anc, ann, ops.BoxLossOptions('iou'))[0][1]) != float(lf[1])


def test_error_codes_and_nothing_enqueued():
    from efficientdet.pytorch_amd import _lib as L
    cls, reg, anc, ann = _device_case('straddle')
    B, A, nc = cls.shape
    N = ann.shape[1]
    lib = L.require('effdet_box_loss_fwd', 'effdet_box_loss_fwd_grad', 'effdet_box_loss_bwd_reg')
    nbytes = int(lib.effdet_loss_workspace_bytes(B, A, nc))
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=cls.device)
    losses = torch.full((2,), 7.0, device=cls.device)
    dld = LC.dld_for(nc)
    dpix = torch.full((B, A // 9, dld), 7.0, device=cls.device)
    dreg = torch.full((B, A // 9, 64), 7.0, device=cls.device)
    gs = _gs()
    EINVAL = -1
    nan, inf = float('nan'), float('inf')

    def fwd(kind, weight, nb=nbytes, n=N):
        return lib.effdet_box_loss_fwd(L.ptr(cls), L.ptr(reg), L.ptr(anc), L.ptr(ann), L.ptr(losses), L.ptr(ws), nb, B, A, nc, n, kind, weight,
                                       L.stream_ptr())

    def fwd_grad(kind, weight, ld=dld):
        return lib.effdet_box_loss_fwd_grad(L.ptr(cls), L.ptr(reg), L.ptr(anc), L.ptr(ann), L.ptr(losses), L.ptr(ws), nbytes, L.ptr(dpix), ld,
                                            L.F32, B, A, nc, N, kind, weight, L.stream_ptr())

    def bwd(kind, weight, reg_ld=64, dtype=L.F32, a=A, out=dreg):
        return lib.effdet_box_loss_bwd_reg(L.ptr(reg), L.ptr(anc), L.ptr(ann), L.ptr(gs), L.ptr(ws), L.ptr(out), reg_ld, dtype, B, a, N, kind,
                                           weight, L.stream_ptr())
    for kind, weight in ((0, 1.0), (5, 1.0), (-1, 1.0), (4, -1.0), (4, nan), (4, inf), (4, -0.5)):
        assert fwd(kind, weight) == EINVAL and fwd_grad(kind, weight) == EINVAL and bwd(kind, weight) == EINVAL, (kind, weight)
    # the twins' conditions
    assert fwd(4, 1.0, nb=nbytes - 1) == EINVAL and fwd(4, 1.0, n=0) == EINVAL
    assert fwd_grad(4, 1.0, ld=0) == EINVAL and fwd_grad(4, 1.0, ld=9 * nc - 4) == EINVAL and fwd_grad(4, 1.0, ld=9 * nc + 2) == EINVAL
    assert bwd(4, 1.0, reg_ld=32) == EINVAL and bwd(4, 1.0, reg_ld=38) == EINVAL and bwd(4, 1.0, a=A + 1) == EINVAL
    assert bwd(4, 1.0, reg_ld=0, dtype=L.F32_SPLIT) == EINVAL and bwd(4, 1.0, reg_ld=48, dtype=L.F32_SPLIT) == EINVAL
    assert bwd(4, 1.0, dtype=7) == EINVAL and bwd(4, 1.0, out=None) == EINVAL
    torch.cuda.synchronize()
    for t in (losses, dpix, dreg):
        assert bool((t == 7.0).all())                                              # no kernel ran
    assert int(ws.max()) == 0
    # and the same buffers are written by a valid call
    assert fwd_grad(4, 1.0) == 0 and bwd(4, 1.0) == 0
    torch.cuda.synchronize()
    assert not bool((losses == 7.0).any()) and not bool((dpix == 7.0).any()) and not bool((dreg == 7.0).any())
