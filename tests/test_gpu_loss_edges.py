"""GPU parity of the detection-loss kernels on the edge cases of tests/loss_cases.py (the branches each reaches are proven on the
CPU by tests/test_loss_cases_host.py): losses and gradients against the fp64 oracle with autograd at the tolerances of
test_gpu_post_loss.test_focal_loss_fwd_bwd, and the per-anchor assignment read back from the gradients themselves --
  positive: a d(reg) row that is not all zero (reg is random, so a positive's smooth-L1 gradient is non-zero almost surely);
  ignored:  a d(cls) row that is exactly zero (every probability lies inside the clamp, so a live row has no zero);
  negative: neither;   the positive's label: the one class whose gradient is negative."""
import functools

import pytest
import torch

from tests import loss_cases as LC
from tests.gpu_util import assert_close
from oracle import effdet_oracle as O

pytestmark = pytest.mark.gpu

GS = (0.7, 1.3)                                    # upstream gradients of the two losses


@functools.lru_cache(maxsize=None)
def _reference(name):
    """-> (case, losses [2], d(logits) [B, A, nc], d(reg) [B, A, 4], states [B, A], skip [B, A]) from the oracle in fp64; computed once
    per case and shared by the dtypes."""
    c = LC.CASES[name]()
    cls = c['cls'].double().requires_grad_(True)
    reg = c['reg'].double().requires_grad_(True)
    cl, rl = O.focal_loss(cls, reg, c['anc'].double(), c['ann'].double())
    (GS[0] * cl.sum() + GS[1] * rl.sum()).backward()
    dlogit = cls.grad * cls.detach() * (1 - cls.detach())
    skip = LC.skip_mask(c) if c['state_check'] == 'skip' else torch.zeros(cls.shape[:2], dtype=torch.bool)
    return c, torch.cat([cl.detach(), rl.detach()]), dlogit, reg.grad, LC.oracle_states(c, torch.float64), skip


def _read_states(dcls, dreg):
    """-> (positive, ignored, label) per anchor from the gradients (see the module docstring)."""
    dcls, dreg = dcls.float().cpu(), dreg.float().cpu()
    pos = (dreg != 0).any(dim=-1)
    ign = (dcls == 0).all(dim=-1)
    vmin, label = dcls.min(dim=-1)
    return pos, ign, torch.where(vmin < 0, label, torch.full_like(label, -1))


def _check_states(name, dcls, dreg, what):
    c, _, _, _, code, skip = _reference(name)
    pos, ign, label = _read_states(dcls, dreg)
    assert not bool((pos & ign).any()), what
    # the hand-derived expectations first: they do not depend on any oracle
    for b, a, state, row in c['expect']:
        got = LC.POS if pos[b, a] else (LC.IGN if ign[b, a] else LC.NEG)
        assert got == state, (what, 'image %d anchor %d is %s, expected %s' % (b, a, got, state))
        if state == LC.POS:
            assert int(label[b, a]) == int(c['ann'][b, row, 4]), (what, 'image %d anchor %d: label %d, expected row %d label %d' % (
                b, a, int(label[b, a]), row, int(c['ann'][b, row, 4])))
    for b, state in c['expect_all'].items():
        assert bool((ign[b] if state == LC.IGN else ~ign[b] & ~pos[b]).all()), (what, b, state)
    if c['state_check'] is None:
        return
    keep = ~skip
    for kind, got, ref in (('positive', pos, code >= 0), ('ignored', ign, code == LC.CODE_IGN)):
        bad = (got != ref) & keep
        assert not bool(bad.any()), (what, '%d anchors differ in %s (first: image, anchor = %s)' % (
            int(bad.sum()), kind, torch.nonzero(bad)[0].tolist()))
    ref_label = torch.full_like(label, -1)
    for b in range(code.shape[0]):
        p = code[b] >= 0
        ref_label[b, p] = c['ann'][b, code[b, p], 4].long()
    bad = (label != ref_label) & keep
    assert not bool(bad.any()), (what, '%d anchors carry another label (first: image, anchor = %s)' % (
        int(bad.sum()), torch.nonzero(bad)[0].tolist()))


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('name', sorted(LC.CASES))
def test_focal_loss_edge_case(name, dtype):
    from efficientdet.pytorch_amd import ops
    c, ref_losses, ref_dlogit, ref_dreg, _, skip = _reference(name)
    B, A, nc = c['cls'].shape
    cls, reg, anc, ann = (c[k].cuda() for k in ('cls', 'reg', 'anc', 'ann'))
    gs = torch.tensor(GS).cuda()
    tol = 1e-3 if dtype == torch.float32 else 1e-2
    hold = (~skip)[:, :, None].double()          # all ones but for the near-threshold anchors of the nested-threshold case (see loss_cases)
    exact_everywhere = not bool(skip.any())

    def check(losses, dcls, dreg, what):
        if exact_everywhere:
            assert_close(losses.cpu(), ref_losses, 2e-4, what + ' losses')
        assert_close(dcls.double().cpu() * hold, ref_dlogit * hold, tol, what + ' dcls_logit')
        assert_close(dreg.double().cpu() * hold, ref_dreg * hold, tol, what + ' dreg')
        _check_states(name, dcls, dreg, what)

    losses, ws = ops.focal_loss_fwd(cls, reg, anc, ann)
    dcls, dreg = ops.focal_loss_bwd(cls, reg, anc, ann, gs, ws, dtype)
    check(losses, dcls, dreg, 'fwd + bwd')
    if nc % 4:
        return
    dld = LC.dld_for(nc)
    dpix, dreg2 = ops.focal_loss_bwd_pix(cls, reg, anc, ann, gs, ws, dtype, dld)
    assert dpix.shape == (B, A // 9, dld)
    assert float(dpix[:, :, 9 * nc:].float().abs().max()) == 0.0                      # pad channels exactly zero
    check(losses, dpix[:, :, :9 * nc].reshape(B, A, nc), dreg2, 'bwd_pix')
    assert torch.equal(dpix[:, :, :9 * nc].reshape(B, A, nc), dcls) and torch.equal(dreg2, dreg)
    # the training path: losses + d(cls) for an upstream gradient of one in a single pass, d(reg) on its own
    losses2, ws2, dpix1 = ops.focal_loss_fwd_grad(cls, reg, anc, ann, dtype, dld)
    dreg3 = ops.focal_loss_bwd_reg(reg, anc, ann, gs, ws2, dtype)
    assert float(dpix1[:, :, 9 * nc:].float().abs().max()) == 0.0
    check(losses2, dpix1[:, :, :9 * nc].reshape(B, A, nc).float() * GS[0], dreg3, 'fwd_grad + bwd_reg')
    assert torch.equal(dreg3, dreg)
