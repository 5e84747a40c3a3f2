"""GPU parity of the ATSS matcher (include/effdet_atss.h, csrc/loss.hip) on the cases of tests/atss_cases.py.

Codes: the workspace's leading [B][A] int32 equals the float32 mirror's codes (tests/atss_restated.py) exactly on every case --
tests/test_atss_host.py proves the margin that makes this a fair demand and pins the exact ties by hand.
Losses: against the float64 restatement (tests/loss_options_restated.py on the mirror's codes), assert_close at 2e-4, the bound of
tests/test_gpu_loss_options.py.
Gradients: that file's rule -- the device may deviate from float64 by FACTOR = 8 times the float32 restatement's largest deviation.
`pytest -s` prints the ratios.  Layouts, determinism and the garbage workspace are bit for bit."""
import ctypes
import functools

import pytest
import torch

from tests import atss_cases as AC
from tests import loss_cases as LC
from tests import loss_options_restated as R
from tests.gpu_util import assert_close

pytestmark = pytest.mark.gpu

FACTOR = 8.0
GS = (0.7, 1.3)
PAPER = dict(gamma=1.5, beta=0.1, reg_weight=50.0)                  # options that a matcher does not replace
RUNS = [(name, None) for name in sorted(AC.CASES)] + [('straddle', 'paper'), ('s128_nc4', 'paper')]


def _ropts(on):
    return R.options(**(PAPER if on else {}))


@functools.lru_cache(maxsize=None)
def _reference(name, on, box=None):
    """-> (float64 run, float32 run) of the loss restatement on the mirror's codes with the upstream gradients GS; read-only."""
    c, codes = AC.get(name), AC.codes(name)
    ref = R.run(c, _ropts(on), box=box, gscale=GS, dtype=torch.float64, codes=codes)
    return ref, R.run(c, _ropts(on), box=box, gscale=GS, dtype=torch.float32, codes=codes)


@functools.lru_cache(maxsize=None)
def _device_case(name):
    c = AC.get(name)
    return tuple(c[k].cuda() for k in ('cls', 'reg', 'anc', 'ann'))


def _kw(name, on=None):
    from efficientdet.pytorch_amd import ops
    c = AC.get(name)
    return dict(loss=ops.LossOptions(**PAPER) if on else None, matcher=ops.ATSSOptions(c['topk']), levels=AC.levels(c))


def _bwd_kw(kw):
    return dict(loss=kw['loss'], matcher=kw['matcher'])


def _gs(a=GS[0], b=GS[1]):
    return torch.tensor([a, b], dtype=torch.float32).cuda()


def _codes(ws, B, A):
    return ws[:B * A * 4].view(torch.int32).reshape(B, A).cpu().long()


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _unpix(dpix, B, A, nc):
    return dpix[:, :, :9 * nc].reshape(B, A, nc)


def _ratio(got, f32, ref):
    return float((got.double().cpu() - ref).abs().max()), float((f32.double() - ref).abs().max())


@pytest.mark.parametrize('run', RUNS, ids=lambda r: '%s-%s' % r)
def test_codes_losses_and_gradients(run):
    from efficientdet.pytorch_amd import ops
    name, on = run
    cls, reg, anc, ann = _device_case(name)
    B, A, nc = cls.shape
    ref, f32 = _reference(name, on)
    kw = _kw(name, on)
    losses, ws = ops.loss_opts_fwd(cls, reg, anc, ann, box=None, **kw)
    codes = _codes(ws, B, A)
    assert torch.equal(codes, ref['codes']), torch.nonzero(codes != ref['codes'])[:4].tolist()
    npos = ws[B * A * 4:].view(torch.int32)                                              # (the stat lines follow assign[], 256-byte aligned)
    off = (-(B * A * 4)) % 256 // 4
    assert [int(npos[off + b * 32 + 2]) for b in range(B)] == ref['num_pos'].tolist()
    assert_close(losses.cpu(), ref['losses'], 2e-4, '%s %s losses' % run)
    dcls = ops.loss_opts_bwd_cls(cls, ann, _gs(), ws, torch.float32, kw['loss'], matcher=kw['matcher'])
    dreg = ops.loss_opts_bwd_reg(reg, anc, ann, _gs(), ws, torch.float32, **_bwd_kw(kw))
    err_c, yard_c = _ratio(dcls, f32['dlogit'], ref['dlogit'])
    err_r, yard_r = _ratio(dreg, f32['dreg'], ref['dreg'])
    print('\n%s %s: losses %.9g %.9g (float64 %.9g %.9g) num_pos %s | dlogit err %.3g yardstick %.3g ratio %.2f | dreg err %.3g '
          'yardstick %.3g ratio %.2f' % (name, on, float(losses[0]), float(losses[1]), float(ref['losses'][0]), float(ref['losses'][1]),
                                         ref['num_pos'].tolist(), err_c, yard_c, err_c / max(yard_c, 1e-300), err_r, yard_r,
                                         err_r / max(yard_r, 1e-300)))
    assert yard_c > 0.0 and err_c <= FACTOR * yard_c, (run, 'dlogit', err_c, yard_c)
    assert err_r <= FACTOR * yard_r, (run, 'dreg', err_r, yard_r)
    # exact +0.0: d(reg) off the positives, d(logit) in an image without a valid row
    got_r, got_c = dreg.cpu(), dcls.cpu()
    assert int(_bits(got_r)[ref['codes'] < 0].abs().max()) == 0
    ign = ref['codes'] == LC.CODE_IGN
    if bool(ign.any()):
        assert int(_bits(got_c)[ign].abs().max()) == 0
    assert bool((got_c[~ign] != 0).all())
    # the training path: one pass over cls for losses and d(logit) at an upstream gradient of one, d(reg) from its workspace
    dld = LC.dld_for(nc)
    l2, ws2, dpix = ops.loss_opts_fwd_grad(cls, reg, anc, ann, torch.float32, dld, **kw)
    assert torch.equal(_codes(ws2, B, A), codes) and torch.equal(_bits(l2[1:2]), _bits(losses[1:2]))
    assert_close(l2.cpu(), ref['losses'], 2e-4, '%s %s fwd_grad losses' % run)
    assert int(_bits(dpix[:, :, 9 * nc:]).abs().max()) == 0
    one = ops.loss_opts_bwd_cls(cls, ann, _gs(1.0, 1.0), ws, torch.float32, kw['loss'], matcher=kw['matcher'])
    assert torch.equal(_bits(_unpix(dpix, B, A, nc)), _bits(one))
    assert torch.equal(_bits(ops.loss_opts_bwd_reg(reg, anc, ann, _gs(), ws2, torch.float32, **_bwd_kw(kw))), _bits(dreg))


def _split_halves(t):
    B, P, ld = t.shape
    h = t.contiguous().view(torch.bfloat16).reshape(B, P, ld // 32, 2, 32)
    return h[:, :, :, 0].reshape(B, P, ld), h[:, :, :, 1].reshape(B, P, ld)


def _same_values(f32_rows, pix, pix_bf16, rows_bf16, split, B, A, per, ld):
    """tests/test_gpu_loss_options.py's relation of the layouts of one gradient to its fp32 row form."""
    want = torch.zeros(B, A // 9, ld, dtype=torch.float32, device=f32_rows.device)
    want[:, :, :9 * per] = f32_rows.reshape(B, A // 9, 9 * per)
    assert torch.equal(_bits(pix), _bits(want))
    assert torch.equal(_bits(rows_bf16), _bits(f32_rows.bfloat16()))
    assert torch.equal(_bits(pix_bf16), _bits(want.bfloat16()))
    hi, lo = _split_halves(split)
    assert torch.equal(_bits(hi), _bits(want.bfloat16()))
    assert torch.equal(_bits(lo), _bits((want - want.bfloat16().float()).bfloat16()))


@pytest.mark.parametrize('name', ['straddle', 's128_nc80'])
def test_output_layouts(name):
    from efficientdet.pytorch_amd import ops
    cls, reg, anc, ann = _device_case(name)
    B, A, nc = cls.shape
    kw = _kw(name)
    dld = LC.dld_for(nc)
    _, ws, pix = ops.loss_opts_fwd_grad(cls, reg, anc, ann, torch.float32, dld, **kw)
    _, _, pix_bf16 = ops.loss_opts_fwd_grad(cls, reg, anc, ann, torch.bfloat16, dld, **kw)
    _, _, split = ops.loss_opts_fwd_grad(cls, reg, anc, ann, torch.float32, dld, split=True, **kw)
    one = _gs(1.0, 1.0)
    bwd_cls = functools.partial(ops.loss_opts_bwd_cls, cls, ann, loss=None, matcher=kw['matcher'])
    rows = bwd_cls(one, ws, torch.float32)
    _same_values(rows, pix, pix_bf16, bwd_cls(one, ws, torch.bfloat16), split, B, A, nc, dld)
    assert float(rows.abs().max()) > 0.0
    gs = _gs()
    rows = bwd_cls(gs, ws, torch.float32)
    want = torch.zeros(B, A // 9, dld, dtype=torch.float32, device=cls.device)
    want[:, :, :9 * nc] = rows.reshape(B, A // 9, 9 * nc)
    assert torch.equal(_bits(bwd_cls(gs, ws, torch.float32, dld=dld)), _bits(want))
    assert torch.equal(_bits(bwd_cls(gs, ws, torch.bfloat16, dld=dld)), _bits(want.bfloat16()))
    fn = functools.partial(ops.loss_opts_bwd_reg, reg, anc, ann, gs, ws, **_bwd_kw(kw))
    rows = fn(torch.float32)
    _same_values(rows, fn(torch.float32, reg_ld=64), fn(torch.bfloat16, reg_ld=64), fn(torch.bfloat16), fn(torch.float32, reg_ld=64, split=True),
                 B, A, 4, 64)
    assert float(rows.abs().max()) > 0.0
    pads = fn(torch.float32, reg_ld=64)[:, :, 36:]
    assert int(_bits(pads).abs().max()) == 0                                             # exact +0.0 in the pad channels


def test_giou_over_the_atss_assignment():
    from efficientdet.pytorch_amd import ops
    name = 's128_nc4'
    cls, reg, anc, ann = _device_case(name)
    B, A, nc = cls.shape
    box = ops.BoxLossOptions('giou', 2.0)
    ref, f32 = _reference(name, None, ('giou', 2.0))
    kw = _kw(name)
    losses, ws = ops.loss_opts_fwd(cls, reg, anc, ann, box=box, **kw)
    assert torch.equal(_codes(ws, B, A), ref['codes'])
    assert_close(losses.cpu(), ref['losses'], 2e-4, 'giou losses')
    dreg = ops.loss_opts_bwd_reg(reg, anc, ann, _gs(), ws, torch.float32, box=box, **_bwd_kw(kw))
    err, yard = _ratio(dreg, f32['dreg'], ref['dreg'])
    print('\ngiou over the ATSS assignment: losses[1] %.9g (float64 %.9g) | dreg err %.3g yardstick %.3g ratio %.2f'
          % (float(losses[1]), float(ref['losses'][1]), err, yard, err / max(yard, 1e-300)))
    assert yard > 0.0 and err <= FACTOR * yard
    assert int(_bits(dreg.cpu())[ref['codes'] < 0].abs().max()) == 0
    plain, ws1 = ops.loss_opts_fwd(cls, reg, anc, ann, **kw)
    assert torch.equal(_bits(plain[0:1]), _bits(losses[0:1])) and not torch.equal(_bits(plain[1:2]), _bits(losses[1:2]))
    assert torch.equal(_bits(ops.box_loss_bwd_reg(reg, anc, ann, _gs(), ws1, torch.float32, options=box)), _bits(dreg))
    l2, _, _ = ops.loss_opts_fwd_grad(cls, reg, anc, ann, torch.float32, LC.dld_for(nc), box=box, **kw)
    assert torch.equal(_bits(l2[1:2]), _bits(losses[1:2]))


def _raw(name, ws, losses, topk=None, starts=None, num_levels=None, low_quality=0, null=False, dpix=None):
    from efficientdet.pytorch_amd import _lib as L
    c = AC.get(name)
    cls, reg, anc, ann = _device_case(name)
    B, A, nc = cls.shape
    N = ann.shape[1]
    starts = c['level_start'] if starts is None else starts
    t = L.Atss(c['topk'] if topk is None else topk, len(starts) - 1 if num_levels is None else num_levels)
    for i, v in enumerate(starts[:9]):
        t.level_start[i] = v
    d = R.DEFAULTS
    o = L.LossOpts(d['alpha'], d['gamma'], d['label_smoothing'], d['beta'], d['reg_weight'], d['pos_iou'], d['neg_iou'], low_quality, 0, 1.0)
    lib = L.require('effdet_loss_atss_fwd', 'effdet_loss_atss_fwd_grad')
    at = None if null else ctypes.byref(t)
    if dpix is None:
        return lib.effdet_loss_atss_fwd(L.ptr(cls), L.ptr(reg), L.ptr(anc), L.ptr(ann), L.ptr(losses), L.ptr(ws), ws.numel(), B, A, nc, N,
                                        ctypes.byref(o), at, L.stream_ptr())
    return lib.effdet_loss_atss_fwd_grad(L.ptr(cls), L.ptr(reg), L.ptr(anc), L.ptr(ann), L.ptr(losses), L.ptr(ws), ws.numel(), L.ptr(dpix),
                                         dpix.shape[2], L.F32, B, A, nc, N, ctypes.byref(o), at, L.stream_ptr())


@pytest.mark.parametrize('name', ['straddle', 's128_nc4'])
def test_two_runs_and_a_garbage_workspace_are_bitwise_equal(name):
    from efficientdet.pytorch_amd import ops
    cls, reg, anc, ann = _device_case(name)
    B, A, nc = cls.shape
    kw = _kw(name)
    runs = []
    for _ in range(2):
        losses, ws, dpix = ops.loss_opts_fwd_grad(cls, reg, anc, ann, torch.float32, LC.dld_for(nc), **kw)
        runs.append((losses.clone(), dpix, ops.loss_opts_bwd_reg(reg, anc, ann, _gs(), ws, torch.float32, **_bwd_kw(kw)),
                     ws[:B * A * 4].view(torch.float32).clone()))
    for a, b in zip(*runs):
        assert torch.equal(_bits(a), _bits(b))
    ws = torch.full((ws.numel(),), 0xFF, dtype=torch.uint8, device=cls.device)
    losses = torch.empty(2, device=cls.device)
    dpix = torch.empty_like(runs[0][1])
    assert _raw(name, ws, losses, dpix=dpix) == 0
    dreg = ops.loss_opts_bwd_reg(reg, anc, ann, _gs(), ws, torch.float32, **_bwd_kw(kw))
    for a, b in zip(runs[0], (losses, dpix, dreg, ws[:B * A * 4].view(torch.float32))):
        assert torch.equal(_bits(a), _bits(b))


def test_error_codes_and_nothing_enqueued():
    from efficientdet.pytorch_amd import _lib as L
    name = 'straddle'
    cls, reg, anc, ann = _device_case(name)
    B, A, nc = cls.shape
    c = AC.get(name)
    t = L.Atss(9, 2)
    t.level_start[1], t.level_start[2] = 252, 261
    nbytes = int(L.require('effdet_loss_atss_workspace_bytes').effdet_loss_atss_workspace_bytes(B, A, nc, ann.shape[1], ctypes.byref(t)))
    assert nbytes > 0
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=cls.device)
    losses = torch.full((2,), 7.0, device=cls.device)
    dpix = torch.full((B, A // 9, LC.dld_for(nc)), 7.0, device=cls.device)
    EINVAL = -1
    bad = [dict(topk=0), dict(topk=17), dict(topk=-3), dict(num_levels=0), dict(starts=list(range(0, 9 * 29, 29)), num_levels=9),
           dict(starts=[0, 252, 252, 261]), dict(starts=[0, 256, 252, 261]), dict(starts=[0, 252, 260]), dict(starts=[0, 252, 262]),
           dict(starts=[1, 252, 261]), dict(low_quality=1), dict(null=True)]
    for kw in bad:
        assert _raw(name, ws, losses, **kw) == EINVAL, kw
        assert _raw(name, ws, losses, dpix=dpix, **kw) == EINVAL, kw
    assert _raw(name, ws[:nbytes - 1], losses) == EINVAL                                 # the twin's conditions
    torch.cuda.synchronize()
    assert bool((losses == 7.0).all()) and bool((dpix == 7.0).all()) and int(ws.max()) == 0      # no kernel ran
    assert _raw(name, ws, losses, dpix=dpix) == 0
    torch.cuda.synchronize()
    assert not bool((losses == 7.0).any()) and not bool((dpix == 7.0).any())
    assert torch.equal(_codes(ws, B, A), AC.codes(name)) and c['topk'] == 9
