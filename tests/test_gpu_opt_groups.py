"""GPU tier, op level, of the parameter groups and the SGD rule of the fused optimizer step: the GROUPED instantiations of
csrc/optim.hip's update kernel behind effdet_opt_step_groups, optim.ClipAdamW with several groups and optim.ClipSGD.

Every comparison is bitwise on parameters, moments, step counters and the norm unless a tolerance is named.  The oracles are the
one-group ClipAdamW (the code of the one-group calls is unchanged), one plain ClipAdamW per group, the NumPy float32 restatements
(tests/opt_groups_restated.py, tests/ema_restated.py) and, within 1e-5, clip_grad_norm_ + torch.optim.AdamW / torch.optim.SGD."""
import copy

import numpy as np
import pytest
import torch

from tests import ema_restated as E
from tests import opt_groups_restated as R
from tests.gpu_util import assert_close

pytestmark = pytest.mark.gpu

F = np.float32
# tests/test_gpu_ema.py's sizes -- one element; below, at and above a float4; a partial chunk; one workgroup chunk (4096) -1 / exact / +1;
# two chunks + 1; the parameter that is a view 4 bytes into a larger buffer (scalar path); the one that never has a gradient -- in the
# table order of the three-group dealing: group 0 ends with the 4096-element tensor (the boundary falls right behind a full chunk),
# group 1 is the single 1-element tensor, group 2 holds only the tensor without a gradient; a fourth group is empty once its frozen
# tensor is filtered out.
SIZES = (3, 4, 5, 1023, 4095, 4097, 8193, 1030, 4096, 1, 517)
VIEW, NO_GRAD, LOSES = 7, 10, 4           # LOSES: has no gradient in the second step only (the SGD tests)
THREE = ((0, 9), (9, 10), (10, 11))       # [first, end) of each group in the table
TWO = ((0, 9), (9, 11))                   # the SGD tests' second dealing: two groups, the boundary behind the 4096-element tensor


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    ps, keep = [], []
    for i, n in enumerate(SIZES):
        x = torch.randn(n, generator=g).cuda()
        if i == VIEW:
            buf = torch.zeros(n + 8, device='cuda')
            buf[1:1 + n].copy_(x)
            p = torch.nn.Parameter(buf[1:1 + n])
            assert p.data_ptr() % 16 == 4 and p.is_contiguous()
            keep.append(buf)
        else:
            p = torch.nn.Parameter(x)
        ps.append(p)
    frozen = torch.nn.Parameter(torch.randn(7, generator=g).cuda(), requires_grad=False)
    return ps, keep + [frozen]


def _groups(ps, frozen, hypers, dealing=THREE):
    gs = [dict(params=ps[a:b], **h) for (a, b), h in zip(dealing, hypers)]
    return gs + [dict(params=[frozen])]                     # empty after requires_grad filtering: legal, its row is never read


def _grads(seed, scale=1.0):
    g = torch.Generator().manual_seed(1000 + seed)
    return [torch.randn(n, generator=g).cuda() * scale for n in SIZES]


def _set_grads(ps, gs, skip=(NO_GRAD,), first=0):
    for i, p in enumerate(ps):
        p.grad = None if (first + i) in skip else gs[first + i].clone()


def _np(ts):
    torch.cuda.synchronize()
    return [t.detach().cpu().numpy().copy() for t in ts]


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _t_bits(a, b):
    return _bits(a.detach().cpu().numpy(), b.detach().cpu().numpy())


def _assert_same(ps, opt, ps_t, opt_t, where, first=0, norm=True):
    """Bitwise: parameters, every moment, step counters and (optionally) the norm of opt against the twin over ps_t, whose table
    starts at tensor `first` of opt's."""
    torch.cuda.synchronize()
    for i, q in enumerate(ps_t):
        p = ps[first + i]
        assert _t_bits(p, q), ('parameter', first + i, where)
        for _, key in opt.MOMENTS:
            assert _t_bits(opt.state[p][key], opt_t.state[q][key]), (key, first + i, where)
    n = len(ps_t)
    assert torch.equal(opt._table['steps'][first:first + n], opt_t._table['steps']), ('steps', where)
    if norm:
        assert _t_bits(opt._table['scratch'][:1], opt_t._table['scratch'][:1]), ('norm', where)
    if opt.ema and opt_t.ema:
        for i in range(n):
            assert _t_bits(opt.ema_params()[first + i], opt_t.ema_params()[i]), ('ema', first + i, where)
        assert opt.ema_updates() == opt_t.ema_updates(), where


def _loss(v):
    return torch.tensor(v, dtype=torch.float32, device='cuda')


# ------------------------------------------------------------------------------------------------ 1: equal rows are the one-group step
@pytest.mark.parametrize('ema,accumulate', [(None, False), (0.5, False), (None, True), (0.5, True)], ids=['plain', 'ema', 'gated', 'gated_ema'])
def test_groups_with_equal_hypers_are_the_one_group_optimizer(ema, accumulate):
    """3 steps.  The gated forms run through accumulate_grads, two micro-steps per step, the second one of step 1 with a zero loss (so
    that step's boundary gate is closed and its gradient rides into step 2's window, as in train.py)."""
    from efficientdet.pytorch_amd.optim import ClipAdamW
    kw = dict(lr=1e-3, max_norm=0.1, ema_decay=ema, accumulate=accumulate)
    ps, keep = _params()
    opt = ClipAdamW(_groups(ps, keep[-1], [{}, {}, {}]), **kw)
    ps_t, keep_t = _params()
    opt_t = ClipAdamW(ps_t, **kw)
    assert len(opt.param_groups) == 4 and len(opt_t.param_groups) == 1
    for step in range(3):
        if accumulate:
            for micro, l in enumerate((1.0, 0.0 if step == 1 else 1.0)):
                gs = _grads(10 * step + micro)
                for q, o in ((ps, opt), (ps_t, opt_t)):
                    _set_grads(q, gs); o.accumulate_grads(_loss(l))
        else:
            gs = _grads(step)
            _set_grads(ps, gs); _set_grads(ps_t, gs)
        opt.step(); opt_t.step()
        _assert_same(ps, opt, ps_t, opt_t, step)
    assert opt._table['grouped'] and not opt_t._table['grouped'] and opt._table['ngroups'] == 4
    assert opt._table['tensor_group'].tolist() == [0] * 9 + [1, 2]
    want = 2 if accumulate else 3
    assert opt._table['steps'].tolist() == [want if i != NO_GRAD else 0 for i in range(len(SIZES))]
    if accumulate:
        assert opt.loss_meter()[1:] == opt_t.loss_meter()[1:] == (5, 1, 2)
    assert torch.equal(keep[-1], _params()[1][-1])           # the frozen tensor of the fourth group was never in the table


# ------------------------------------------------------------------------------------------------ 2, 3: distinct rows, one global norm
HYPERS = [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2),
          dict(lr=3e-2, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.0),
          dict(lr=5e-4, betas=(0.95, 0.9), eps=1e-3, weight_decay=0.3)]


def _twins(ema=None):
    from efficientdet.pytorch_amd.optim import ClipAdamW
    ps_t, keep_t = _params()
    return ps_t, keep_t, [ClipAdamW(ps_t[a:b], max_norm=0.0, ema_decay=ema, **h) for (a, b), h in zip(THREE, HYPERS)]


@pytest.mark.parametrize('ema', [None, 0.5], ids=['plain', 'ema'])
def test_distinct_hypers_without_clipping_are_one_optimizer_per_group(ema):
    from efficientdet.pytorch_amd.optim import ClipAdamW
    ps, keep = _params()
    opt = ClipAdamW(_groups(ps, keep[-1], HYPERS), max_norm=0.0, ema_decay=ema)
    ps_t, keep_t, twins = _twins(ema)
    for step in range(3):
        gs = _grads(step)
        _set_grads(ps, gs); opt.step()
        for (a, b), tw in zip(THREE, twins):
            _set_grads(ps_t[a:b], gs, first=a); tw.step()
            _assert_same(ps, opt, ps_t[a:b], tw, (step, a), first=a, norm=False)
        if step == 0:
            # the rows really differ: AdamW's first update is lr * g / (|g| + eps), so group 1's tensor moved by its lr of 3e-2 and
            # group 0's by theirs of 1e-3 (plus the decay term lr * wd * |p| <= 1e-5 * 5)
            p0 = _params()[0]
            d9, d8 = float((ps[9] - p0[9]).detach().abs().max()), float((ps[8] - p0[8]).detach().abs().max())
            assert 0.029 < d9 < 0.031 and 0.0009 < d8 < 0.0011, (d9, d8)


def test_all_groups_share_the_one_global_norm():
    """max_norm = 0.1: every per-group twin runs WITHOUT clipping on grad * coef, coef = min(1, 0.1 / (norm + 1e-6)) computed here in
    float32 from the grouped optimizer's grad_norm(): a norm per group would give other coefficients.  Step 0 has small gradients
    (coef == 1), steps 1 and 2 are clipped.  Against clip_grad_norm_ + a grouped torch.optim.AdamW on the same GPU tensors: parameters
    within 1e-5 (tests/gpu_util.assert_close, test_clip_adamw_matches_torch's gate), the norm within 2e-6 relative."""
    from efficientdet.pytorch_amd.optim import ClipAdamW
    ps, keep = _params()
    opt = ClipAdamW(_groups(ps, keep[-1], HYPERS), max_norm=0.1)
    ps_t, keep_t, twins = _twins()
    ps_r, keep_r = _params()
    ref = torch.optim.AdamW([dict(params=ps_r[a:b], **h) for (a, b), h in zip(THREE, HYPERS)])
    coefs = []
    for step in range(3):
        gs = _grads(step, 1e-4 if step == 0 else 1.0)
        _set_grads(ps, gs); opt.step()
        norm = F(float(opt.grad_norm()))
        coef = R.clip_coef(0.1, norm)
        coefs.append(float(coef))
        one_group_norm = torch.cat([g.reshape(-1) for i, g in enumerate(gs) if i != NO_GRAD]).double().norm()
        assert abs(float(norm) - float(one_group_norm)) <= 2e-6 * float(one_group_norm)
        scaled = [g * torch.tensor(coef, device='cuda') for g in gs]          # one fp32 product per element, as the kernel's coef * g
        for (a, b), tw in zip(THREE, twins):
            _set_grads(ps_t[a:b], scaled, first=a); tw.step()
            _assert_same(ps, opt, ps_t[a:b], tw, (step, a), first=a, norm=False)
        _set_grads(ps_r, gs)
        ref_norm = torch.nn.utils.clip_grad_norm_(ps_r, 0.1)
        ref.step()
        assert abs(float(norm) - float(ref_norm)) <= 2e-6 * float(ref_norm)
        for i, (p, q) in enumerate(zip(ps, ps_r)):
            assert_close(p, q, 1e-5, 'parameter %d step %d' % (i, step))
    assert coefs[0] == 1.0 and coefs[1] < 1.0 and coefs[2] < 1.0, coefs


# ------------------------------------------------------------------------------------------------ 4: a group held still
@pytest.mark.parametrize('ema', [None, 0.5], ids=['plain', 'ema'])
def test_a_group_with_zero_lr_and_decay_stands_still(ema):
    from efficientdet.pytorch_amd.optim import ClipAdamW
    ps, keep = _params()
    still = dict(HYPERS[0], lr=0.0, weight_decay=0.0)
    opt = ClipAdamW(_groups(ps, keep[-1], [still, HYPERS[1], HYPERS[2]]), max_norm=0.1, ema_decay=ema)
    p0 = _np(ps)
    for step in range(3):
        _set_grads(ps, _grads(step)); opt.step()
    p1 = _np(ps)
    for i in range(9):                                       # group 0: not a bit moved, yet its moments and counters advanced
        assert _bits(p1[i], p0[i]), i
        assert float(opt.state[ps[i]]['exp_avg'].abs().max()) > 0 and float(opt.state[ps[i]]['exp_avg_sq'].abs().max()) > 0, i
    assert opt._table['steps'].tolist() == [3] * 10 + [0]
    assert not _bits(p1[9], p0[9]) and _bits(p1[NO_GRAD], p0[NO_GRAD])       # group 1 moved; the tensor without a gradient did not
    if ema:
        e = _np(opt.ema_params())
        for i in range(9):
            assert _bits(e[i], p0[i]), i                     # the average stays on the parameters it started on
        assert not _bits(e[9], p1[9]) and opt.ema_updates() == 3
    # the row is read at run time: restoring the lr moves the group again
    opt.param_groups[0]['lr'] = 1e-3
    _set_grads(ps, _grads(3)); opt.step()
    assert not any(_bits(a, b) for a, b in zip(_np(ps[:9]), p0[:9]))


# ------------------------------------------------------------------------------------------------ 5: ClipSGD
SGD_CONFIGS = {
    'momentum0': (TWO, [dict(momentum=0.0, weight_decay=0.0), dict(momentum=0.0, weight_decay=4e-5)]),
    'momentum': (TWO, [dict(momentum=0.9, weight_decay=4e-5), dict(momentum=0.9, weight_decay=0.0, lr=0.01)]),
    'nesterov': (TWO, [dict(momentum=0.9, nesterov=True, weight_decay=4e-5), dict(momentum=0.5, nesterov=True)]),
    'dampening': (TWO, [dict(momentum=0.9, dampening=0.1, weight_decay=4e-5), dict(momentum=0.9, dampening=0.1)]),
    'mixed3': (THREE, [dict(momentum=0.9, nesterov=True, weight_decay=4e-5), dict(momentum=0.0, lr=0.2), dict(momentum=0.9, dampening=0.1)]),
}
SGD_LR = 0.05


def _sgd(name, max_norm=0.1, **kw):
    from efficientdet.pytorch_amd.optim import ClipSGD
    dealing, hypers = SGD_CONFIGS[name]
    ps, keep = _params()
    opt = ClipSGD(_groups(ps, keep[-1], hypers, dealing), lr=SGD_LR, max_norm=max_norm, **kw)
    opt._keep = keep
    return ps, opt


def _hyper_of_tensor(name):
    dealing, hypers = SGD_CONFIGS[name]
    out = []
    for (a, b), h in zip(dealing, hypers):
        h = dict(dict(lr=SGD_LR, momentum=0.0, dampening=0.0, nesterov=False, weight_decay=0.0), **h)
        out += [h] * (b - a)
    return out


def _skip(step):
    return (NO_GRAD, LOSES) if step == 1 else (NO_GRAD,)


@pytest.mark.parametrize('max_norm', [0.1, 0.0])
@pytest.mark.parametrize('name', list(SGD_CONFIGS))
def test_clip_sgd_is_the_restatement_and_matches_torch(name, max_norm):
    """4 steps; tensor 4 loses its gradient in the second step (its buffer stays, its count lags), tensor 10 never has one.  Bitwise
    against the restatement driven by the device's own grad_norm(); within 1e-5 (assert_close, the AdamW test's gate -- generous here:
    the rule has no division and no square root) against clip_grad_norm_ + torch.optim.SGD on the same GPU tensors."""
    ps, opt = _sgd(name, max_norm)
    hy = _hyper_of_tensor(name)
    dealing, hypers = SGD_CONFIGS[name]
    ps_r, keep_r = _params()
    ref = torch.optim.SGD([dict(params=ps_r[a:b], **h) for (a, b), h in zip(dealing, hypers)], lr=SGD_LR)
    mine, bufs, counts = _np(ps), [np.zeros(n, F) for n in SIZES], [0] * len(SIZES)
    for step in range(4):
        gs = _grads(step, 1e-4 if step == 0 else 1.0)
        _set_grads(ps, gs, _skip(step)); opt.step()
        _set_grads(ps_r, gs, _skip(step))
        if max_norm:
            ref_norm = torch.nn.utils.clip_grad_norm_(ps_r, max_norm)
            assert abs(float(opt.grad_norm()) - float(ref_norm)) <= 2e-6 * float(ref_norm)
        ref.step()
        coef = R.clip_coef(max_norm, F(float(opt.grad_norm())))
        assert (coef == 1.0) == (step == 0 or not max_norm)
        for i in range(len(SIZES)):
            if i in _skip(step):
                continue
            counts[i] += 1
            h = hy[i]
            mine[i], bufs[i] = R.sgd(mine[i], bufs[i], gs[i].cpu().numpy(), counts[i], h['lr'], h['momentum'], h['dampening'], h['nesterov'],
                                     h['weight_decay'], coef)
        got, got_b = _np(ps), _np([opt.state[p]['momentum_buffer'] for p in ps])
        for i in range(len(SIZES)):
            assert _bits(got[i], mine[i]), ('parameter', i, SIZES[i], step)
            assert _bits(got_b[i], bufs[i]), ('momentum buffer', i, SIZES[i], step)
            assert_close(ps[i], ps_r[i], 1e-5, 'parameter %d step %d against torch.optim.SGD' % (i, step))
        assert opt._table['steps'].tolist() == counts
    assert counts == [4] * 4 + [3] + [4] * 5 + [0]
    assert not hasattr(opt, 'exp_avg') and len(opt.moment_arenas()) == 1
    assert opt._keep[0][0] == 0 and opt._keep[0][1 + SIZES[VIEW]] == 0       # the view's neighbours


@pytest.mark.parametrize('name', ['momentum', 'mixed3'])
def test_clip_sgd_average_is_the_restatement_over_the_sgd_trajectory(name):
    """As tests/test_gpu_ema.py does over AdamW's: the step with the average is bit for bit the step without it, and the average is
    tests/ema_restated.py driven by that trajectory (decay 0.5 crosses the end of the warm-up at t = 8)."""
    decay = 0.5
    ps, opt = _sgd(name, ema_decay=decay)
    ps_t, opt_t = _sgd(name)
    ema = _np(ps)
    for step in range(10):
        gs = _grads(step)
        _set_grads(ps, gs, _skip(step)); _set_grads(ps_t, gs, _skip(step))
        opt.step(); opt_t.step()
        _assert_same(ps, opt, ps_t, opt_t, step)
        ema = [E.update(e, p, decay, True, step) for e, p in zip(ema, _np(ps_t))]
        for i, (a, b) in enumerate(zip(_np(opt.ema_params()), ema)):
            assert _bits(a, b), ('ema', i, step)
    assert opt.ema_updates() == 10
    assert torch.equal(opt.ema_params()[NO_GRAD], ps[NO_GRAD]) and not torch.equal(opt.ema_params()[6], ps[6])
    p_before = _np(ps)
    opt.swap_ema()                                           # the swap and the context manager are the shared surface
    assert all(_bits(a, b) for a, b in zip(_np(ps), ema))
    with pytest.raises(RuntimeError, match='swapped in'):
        opt.step()
    opt.swap_ema()
    assert all(_bits(a, b) for a, b in zip(_np(ps), p_before))


@pytest.mark.parametrize('ema', [None, 0.5], ids=['gated', 'gated_ema'])
def test_clip_sgd_gated_forms_apply_or_leave_everything_untouched(ema):
    """Window of two, micro-losses 1, 0, 1, 1, 0, 1 with step() on every second micro-step and once more behind the fifth (the sequence
    of tests/test_gpu_ema.py): an open gate is the ungated step on the window's sum, a closed one leaves parameters, buffer, counters,
    average and its counter untouched."""
    ps, opt = _sgd('mixed3', accumulate=True, ema_decay=ema)
    ps_t, opt_t = _sgd('mixed3', ema_decay=ema)
    losses = [1.0, 0.0, 1.0, 1.0, 0.0, 1.0]
    pend, applied = [], 0

    def arenas():
        torch.cuda.synchronize()
        a = [torch.cat([p.detach().reshape(-1) for p in ps]).clone(), opt.momentum_buf.clone(), opt._table['steps'].clone()]
        return a + ([opt.ema_avg.clone(), opt._table['ectl'].clone()] if ema else [])
    for idx, l in enumerate(losses):
        gs = _grads(idx)
        _set_grads(ps, gs)
        opt.accumulate_grads(_loss(l))
        if l != 0.0:
            pend.append(gs)
        for _ in ([True] if (idx + 1) % 2 == 0 else []) + ([True] if idx == 4 else []):
            before = arenas()
            opt.step()
            open_gate = l != 0.0 and bool(pend)
            if open_gate:
                acc = pend[0]
                for g in pend[1:]:
                    acc = [a + b for a, b in zip(acc, g)]
                pend = []
                _set_grads(ps_t, acc); opt_t.step()
                applied += 1
                _assert_same(ps, opt, ps_t, opt_t, idx)
            else:
                for a, b in zip(arenas(), before):
                    assert torch.equal(a, b), idx
            assert opt.loss_meter()[3] == applied
    assert applied == 2 and opt.loss_meter()[1:] == (4, 2, 2) and opt.pending() == 0


# ------------------------------------------------------------------------------------------------ 6: checkpoints
def _run(opt, ps, steps, first, skip=_skip):
    for s in range(first, first + steps):
        _set_grads(ps, _grads(s), skip(s)); opt.step()
    torch.cuda.synchronize()


def test_grouped_clip_adamw_resumes_bit_equal_and_loads_torch_adamw():
    from efficientdet.pytorch_amd.optim import ClipAdamW
    mk = lambda ps, keep: ClipAdamW(_groups(ps, keep[-1], copy.deepcopy(HYPERS)), max_norm=0.1, ema_decay=0.5)
    ps_w, keep_w = _params(); whole = mk(ps_w, keep_w)
    _run(whole, ps_w, 5, 0)
    ps_f, keep_f = _params(); first = mk(ps_f, keep_f)
    _run(first, ps_f, 3, 0)
    sd = copy.deepcopy(first.state_dict())
    assert len(sd['param_groups']) == 4 and [len(g['params']) for g in sd['param_groups']] == [9, 1, 1, 1]
    assert [g['lr'] for g in sd['param_groups'][:3]] == [h['lr'] for h in HYPERS] and sd['ema_updates'] == 3
    assert [float(sd['state'][i]['step']) for i in range(11)] == [3.0, 3.0, 3.0, 3.0, 2.0, 3.0, 3.0, 3.0, 3.0, 3.0, 0.0]
    ps_r, keep_r = _params(seed=5)                           # other weights: everything must come from the checkpoint
    with torch.no_grad():
        for p, q in zip(ps_r, ps_f):
            p.copy_(q)
    resumed = mk(ps_r, keep_r)
    for g in resumed.param_groups:
        g['lr'] = 123.0                                      # ... the groups' hypers included
    resumed.load_state_dict(sd)
    assert [g['lr'] for g in resumed.param_groups[:3]] == [h['lr'] for h in HYPERS]
    _run(resumed, ps_r, 2, 3)
    _assert_same(ps_w, whole, ps_r, resumed, 'resumed')
    # a grouped torch.optim.AdamW state over the same parameter lists
    ps_a, keep_a = _params()
    ref = torch.optim.AdamW([dict(params=ps_a[a:b], **h) for (a, b), h in zip(THREE, HYPERS)] + [dict(params=[keep_a[-1]])])
    for s in range(2):
        _set_grads(ps_a, _grads(s)); ref.step()
    ps_l, keep_l = _params()
    loaded = ClipAdamW(_groups(ps_l, keep_l[-1], copy.deepcopy(HYPERS)), max_norm=0.1)
    loaded.load_state_dict(ref.state_dict())
    assert loaded._table['steps'].tolist() == [2] * 10 + [0] and all(g['max_norm'] == 0.1 for g in loaded.param_groups)
    for p, q in zip(ps_l, ps_a):
        if ref.state.get(q):
            assert torch.equal(loaded.state[p]['exp_avg'], ref.state[q]['exp_avg'])
            assert torch.equal(loaded.state[p]['exp_avg_sq'], ref.state[q]['exp_avg_sq'])
    with torch.no_grad():
        for p, q in zip(ps_l, ps_a):
            p.copy_(q)
    _set_grads(ps_l, _grads(2)); loaded.step()               # and steps on with them: the third step of every group's own schedule
    torch.cuda.synchronize()
    assert loaded._table['steps'].tolist() == [3] * 10 + [0]


def test_clip_sgd_checkpoints_speak_torch_sgd():
    from efficientdet.pytorch_amd.optim import ClipSGD
    ps_w, whole = _sgd('mixed3', ema_decay=0.5)
    _run(whole, ps_w, 5, 0)
    ps_f, first = _sgd('mixed3', ema_decay=0.5)
    _run(first, ps_f, 3, 0)
    sd = copy.deepcopy(first.state_dict())
    assert sd['state'][0]['momentum_buffer'] is not None and float(sd['state'][LOSES]['step']) == 2.0
    assert sd['state'][9]['momentum_buffer'] is None          # group 1 has momentum 0: torch keeps None there
    assert sd['state'][NO_GRAD]['momentum_buffer'] is None     # never stepped
    assert sorted(sd['param_groups'][0]) == ['dampening', 'ema_decay', 'lr', 'max_norm', 'momentum', 'nesterov', 'params', 'weight_decay']
    ps_r, resumed = _sgd('mixed3', ema_decay=0.5)
    with torch.no_grad():
        for p, q in zip(ps_r, ps_f):
            p.copy_(q)
    resumed.load_state_dict(sd)
    _run(resumed, ps_r, 2, 3)
    _assert_same(ps_w, whole, ps_r, resumed, 'resumed')
    # torch.optim.SGD's own state: momentum_buffer per parameter and no step; a tensor with a buffer continues (step 1), one without starts
    dealing, hypers = SGD_CONFIGS['momentum']
    ps_a, keep_a = _params()
    torch_groups = lambda: [dict(params=ps_a[a:b], **h) for (a, b), h in zip(dealing, hypers)] + [dict(params=[keep_a[-1]])]
    ref = torch.optim.SGD(torch_groups(), lr=SGD_LR)
    for s in range(2):
        _set_grads(ps_a, _grads(s)); ref.step()
    ps_l, loaded = _sgd('momentum', max_norm=0.0)
    loaded.load_state_dict(ref.state_dict())
    assert loaded._table['steps'].tolist() == [1] * 10 + [0] and all(g['max_norm'] == 0.0 for g in loaded.param_groups)
    for p, q in zip(ps_l[:10], ps_a[:10]):
        assert torch.equal(loaded.state[p]['momentum_buffer'], ref.state[q]['momentum_buffer'])
    with torch.no_grad():
        for p, q in zip(ps_l, ps_a):
            p.copy_(q)
    _set_grads(ps_l, _grads(2)); loaded.step()
    _set_grads(ps_a, _grads(2)); ref.step()
    for i, (p, q) in enumerate(zip(ps_l, ps_a)):
        assert_close(p, q, 1e-5, 'parameter %d after the loaded state' % i)
    # and back: torch.optim.SGD loads ClipSGD's state
    back = torch.optim.SGD(torch_groups(), lr=SGD_LR)
    back.load_state_dict(loaded.state_dict())
    assert torch.equal(back.state[ps_a[0]]['momentum_buffer'], loaded.state[ps_l[0]]['momentum_buffer'])


def test_add_param_group_after_the_first_step_raises():
    from efficientdet.pytorch_amd.optim import ClipAdamW
    for make in (lambda ps, keep: ClipAdamW(_groups(ps, keep[-1], HYPERS), max_norm=0.1), lambda ps, keep: _sgd('momentum')[1]):
        ps, keep = _params()
        opt = make(ps, keep)
        extra = torch.nn.Parameter(torch.zeros(5, device='cuda'))
        late = torch.nn.Parameter(torch.zeros(5, device='cuda'))
        opt.add_param_group({'params': [extra]})             # before the tables exist: one more row
        ps2 = [p for g in opt.param_groups for p in g['params'] if p.requires_grad]
        for p in ps2:
            p.grad = torch.ones_like(p)
        opt.step()
        assert opt._table['ngroups'] == len(opt.param_groups) and opt._table['n'] == len(ps2)
        with pytest.raises(RuntimeError, match='add_param_group'):
            opt.add_param_group({'params': [late]})
