"""GPU tier of the parameter EMA: the EMA instantiations of csrc/optim.hip's step kernels, ema_swap_kernel, optim.ClipAdamW(ema_decay=...),
the captured steps of graph.py and checkpoint.ema_state_dict.

Every comparison is bitwise.  The average is pinned by the NumPy float32 restatement (tests/ema_restated.py) driven by the parameter
trajectory of a twin ClipAdamW WITHOUT the average, which must itself stay bit-equal to the one with it: the EMA instantiations run the
EMA-less kernels' arithmetic and add a stream, and the recurrence is three separately rounded fp32 operations (a contracted FMA would
differ in the last bit on a fraction of the elements)."""
import numpy as np
import pytest
import torch

from oracle import effdet_oracle as O
from tests import ema_restated as R

pytestmark = pytest.mark.gpu

# one element; below, at and above a float4; a partial chunk; one workgroup chunk (4096) -1 / exact / +1; two chunks + 1; then the
# parameter that is a view 4 bytes into a larger buffer (scalar path for p, m, v) and the one that never has a gradient
SIZES = (1, 3, 4, 5, 1023, 4095, 4096, 4097, 8193, 1030, 517)
VIEW, NO_GRAD = 9, 10
NC = 8


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
    return ps, keep


def _opt(ema_decay=None, accumulate=False, seed=0, **kw):
    from efficientdet.pytorch_amd.optim import ClipAdamW
    ps, keep = _params(seed)
    opt = ClipAdamW(ps, lr=1e-3, max_norm=0.1, accumulate=accumulate, ema_decay=ema_decay, **kw)
    opt._keep = keep
    return ps, opt


def _grads(seed):
    g = torch.Generator().manual_seed(1000 + seed)
    return [torch.randn(n, generator=g).cuda() for n in SIZES]


def _set_grads(ps, gs):
    for i, (p, g) in enumerate(zip(ps, gs)):
        p.grad = None if i == NO_GRAD else g.clone()


def _np(ts):
    torch.cuda.synchronize()
    return [t.detach().cpu().numpy().copy() for t in ts]


def _bits_equal(a, b, equal_nan=False):
    a, b = np.asarray(a), np.asarray(b)
    if equal_nan:
        return np.array_equal(a, b, equal_nan=True)
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _assert_twin(ps, opt, ps_t, opt_t, where):
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(ps, ps_t)):
        assert _bits_equal(a.detach().cpu().numpy(), b.detach().cpu().numpy(), equal_nan=True), ('parameter', i, where)
    for i, (p, q) in enumerate(zip(ps, ps_t)):
        for k in ('exp_avg', 'exp_avg_sq'):
            assert _bits_equal(opt.state[p][k].cpu().numpy(), opt_t.state[q][k].cpu().numpy(), equal_nan=True), (k, i, where)
    assert torch.equal(opt._table['steps'], opt_t._table['steps']), ('steps', where)
    assert _bits_equal(opt._table['scratch'][:1].cpu().numpy(), opt_t._table['scratch'][:1].cpu().numpy(), equal_nan=True), ('norm', where)


def _assert_ema(opt, want, where, equal_nan=False):
    got = _np(opt.ema_params())
    for i, (a, b) in enumerate(zip(got, want)):
        if not _bits_equal(a, b, equal_nan):
            bad = np.nonzero(~((a == b) | (np.isnan(a) & np.isnan(b))))[0]
            raise AssertionError(('ema', i, SIZES[i], where, len(bad), int(bad[0]), float(a[bad[0]]), float(b[bad[0]])))


# ------------------------------------------------------------------------------------------------ 1, 2: op level, no model
@pytest.mark.parametrize('decay', [0.5, 0.9998])
def test_average_is_the_restatement_and_the_step_is_the_plain_one(decay):
    """12 steps: decay 0.5 crosses the end of the warm-up at t = 8; 0.9998 stays inside it."""
    ps, opt = _opt(decay)
    ps_t, opt_t = _opt(None)
    ema = _np(ps)                                            # e = p when the tables are built
    for step in range(12):
        gs = _grads(step)
        _set_grads(ps, gs); _set_grads(ps_t, gs)
        opt.step(); opt_t.step()
        _assert_twin(ps, opt, ps_t, opt_t, step)
        if step == 0:
            assert opt._table['e_ptr'][VIEW] % 16 == 0 and ps[VIEW].data_ptr() % 16 == 4
        ema = [R.update(e, p, decay, True, step) for e, p in zip(ema, _np(ps_t))]
        _assert_ema(opt, ema, step)
    assert opt.ema_updates() == 12
    assert opt._table['steps'].tolist() == [12 if i != NO_GRAD else 0 for i in range(len(SIZES))]
    # the tensor without a gradient was not touched by AdamW and its average sits on it (a fixed point from the start)
    assert torch.equal(ps[NO_GRAD], _params()[0][NO_GRAD]) and torch.equal(opt.ema_params()[NO_GRAD], ps[NO_GRAD])
    assert not torch.equal(opt.ema_params()[8], ps[8])       # ... and the others trail their parameters


def test_non_finite_parameters_reach_the_average_as_ieee_says():
    ps, opt = _opt(0.5, ema_warmup=False)
    ps_t, opt_t = _opt(None)
    gs = _grads(0)
    _set_grads(ps, gs); _set_grads(ps_t, gs)
    opt.step(); opt_t.step()
    ema = [R.update(e, p, 0.5, False, 0) for e, p in zip(_np(_params()[0]), _np(ps_t))]
    with torch.no_grad():
        for q in (ps, ps_t):
            q[5][7] = float('nan'); q[6][100] = float('inf'); q[8][8192] = float('-inf')
            q[NO_GRAD][3] = float('inf'); q[NO_GRAD][4] = float('nan'); q[VIEW][1029] = float('nan')
    for step in (1, 2):                                      # the second step meets Inf - Inf in the untouched tensor's average
        gs = _grads(step)
        _set_grads(ps, gs); _set_grads(ps_t, gs)
        opt.step(); opt_t.step()
        _assert_twin(ps, opt, ps_t, opt_t, step)
        ema = [R.update(e, p, 0.5, False, step) for e, p in zip(ema, _np(ps_t))]
        _assert_ema(opt, ema, step, equal_nan=True)
    e = _np(opt.ema_params())
    assert np.isnan(e[5][7]) and np.isnan(e[NO_GRAD][4]) and np.isnan(e[NO_GRAD][3]) and np.isnan(e[VIEW][1029])
    assert np.isfinite(e[5][:7]).all() and np.isfinite(e[NO_GRAD][5:]).all()
    assert opt.ema_updates() == 3


# ------------------------------------------------------------------------------------------------ 3: the gated form
def test_gated_average_advances_exactly_when_a_step_is_applied():
    """Window of two, micro-losses 1, 0, 1, 1, 0, 1 with step() on every second micro-step as train.py calls it, and once more behind
    the fifth (a zero loss with nothing pending: both reasons for a closed gate at once).  Gates: idx 1 closed (zero loss on the
    boundary), idx 3 open (g0 + g2 + g3), behind idx 4 closed, idx 5 open (g5)."""
    decay = 0.5
    ps, opt = _opt(decay, accumulate=True)
    ps_t, opt_t = _opt(None)
    losses = [1.0, 0.0, 1.0, 1.0, 0.0, 1.0]
    ema0 = _np(ps)
    ema, applied, pend = ema0, 0, []
    for idx, l in enumerate(losses):
        gs = _grads(idx)
        _set_grads(ps, gs)
        opt.accumulate_grads(torch.tensor(l, dtype=torch.float32, device='cuda'))
        if l != 0.0:
            pend.append(gs)
        for tail in ([True] if (idx + 1) % 2 == 0 else []) + ([True] if idx == 4 else []):
            before = (opt.ema_avg.clone(), opt._table['ectl'].clone(), opt.loss_meter()[3])
            opt.step()
            torch.cuda.synchronize()
            now = opt.loss_meter()[3]
            open_gate = l != 0.0 and bool(pend)
            assert now - before[2] == (1 if open_gate else 0), (idx, now, before[2])
            if open_gate:
                acc = pend[0]
                for g in pend[1:]:
                    acc = [a + b for a, b in zip(acc, g)]
                pend = []
                _set_grads(ps_t, acc); opt_t.step()
                _assert_twin(ps, opt, ps_t, opt_t, idx)
                ema = [R.update(e, p, decay, True, applied) for e, p in zip(ema, _np(ps_t))]
                applied += 1
            else:
                assert torch.equal(opt.ema_avg, before[0]) and torch.equal(opt._table['ectl'], before[1]), idx
            assert opt.ema_updates() == applied == now
            _assert_ema(opt, ema, idx)
    assert applied == 2 and opt.loss_meter()[1:] == (4, 2, 2) and opt.pending() == 0
    assert not _bits_equal(_np(opt.ema_params())[8], ema0[8])


# ------------------------------------------------------------------------------------------------ 4: the swap
def test_swap_exchanges_parameters_and_average_in_place():
    ps, opt = _opt(0.5)
    for step in range(2):
        _set_grads(ps, _grads(step)); opt.step()
    p0, e0 = _np(ps), _np(opt.ema_params())
    ptrs = [p.data_ptr() for p in ps]
    opt.swap_ema()
    p1, e1 = _np(ps), _np(opt.ema_params())
    for i in range(len(SIZES)):
        assert _bits_equal(p1[i], e0[i]) and _bits_equal(e1[i], p0[i]), i
    assert [p.data_ptr() for p in ps] == ptrs and opt._keep[0][0] == 0 and opt._keep[0][1 + SIZES[VIEW]] == 0      # the view's neighbours
    _set_grads(ps, _grads(2))
    with pytest.raises(RuntimeError, match='swapped in'):
        opt.step()
    with pytest.raises(RuntimeError, match='swapped in'):
        opt.ema_weights().__enter__()
    opt.swap_ema()
    for i, (a, b) in enumerate(zip(_np(ps) + _np(opt.ema_params()), p0 + e0)):
        assert _bits_equal(a, b), i                          # two swaps are the identity
    with pytest.raises(ZeroDivisionError):
        with opt.ema_weights():
            assert _bits_equal(_np(ps)[8], e0[8])
            1 / 0
    assert _bits_equal(_np(ps)[8], p0[8]) and opt.ema_updates() == 2      # swapped back on the way out of the exception
    opt.step()                                               # and training goes on
    assert opt.ema_updates() == 3
    acc = _opt(0.5, accumulate=True)[1]
    acc._ensure_table(); acc.swap_ema()
    with pytest.raises(RuntimeError, match='swapped in'):
        acc.accumulate_grads(torch.ones((), device='cuda'))


def _model(seed=0, train=True):
    """(restated from tests/test_gpu_train_loop.py) D0 with 8 classes on the seeded oracle weights, frozen BN, drop_connect active in
    training, dead parameters frozen."""
    from efficientdet.pytorch_amd import EfficientDet, EFFICIENTDET, ddp
    c = EFFICIENTDET['efficientdet-d0']
    torch.manual_seed(21)
    m = EfficientDet(NC, network='efficientdet-d0', W_bifpn=c['W_bifpn'], D_bifpn=c['D_bifpn'], D_class=c['D_class'],
                     compute_dtype=torch.float32)
    m.load_state_dict(O.make_state_dict('efficientdet-d0', NC, seed=seed))
    m = m.cuda()
    _mode(m, train)
    ddp.freeze_dead_parameters(m)
    return m, [p for p in m.parameters() if p.requires_grad]


def _mode(m, train):
    m.train(train); m.is_training = train; m.freeze_bn()


def _batch(seed, B=2):
    img, ann = O.synthetic_batch(B, 128, seed=seed, num_classes=NC)
    return img.cuda(), ann.cuda()


def _flat(ts):
    return torch.cat([t.detach().reshape(-1) for t in ts]).clone()


def _same_dets(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for da, db in zip(a, b) for x, y in zip(da, db))


def test_detect_with_the_averaged_weights_is_the_published_checkpoint():
    """detect() inside ema_weights() == detect() of a second model loaded from checkpoint.ema_state_dict(), bit for bit; outside the
    context it is the pre-swap output again.  A swap that forgot ops.bump_param_generation() would leave the packed weights of the
    previous call in place and fail both."""
    from efficientdet.pytorch_amd import checkpoint
    from efficientdet.pytorch_amd.optim import ClipAdamW
    m, params = _model()
    opt = ClipAdamW(params, lr=1e-3, max_norm=0.1, ema_decay=0.5, ema_warmup=False)
    for s in range(3):
        opt.zero_grad(set_to_none=True)
        cl, rl = m(list(_batch(10 + s))); (cl.mean() + rl.mean()).backward(); opt.step()
    del cl, rl
    img = _batch(40, B=1)[0]
    _mode(m, False)
    with torch.no_grad():
        raw_trained = m.forward_raw(img)[0].clone()
    # a score threshold that keeps some fifty candidates of THIS model (seeded weights three steps into training score low everywhere)
    m.threshold = 0.5 * float(raw_trained.max(dim=2).values.reshape(-1).topk(50).values[-1])
    trained = m.detect(img)
    with opt.ema_weights():
        averaged = m.detect(img)
        with torch.no_grad():
            raw_avg = m.forward_raw(img)[0].clone()
    again = m.detect(img)
    assert trained[0][0].numel() > 0 and averaged[0][0].numel() > 0
    assert not torch.equal(raw_avg, raw_trained)             # three steps at lr 1e-3 and decay 0.5: the average is another model
    assert _same_dets(again, trained)
    sd = checkpoint.ema_state_dict(m, opt)
    assert _same_dets(m.detect(img), trained) and not opt._swapped
    m2, _ = _model(seed=1, train=False)
    m2.load_state_dict(sd)
    m2.threshold = m.threshold
    assert _same_dets(m2.detect(img), averaged)
    names = [k for k, p in m.named_parameters() if p.requires_grad]
    for k, e in zip(names, opt.ema_params()):
        assert torch.equal(sd[k], e), k


# ------------------------------------------------------------------------------------------------ 5: captured
def test_captured_step_keeps_the_average_and_follows_the_decay():
    from efficientdet.pytorch_amd.graph import GraphedTrainStep, replay_vs_eager
    from efficientdet.pytorch_amd.optim import ClipAdamW
    m, params = _model()
    opt = ClipAdamW(params, lr=1e-3, max_norm=0.1, ema_decay=0.9, ema_warmup=False)
    g = GraphedTrainStep(m, opt, *_batch(10), warmup=2)
    u0 = opt.ema_updates()
    assert u0 == 2                                           # the warm-up's two eager steps; the capture itself runs nothing
    r = replay_vs_eager(g)
    print('replay vs eager with the average:', r)
    assert r['finite'] and r['update_norm'] > 0 and r['ema_update_norm'] > 0
    assert r['eager_vs_eager'] == 0.0 and r['replay_vs_replay'] == 0.0 and r['replay_vs_eager'] <= 1e-6, r
    assert r['ema_eager_vs_eager'] == 0.0 and r['ema_replay_vs_replay'] == 0.0 and r['ema_replay_vs_eager'] <= 1e-6, r
    assert r['ema_updates'] == (u0 + 1, u0 + 1, u0) and opt.ema_updates() == u0 + 1
    # the decay travels in the device hyper buffer: a replay after a change uses the new one
    for decay in (0.25, 0.9):
        e_before = _np(opt.ema_params())
        opt.param_groups[0]['ema_decay'] = decay
        g()
        want = [R.update(e, p, decay, False, 0) for e, p in zip(e_before, _np(params))]
        other = [R.update(e, p, 1.15 - decay, False, 0) for e, p in zip(e_before, _np(params))]
        got = _np(opt.ema_params())
        assert all(_bits_equal(a, b) for a, b in zip(got, want)), decay
        assert not all(_bits_equal(a, b) for a, b in zip(got, other)), decay
    assert opt.ema_updates() == u0 + 3
    with pytest.raises(ValueError, match='ema_decay'):
        opt.param_groups[0]['ema_decay'] = 1.0
        g()
    opt.param_groups[0]['ema_decay'] = 0.9


def test_captured_loop_keeps_the_average_of_the_eager_loop():
    """GraphedTrainLoop(accumulation_steps=2) over four calls against the transcription of tests/test_gpu_train_loop.py (train.py's loop
    body over the ungated step), both with the average: parameters, moments, counters, EMA arena and EMA counter."""
    from efficientdet.pytorch_amd.graph import GraphedTrainLoop
    from efficientdet.pytorch_amd.optim import ClipAdamW
    batches = {k: _batch(10 + i) for i, k in enumerate('ABCD')}
    order, steps, decay = 'ABCD', 2, 0.5
    m, params = _model()
    opt = ClipAdamW(params, lr=1e-3, max_norm=0.1, ema_decay=decay)
    for _ in range(2):                                       # the two warm-up steps GraphedTrainLoop's constructor runs on its batch
        opt.zero_grad(set_to_none=True)
        cl, rl = m(list(batches['A'])); (cl.mean() + rl.mean()).backward(); opt.step()
    del cl, rl
    opt.zero_grad()
    for idx, k in enumerate(order):
        cl, rl = m(list(batches[k]))
        loss = cl.mean() + rl.mean()
        if bool(loss == 0):
            continue
        loss.backward()
        if (idx + 1) % steps == 0:
            opt.step()
            opt.zero_grad()
    torch.cuda.synchronize()
    ref = (_flat(params), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt._table['steps'].clone(), opt.ema_avg.clone(), opt.ema_updates())
    assert ref[5] == 4 and not torch.equal(_flat(opt.ema_params()), ref[0])
    del loss, cl, rl, m, opt
    m, params = _model()
    opt = ClipAdamW(params, lr=1e-3, max_norm=0.1, accumulate=True, ema_decay=decay)
    loop = GraphedTrainLoop(m, opt, *batches['A'], accumulation_steps=steps, warmup=2)
    loop.reset_epoch()
    assert opt.ema_updates() == 2                            # reset_epoch() is an epoch boundary of the loop, not of the average
    for k in order:
        loop.images.copy_(batches[k][0]); loop.annotations.copy_(batches[k][1])
        loop()
    torch.cuda.synchronize()
    got = (_flat(params), opt.exp_avg, opt.exp_avg_sq, opt._table['steps'], opt.ema_avg, opt.ema_updates())
    for name, a, b in zip(('parameters', 'exp_avg', 'exp_avg_sq', 'steps', 'ema'), got, ref):
        assert torch.equal(a, b), (name, float((a.double() - b.double()).abs().max()))
    assert got[5] == ref[5] and opt.loss_meter()[1:] == (4, 0, 2)


# ------------------------------------------------------------------------------------------------ 6: checkpoint
class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        torch.manual_seed(3)
        self.a, self.b = torch.nn.Linear(37, 129), torch.nn.Linear(129, 5)
        self.unused = torch.nn.Parameter(torch.randn(11))    # never has a gradient

    def forward(self, x):
        return self.b(torch.tanh(self.a(x))).square().mean()


def _train(net, opt, steps, first):
    for s in range(first, first + steps):
        x = torch.randn(16, 37, generator=torch.Generator().manual_seed(50 + s)).cuda()
        opt.zero_grad(set_to_none=True)
        net(x).backward()
        opt.step()
    torch.cuda.synchronize()


def _ck_state(net, opt):
    return ([p.detach().clone() for p in net.parameters()], opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt._table['steps'].clone(),
            opt.ema_avg.clone(), opt.ema_updates())


def test_resuming_from_a_checkpoint_continues_the_average(tmp_path):
    from efficientdet.pytorch_amd import checkpoint
    from efficientdet.pytorch_amd.optim import ClipAdamW
    mk = lambda net, **kw: ClipAdamW(net.parameters(), lr=1e-2, max_norm=0.1, **kw)
    whole = _Net().cuda(); opt_w = mk(whole, ema_decay=0.9998)
    _train(whole, opt_w, 5, 0)
    first = _Net().cuda(); opt_f = mk(first, ema_decay=0.9998)
    _train(first, opt_f, 3, 0)
    path = str(tmp_path / 'ck.pth')
    checkpoint.save_checkpoint(path, first, 0, optimizer=opt_f)
    fresh = _Net().cuda()
    with torch.no_grad():
        for p in fresh.parameters():
            p.add_(1.0)                                      # (not the initial weights: everything must come from the file)
    opt_r = mk(fresh, ema_decay=0.9998)
    ck = checkpoint.load_checkpoint(path, fresh, opt_r)
    assert ck['optimizer']['ema_updates'] == 3 and opt_r.ema_updates() == 3
    assert all('ema' in st for st in ck['optimizer']['state'].values())
    _train(fresh, opt_r, 2, 3)
    a, b = _ck_state(fresh, opt_r), _ck_state(whole, opt_w)
    for x, y in zip(a[0], b[0]):
        assert torch.equal(x, y)
    for name, x, y in zip(('exp_avg', 'exp_avg_sq', 'steps', 'ema'), a[1:5], b[1:5]):
        assert torch.equal(x, y), name
    assert a[5] == b[5] == 5
    same = [torch.equal(e, p) for e, p in zip(opt_r.ema_params(), fresh.parameters())]
    assert same == [n == 'unused' for n, _ in fresh.named_parameters()], same      # the average trails every trained tensor
    # a state saved with the average off: e = the current p, updates = 0
    plain = _Net().cuda(); opt_p = mk(plain)
    _train(plain, opt_p, 2, 0)
    sd = opt_p.state_dict()
    assert 'ema_updates' not in sd and all('ema' not in st for st in sd['state'].values())
    opt_l = mk(plain, ema_decay=0.5)
    opt_l.load_state_dict(sd)
    assert opt_l.ema_updates() == 0 and opt_l.param_groups[0]['ema_decay'] == 0.5
    for e, p in zip(opt_l.ema_params(), plain.parameters()):
        assert torch.equal(e, p)
    assert torch.equal(opt_l.exp_avg, opt_p.exp_avg) and torch.equal(opt_l._table['steps'], opt_p._table['steps'])
    # ... and the other way round: a plain optimizer loads a state that carries an average and ignores it
    opt_q = mk(fresh)
    opt_q.load_state_dict(opt_r.state_dict())
    assert not opt_q.ema and 'ema_decay' not in opt_q.param_groups[0] and torch.equal(opt_q.exp_avg, opt_r.exp_avg)
