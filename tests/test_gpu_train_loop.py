"""GPU tier of the captured training loop: the device gates of csrc/optim.hip (zero-loss skip, gradient accumulation, loss meter),
optim.ClipAdamW(accumulate=True) and graph.GraphedTrainLoop against a line-for-line transcription of the reference's loop body
(train.py:104-120) over the ungated ClipAdamW.step().

Every comparison is torch.equal: the path has no float atomics and the gated step kernels are the ungated template behind an early exit.
The one tolerance is the loss meter's: a sequential fp64 sum of n same-sign terms is within (n - 1) * 2^-53 relative of the exact sum."""
import math

import numpy as np
import pytest
import torch

from oracle import effdet_oracle as O

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 4095, 4096, 4097, 8193)      # one element; below a float4; one workgroup chunk (4096) -1 / exact / +1; two chunks + 1
NO_GRAD, MISALIGNED = 1, 4                  # SIZES[1] never has a gradient; SIZES[4]'s gradient starts one float into a larger buffer
NC = 8


def meter_bound(n):
    return max(n - 1, 0) * 2.0 ** -53


# ------------------------------------------------------------------------------------------------ (a), (b): op level, no model
def _opt(accumulate, seed=0, **kw):
    from efficientdet.pytorch_amd.optim import ClipAdamW
    g = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(n, generator=g).cuda()) for n in SIZES]
    return ps, ClipAdamW(ps, lr=1e-3, max_norm=0.1, accumulate=accumulate, **kw)


def _grads(seed):
    g = torch.Generator().manual_seed(1000 + seed)
    return [torch.randn(n, generator=g).cuda() for n in SIZES]


def _set_grads(ps, gs, misalign):
    """p.grad = the given values; with misalign, tensor MISALIGNED's gradient is a view one float into a larger buffer (the address of a
    DistributedDataParallel bucket view).  Returns the tensors that must stay alive."""
    keep = []
    for i, (p, g) in enumerate(zip(ps, gs)):
        if i == NO_GRAD:
            p.grad = None
        elif i == MISALIGNED and misalign:
            buf = torch.zeros(g.numel() + 8, device='cuda')
            buf[1:1 + g.numel()].copy_(g)
            p.grad = buf[1:1 + g.numel()]
            assert p.grad.data_ptr() % 16 == 4
            keep.append(buf)
        else:
            p.grad = g.clone()
    return keep


def _loss(v):
    return torch.tensor(v, dtype=torch.float32, device='cuda')


def _state(ps, opt):
    torch.cuda.synchronize()
    return ([p.detach().clone() for p in ps], opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt._table['steps'].clone())


def _assert_same_state(a, b):
    for i, (x, y) in enumerate(zip(a[0], b[0])):
        assert torch.equal(x, y), ('parameter', i, float((x - y).abs().max()))
    assert torch.equal(a[1], b[1]), 'exp_avg'
    assert torch.equal(a[2], b[2]), 'exp_avg_sq'
    assert torch.equal(a[3], b[3]), ('steps', a[3].tolist(), b[3].tolist())


def test_two_accumulated_micro_batches_are_one_step_on_their_sum():
    ps_n, opt_n = _opt(True)
    ps_t, opt_t = _opt(False)
    for window in range(2):                                  # the second window proves the arena was released and is overwritten
        g0, g1 = _grads(2 * window), _grads(2 * window + 1)
        for g in (g0, g1):
            keep = _set_grads(ps_n, g, misalign=True)
            opt_n.accumulate_grads(_loss(1.0 + window))
        opt_n.step()
        _set_grads(ps_t, [a + b for a, b in zip(g0, g1)], misalign=False)
        opt_t.step()
        sn, st = _state(ps_n, opt_n), _state(ps_t, opt_t)
        _assert_same_state(sn, st)
        assert sn[3].tolist() == [window + 1 if i != NO_GRAD else 0 for i in range(len(SIZES))]
        assert opt_n.pending() == 0
        del keep
    assert opt_n.loss_meter() == (1.5, 4, 0, 2)
    assert float((sn[0][5] - _opt(False)[0][5]).abs().max()) > 1e-4          # the steps moved something


@pytest.mark.parametrize('zero', [0.0, -0.0])
def test_a_zero_loss_leaves_everything_untouched_whatever_the_gradients_hold(zero):
    ps, opt = _opt(True)
    g0, g1 = _grads(0), _grads(1)
    _set_grads(ps, g0, misalign=True); opt.accumulate_grads(_loss(0.5)); opt.step()          # moments and counters are not trivial
    _set_grads(ps, g0, misalign=True); opt.accumulate_grads(_loss(0.5))                      # one micro-batch pending
    before, arena, norm = _state(ps, opt), opt.grad_acc.clone(), opt._table['scratch'].clone()
    assert opt.pending() == 1
    nan = [torch.full_like(g, float('nan')) for g in g0]
    _set_grads(ps, nan, misalign=True)
    opt.accumulate_grads(_loss(zero))
    opt.step()
    _assert_same_state(_state(ps, opt), before)
    assert torch.equal(opt.grad_acc, arena) and torch.equal(opt._table['scratch'], norm)
    assert opt.pending() == 1
    assert opt.loss_meter()[1:] == (2, 1, 1)
    # ... and the window goes on: the next micro-batch joins the pending one
    _set_grads(ps, g1, misalign=True); opt.accumulate_grads(_loss(0.25)); opt.step()
    ps_t, opt_t = _opt(False)
    _set_grads(ps_t, g0, misalign=False); opt_t.step()
    _set_grads(ps_t, [a + b for a, b in zip(g0, g1)], misalign=False); opt_t.step()
    _assert_same_state(_state(ps, opt), _state(ps_t, opt_t))
    assert opt.loss_meter()[1:] == (3, 1, 2) and opt.pending() == 0


def test_a_step_with_nothing_pending_is_a_no_op():
    ps, opt = _opt(True)
    _set_grads(ps, _grads(0), misalign=True); opt.accumulate_grads(_loss(0.5)); opt.step()
    before = _state(ps, opt)
    opt.step()                                               # skip is clear, pending == 0
    _assert_same_state(_state(ps, opt), before)
    assert opt.loss_meter()[3] == 1


def test_a_nan_loss_is_not_skipped():
    """bool(nan == 0) is False: the reference goes on to backward() and step()."""
    ps, opt = _opt(True)
    ps_t, opt_t = _opt(False)
    g0 = _grads(0)
    _set_grads(ps, g0, misalign=True); opt.accumulate_grads(_loss(float('nan'))); opt.step()
    _set_grads(ps_t, g0, misalign=False); opt_t.step()
    _assert_same_state(_state(ps, opt), _state(ps_t, opt_t))
    mean, count, skipped, applied = opt.loss_meter()
    assert math.isnan(mean) and (count, skipped, applied) == (1, 0, 1)
    _set_grads(ps, g0, misalign=True); opt.accumulate_grads(_loss(float('inf')))
    assert opt.loss_meter()[1:3] == (2, 0) and opt.pending() == 1          # Inf is not skipped either


def test_loss_meter_is_the_mean_of_the_losses_that_were_not_skipped():
    ps, opt = _opt(True)
    g0 = _grads(0)
    ls = [float(np.float32(v)) for v in (0.7316, 0.0, 1234.567, 3.1e-3)]
    for l in ls:
        _set_grads(ps, g0, misalign=False); opt.accumulate_grads(_loss(l))
    mean, count, skipped, applied = opt.loss_meter()
    want = math.fsum(l for l in ls if l != 0.0) / 3
    print('meter: mean %r, fsum / 3 %r, relative difference %.3g (bound %.3g)' % (mean, want, abs(mean - want) / want, meter_bound(3)))
    assert (count, skipped, applied) == (3, 1, 0)
    assert abs(mean - want) <= meter_bound(3) * want
    opt.reset_epoch()
    mean, count, skipped, applied = opt.loss_meter()
    assert math.isnan(mean) and (count, skipped, applied) == (0, 0, 0) and opt.pending() == 0


def test_a_changed_gradient_set_is_refused():
    ps, opt = _opt(True)
    g0 = _grads(0)
    _set_grads(ps, g0, misalign=False); opt.accumulate_grads(_loss(1.0))
    ps[2].grad = None
    with pytest.raises(RuntimeError, match='set of tensors that have a gradient changed'):
        opt.accumulate_grads(_loss(1.0))
    opt.reset_epoch()                                        # an epoch boundary drops what was pending: a new set is fine
    opt.accumulate_grads(_loss(1.0)); opt.step()
    assert opt.loss_meter()[1:] == (1, 0, 1)
    with pytest.raises(ValueError, match='fp32 GPU tensor'):
        opt.accumulate_grads(1.0)


# ------------------------------------------------------------------------------------------------ (c)-(f): the loop, D0 B = 2 @128
def _model(seed=0):
    """(restated from tests/test_gpu_pipeline.py) D0 with 8 classes on the seeded oracle weights, training mode, frozen BN,
    drop_connect ACTIVE (the device-side step counter draws the masks), dead parameters frozen."""
    from efficientdet.pytorch_amd import EfficientDet, EFFICIENTDET, ddp
    c = EFFICIENTDET['efficientdet-d0']
    torch.manual_seed(21)
    m = EfficientDet(NC, network='efficientdet-d0', W_bifpn=c['W_bifpn'], D_bifpn=c['D_bifpn'], D_class=c['D_class'],
                     compute_dtype=torch.float32)
    m.load_state_dict(O.make_state_dict('efficientdet-d0', NC, seed=seed))
    m = m.cuda()
    m.train(); m.is_training = True; m.freeze_bn()
    assert m.backbone.drop_connect_rate > 0
    ddp.freeze_dead_parameters(m)
    return m, [p for p in m.parameters() if p.requires_grad]


def _batch(seed, boxes=True):
    img, ann = O.synthetic_batch(2, 128, seed=seed, num_classes=NC)
    if not boxes:
        ann.fill_(-1.0)
    return img.cuda(), ann.cuda()


@pytest.fixture(scope='module')
def batches():
    b = {k: _batch(10 + i) for i, k in enumerate('ABCDEF')}
    b['Z'] = _batch(30, boxes=False)
    return b


def _flat(params):
    return torch.cat([p.detach().reshape(-1) for p in params]).clone()


def _feed(loop, batch):
    loop.images.copy_(batch[0]); loop.annotations.copy_(batch[1])


def test_the_loop_is_train_py_bit_for_bit(batches):
    from efficientdet.pytorch_amd.graph import GraphedTrainLoop
    from efficientdet.pytorch_amd.optim import ClipAdamW
    order, steps, lr = 'ABZCDZEF', 2, 1e-3
    # ---- the reference's loop (train.py:97, 104-120), written out; clip_grad_norm_(0.1) + optimizer.step() is today's ClipAdamW.step()
    m, params = _model()
    opt = ClipAdamW(params, lr=lr, max_norm=0.1)
    for _ in range(2):                                       # the two warm-up steps GraphedTrainLoop's constructor runs on its batch
        opt.zero_grad(set_to_none=True)
        cl, rl = m(list(batches['A'])); (cl.mean() + rl.mean()).backward(); opt.step()
    del cl, rl
    total_loss, seen, stepped = [], [], []
    opt.zero_grad()
    for idx, k in enumerate(order):
        classification_loss, regression_loss = m(list(batches[k]))
        classification_loss = classification_loss.mean()
        regression_loss = regression_loss.mean()
        loss = classification_loss + regression_loss
        seen.append((classification_loss.detach().clone(), regression_loss.detach().clone()))
        if bool(loss == 0):
            continue
        loss.backward()
        if (idx + 1) % steps == 0:
            opt.step()
            opt.zero_grad()
            stepped.append(idx)
        total_loss.append(loss.item())
    assert stepped == [1, 3, 7] and len(total_loss) == 6
    for idx, k in enumerate(order):                          # a batch without boxes has a loss of exactly 0 (models/losses.py:54-58)
        assert (float(seen[idx][0]) + float(seen[idx][1]) == 0.0) == (k == 'Z'), (idx, k, seen[idx])
    ref = (_flat(params), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt._table['steps'].clone())
    del loss, classification_loss, regression_loss, m, opt
    # ---- the captured loop
    m, params = _model()
    opt = ClipAdamW(params, lr=lr, max_norm=0.1, accumulate=True)
    loop = GraphedTrainLoop(m, opt, *batches['A'], accumulation_steps=steps, warmup=2)
    loop.reset_epoch()
    for idx, k in enumerate(order):
        _feed(loop, batches[k])
        cl, rl = loop()
        assert torch.equal(cl.reshape(()), seen[idx][0].reshape(())) and torch.equal(rl.reshape(()), seen[idx][1].reshape(())), \
            (idx, k, float(cl), float(rl), seen[idx])
    torch.cuda.synchronize()
    got = (_flat(params), opt.exp_avg, opt.exp_avg_sq, opt._table['steps'])
    for name, a, b in zip(('parameters', 'exp_avg', 'exp_avg_sq', 'steps'), got, ref):
        assert torch.equal(a, b), (name, float((a.double() - b.double()).abs().max()))
    mean, count, skipped, applied = opt.loss_meter()
    want = float(np.mean(total_loss))
    print('epoch mean %r, np.mean(total_loss) %r, relative difference %.3g (bound %.3g)'
          % (mean, want, abs(mean - want) / want, meter_bound(6)))
    assert (count, skipped, applied) == (6, 2, 3) and opt.pending() == 0
    assert loop.epoch_mean() == mean and abs(mean - want) <= meter_bound(6) * want
    loop.reset_epoch()
    assert loop.idx == 0 and math.isnan(loop.epoch_mean())


def test_one_micro_batch_per_step_is_the_graphed_step_except_on_a_zero_loss(batches):
    from efficientdet.pytorch_amd.graph import GraphedTrainLoop, GraphedTrainStep
    from efficientdet.pytorch_amd.optim import ClipAdamW
    m1, p1 = _model()
    step = GraphedTrainStep(m1, ClipAdamW(p1, lr=1e-3, max_norm=0.1), *batches['A'], warmup=2)
    m2, p2 = _model()
    loop = GraphedTrainLoop(m2, ClipAdamW(p2, lr=1e-3, max_norm=0.1, accumulate=True), *batches['A'], accumulation_steps=1, warmup=2)
    assert torch.equal(_flat(p1), _flat(p2))
    for k in 'BCD':
        _feed(step, batches[k]); _feed(loop, batches[k])
        step(); loop()
    torch.cuda.synchronize()
    a, b = _flat(p1), _flat(p2)
    assert torch.equal(a, b), float((a - b).abs().max())
    assert loop.optimizer.loss_meter()[1:] == (3, 0, 3)
    # the behaviour the loop exists for: a batch without boxes
    _feed(step, batches['Z']); _feed(loop, batches['Z'])
    cl1, rl1 = step(); cl2, rl2 = loop()
    torch.cuda.synchronize()
    assert float(cl1) + float(rl1) == 0.0 and float(cl2) + float(rl2) == 0.0
    assert torch.equal(_flat(p2), b)                         # the reference's `continue`: nothing moves
    assert not torch.equal(_flat(p1), a)                     # AdamW on zero gradients: weight decay and the first moments move the weights
    assert loop.optimizer.loss_meter()[1:] == (3, 1, 3)


def test_the_loop_follows_the_lr_schedule(batches):
    from efficientdet.pytorch_amd.graph import GraphedTrainLoop
    from efficientdet.pytorch_amd.optim import ClipAdamW
    m, params = _model()
    opt = ClipAdamW(params, lr=1e-3, max_norm=0.1, weight_decay=0.0, accumulate=True)
    loop = GraphedTrainLoop(m, opt, *batches['A'], accumulation_steps=2, warmup=1)
    p0 = _flat(params)
    loop(); p1 = _flat(params)
    assert torch.equal(p1, p0)                               # idx 0 of a window of two: no step
    loop(); p2 = _flat(params)
    assert float((p2 - p1).abs().max()) > 1e-4
    opt.param_groups[0]['lr'] = 0.0
    loop(); loop(); p3 = _flat(params)
    assert torch.equal(p3, p2)                               # lr = 0 (and no weight decay): the applied step moves nothing ...
    assert opt.loss_meter()[3] == 2                          # ... but it was applied
    opt.param_groups[0]['lr'] = 1e-3
    loop(); loop(); p4 = _flat(params)
    assert float((p4 - p3).abs().max()) > 1e-4


def test_a_distributed_model_is_refused(tmp_path):
    import torch.distributed as dist
    from efficientdet.pytorch_amd.graph import GraphedTrainLoop
    from efficientdet.pytorch_amd.optim import ClipAdamW
    lin = torch.nn.Linear(4, 4).cuda()
    opt = ClipAdamW(lin.parameters(), accumulate=True)
    x = torch.zeros(1, device='cuda')
    dist.init_process_group('gloo', store=dist.FileStore(str(tmp_path / 'store'), 1), rank=0, world_size=1)
    try:
        wrapped = torch.nn.parallel.DistributedDataParallel(lin)
        with pytest.raises(NotImplementedError, match='DistributedDataParallel'):
            GraphedTrainLoop(wrapped, opt, x, x)
    finally:
        dist.destroy_process_group()
    with pytest.raises(RuntimeError, match='accumulate=True'):
        GraphedTrainLoop(lin, ClipAdamW(lin.parameters()), x, x)
