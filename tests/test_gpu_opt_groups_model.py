"""GPU tier, model level, of the parameter groups and the SGD rule: optim.split_param_groups on D0 under graph.GraphedTrainStep and
graph.GraphedTrainLoop (the model and batch of tests/test_gpu_ema.py's captured tests: D0, 8 classes, B = 2 at 128 x 128).  A captured
step reads every group's row from the device table, so a group's lr set to 0 after the capture freezes that group's tensors on the next
replay and nothing else."""
import pytest
import torch

from oracle import effdet_oracle as O

pytestmark = pytest.mark.gpu

NC = 8


def _model(seed=0):
    """(restated from tests/test_gpu_ema.py) D0 with 8 classes on the seeded oracle weights, training mode, frozen BN, drop_connect
    active, dead parameters frozen."""
    from efficientdet.pytorch_amd import EfficientDet, EFFICIENTDET, ddp
    c = EFFICIENTDET['efficientdet-d0']
    torch.manual_seed(21)
    m = EfficientDet(NC, network='efficientdet-d0', W_bifpn=c['W_bifpn'], D_bifpn=c['D_bifpn'], D_class=c['D_class'],
                     compute_dtype=torch.float32)
    m.load_state_dict(O.make_state_dict('efficientdet-d0', NC, seed=seed))
    m = m.cuda()
    m.train(); m.is_training = True; m.freeze_bn()
    ddp.freeze_dead_parameters(m)
    return m


def _batch(seed):
    img, ann = O.synthetic_batch(2, 128, seed=seed, num_classes=NC)
    return img.cuda(), ann.cuda()


def _flat(ts):
    return torch.cat([t.detach().reshape(-1) for t in ts]).clone()


def _scaled(opt):
    for g in opt.param_groups:                               # split_param_groups leaves the multiplication to the caller
        g['lr'] *= g['lr_scale']
    return opt


def _snapshot(m):
    torch.cuda.synchronize()
    return {n: p.detach().clone() for n, p in m.named_parameters() if p.requires_grad}


def _moved(before, after):
    return {n for n in before if not torch.equal(before[n], after[n])}


def _freeze_and_restore(m, opt, g):
    """An ordinary replay, one with the backbone groups' lr at 0, one with it restored.  Frozen: NO backbone tensor changes by a bit;
    of the other tensors that move in the ordinary replay at least nine in ten move again (an update can fall below a tensor's ulp
    in one replay and not in the next, so the sets are not held equal).  Restored: the backbone moves again, by the same measure."""
    names = set(_snapshot(m))
    backbone = {n for n in names if n.startswith('backbone.')}
    assert backbone and names - backbone
    c0 = opt._table['steps'].clone()
    s0 = _snapshot(m); g(); s1 = _snapshot(m)
    c1 = opt._table['steps'].clone()
    ordinary = _moved(s0, s1)
    assert len(ordinary & backbone) >= 1 and len(ordinary - backbone) >= 1
    back_groups = [pg for pg in opt.param_groups if pg['name'].startswith('backbone_')]
    assert len(back_groups) == 2 and sum(len(pg['params']) for pg in back_groups) == len(backbone)
    saved = [pg['lr'] for pg in back_groups]
    for pg in back_groups:
        pg['lr'] = 0.0
    g(); s2 = _snapshot(m)
    frozen = _moved(s1, s2)
    assert not frozen & backbone, sorted(frozen & backbone)[:5]
    assert len(frozen & ordinary) >= 0.9 * len(ordinary - backbone), (len(frozen), len(ordinary - backbone))
    c2 = opt._table['steps'].clone()
    assert torch.equal(c2 - c1, c1 - c0) and int((c1 - c0).max()) == 1      # the counters of the frozen tensors went on as everybody's
    for pg, lr in zip(back_groups, saved):
        pg['lr'] = lr
    g(); s3 = _snapshot(m)
    again = _moved(s2, s3)
    assert len(again & backbone & ordinary) >= 0.9 * len(ordinary & backbone) and len(again - backbone) >= 0.9 * len(ordinary - backbone)
    print('tensors moved: ordinary %d (backbone %d of %d), backbone lr 0: %d, restored: %d'
          % (len(ordinary), len(ordinary & backbone), len(backbone), len(frozen), len(again)))


def test_captured_adamw_step_reads_every_groups_row():
    from efficientdet.pytorch_amd.graph import GraphedTrainStep, replay_vs_eager
    from efficientdet.pytorch_amd.optim import ClipAdamW, split_param_groups
    m = _model()
    opt = _scaled(ClipAdamW(split_param_groups(m, 4e-5, backbone_lr_scale=0.1), lr=1e-3, max_norm=0.1))
    assert [pg['name'] for pg in opt.param_groups] == ['decay', 'no_decay', 'backbone_decay', 'backbone_no_decay']
    assert [pg['lr'] for pg in opt.param_groups] == pytest.approx([1e-3, 1e-3, 1e-4, 1e-4], rel=1e-12)
    g = GraphedTrainStep(m, opt, *_batch(10), warmup=2)
    assert opt._table['grouped'] and opt._table['ngroups'] == 4
    r = replay_vs_eager(g)
    print('replay vs eager, four groups:', r)
    assert r['finite'] and r['update_norm'] > 0
    assert r['eager_vs_eager'] == 0.0 and r['replay_vs_replay'] == 0.0 and r['replay_vs_eager'] <= 1e-6, r
    _freeze_and_restore(m, opt, g)
    # a torch scheduler drives the captured step group by group: LambdaLR scales every group's own initial lr
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda epoch: 0.5 ** epoch)
    sched.step()
    assert [pg['lr'] for pg in opt.param_groups] == pytest.approx([5e-4, 5e-4, 5e-5, 5e-5], rel=1e-12)
    g()
    torch.cuda.synchronize()
    assert opt._table['hyper'].view(4, 8)[:, 1].cpu().tolist() == pytest.approx([5e-4, 5e-4, 5e-5, 5e-5], rel=1e-6)      # (fp32 on the device)


def test_captured_sgd_step_with_nesterov_and_the_average():
    from efficientdet.pytorch_amd.graph import GraphedTrainStep, replay_vs_eager
    from efficientdet.pytorch_amd.optim import ClipSGD, split_param_groups
    m = _model()
    opt = _scaled(ClipSGD(split_param_groups(m, 4e-5, backbone_lr_scale=0.1), lr=0.05, momentum=0.9, nesterov=True, max_norm=0.1,
                          ema_decay=0.9))
    g = GraphedTrainStep(m, opt, *_batch(10), warmup=2)
    u0 = opt.ema_updates()
    assert u0 == 2 and len(opt.moment_arenas()) == 1
    r = replay_vs_eager(g)
    print('replay vs eager, SGD with the average:', r)
    assert r['finite'] and r['update_norm'] > 0 and r['ema_update_norm'] > 0
    assert r['eager_vs_eager'] == 0.0 and r['replay_vs_replay'] == 0.0 and r['replay_vs_eager'] <= 1e-6, r
    assert r['ema_eager_vs_eager'] == 0.0 and r['ema_replay_vs_replay'] == 0.0 and r['ema_replay_vs_eager'] <= 1e-6, r
    assert r['ema_updates'] == (u0 + 1, u0 + 1, u0)
    _freeze_and_restore(m, opt, g)
    assert opt.ema_updates() == u0 + 4


def test_captured_loop_with_two_groups_is_the_eager_loop():
    """GraphedTrainLoop(accumulation_steps=2) over four calls against the transcription of tests/test_gpu_train_loop.py (train.py's loop
    body over the ungated step), both with split_param_groups' decay / no-decay groups: parameters, moments and counters, bit for bit."""
    from efficientdet.pytorch_amd.graph import GraphedTrainLoop
    from efficientdet.pytorch_amd.optim import ClipAdamW, split_param_groups
    batches = {k: _batch(10 + i) for i, k in enumerate('ABCD')}
    order, steps = 'ABCD', 2
    mk = lambda m, **kw: ClipAdamW(split_param_groups(m, 1e-2), lr=1e-3, max_norm=0.1, **kw)
    m = _model()
    opt = mk(m)
    assert [pg['name'] for pg in opt.param_groups] == ['decay', 'no_decay'] and [pg['weight_decay'] for pg in opt.param_groups] == [1e-2, 0.0]
    params = [p for pg in opt.param_groups for p in pg['params']]
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
    assert opt._table['grouped']
    ref = (_flat(params), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt._table['steps'].clone())
    del loss, cl, rl, m, opt, params
    m = _model()
    opt = mk(m, accumulate=True)
    params = [p for pg in opt.param_groups for p in pg['params']]
    loop = GraphedTrainLoop(m, opt, *batches['A'], accumulation_steps=steps, warmup=2)
    loop.reset_epoch()
    for k in order:
        loop.images.copy_(batches[k][0]); loop.annotations.copy_(batches[k][1])
        loop()
    torch.cuda.synchronize()
    got = (_flat(params), opt.exp_avg, opt.exp_avg_sq, opt._table['steps'])
    for name, a, b in zip(('parameters', 'exp_avg', 'exp_avg_sq', 'steps'), got, ref):
        assert torch.equal(a, b), (name, float((a.double() - b.double()).abs().max()))
    assert opt.loss_meter()[1:] == (4, 0, 2)
