"""EfficientDet.set_matcher through the training node (_HeadLossFn), at the geometry of tests/test_gpu_loss_options_model.py: D0 at
128 x 128, B = 2, num_classes 4; the one test about the split d(reg) and the sparse regression-tower backward runs at 512 x 512, B = 1."""
import pytest
import torch

from oracle import effdet_oracle as O

pytestmark = pytest.mark.gpu

LEVELS_128 = [2304, 576, 144, 36, 9]
SMALL_BOX = (58.3, 58.7, 62.3, 62.7)                 # 4 x 4 around the level-3 anchor centre (60, 60): IoU <= 16 / 484 with every anchor


def _model(nc, arith):
    from efficientdet.pytorch_amd import EfficientDet, EFFICIENTDET
    net = 'efficientdet-d0'
    c = EFFICIENTDET[net]
    m = EfficientDet(nc, network=net, W_bifpn=c['W_bifpn'], D_bifpn=c['D_bifpn'], D_class=c['D_class'], compute_dtype=torch.float32,
                     f32_arith=arith)
    m.load_state_dict(O.make_state_dict(net, nc, seed=3)); m.backbone.drop_connect_rate = 0.0
    m = m.cuda(); m.train(); m.is_training = True; m.freeze_bn()
    return m


def _batch(nc, S=128, B=2):
    img, ann = O.synthetic_batch(B, S, seed=6, num_classes=nc)
    return img.cuda(), ann.cuda()


def _step(m, img, ann):
    m.zero_grad(set_to_none=True)
    cl, rl = m([img, ann])
    (cl.mean() + rl.mean()).backward()
    torch.cuda.synchronize()
    return cl.detach().clone(), rl.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}


def _same(a, b):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert a[2].keys() == b[2].keys() and len(a[2]) > 200
    bad = [k for k in a[2] if not torch.equal(a[2][k], b[2][k])]
    assert not bad, bad[:8]


@pytest.mark.parametrize('arith', ['f32', 'f32_hf16x3_bwd_bf16x3'])
def test_atss_step_and_back_to_the_default(arith):
    from efficientdet.pytorch_amd import ATSSOptions, ops
    from tests import loss_cases as LC
    nc = 4
    img, ann = _batch(nc)
    fresh = _step(_model(nc, arith), img, ann)
    m = _model(nc, arith)
    opt = ATSSOptions()
    assert m.set_matcher(opt) is m
    atss = _step(m, img, ann)
    assert bool(torch.isfinite(atss[0]).all()) and bool(torch.isfinite(atss[1]).all()) and float(atss[0]) > 0.0 and float(atss[1]) > 0.0
    assert all(bool(torch.isfinite(g).all()) for g in atss[2].values())
    assert not torch.equal(atss[0], fresh[0]) and not torch.equal(atss[1], fresh[1])
    assert any(not torch.equal(atss[2][k], fresh[2][k]) for k in atss[2] if 'reg_convs' in k)
    # the losses are the op-level call on the stand-alone head's outputs of the same weights: the call the node makes
    cls, reg, anc = m.forward_raw(img)
    cls, reg, a32 = cls.detach().contiguous(), reg.detach().contiguous(), ann.float().contiguous()
    losses, _, _ = ops.loss_opts_fwd_grad(cls, reg, anc, a32, torch.float32, LC.dld_for(nc), matcher=opt, levels=LEVELS_128)
    assert torch.equal(losses[0:1], atss[0].reshape(1)) and torch.equal(losses[1:2], atss[1].reshape(1))
    # FocalLoss reads the levels off the table; another summation order of the class partials, the box term bit for bit
    assert m.criterion.table_levels(anc) == LEVELS_128
    cl, rl = m.criterion(cls, reg, anc, ann)
    assert torch.equal(rl, atss[1].reshape(1)) and abs(float(cl) - float(atss[0])) <= 1e-5 * float(atss[0])
    # None, then a model from before the option existed: a fresh model's step, bit for bit
    m.set_matcher(None)
    _same(_step(m, img, ann), fresh)
    del m.__dict__['matcher'], m.criterion.__dict__['matcher']
    _same(_step(m, img, ann), fresh)
    with torch.no_grad():
        assert torch.equal(m.criterion(cls, reg, anc, ann)[1], fresh[1].reshape(1))


def test_atss_trains_a_box_no_anchor_reaches():
    """One 4 x 4 box (IoU < 0.04 with every anchor): no positive and no regression gradient under the bands; under ATSS the
    candidates around its centre whose IoU reaches their own mean + std are positive and the regression tower trains."""
    from efficientdet.pytorch_amd import ATSSOptions
    nc = 4
    img, _ = _batch(nc)
    ann = torch.full((2, 3, 5), -1.0)
    ann[0, 1] = torch.tensor(list(SMALL_BOX) + [1.0])
    ann = ann.cuda()
    m = _model(nc, 'f32')
    cl, rl, grads = _step(m, img, ann)
    assert float(rl) == 0.0 and all(float(g.abs().max()) == 0.0 for k, g in grads.items() if 'reg_convs' in k or 'retina_reg' in k)
    m.set_matcher(ATSSOptions())
    cl, rl, grads = _step(m, img, ann)
    assert float(rl) > 0.0 and bool(torch.isfinite(rl).all()) and bool(torch.isfinite(cl).all())
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    assert any(float(g.abs().max()) > 0.0 for k, g in grads.items() if 'retina_reg' in k)


def test_atss_keeps_the_sparse_regression_tower_backward_exact():
    """The split-layout head at 512 x 512, B = 1 (where functional.HEAD_SPARSE_REG acts): parameter gradients bit-equal with the switch
    off and on, so the tower still sees exact zeros away from the ATSS positives."""
    from efficientdet.pytorch_amd import ATSSOptions, functional as Fn
    nc, arith = 4, 'f32_hf16x3_bwd_bf16x3'
    assert Fn.head_uses_split(1, [(64 >> i, 64 >> i) for i in range(5)], 64, torch.float32, 'bf16x3')
    m = _model(nc, arith).set_matcher(ATSSOptions())
    img, ann = _batch(nc, 512, B=1)
    old = Fn.HEAD_SPARSE_REG
    outs = []
    try:
        for on in (False, True):
            Fn.HEAD_SPARSE_REG = on
            outs.append(_step(m, img, ann))
    finally:
        Fn.HEAD_SPARSE_REG = old
    _same(*outs)
    assert bool(torch.isfinite(outs[0][1]).all()) and float(outs[0][1]) > 0.0


def test_a_graph_replay_is_the_eager_step_with_the_matcher():
    from efficientdet.pytorch_amd import ATSSOptions, ddp
    from efficientdet.pytorch_amd.graph import GraphedTrainStep, replay_vs_eager
    from efficientdet.pytorch_amd.optim import ClipAdamW
    nc, arith = 4, 'f32_hf16x3_bwd_bf16x3'
    img, ann = _batch(nc)
    m = _model(nc, arith).set_matcher(ATSSOptions())
    ddp.freeze_dead_parameters(m)
    opt = ClipAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-4, max_norm=0.1)
    g = GraphedTrainStep(m, opt, img, ann, warmup=2)
    g()
    r = replay_vs_eager(g)
    print('replay vs eager (ATSS, %s): %s' % (arith, r))
    assert r['finite'] and r['update_norm'] > 0
    assert r['eager_vs_eager'] == 0.0 and r['replay_vs_replay'] == 0.0, r
    assert r['replay_vs_eager'] == 0.0, r
    for a, b in zip(r['losses_replay'], r['losses_eager']):
        assert a == b, r
