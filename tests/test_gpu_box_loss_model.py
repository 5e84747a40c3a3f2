"""EfficientDet.set_box_loss through the training node (_HeadLossFn): D0 at 128 x 128, B = 2, num_classes 4 (the fused
fwd_grad + bwd_reg branch) and 5 (the fallback branch for num_classes % 4 != 0), arithmetic 'f32' and the headline
'f32_hf16x3_bwd_bf16x3'.  At 128 x 128 the head's pyramid is too small for the split layout, so the one test that is about the split
d(reg) and the sparse regression-tower backward runs at 512 x 512."""
import pytest
import torch

from oracle import effdet_oracle as O

pytestmark = pytest.mark.gpu

ARITHS = ['f32', 'f32_hf16x3_bwd_bf16x3']


def _model(nc, arith):
    from efficientdet.pytorch_amd import EfficientDet, EFFICIENTDET
    net = 'efficientdet-d0'
    c = EFFICIENTDET[net]
    m = EfficientDet(nc, network=net, W_bifpn=c['W_bifpn'], D_bifpn=c['D_bifpn'], D_class=c['D_class'], compute_dtype=torch.float32,
                     f32_arith=arith)
    m.load_state_dict(O.make_state_dict(net, nc, seed=3)); m.backbone.drop_connect_rate = 0.0
    m = m.cuda(); m.train(); m.is_training = True; m.freeze_bn()
    return m


def _batch(nc, S=128):
    img, ann = O.synthetic_batch(2, S, seed=6, num_classes=nc)
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


@pytest.mark.parametrize('arith', ARITHS)
@pytest.mark.parametrize('nc', [4, 5])
def test_ciou_step_and_back_to_the_default(nc, arith):
    from efficientdet.pytorch_amd import BoxLossOptions, ops
    img, ann = _batch(nc)
    fresh = _step(_model(nc, arith), img, ann)
    m = _model(nc, arith)
    opt = BoxLossOptions('ciou', 2.0)
    m.set_box_loss(opt)
    ciou = _step(m, img, ann)
    assert bool(torch.isfinite(ciou[0]).all()) and bool(torch.isfinite(ciou[1]).all()) and float(ciou[1]) > 0.0
    assert all(bool(torch.isfinite(g).all()) for g in ciou[2].values())
    assert torch.equal(ciou[0], fresh[0]) and not torch.equal(ciou[1], fresh[1])          # the class term is not touched
    assert any(not torch.equal(ciou[2][k], fresh[2][k]) for k in ciou[2] if 'reg_convs' in k)
    # losses[1] is the op-level forward on the head outputs of the same weights (the stand-alone head node)
    cls, reg, anc = m.forward_raw(img)
    losses, _ = ops.box_loss_fwd(cls.detach().contiguous(), reg.detach().contiguous(), anc, ann.float().contiguous(), opt)
    assert torch.equal(losses[1:2], ciou[1].reshape(1))
    assert torch.equal(m.criterion(cls.detach(), reg.detach(), anc, ann)[1], ciou[1].reshape(1))
    # smooth_l1 through the option, then None: both are a fresh model's step, bit for bit
    m.set_box_loss(BoxLossOptions('smooth_l1'))
    _same(_step(m, img, ann), fresh)
    m.set_box_loss(None)
    _same(_step(m, img, ann), fresh)


def test_ciou_keeps_the_sparse_regression_tower_backward_exact():
    """The split-layout head at 512 x 512 (where functional.HEAD_SPARSE_REG acts): parameter gradients bit-equal with the switch off and
    on, so the tower still sees exact zeros away from the positives."""
    from efficientdet.pytorch_amd import BoxLossOptions, functional as Fn
    nc, arith = 4, 'f32_hf16x3_bwd_bf16x3'
    assert Fn.head_uses_split(2, [(64 >> i, 64 >> i) for i in range(5)], 64, torch.float32, 'bf16x3')
    m = _model(nc, arith).set_box_loss(BoxLossOptions('ciou'))
    img, ann = _batch(nc, 512)
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


@pytest.mark.parametrize('arith', ARITHS)
def test_a_graph_replay_is_the_eager_step_with_ciou(arith):
    from efficientdet.pytorch_amd import BoxLossOptions, ddp
    from efficientdet.pytorch_amd.graph import GraphedTrainStep, replay_vs_eager
    from efficientdet.pytorch_amd.optim import ClipAdamW
    nc = 4
    img, ann = _batch(nc)
    m = _model(nc, arith).set_box_loss(BoxLossOptions('ciou'))
    ddp.freeze_dead_parameters(m)
    opt = ClipAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-4, max_norm=0.1)
    g = GraphedTrainStep(m, opt, img, ann, warmup=2)
    g()
    r = replay_vs_eager(g)
    print('replay vs eager (ciou, %s): %s' % (arith, r))
    assert r['finite'] and r['update_norm'] > 0
    assert r['eager_vs_eager'] == 0.0 and r['replay_vs_replay'] == 0.0, r
    assert r['replay_vs_eager'] <= 1e-6, r
    for a, b in zip(r['losses_replay'], r['losses_eager']):
        assert abs(a - b) <= 1e-6 * abs(b), r


@pytest.mark.parametrize('nc', [4, 5])
def test_a_batch_with_annotations_but_no_positive_trains_without_nan(nc):
    from efficientdet.pytorch_amd import BoxLossOptions
    img, _ = _batch(nc)
    ann = torch.full((2, 3, 5), -1.0)
    ann[0, 1] = torch.tensor([60.3, 60.7, 64.3, 64.7, 1.0])           # a 4 x 4 box: IoU < 0.02 with every anchor
    m = _model(nc, 'f32').set_box_loss(BoxLossOptions('ciou'))
    cl, rl, grads = _step(m, img, ann.cuda())
    assert float(rl) == 0.0 and float(cl) > 0.0 and bool(torch.isfinite(cl).all())
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    assert all(float(g.abs().max()) == 0.0 for k, g in grads.items() if 'reg_convs' in k or 'retina_reg' in k)
