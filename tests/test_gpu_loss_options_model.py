"""EfficientDet.set_loss through the training node (_HeadLossFn), at the geometry of tests/test_gpu_box_loss_model.py: D0 at 128 x 128,
B = 2, num_classes 4 (the fused fwd_grad + bwd_reg branch) and 5 (the fallback branch for num_classes % 4 != 0), arithmetic 'f32' and
the headline 'f32_hf16x3_bwd_bf16x3'; the one test about the split d(reg) and the sparse regression-tower backward runs at 512 x 512."""
import pytest
import torch

from oracle import effdet_oracle as O

pytestmark = pytest.mark.gpu

ARITHS = ['f32', 'f32_hf16x3_bwd_bf16x3']
PAPER = dict(gamma=1.5, beta=0.1, reg_weight=50.0, low_quality=True)


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
def test_paper_step_and_back_to_the_default(nc, arith):
    from efficientdet.pytorch_amd import LossOptions, ops
    from tests import loss_cases as LC
    img, ann = _batch(nc)
    fresh = _step(_model(nc, arith), img, ann)
    m = _model(nc, arith)
    opt = LossOptions(**PAPER)
    assert m.set_loss(opt) is m
    paper = _step(m, img, ann)
    assert bool(torch.isfinite(paper[0]).all()) and bool(torch.isfinite(paper[1]).all()) and float(paper[0]) > 0.0 and float(paper[1]) > 0.0
    assert all(bool(torch.isfinite(g).all()) for g in paper[2].values())
    assert not torch.equal(paper[0], fresh[0]) and not torch.equal(paper[1], fresh[1])
    assert any(not torch.equal(paper[2][k], fresh[2][k]) for k in paper[2] if 'reg_convs' in k)
    assert any(not torch.equal(paper[2][k], fresh[2][k]) for k in paper[2] if 'cls_convs' in k)
    # the losses are the op-level forward on the head outputs of the same weights (the stand-alone head node): the call the node makes
    cls, reg, anc = m.forward_raw(img)
    cls, reg, a32 = cls.detach().contiguous(), reg.detach().contiguous(), ann.float().contiguous()
    if nc % 4 == 0:
        losses, _, _ = ops.loss_opts_fwd_grad(cls, reg, anc, a32, torch.float32, LC.dld_for(nc), loss=opt)
    else:
        losses, _ = ops.loss_opts_fwd(cls, reg, anc, a32, opt)
    assert torch.equal(losses[0:1], paper[0].reshape(1)) and torch.equal(losses[1:2], paper[1].reshape(1))
    # FocalLoss (the forward-only pass: another summation order of the class partials) agrees in the box term bit for bit
    cl, rl = m.criterion(cls, reg, anc, ann)
    assert torch.equal(rl, paper[1].reshape(1)) and abs(float(cl) - float(paper[0])) <= 1e-5 * float(paper[0])
    # the defaults through the option, then None, then a model from before the option existed: a fresh model's step, bit for bit
    m.set_loss(LossOptions())
    _same(_step(m, img, ann), fresh)
    m.set_loss(None)
    _same(_step(m, img, ann), fresh)
    del m.__dict__['loss_options'], m.criterion.__dict__['loss']
    _same(_step(m, img, ann), fresh)
    with torch.no_grad():
        assert torch.equal(m.criterion(cls, reg, anc, ann)[1], fresh[1].reshape(1))


def test_low_quality_trains_a_box_no_anchor_reaches():
    """One 4 x 4 box (IoU < 0.02 with every anchor): no positive and no regression gradient at the defaults; with low_quality its best
    anchors are promoted and the regression tower trains."""
    from efficientdet.pytorch_amd import LossOptions
    nc = 4
    img, _ = _batch(nc)
    ann = torch.full((2, 3, 5), -1.0)
    ann[0, 1] = torch.tensor([60.3, 60.7, 64.3, 64.7, 1.0])
    ann = ann.cuda()
    m = _model(nc, 'f32')
    cl, rl, grads = _step(m, img, ann)
    assert float(rl) == 0.0 and all(float(g.abs().max()) == 0.0 for k, g in grads.items() if 'reg_convs' in k or 'retina_reg' in k)
    m.set_loss(LossOptions(low_quality=True))
    cl, rl, grads = _step(m, img, ann)
    assert float(rl) > 0.0 and bool(torch.isfinite(rl).all()) and bool(torch.isfinite(cl).all())
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    assert any(float(g.abs().max()) > 0.0 for k, g in grads.items() if 'retina_reg' in k)


def test_paper_options_keep_the_sparse_regression_tower_backward_exact():
    """The split-layout head at 512 x 512 (where functional.HEAD_SPARSE_REG acts): parameter gradients bit-equal with the switch off and
    on, so the tower still sees exact zeros away from the positives, promoted ones included."""
    from efficientdet.pytorch_amd import LossOptions, functional as Fn
    nc, arith = 4, 'f32_hf16x3_bwd_bf16x3'
    assert Fn.head_uses_split(2, [(64 >> i, 64 >> i) for i in range(5)], 64, torch.float32, 'bf16x3')
    m = _model(nc, arith).set_loss(LossOptions(**PAPER))
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
def test_a_graph_replay_is_the_eager_step_with_the_paper_options(arith):
    from efficientdet.pytorch_amd import LossOptions, ddp
    from efficientdet.pytorch_amd.graph import GraphedTrainStep, replay_vs_eager
    from efficientdet.pytorch_amd.optim import ClipAdamW
    nc = 4
    img, ann = _batch(nc)
    m = _model(nc, arith).set_loss(LossOptions(**PAPER))
    ddp.freeze_dead_parameters(m)
    opt = ClipAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-4, max_norm=0.1)
    g = GraphedTrainStep(m, opt, img, ann, warmup=2)
    g()
    r = replay_vs_eager(g)
    print('replay vs eager (paper options, %s): %s' % (arith, r))
    assert r['finite'] and r['update_norm'] > 0
    assert r['eager_vs_eager'] == 0.0 and r['replay_vs_replay'] == 0.0, r
    assert r['replay_vs_eager'] == 0.0, r
    for a, b in zip(r['losses_replay'], r['losses_eager']):
        assert a == b, r
