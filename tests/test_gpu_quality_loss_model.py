"""EfficientDet.set_quality_loss through the training node (_HeadLossFn), at the geometry of tests/test_gpu_loss_options_model.py: D0 at
128 x 128, B = 2, num_classes 4; the test about the needed-tile regression-tower forward runs at 512 x 512, B = 1, where that forward
acts."""
import pytest
import torch

from oracle import effdet_oracle as O

pytestmark = pytest.mark.gpu

LEVELS_128 = [2304, 576, 144, 36, 9]
KINDS = ['qfl', 'vfl']
# Parameter gradients of the fused node against the unfused composition, per tensor relative to its largest element.  The two differ
# only by roundings: the unfused chain turns d(logit) into d(probability) and back (a division and a multiplication by p (1 - p): 1.5
# ulp, 9e-8) and applies the upstream scale before instead of after the linear head, and the gradient convs then sum the same products
# in the same order.  Carried through the ~100 fp32 layers below the head as independent roundings that is about 1e-6; 1e-5 leaves a
# decade for the layers' own conditioning.  (A wrong gradient is wrong by O(1).)
GRAD_TOL = 1e-5


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


def _grads(m):
    return {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}


def _step(m, img, ann):
    m.zero_grad(set_to_none=True)
    cl, rl = m([img, ann])
    (cl.mean() + rl.mean()).backward()
    torch.cuda.synchronize()
    return cl.detach().clone(), rl.detach().clone(), _grads(m)


def _same(a, b):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert a[2].keys() == b[2].keys() and len(a[2]) > 200
    bad = [k for k in a[2] if not torch.equal(a[2][k], b[2][k])]
    assert not bad, bad[:8]


@pytest.mark.parametrize('kind', KINDS)
def test_quality_step_against_the_unfused_composition_and_back_to_the_default(kind):
    from efficientdet.pytorch_amd import ATSSOptions, BoxLossOptions, QualityLossOptions, ops
    from tests import loss_cases as LC
    nc, arith = 4, 'f32'
    img, ann = _batch(nc)
    fresh = _step(_model(nc, arith), img, ann)
    m = _model(nc, arith)
    opt = QualityLossOptions(kind)
    assert m.set_quality_loss(opt) is m
    alone = _step(m, img, ann)
    assert bool(torch.isfinite(alone[0]).all()) and float(alone[0]) > 0.0 and not torch.equal(alone[0], fresh[0])
    assert any(not torch.equal(alone[2][k], fresh[2][k]) for k in alone[2] if 'cls_convs' in k)
    # the GFL / VFNet recipe: ATSS + GIoU + the quality loss
    matcher, box = ATSSOptions(), BoxLossOptions('giou', 2.0)
    m.set_matcher(matcher).set_box_loss(box)
    full = _step(m, img, ann)
    assert bool(torch.isfinite(full[0]).all()) and bool(torch.isfinite(full[1]).all()) and float(full[0]) > 0.0 and float(full[1]) > 0.0
    assert all(bool(torch.isfinite(g).all()) for g in full[2].values())
    # ---- the losses are the op-level call on the stand-alone head's outputs of the same weights: the call the node makes
    m.zero_grad(set_to_none=True)
    cls, reg, anc = m.forward_raw(img)
    c0, r0, a32 = cls.detach().contiguous(), reg.detach().contiguous(), ann.float().contiguous()
    kw = dict(box=box, matcher=matcher, quality=opt)
    losses, ws, _ = ops.loss_opts_fwd_grad(c0, r0, anc, a32, torch.float32, LC.dld_for(nc), levels=LEVELS_128, **kw)
    assert torch.equal(losses[0:1], full[0].reshape(1)) and torch.equal(losses[1:2], full[1].reshape(1))
    # FocalLoss(quality=) reads the levels off the table: another summation order of the class partials, the box term bit for bit
    cl, rl = m.criterion(c0, r0, anc, ann)
    assert torch.equal(rl, full[1].reshape(1)) and abs(float(cl) - float(full[0])) <= 1e-5 * float(full[0])
    q = ops.loss_quality_targets(m.criterion.last_workspace, 2, sum(LEVELS_128), ann.shape[1], matcher=matcher)
    codes = ws[:2 * sum(LEVELS_128) * 4].view(torch.int32).reshape(2, -1)
    assert torch.equal(q, ops.loss_quality_targets(ws, 2, sum(LEVELS_128), ann.shape[1])) and bool((~(q > 0) | (codes >= 0)).all())
    assert 0.0 < float(q.sum() / (codes >= 0).sum()) < 1.0                                      # the mean IoU of the positives
    # ---- every parameter gradient: the ops backward calls fed to the stand-alone head node
    gs = torch.ones(2, device=img.device)
    dlogit = ops.loss_opts_bwd_cls(c0, a32, gs, ws, torch.float32, None, matcher=matcher, quality=opt)
    dreg = ops.loss_opts_bwd_reg(r0, anc, a32, gs, ws, torch.float32, **kw)
    torch.autograd.backward([cls, reg], [dlogit / (c0 * (1.0 - c0)), dreg])
    torch.cuda.synchronize()
    unfused = _grads(m)
    assert unfused.keys() == full[2].keys()
    worst = max(float((full[2][k] - unfused[k]).abs().max()) / float(unfused[k].abs().max()) for k in unfused)
    print('\n%s: fused vs unfused parameter gradients, worst error relative to the tensor\'s largest element: %.3g' % (kind, worst))
    for k in unfused:
        assert float((full[2][k] - unfused[k]).abs().max()) <= GRAD_TOL * float(unfused[k].abs().max()), k
    # ---- None afterwards, then a model from before the option existed: a fresh model's step, bit for bit
    m.set_matcher(None).set_box_loss(None)
    _same(_step(m, img, ann), alone)
    m.set_quality_loss(None)
    _same(_step(m, img, ann), fresh)
    del m.__dict__['quality_loss'], m.criterion.__dict__['quality']
    _same(_step(m, img, ann), fresh)


def test_the_fallback_branch_for_other_class_counts():
    """num_classes % 4 != 0: forward and class backward as two calls, flat d(logit)."""
    from efficientdet.pytorch_amd import QualityLossOptions, ops
    nc = 5
    img, ann = _batch(nc)
    m = _model(nc, 'f32').set_quality_loss(QualityLossOptions('vfl'))
    cl, rl, grads = _step(m, img, ann)
    assert float(cl) > 0.0 and all(bool(torch.isfinite(g).all()) for g in grads.values())
    cls, reg, anc = m.forward_raw(img)
    losses, _ = ops.loss_opts_fwd(cls.detach().contiguous(), reg.detach().contiguous(), anc, ann.float().contiguous(),
                                  quality=m.quality_loss)
    assert torch.equal(losses[0:1], cl.reshape(1)) and torch.equal(losses[1:2], rl.reshape(1))


@pytest.mark.parametrize('kind', KINDS)
def test_the_needed_tile_forward_stays_on_and_changes_nothing(kind):
    """The headline arithmetic at 512 x 512, B = 1: with a quality loss alone (default matcher, no LossOptions) the regression tower
    still computes the needed tiles only -- q reads `reg` at positive anchors -- and the step is bit for bit the dense forward's."""
    from efficientdet.pytorch_amd import BoxLossOptions, QualityLossOptions, functional as Fn
    nc, arith = 4, 'f32_hf16x3_bwd_bf16x3'
    m = _model(nc, arith).set_quality_loss(QualityLossOptions(kind)).set_box_loss(BoxLossOptions('giou'))
    img, ann = _batch(nc, 512, B=1)
    old = Fn.HEAD_SPARSE_REG_FWD
    outs, taken = [], []
    real = Fn.head_fwd

    def spy(*a, **k):
        taken.append(k.get('reg_needed') is not None)
        return real(*a, **k)
    try:
        Fn.head_fwd = spy
        for on in (False, True):
            Fn.HEAD_SPARSE_REG_FWD = on
            outs.append(_step(m, img, ann))
    finally:
        Fn.HEAD_SPARSE_REG_FWD = old
        Fn.head_fwd = real
    assert taken == [False, True]
    _same(*outs)
    assert bool(torch.isfinite(outs[0][0]).all()) and float(outs[0][0]) > 0.0 and float(outs[0][1]) > 0.0


@pytest.mark.parametrize('kind', KINDS)
def test_a_graph_replay_is_the_eager_step_after_a_fresh_capture(kind):
    from efficientdet.pytorch_amd import ATSSOptions, BoxLossOptions, QualityLossOptions, ddp
    from efficientdet.pytorch_amd.graph import GraphedTrainStep, replay_vs_eager
    from efficientdet.pytorch_amd.optim import ClipAdamW
    nc, arith = 4, 'f32_hf16x3_bwd_bf16x3'
    img, ann = _batch(nc)
    m = _model(nc, arith).set_quality_loss(QualityLossOptions(kind)).set_matcher(ATSSOptions()).set_box_loss(BoxLossOptions('giou'))
    ddp.freeze_dead_parameters(m)
    opt = ClipAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-4, max_norm=0.1)
    g = GraphedTrainStep(m, opt, img, ann, warmup=2)
    g()
    r = replay_vs_eager(g)
    print('replay vs eager (%s + ATSS + GIoU, %s): %s' % (kind, arith, r))
    assert r['finite'] and r['update_norm'] > 0
    assert r['eager_vs_eager'] == 0.0 and r['replay_vs_replay'] == 0.0, r
    assert r['replay_vs_eager'] == 0.0, r
    for a, b in zip(r['losses_replay'], r['losses_eager']):
        assert a == b, r
