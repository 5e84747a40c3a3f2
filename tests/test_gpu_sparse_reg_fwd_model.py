"""Sparse forward pass of the RetinaHead's regression tower, whole model (functional.HEAD_SPARSE_REG_FWD; include/effdet_needed_tiles.h).

D0, 8 classes, B = 2 @512 -- the smallest input at which the split head applies.  Image 0 has three boxes (one touching the image
corner, one small box that is positive at the finest level only), image 1 only padding rows.  With the switch on the regression tower
computes the tiles that can reach a positive anchor and writes zeros elsewhere; both losses, every parameter gradient and the five
pyramid gradients must be bit for bit those of the dense forward.  Every comparison is exact."""
import pytest
import torch

from oracle import effdet_oracle as O

pytestmark = pytest.mark.gpu

ARITH = 'f32_hf16x3_bwd_bf16x3'
_MODELS = {}


def _model(tag='a'):
    from efficientdet.pytorch_amd import EfficientDet, EFFICIENTDET
    if tag not in _MODELS:
        net, nc = 'efficientdet-d0', 8
        c = EFFICIENTDET[net]
        torch.manual_seed(5)                                     # (the drop_connect seed is one draw from the default generator)
        m = EfficientDet(nc, network=net, W_bifpn=c['W_bifpn'], D_bifpn=c['D_bifpn'], D_class=c['D_class'], compute_dtype=torch.float32,
                         f32_arith=ARITH)
        m.load_state_dict(O.make_state_dict(net, nc, seed=3))
        m = m.cuda(); m.train(); m.is_training = True; m.freeze_bn()
        _MODELS[tag] = m
    return _MODELS[tag]


def _batch():
    img = O.synthetic_batch(2, 512, seed=2, num_classes=8)[0].cuda()
    ann = torch.full((2, 4, 5), -1.0)
    ann[0, 0] = torch.tensor([0.0, 0.0, 150.0, 90.0, 1.0])              # touches the image corner
    ann[0, 2] = torch.tensor([100.0, 140.0, 126.0, 166.0, 3.0])         # 26 x 26 inside one 32 x 32 anchor: IoU 0.66 there, < 0.5 with every coarser anchor
    ann[0, 3] = torch.tensor([260.0, 200.0, 420.0, 330.0, 6.0])
    return img, ann.cuda()


def _dc_counters(m):
    return [v for k, v in m._dc.items() if isinstance(k, tuple) and k[0] == 'step_dev']


def _step(m, img, ann):
    """one train-mode forward + backward -> (cls loss, reg loss, parameter gradients by name, the five pyramid gradients)"""
    held = []
    neck = m._neck

    def keep(feats):
        p = neck(feats)
        for t in p:
            t.retain_grad()
        held[:] = p
        return p
    m._neck = keep
    try:
        m.zero_grad(set_to_none=True)
        cl, rl = m([img, ann])
        (cl.mean() + rl.mean()).backward()
        torch.cuda.synchronize()
    finally:
        del m._neck                                               # (the instance attribute: the method is back)
    return (cl.detach().clone(), rl.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None},
            [t.grad.clone() for t in held])


def _on_and_off(m, img, ann):
    """the step with the switch off, then on, from the same weights and the same drop_connect counter -> (off, on, needed-tile launches
    each made)"""
    from efficientdet.pytorch_amd import ops, functional as Fn
    if not _dc_counters(m):
        _step(m, img, ann)                                        # (the first forward draws the seed and creates the device counter)
    saved = [t.clone() for t in _dc_counters(m)]
    outs, launches = [], []
    old = Fn.HEAD_SPARSE_REG_FWD
    try:
        for on in (False, True):
            Fn.HEAD_SPARSE_REG_FWD = on
            for t, s in zip(_dc_counters(m), saved):
                t.copy_(s)
            n0 = ops.NEEDED_LAUNCHES[0]
            outs.append(_step(m, img, ann))
            launches.append(ops.NEEDED_LAUNCHES[0] - n0)
    finally:
        Fn.HEAD_SPARSE_REG_FWD = old
    return outs[0], outs[1], launches


def _assert_equal(a, b):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (a[0], b[0], a[1], b[1])
    assert a[2].keys() == b[2].keys() and len(a[2]) == 274
    bad = [k for k in a[2] if not torch.equal(a[2][k], b[2][k])]
    assert not bad, bad[:8]
    assert len(a[3]) == len(b[3]) == 5
    assert all(torch.equal(x, y) for x, y in zip(a[3], b[3]))
    assert float(a[1]) > 0 and all(bool(torch.isfinite(g).all()) for g in a[2].values())


@pytest.mark.parametrize('paired', [True, False])
def test_losses_and_gradients_equal_the_dense_forward(paired):
    """Paired towers (layer t of both in one launch, flags from the second half on) and unpaired (the regression tower's own launches):
    five flagged launches per forward with the switch on, none with it off."""
    from efficientdet.pytorch_amd import functional as Fn
    m = _model()
    img, ann = _batch()
    old = Fn.HEAD_PAIR_TOWERS
    try:
        Fn.HEAD_PAIR_TOWERS = paired
        off, on, launches = _on_and_off(m, img, ann)
    finally:
        Fn.HEAD_PAIR_TOWERS = old
    assert launches == [0, 5], launches
    _assert_equal(off, on)


def test_the_flags_leave_most_tiles_out():
    """(what the equalities above are worth: on this batch the flags of every radius skip tiles, image 1's at the fine levels among them)"""
    from efficientdet.pytorch_amd import ops
    _, ann = _batch()
    sizes = [(64 >> i, 64 >> i) for i in range(5)]
    need = ops.needed_tiles(ops.anchors(512, 512, 'cuda'), ann, 2, sizes).cpu()
    frac = need.float().mean(dim=1).tolist()
    assert 0.0 < frac[0] <= frac[1] <= frac[2] <= frac[3] <= frac[4] < 0.6, frac
    assert not bool(need[4][32:64].any())                         # level 0 (64 tiles of 128 pixels): image 1 is tiles 32 .. 63


def test_an_iou_box_loss_takes_the_sparse_forward():
    from efficientdet.pytorch_amd import ops
    m = _model()
    img, ann = _batch()
    m.set_box_loss(ops.BoxLossOptions('giou'))
    try:
        off, on, launches = _on_and_off(m, img, ann)
    finally:
        m.set_box_loss(None)
    assert launches == [0, 5], launches
    _assert_equal(off, on)


def test_non_default_loss_options_run_dense():
    """A non-default set_loss may move the matcher's bands: the positives are not the default matcher's, so no needed-tile launch is made."""
    from efficientdet.pytorch_amd import ops
    m = _model()
    img, ann = _batch()
    m.set_loss(ops.LossOptions(pos_iou=0.6, neg_iou=0.3))
    try:
        off, on, launches = _on_and_off(m, img, ann)
    finally:
        m.set_loss(None)
    assert launches == [0, 0], launches
    _assert_equal(off, on)


def test_a_captured_step_follows_its_annotations():
    """graph.replay_vs_eager with the switch on: 0.0.  Then the static annotations are overwritten with padding rows only (no positive
    anywhere: every regression tile is skipped) -- map and flags are kernels inside the graph, so the replay is again the eager step."""
    from efficientdet.pytorch_amd import ddp, ops, functional as Fn
    from efficientdet.pytorch_amd.graph import GraphedTrainStep, replay_vs_eager
    from efficientdet.pytorch_amd.optim import ClipAdamW
    assert Fn.HEAD_SPARSE_REG_FWD
    m = _model('graph')
    img, ann = _batch()
    ddp.freeze_dead_parameters(m)
    opt = ClipAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-4, max_norm=0.1)
    for _ in range(2):
        opt.zero_grad(set_to_none=True)
        cl, rl = m([img, ann]); (cl.mean() + rl.mean()).backward(); opt.step()
    del cl, rl
    g = GraphedTrainStep(m, opt, img, ann, warmup=2)
    g()
    r = replay_vs_eager(g)
    print('replay vs eager:', r)
    assert r['finite'] and r['update_norm'] > 0 and r['losses_eager'][1] > 0
    assert r['eager_vs_eager'] == 0.0 and r['replay_vs_replay'] == 0.0 and r['replay_vs_eager'] == 0.0, r
    assert r['losses_replay'] == r['losses_eager'], r
    g.annotations.copy_(ann[1:2].expand_as(ann))
    r = replay_vs_eager(g)
    print('replay vs eager, no positives:', r)
    assert not bool(ops.needed_tiles(ops.anchors(512, 512, 'cuda'), g.annotations, 2, [(64 >> i, 64 >> i) for i in range(5)]).any())
    assert r['finite'] and r['losses_replay'] == r['losses_eager'], r
    assert r['eager_vs_eager'] == 0.0 and r['replay_vs_replay'] == 0.0 and r['replay_vs_eager'] == 0.0, r
