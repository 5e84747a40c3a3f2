"""Gathered 32-pixel units in the regression tower's flagged launches, whole model (functional.HEAD_SPARSE_UNITS;
include/effdet_unit_lists.h).

D0, 8 classes, B = 2 @512 -- the smallest input at which the split head applies -- with boxes in BOTH images.  With the switch on the
five flagged forward launches and the five flagged data-gradient launches of the regression tower compute their flagged units, four to
a tile, instead of every tile holding one; both losses, every parameter gradient and the five pyramid gradients must be bit for bit
those of the switch off, and a captured replay must be the eager step.  Every comparison is exact."""
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
    ann[0, 2] = torch.tensor([100.0, 140.0, 126.0, 166.0, 3.0])         # positive at the finest level only
    ann[1, 1] = torch.tensor([260.0, 200.0, 420.0, 330.0, 6.0])
    ann[1, 3] = torch.tensor([380.0, 400.0, 511.0, 511.0, 2.0])         # touches the opposite corner
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
    """the step with the switch off, then on, from the same weights and the same drop_connect counter -> (off, on, gathered launches each
    made)"""
    from efficientdet.pytorch_amd import ops, functional as Fn
    if not _dc_counters(m):
        _step(m, img, ann)                                        # (the first forward draws the seed and creates the device counter)
    saved = [t.clone() for t in _dc_counters(m)]
    outs, launches = [], []
    old = Fn.HEAD_SPARSE_UNITS
    try:
        for on in (False, True):
            Fn.HEAD_SPARSE_UNITS = on
            for t, s in zip(_dc_counters(m), saved):
                t.copy_(s)
            n0 = ops.UNIT_LAUNCHES[0]
            outs.append(_step(m, img, ann))
            launches.append(ops.UNIT_LAUNCHES[0] - n0)
    finally:
        Fn.HEAD_SPARSE_UNITS = old
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
def test_losses_and_gradients_equal_the_tile_flags(paired):
    """Paired towers (the flagged segments behind the dense classification tower's) and unpaired: five gathered launches forwards and
    five backwards with the switch on, none with it off."""
    from efficientdet.pytorch_amd import functional as Fn
    m = _model()
    img, ann = _batch()
    old = Fn.HEAD_PAIR_TOWERS
    try:
        Fn.HEAD_PAIR_TOWERS = paired
        off, on, launches = _on_and_off(m, img, ann)
    finally:
        Fn.HEAD_PAIR_TOWERS = old
    assert launches == [0, 10], launches
    _assert_equal(off, on)


def test_the_device_takes_the_gathered_form_on_this_batch():
    """(what the equalities above are worth: at every radius the batch's units fill at most 15/16 of its tiles, so the device-side word
    says gather, and both images contribute units)"""
    from efficientdet.pytorch_amd import ops
    _, ann = _batch()
    sizes = [(64 >> i, 64 >> i) for i in range(5)]
    pm = ops.positive_pixel_map(ops.anchors(512, 512, 'cuda'), ann, sizes)
    l32, l128 = ops.live_tiles_from_map(pm, 2, sizes)
    ul = ops.UnitLists(l32, l128)
    c = ul.counts.cpu()
    # (tools/unit_count.py's numpy restatement on these annotations: units / tiles / gathered tiles per radius)
    assert c[:, 0].tolist() == [14, 21, 28, 32, 38, 42] and c[:, 1].tolist() == [7, 10, 10, 12, 13, 16], c
    assert c[:, 2].tolist() == [1] * 6, c
    per_image = torch.cat([pm[o:o + 2 * h * w].view(2, -1) for (h, w), o in zip(sizes, [0, 8192, 10240, 10752, 10880])], dim=1)
    assert bool(per_image.any(dim=1).all())


def test_a_captured_step_is_the_eager_step():
    """graph.replay_vs_eager with the switch on: 0.0 -- lists and counts are kernels inside the graph and the grid never depends on them.
    Then the static annotations are overwritten with padding rows only: no unit anywhere, every flagged row is zero bytes."""
    from efficientdet.pytorch_amd import ddp, functional as Fn
    from efficientdet.pytorch_amd.graph import GraphedTrainStep, replay_vs_eager
    from efficientdet.pytorch_amd.optim import ClipAdamW
    assert Fn.HEAD_SPARSE_UNITS and Fn.HEAD_SPARSE_REG_FWD and Fn.HEAD_SPARSE_REG
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
    g.annotations.copy_(torch.full_like(ann, -1.0))
    r = replay_vs_eager(g)
    print('replay vs eager, no positives:', r)
    assert r['finite'] and r['losses_replay'] == r['losses_eager'], r
    assert r['eager_vs_eager'] == 0.0 and r['replay_vs_replay'] == 0.0 and r['replay_vs_eager'] == 0.0, r
