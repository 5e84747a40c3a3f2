"""EfficientDet.set_matcher(TaskAlignedOptions()) through the training node (_HeadLossFn), at the geometry of
tests/test_gpu_atss_model.py: D0 at 128 x 128, B = 2, num_classes 4, with the recipe the matcher is meant for -- the task-aligned
assignment, the quality focal loss on the aligned target, GIoU."""
import pytest
import torch

from tests.gpu_util import assert_close_scale
from tests.test_gpu_atss_model import _batch, _model, _same, _step

pytestmark = pytest.mark.gpu


def _recipe(m):
    from efficientdet.pytorch_amd import BoxLossOptions, QualityLossOptions, TaskAlignedOptions
    opt, q, box = TaskAlignedOptions(), QualityLossOptions('qfl'), BoxLossOptions('giou')
    assert m.set_matcher(opt).set_quality_loss(q).set_box_loss(box) is m
    return opt, q, box


@pytest.mark.parametrize('arith', ['f32', 'f32_hf16x3_bwd_bf16x3'])
def test_tal_step_and_back_to_the_default(arith):
    from efficientdet.pytorch_amd import ops
    from tests import loss_cases as LC
    nc = 4
    img, ann = _batch(nc)
    m = _model(nc, arith)
    fresh = _step(m, img, ann)                                                               # before the matcher is set
    opt, q, box = _recipe(m)
    tal = _step(m, img, ann)
    assert bool(torch.isfinite(tal[0]).all()) and bool(torch.isfinite(tal[1]).all()) and float(tal[0]) > 0.0 and float(tal[1]) > 0.0
    live = {id(p) for p in m.live_parameters()}
    named = {k: p for k, p in m.named_parameters() if id(p) in live}
    assert len(named) > 200 and set(named) <= set(tal[2])                                    # all live parameters get a gradient ...
    assert all(bool(torch.isfinite(g).all()) for g in tal[2].values())                       # ... and a finite one
    assert not torch.equal(tal[0], fresh[0]) and not torch.equal(tal[1], fresh[1])
    # the losses are the op-level call on the stand-alone head's outputs of the same weights: the call the node makes (no levels)
    cls, reg, anc = m.forward_raw(img)
    cls, reg, a32 = cls.detach().contiguous(), reg.detach().contiguous(), ann.float().contiguous()
    losses, ws, _ = ops.loss_opts_fwd_grad(cls, reg, anc, a32, torch.float32, LC.dld_for(nc), box=box, matcher=opt, quality=q)
    assert torch.equal(losses[0:1], tal[0].reshape(1)) and torch.equal(losses[1:2], tal[1].reshape(1))
    B, A, _ = cls.shape
    codes = ws[:B * A * 4].view(torch.int32).reshape(B, A)
    tq = ops.loss_quality_targets(ws, B, A, a32.shape[1], matcher=opt)
    assert int((codes >= 0).sum()) >= 8 and float(tq.max()) > 0.0 and bool((tq[codes < 0] == 0).all())
    # FocalLoss makes the two-pass call without levels (no device -> host sync for them): the box term bit for bit
    cl, rl = m.criterion(cls, reg, anc, ann)
    assert torch.equal(rl, tal[1].reshape(1)) and abs(float(cl) - float(tal[0])) <= 1e-5 * float(tal[0])
    # back to the default: the step taken before the matcher was set, bit for bit
    m.set_matcher(None).set_quality_loss(None).set_box_loss(None)
    _same(_step(m, img, ann), fresh)


def test_forward_gradient_path_and_two_pass_path_agree():
    """tests/test_gpu_model.py's relation of the two training paths (the class gradient written in forward for an upstream gradient
    of one, or in backward with the upstream scalar), with the matcher: the forward is bitwise the same, so the assignment is too."""
    from efficientdet.pytorch_amd import efficientdet as E
    nc = 4
    img, ann = _batch(nc)
    m = _model(nc, 'f32')
    _recipe(m)
    out = {}
    old = E.LOSS_FWD_GRAD
    try:
        for flag in (True, False):
            E.LOSS_FWD_GRAD = flag
            m.zero_grad(set_to_none=True)
            cl, rl = m([img, ann])
            (0.37 * cl.sum() + 1.9 * rl.sum()).backward()
            torch.cuda.synchronize()
            out[flag] = (cl.detach().clone(), rl.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None})
    finally:
        E.LOSS_FWD_GRAD = old
    assert torch.equal(out[True][1], out[False][1]) and abs(float(out[True][0]) - float(out[False][0])) <= 1e-5 * float(out[False][0])
    assert out[True][2].keys() == out[False][2].keys()
    for k in out[True][2]:
        a, b = out[True][2][k].double(), out[False][2][k].double()
        assert float((a - b).norm()) <= 1e-4 * float(b.norm()) + 1e-12, k
        assert_close_scale(out[True][2][k], out[False][2][k], 1e-3, k)


def test_a_graph_replay_is_the_eager_step_with_the_matcher():
    from efficientdet.pytorch_amd import ddp
    from efficientdet.pytorch_amd.graph import GraphedTrainStep, replay_vs_eager
    from efficientdet.pytorch_amd.optim import ClipAdamW
    nc, arith = 4, 'f32_hf16x3_bwd_bf16x3'
    img, ann = _batch(nc)
    m = _model(nc, arith)
    _recipe(m)
    ddp.freeze_dead_parameters(m)
    opt = ClipAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-4, max_norm=0.1)
    g = GraphedTrainStep(m, opt, img, ann, warmup=2)
    g()
    r = replay_vs_eager(g)
    print('replay vs eager (task-aligned matcher + QFL + GIoU, %s): %s' % (arith, r))
    assert r['finite'] and r['update_norm'] > 0
    assert r['eager_vs_eager'] == 0.0 and r['replay_vs_replay'] == 0.0, r
    assert r['replay_vs_eager'] == 0.0, r
    for a, b in zip(r['losses_replay'], r['losses_eager']):
        assert a == b, r
