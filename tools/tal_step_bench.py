"""Cost of the task-aligned matcher in the training step: the D0 train step (B = 32 @ 512, the bench's headline arithmetic)
with `--matcher none` (the default assignment and loss), `atss` (set_matcher(ATSSOptions()) + QFL + GIoU) or `tal`
(set_matcher(TaskAlignedOptions()) + QFL + GIoU), timed with device events over `--steps` replays of the captured step after `--warmup`.
Run the modes in alternating processes on one device and compare the medians.  `--select ROWS` times the select kernel's forward call
alone instead (ops.loss_opts_fwd with the matcher against the same call with ATSS, on random head outputs with ROWS valid annotations
per image): the difference between two rows counts is the select kernel's, the rest of the call does not depend on the rows.  Prints
one JSON line."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _median_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(steps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(); fn(); t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1))
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def _select(a):
    """The loss forward call alone at `--select` valid rows per image: default bands / ATSS / the task-aligned matcher."""
    from efficientdet.pytorch_amd import ATSSOptions, TaskAlignedOptions, ops
    B, S, nc, rows = a.batch, a.size, a.num_classes, a.select
    anc = ops.anchors(S, S, torch.device('cuda'))
    A = anc.shape[1]
    levels = [9 * (S >> l) * (S >> l) for l in range(3, 8)]
    g = torch.Generator().manual_seed(5)
    cls = torch.sigmoid(torch.randn(B, A, nc, generator=g) * 2.0).cuda()
    reg = (torch.randn(B, A, 4, generator=g) * 0.5).cuda()
    wh = 24.0 + (S / 3.0) * torch.rand(B, rows, 2, generator=g)
    xy = torch.rand(B, rows, 2, generator=g) * (S - 2.0 - wh) + 1.0
    ann = torch.cat([xy, xy + wh, torch.randint(0, nc, (B, rows, 1), generator=g).float()], 2).cuda()
    out = {}
    for name, kw in (('bands', dict()), ('atss', dict(matcher=ATSSOptions(), levels=levels)), ('tal', dict(matcher=TaskAlignedOptions()))):
        out[name + '_ms'] = _median_ms(lambda: ops.loss_opts_fwd(cls, reg, anc, ann, **kw), a.steps, a.warmup)[0]
    print(json.dumps(dict(out, tool='tal_step_bench', select_rows=rows, batch=B, size=S, anchors=A, num_classes=nc, steps=a.steps)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--matcher', choices=['none', 'atss', 'tal'], default='tal')
    ap.add_argument('--select', type=int, default=0, help='time the loss forward call alone at this many valid rows per image')
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--num-classes', type=int, default=80)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tal_step_bench needs a GPU: a step time comes from a run on the device')
    if a.select:
        return _select(a)
    from efficientdet.pytorch_amd import (ATSSOptions, BoxLossOptions, EfficientDet, EFFICIENTDET, QualityLossOptions, TaskAlignedOptions,
                                          ddp)
    from efficientdet.pytorch_amd.graph import GraphedTrainStep
    from efficientdet.pytorch_amd.optim import ClipAdamW
    from oracle import effdet_oracle as O
    net = 'efficientdet-d0'
    c = EFFICIENTDET[net]
    m = EfficientDet(a.num_classes, network=net, W_bifpn=c['W_bifpn'], D_bifpn=c['D_bifpn'], D_class=c['D_class'],
                     compute_dtype=torch.float32, f32_arith='f32_hf16x3_bwd_bf16x3')
    m.load_state_dict(O.make_state_dict(net, a.num_classes, seed=0)); m.backbone.drop_connect_rate = 0.0
    m = m.cuda(); m.train(); m.is_training = True; m.freeze_bn()
    if a.matcher != 'none':
        m.set_matcher(ATSSOptions() if a.matcher == 'atss' else TaskAlignedOptions())
        m.set_quality_loss(QualityLossOptions('qfl')).set_box_loss(BoxLossOptions('giou'))
    img, ann = O.synthetic_batch(a.batch, a.size, seed=1, num_classes=a.num_classes)
    img, ann = img.cuda(), ann.cuda()
    ddp.freeze_dead_parameters(m)
    opt = ClipAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-4, max_norm=0.1)
    g = GraphedTrainStep(m, opt, img, ann, warmup=2)
    med, lo, hi = _median_ms(g, a.steps, a.warmup)
    print(json.dumps({'tool': 'tal_step_bench', 'matcher': a.matcher, 'batch': a.batch, 'size': a.size, 'steps': a.steps,
                      'ms_median': med, 'ms_min': lo, 'ms_max': hi,
                      'annotations_per_image': float((ann[:, :, 4] != -1).sum(1).float().mean()), 'rows_per_image': int(ann.shape[1])}))


if __name__ == '__main__':
    main()
