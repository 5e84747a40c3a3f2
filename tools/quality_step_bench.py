"""Cost of the IoU-aware class loss in the training step: the D0 train step (B = 32 @ 512, the bench's headline arithmetic)
with set_matcher(ATSSOptions()) + set_box_loss(BoxLossOptions('giou')) and `--quality qfl | vfl` (set_quality_loss) or `--quality none`
(the focal term), timed with device events over `--steps` replays of the captured step after `--warmup`.  Run the modes in alternating
processes on one device and compare the medians.  `--eager` runs the steps as eager launches instead (for a kernel trace: the captured
step's launches are the same ones).  Prints one JSON line with ms per step and the valid annotations per image."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--quality', choices=['none', 'qfl', 'vfl'], default='qfl')
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--num-classes', type=int, default=80)
    ap.add_argument('--eager', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('quality_step_bench needs a GPU: a step time comes from a run on the device')
    from efficientdet.pytorch_amd import ATSSOptions, BoxLossOptions, EfficientDet, EFFICIENTDET, QualityLossOptions, ddp
    from efficientdet.pytorch_amd.graph import GraphedTrainStep
    from efficientdet.pytorch_amd.optim import ClipAdamW
    from oracle import effdet_oracle as O
    net = 'efficientdet-d0'
    c = EFFICIENTDET[net]
    m = EfficientDet(a.num_classes, network=net, W_bifpn=c['W_bifpn'], D_bifpn=c['D_bifpn'], D_class=c['D_class'],
                     compute_dtype=torch.float32, f32_arith='f32_hf16x3_bwd_bf16x3')
    m.load_state_dict(O.make_state_dict(net, a.num_classes, seed=0)); m.backbone.drop_connect_rate = 0.0
    m = m.cuda(); m.train(); m.is_training = True; m.freeze_bn()
    m.set_matcher(ATSSOptions()).set_box_loss(BoxLossOptions('giou'))
    if a.quality != 'none':
        m.set_quality_loss(QualityLossOptions(a.quality))
    img, ann = O.synthetic_batch(a.batch, a.size, seed=1, num_classes=a.num_classes)
    img, ann = img.cuda(), ann.cuda()
    ddp.freeze_dead_parameters(m)
    opt = ClipAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-4, max_norm=0.1)
    if a.eager:
        def g():
            opt.zero_grad(set_to_none=True)
            cl, rl = m([img, ann])
            (cl.mean() + rl.mean()).backward()
            opt.step()
    else:
        g = GraphedTrainStep(m, opt, img, ann, warmup=2)
    for _ in range(a.warmup):
        g()
    times = []
    for _ in range(a.steps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(); g(); t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1))
    times.sort()
    print(json.dumps({'tool': 'quality_step_bench', 'quality': a.quality, 'eager': a.eager, 'batch': a.batch, 'size': a.size,
                      'steps': a.steps, 'ms_median': times[len(times) // 2], 'ms_min': times[0], 'ms_max': times[-1],
                      'annotations_per_image': float((ann[:, :, 4] != -1).sum(1).float().mean()), 'rows_per_image': int(ann.shape[1])}))


if __name__ == '__main__':
    main()
