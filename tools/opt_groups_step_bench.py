"""Device time of the fused optimizer step: one-group ClipAdamW against the grouped step and against ClipSGD (DESIGN §4 "Parameter groups").

Each variant steps the trainable parameters of a D0 model (80 classes) with fixed random gradients.  Its step() is captured once as a
hipGraph (the gradient-pointer upload + the three launches), and a window is `--replays` replays between two device events, so the host
side of step() is not in the number.  The variants alternate, window by window, for `--rounds` rounds in ONE process; per variant the
median, the smallest and the largest window are reported in microseconds per step, with the bytes the step must move.

    python tools/opt_groups_step_bench.py --out profiles/opt_groups_step_bench.jsonl

  adamw_one      ClipAdamW(params)                                          the one-group calls (unchanged code)
  adamw_groups   ClipAdamW(split_param_groups(model, 4e-5, 0.1))            four groups through effdet_opt_step_groups
  sgd_groups     ClipSGD(split_param_groups(model, 4e-5, 0.1), momentum 0.9, nesterov)"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--replays', type=int, default=1000)
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--num-classes', type=int, default=80)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('opt_groups_step_bench needs a GPU: a step time comes from a run on the device')
    from efficientdet.pytorch_amd import EfficientDet, EFFICIENTDET, ddp
    from efficientdet.pytorch_amd.optim import ClipAdamW, ClipSGD, split_param_groups
    c = EFFICIENTDET['efficientdet-d0']

    def variant(kind):
        torch.manual_seed(0)
        m = EfficientDet(a.num_classes, network='efficientdet-d0', W_bifpn=c['W_bifpn'], D_bifpn=c['D_bifpn'], D_class=c['D_class']).cuda()
        ddp.freeze_dead_parameters(m)
        if kind == 'adamw_one':
            opt = ClipAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-4, weight_decay=4e-5, max_norm=0.1)
        elif kind == 'adamw_groups':
            opt = ClipAdamW(split_param_groups(m, 4e-5, backbone_lr_scale=0.1), lr=1e-4, max_norm=0.1)
        else:
            opt = ClipSGD(split_param_groups(m, 4e-5, backbone_lr_scale=0.1), lr=1e-2, momentum=0.9, nesterov=True, max_norm=0.1)
        for g in opt.param_groups:
            g['lr'] *= g.get('lr_scale', 1.0)
        params = [p for g in opt.param_groups for p in g['params'] if p.requires_grad]
        for p in params:
            p.grad = torch.randn_like(p) * 1e-3
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                opt.step()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            opt.step()
        torch.cuda.synchronize()
        n = sum(p.numel() for p in params)
        per = {'adamw_one': 28, 'adamw_groups': 28, 'sgd_groups': 24}[kind]      # g twice, p and each moment read + written
        return {'kind': kind, 'graph': graph, 'keep': (m, opt), 'groups': len(opt.param_groups), 'tensors': len(params), 'parameters': n,
                'bytes_per_step': n * per, 'windows': []}

    vs = [variant(k) for k in ('adamw_one', 'adamw_groups', 'sgd_groups')]
    for v in vs:                                             # warm every graph once more before the first timed window
        for _ in range(20):
            v['graph'].replay()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for v in vs:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.replays):
                v['graph'].replay()
            t1.record()
            torch.cuda.synchronize()
            v['windows'].append(t0.elapsed_time(t1) * 1e3 / a.replays)
    lines = []
    for v in vs:
        w = v['windows']
        med = statistics.median(w)
        lines.append(json.dumps({'tool': 'opt_groups_step_bench', 'variant': v['kind'], 'groups': v['groups'], 'tensors': v['tensors'],
                                 'parameters': v['parameters'], 'bytes_per_step': v['bytes_per_step'], 'replays_per_window': a.replays,
                                 'rounds': a.rounds, 'us_per_step_median': round(med, 3), 'us_per_step_min': round(min(w), 3),
                                 'us_per_step_max': round(max(w), 3), 'tb_per_s_at_median': round(v['bytes_per_step'] / med / 1e6, 3),
                                 'us_per_step_windows': [round(x, 3) for x in w]}))
    for l in lines:
        print(l)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
