"""Workload for timing the optimizer's update kernel with and without the parameter EMA (DESIGN §5 "Parameter EMA").

Runs ClipAdamW.step() over the trainable parameters of a D0 model with fixed random gradients: `--warmup` steps, then `--steps`; with
`--ema-decay` the EMA instantiation runs, and `--swaps N` adds N in-place weight swaps at the end (use an even number).  The script takes
no time itself: run it under the kernel tracer in a process of its own and read `opt_adamw_kernel` / `ema_swap_kernel` in the statistics,

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o NAME -- python tools/ema_step_bench.py --ema-decay 0.9998

A library of another commit is timed through the binding's EFFDET_HIP_LIB override (with the EMA off).  Prints one JSON line with the
parameter count and the bytes per step the kernel must move (28 B per parameter, 36 with the average)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ema-decay', type=float, default=None)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--swaps', type=int, default=0)
    ap.add_argument('--num-classes', type=int, default=80)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('ema_step_bench needs a GPU: a kernel time comes from a run on the device')
    from efficientdet.pytorch_amd import EfficientDet, EFFICIENTDET, ddp
    from efficientdet.pytorch_amd.optim import ClipAdamW
    c = EFFICIENTDET['efficientdet-d0']
    torch.manual_seed(0)
    m = EfficientDet(a.num_classes, network='efficientdet-d0', W_bifpn=c['W_bifpn'], D_bifpn=c['D_bifpn'], D_class=c['D_class']).cuda()
    ddp.freeze_dead_parameters(m)
    params = [p for p in m.parameters() if p.requires_grad]
    grads = [torch.randn_like(p) * 1e-3 for p in params]
    opt = ClipAdamW(params, lr=1e-4, max_norm=0.1, ema_decay=a.ema_decay)
    for _ in range(a.warmup + a.steps):
        for p, g in zip(params, grads):
            p.grad = g
        opt.step()
    for _ in range(a.swaps):
        opt.swap_ema()
    torch.cuda.synchronize()
    n = sum(p.numel() for p in params)
    print(json.dumps({'tool': 'ema_step_bench', 'ema_decay': a.ema_decay, 'steps': a.steps, 'warmup': a.warmup, 'swaps': a.swaps,
                      'tensors': len(params), 'parameters': n, 'update_bytes_per_step': n * (36 if a.ema_decay is not None else 28),
                      'swap_bytes': n * 16, 'ema_updates': opt.ema_updates() if a.ema_decay is not None else None,
                      'lib': os.environ.get('EFFDET_HIP_LIB') or 'in-tree'}))


if __name__ == '__main__':
    main()
