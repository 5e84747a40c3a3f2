"""Time graph.GraphedTrainLoop against graph.GraphedTrainStep on the headline workload (D0, B = 32 @512, 80 classes, arithmetic
f32_hf16x3_bwd_bf16x3, drop_connect active), and the accumulate pass alone.  Prints one JSON line.

  python tools/train_loop_bench.py [--batch 32 --size 512 --calls 20 --rounds 5]

  step_ms / loop1_ms / loop4_ms   ms per call: `calls` replays between two device synchronisations, host clock; the three are
                                  alternated `rounds` times in one process; median and (min, max) over the rounds
  accumulate_us                   effdet_grad_accumulate (acc += g over every parameter, + its one-thread follow-up launch): 50 calls captured
                                  as one hipGraph, device events around a replay, median of `rounds`; accumulate_TBps = 12 bytes per parameter
                                  over that time (the arena and the gradients of a D0 fit the Infinity Cache: not an HBM figure)
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--network', default='efficientdet-d0')
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--arith', default='f32_hf16x3_bwd_bf16x3')
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    import torch
    from efficientdet.pytorch_amd import EfficientDet, EFFICIENTDET, ddp, _lib as L
    from efficientdet.pytorch_amd.graph import GraphedTrainLoop, GraphedTrainStep
    from efficientdet.pytorch_amd.optim import ClipAdamW
    from efficientdet.pytorch_amd.synthetic import synthetic_batch
    if not torch.cuda.is_available():
        raise SystemExit('train_loop_bench needs a GPU (a CPU run says nothing about these times)')
    img, ann = synthetic_batch(a.batch, a.size, seed=1, num_classes=80)
    img, ann = img.cuda(), ann.cuda()

    def model():
        cfg = EFFICIENTDET[a.network]
        torch.manual_seed(0)
        m = EfficientDet(num_classes=80, network=a.network, W_bifpn=cfg['W_bifpn'], D_bifpn=cfg['D_bifpn'], D_class=cfg['D_class'],
                         is_training=True, compute_dtype=torch.float32, f32_arith=a.arith).cuda()
        m.train(); m.is_training = True; m.freeze_bn()
        ddp.freeze_dead_parameters(m)
        return m, [p for p in m.parameters() if p.requires_grad]

    legs = {}
    m, ps = model()
    legs['step'] = GraphedTrainStep(m, ClipAdamW(ps, lr=1e-4, max_norm=0.1), img, ann, warmup=2)
    for name, k in (('loop1', 1), ('loop4', 4)):
        m, ps = model()
        legs[name] = GraphedTrainLoop(m, ClipAdamW(ps, lr=1e-4, max_norm=0.1, accumulate=True), img, ann, accumulation_steps=k, warmup=2)
    times = {k: [] for k in legs}
    for k, leg in legs.items():                       # every leg's replays warm before the timed rounds
        for _ in range(4):
            leg()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for k, leg in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.calls):
                leg()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3 / a.calls)
    out = {'network': a.network, 'batch': a.batch, 'size': a.size, 'arith': a.arith, 'calls': a.calls, 'rounds': a.rounds}
    for k, v in times.items():
        out[k + '_ms'] = round(statistics.median(v), 4); out[k + '_ms_range'] = [round(min(v), 4), round(max(v), 4)]
    mean, count, skipped, applied = legs['loop4'].optimizer.loss_meter()
    out['loop4_meter'] = {'mean': mean, 'count': count, 'skipped': skipped, 'applied': applied}

    # ---- the accumulate pass alone, on loop1's optimizer (pending != 0: the adding form, 12 bytes per parameter)
    opt = legs['loop1'].optimizer
    t = opt._table
    with torch.cuda.stream(legs['loop1'].stream):
        legs['loop1']._micro()                        # eager: p.grad and its pointer table are current, skip is clear, pending == 1
    torch.cuda.synchronize()
    Lb = L.require('effdet_grad_accumulate')
    reps = 50
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            L.check(Lb.effdet_grad_accumulate(L.ptr(t['g_ptr']), L.ptr(t['a_ptr']), L.ptr(t['numel']), L.ptr(t['block_tensor']),
                                              L.ptr(t['block_first']), t['n'], t['nblocks'], L.ptr(t['ctl']), L.stream_ptr()),
                    'effdet_grad_accumulate')
    g.replay(); torch.cuda.synchronize()
    us = []
    for _ in range(a.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); g.replay(); e1.record(); torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / reps)
    nparam = sum(p.numel() for p in t['params'] if p.grad is not None)
    out['parameters'] = nparam
    out['accumulate_us'] = round(statistics.median(us), 3); out['accumulate_us_range'] = [round(min(us), 3), round(max(us), 3)]
    out['accumulate_TBps'] = round(12.0 * nparam / (statistics.median(us) * 1e-6) / 1e12, 3)
    opt.reset_epoch()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
