"""Time the device-side get_augumentation (data.DeviceAugmentation) on a batch of 32 COCO-like images (mixed sizes around
640 x 480, 7 boxes each) at 512 x 512 and 1024 x 1024.  Prints one JSON line per size (ms per batch):

  device_train   the 'train' chain's kernels (ops.augment_train + augment_boxes, inputs already on the device; CLAHE on every
                 image, the worst case), device-event time;
  device_valid   the 'valid' chain's kernels (ops.augment_resize + augment_boxes);
  collate_train  one full aug(samples) call with sampled parameters, host wall time including staging, copies and the
                 device-to-host read of the kept-box counts.

  python tools/augment_bench.py [--iters 50]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def samples(B=32, seed=0):
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(B):
        h, w = int(rng.randint(360, 641)), int(rng.randint(360, 641))
        img = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        x1 = rng.uniform(0, w * 0.7, 7); y1 = rng.uniform(0, h * 0.7, 7)
        ann = np.stack([x1, y1, x1 + rng.uniform(8, w * 0.3, 7), y1 + rng.uniform(8, h * 0.3, 7), rng.randint(0, 80, 7)], 1)
        out.append({'img': img, 'annot': ann.astype(np.float32)})
    return out


def _time_device(fn, iters):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--batch', type=int, default=32)
    a = ap.parse_args()
    import torch
    from efficientdet.pytorch_amd import data as D, ops
    from efficientdet.pytorch_amd.functional import chunk_elems
    S_list = (512, 1024)
    smp = samples(a.batch)
    for S in S_list:
        dt = torch.bfloat16
        aug = D.DeviceAugmentation('train', width=S, height=S, dtype=dt, seed=0)
        stage, slot, offs, hw = aug._stage_images(smp)
        src, d_off, d_hw = aug._upload_images(stage, slot, offs, hw)
        table = D.sample_augment_table(np.random.RandomState(1), a.batch, S)
        table[:, D.AUG['clahe']] = 1
        table[:, D.AUG['clip_limit']] = 2.5
        d_tab = torch.from_numpy(table).cuda()
        d_ann = torch.from_numpy(aug._padded_annots(smp)).cuda()
        ce = chunk_elems(dt)
        train = _time_device(lambda: (ops.augment_train(src, d_off, d_hw, d_tab, S, dt, ce, D.MEAN, D.STD),
                                      ops.augment_boxes(d_hw, d_tab, S, S, d_ann)), a.iters)
        valid = _time_device(lambda: (ops.augment_resize(src, d_off, d_hw, S, S, dt, ce, D.MEAN, D.STD),
                                      ops.augment_boxes(d_hw, None, S, S, d_ann)), a.iters)
        for _ in range(3):
            aug(smp)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            aug(smp)
        torch.cuda.synchronize()
        coll = (time.perf_counter() - t0) * 1e3 / a.iters
        print(json.dumps({'size': S, 'batch': a.batch, 'dtype': 'bf16', 'device_train_ms': round(train, 4),
                          'device_valid_ms': round(valid, 4), 'collate_train_ms': round(coll, 3), 'budget_ms_512': 1.0}), flush=True)


if __name__ == '__main__':
    main()
