"""Workload for timing mosaic_compose_kernel (csrc/mosaic.hip) against resize_pad_kernel (launch 1 of the 'train' chain, the same
bilinear work per output pixel) in one process: one batch of 32 sources of 500 x 375 at S = 512, every output image a mosaic.  Each
iteration launches ops.mosaic_compose and ops.augment_train on the same sources.  Kernel times come from the profiler:

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o off -- python tools/mosaic_bench.py --mixup off
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o on  -- python tools/mosaic_bench.py --mixup on

It prints one JSON line with the bytes a launch has to move (the canvas written once plus every source of the batch read once), so
that bytes / kernel time is the achieved rate; a mosaic reads a source several times or not at all, which the figure ignores.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mixup', choices=('off', 'on'), default='off')
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=512)
    a = ap.parse_args()
    import torch
    from efficientdet.pytorch_amd import data as D, ops
    from efficientdet.pytorch_amd.functional import chunk_elems
    B, S, h, w = a.batch, a.size, 375, 500
    rng = np.random.RandomState(0)
    col = D.DeviceCollater(device='cuda')
    samples = [{'img': rng.randint(0, 256, (h, w, 3)).astype(np.uint8)} for _ in range(B)]
    src, off, hw, host_hw = col._upload(samples, col._stage_batch(samples))
    opts = D.MosaicOptions(p=1.0, mixup_p=1.0 if a.mixup == 'on' else 0.0)
    mt = D.check_mosaic_table(D.sample_mosaic_table(rng, B, S, opts), B, S, host_hw)
    d_mt = torch.from_numpy(mt).cuda()
    d_at = torch.from_numpy(D.sample_augment_table(rng, B, S)).cuda()
    for _ in range(5 + a.iters):
        ops.mosaic_compose(src, off, hw, d_mt, S, opts.fill)
        ops.augment_train(src, off, hw, d_at, S, torch.bfloat16, chunk_elems(torch.bfloat16), D.MEAN, D.STD)
    torch.cuda.synchronize()
    source = B * h * w * 3
    print(json.dumps({'mixup': a.mixup, 'B': B, 'S': S, 'source_hw': [h, w], 'launches': 5 + a.iters, 'output_pixels': B * S * S,
                      'mosaic_compose_kernel_bytes': B * S * S * 3 + source, 'resize_pad_kernel_bytes': B * S * S * 4 + source}))


if __name__ == '__main__':
    main()
