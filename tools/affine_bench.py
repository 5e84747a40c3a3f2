"""Stage time of the affine / perspective warp (csrc/affine.hip: ops.affine_warp + ops.affine_boxes) next to the time of the 'train'
chain (ops.augment_train + ops.augment_boxes) on the same sources, in one process: one batch of 32 sources of 500 x 375 at S = 512,
every image warped (rotation, shear, scale and translation drawn by data.sample_affine_table).  Two configurations:

  alone      the sources are the dataset images
  canvas2    the sources are the 2S x 2S canvases of a mosaic composed once in front (AffineOptions(canvas=2)); the mosaic's own
             time is printed beside it

Times come from device events around windows of `--inner` calls; the windows of the stage and of the chain alternate, so a drift of
the machine falls on both.  One JSON line: per configuration the median, minimum and maximum over the windows, in microseconds per
call, and the bytes a warp launch has to move at the least (the output written once plus every source read once).

  python tools/affine_bench.py [--windows 20] [--inner 20]
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
    ap.add_argument('--windows', type=int, default=20)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--boxes', type=int, default=32)
    a = ap.parse_args()
    import torch
    from efficientdet.pytorch_amd import data as D, ops
    from efficientdet.pytorch_amd.functional import chunk_elems
    if not torch.cuda.is_available():
        raise SystemExit('affine_bench needs a GPU: a time taken anywhere else says nothing')
    B, S, M, h, w = a.batch, a.size, a.boxes, 375, 500
    rng = np.random.RandomState(0)
    col = D.DeviceCollater(device='cuda')
    samples = [{'img': rng.randint(0, 256, (h, w, 3)).astype(np.uint8)} for _ in range(B)]
    src, off, hw, host_hw = col._upload(samples, col._stage_batch(samples))
    x1, y1 = rng.uniform(0, 0.7 * w, (B, M)), rng.uniform(0, 0.7 * h, (B, M))
    ann = np.stack([x1, y1, x1 + rng.uniform(8, 0.3 * w, (B, M)), y1 + rng.uniform(8, 0.3 * h, (B, M)), rng.randint(0, 20, (B, M))], 2)
    d_ann = torch.from_numpy(ann.astype(np.float32)).cuda()
    d_at = torch.from_numpy(D.sample_augment_table(rng, B, S)).cuda()
    bf16, cpad = torch.bfloat16, chunk_elems(torch.bfloat16)

    def sources(name):
        """-> (src, off, hw on the device, host hw, annots, the mosaic call or None)"""
        if name == 'alone':
            return src, off, hw, host_hw, d_ann, None
        mo = D.MosaicOptions()
        mt = torch.from_numpy(D.check_mosaic_table(D.sample_mosaic_table(rng, B, 2 * S, mo), B, 2 * S, host_hw)).cuda()
        compose = lambda: (ops.mosaic_compose(src, off, hw, mt, 2 * S, mo.fill), ops.mosaic_boxes(hw, mt, 2 * S, d_ann))   # noqa: E731
        canvas, (boxes, _) = compose()
        return (canvas.view(-1), torch.arange(B, dtype=torch.int64, device='cuda') * (4 * S * S * 3),
                torch.full((B, 2), 2 * S, dtype=torch.int32, device='cuda'), np.full((B, 2), 2 * S), boxes, compose)

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.inner):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.inner                    # us per call

    def stats(v):
        return {'median_us': round(float(np.median(v)), 2), 'min_us': round(float(np.min(v)), 2), 'max_us': round(float(np.max(v)), 2)}

    out = {'B': B, 'S': S, 'source_hw': [h, w], 'boxes_per_image': M, 'windows': a.windows, 'inner': a.inner}
    for name in ('alone', 'canvas2'):
        s_src, s_off, s_hw, s_host, s_ann, compose = sources(name)
        opts = D.AffineOptions(degrees=10.0, shear=2.0, canvas=2 if name == 'canvas2' else 1)
        wt = torch.from_numpy(D.check_affine_table(D.sample_affine_table(rng, B, S, s_host, opts), B, S)).cuda()
        fns = {'affine_stage': lambda: (ops.affine_warp(s_src, s_off, s_hw, wt, S, opts.fill),
                                        ops.affine_boxes(s_hw, wt, S, s_ann, opts.wh_thr, opts.ar_thr, opts.area_thr)),
               'chain': lambda: (ops.augment_train(s_src, s_off, s_hw, d_at, S, bf16, cpad, D.MEAN, D.STD),
                                 ops.augment_boxes(s_hw, d_at, S, S, s_ann))}
        if compose is not None:
            fns['mosaic_stage_2S'] = compose
        for fn in fns.values():                                        # warm every shape the windows use
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in fns}
        for _ in range(a.windows):
            for k, fn in fns.items():                                  # interleaved
                times[k].append(window(fn))
        h_s, w_s = int(s_host[0, 0]), int(s_host[0, 1])
        out[name] = {k: stats(v) for k, v in times.items()}
        out[name]['affine_warp_kernel_bytes'] = B * S * S * 3 + B * h_s * w_s * 3
    print(json.dumps(out))


if __name__ == '__main__':
    main()
