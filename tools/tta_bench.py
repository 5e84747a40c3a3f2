"""What flip TTA and the weighted boxes fusion cost: eager detect() plain and with TTAOptions(hflip=True) on the same model and batch,
alternated in one process, and ops.fuse_detections alone at 200 (2 views x 100 rows) and 4096 (4 views x 1024 rows) candidates per image
on seeded boxes (every other row of a later view a jittered copy of a row of view 0, four labels, a 512-pixel frame).  Random-init
weights: every anchor is an NMS candidate and every view hands the fusion its full top_n rows -- the worst case of both stages.
Times are device events around `reps` calls after a warm-up, the median of `rounds` windows; a record for DESIGN.md section 7, not a gate.
    python tools/tta_bench.py [--network efficientdet-d0 --batch 8 --size 512 --reps 10 --rounds 5 --dtype f32_hf16x3|f32_bf16x3|f32|bf16]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from efficientdet.pytorch_amd import EfficientDet, EFFICIENTDET, TTAOptions, WBFOptions, ops       # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--network', default='efficientdet-d0'); ap.add_argument('--batch', type=int, default=8)
ap.add_argument('--size', type=int, default=512); ap.add_argument('--reps', type=int, default=10)
ap.add_argument('--rounds', type=int, default=5); ap.add_argument('--dtype', default='f32_hf16x3')
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit('tta_bench needs the GPU: there is nothing to time without one')


def window(fn):
    """ms per call over one window of a.reps calls (device events; the window ends in a synchronise)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / a.reps


def alternate(fns):
    """Median ms per call of each fn, their windows interleaved (what shares the machine then touches all of them alike)."""
    for fn in fns:
        fn(); fn()
    torch.cuda.synchronize()
    t = [[] for _ in fns]
    for _ in range(a.rounds):
        for i, fn in enumerate(fns):
            t[i].append(window(fn))
    return [(statistics.median(x), min(x), max(x)) for x in t]


def fusion_views(V, rows, B, seed):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0, 414, (B, rows, 2)); wh = rng.uniform(8, 98, (B, rows, 2))
    base = np.concatenate([xy, xy + wh], 2)
    lab = rng.integers(0, 4, (B, rows))
    views = []
    for v in range(V):
        b, l = base.copy(), lab.copy()
        if v:
            b += rng.uniform(-2, 2, b.shape)
            xy = rng.uniform(0, 414, (B, rows, 2)); wh = rng.uniform(8, 98, (B, rows, 2))
            b[:, 1::2] = np.concatenate([xy, xy + wh], 2)[:, 1::2]
            l[:, 1::2] = rng.integers(0, 4, (B, rows))[:, 1::2]
        s = np.sort(rng.uniform(0.05, 1.0, (B, rows)), 1)[:, ::-1].copy()
        views.append((torch.from_numpy(s.astype(np.float32)).cuda(), torch.from_numpy(l.astype(np.int64)).cuda(),
                      torch.from_numpy(b.astype(np.float32)).cuda(), torch.full((B,), rows, dtype=torch.int32, device='cuda')))
    return views


cfg = EFFICIENTDET[a.network]
torch.manual_seed(0)
m = EfficientDet(80, network=a.network, W_bifpn=cfg['W_bifpn'], D_bifpn=cfg['D_bifpn'], D_class=cfg['D_class'], is_training=False,
                 compute_dtype=torch.bfloat16 if a.dtype == 'bf16' else torch.float32,
                 f32_arith={'f32_bf16x3': 'bf16x3', 'f32_hf16x3': 'f32_hf16x3_bwd_bf16x3'}.get(a.dtype, 'f32')).cuda().eval()
img = torch.randn(a.batch, 3, a.size, a.size, device='cuda')
tta = TTAOptions(hflip=True)


def detect_with(options):
    def run():
        m.set_tta(options)
        try:
            return m.detect(img)
        finally:
            m.set_tta(None)
    return run


plain, flip = alternate([detect_with(None), detect_with(tta)])
kept = [len(d[0]) for d in detect_with(None)()]
fused = [len(d[0]) for d in detect_with(tta)()]
print('%s B=%d @%d %s eager detect: plain %.3f ms/batch (min %.3f max %.3f) | flip TTA %.3f ms/batch (min %.3f max %.3f) = %.2fx | '
      'detections per image: plain %d..%d, fused %d..%d'
      % ((a.network, a.batch, a.size, a.dtype) + plain + flip + (flip[0] / plain[0], min(kept), max(kept), min(fused), max(fused))))
for V, rows in ((2, 100), (4, 1024)):
    views = fusion_views(V, rows, a.batch, 7)
    opt = WBFOptions(top_n=rows)
    (t,) = alternate([lambda: ops.fuse_detections(views, options=opt)])
    count = ops.fuse_detections(views, options=opt)[3].tolist()
    print('fuse_detections B=%d, %d views x %d rows = %d candidates per image: %.3f ms/batch (min %.3f max %.3f), %.2f us per candidate step; '
          'clusters per image %d..%d' % ((a.batch, V, rows, V * rows) + t + (t[0] * 1e3 / (V * rows), min(count), max(count))))
