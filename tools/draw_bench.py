"""Time ops.draw_detections alone (csrc/draw.hip): B frames of H x W uint8 RGB, n rows per frame on a grid of boxes (track rows of 8
floats with ids), painted in place.  The call is captured once in a graph and replayed --reps times between two device events after
--warmup replays (repainting a painted frame does the same work: the geometry does not depend on the pixels).  Prints one JSON line
per case: the time per call, the pixels under any primitive (counted on the device: a pixel is under one exactly when painting a black
and a white frame gives the same value), the bytes the rule has to move for them (each read once and written once when a fill blends,
written once otherwise) and the bandwidth that implies -- to be read next to tools/probe/stream_bw's figure on the same machine.

  python tools/draw_bench.py                       # the four cases of DESIGN.md section 5
  python tools/draw_bench.py --frames 8 --size 1080 1920 --rows 256 --no-label
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scene(B, n, H, W, seed=0):
    """rows [B, n, 8] float32 (boxes on a jittered grid, scores descending, 20 classes) and ids [B, n] int32"""
    rng = np.random.RandomState(seed)
    side = int(np.ceil(np.sqrt(n)))
    cw, ch = W / side, H / side
    k = np.arange(n)
    cx = np.tile((k % side + 0.5) * cw, (B, 1)) + rng.uniform(-3, 3, (B, n))
    cy = np.tile((k // side + 0.5) * ch, (B, 1)) + rng.uniform(-3, 3, (B, n))
    w, h = rng.uniform(0.5, 0.8, (B, n)) * cw, rng.uniform(0.6, 0.9, (B, n)) * ch
    score = -np.sort(-rng.uniform(0.15, 0.95, (B, n)), axis=1)
    rows = np.zeros((B, n, 8), dtype=np.float32)
    rows[:, :, :6] = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2, score, rng.randint(0, 20, (B, n)).astype(np.float64)], axis=-1)
    return rows, (np.arange(B * n).reshape(B, n) % 997 + 1).astype(np.int32)


def one(torch, ops, B, H, W, n, label, fill_alpha, warmup, reps):
    rows, ids = scene(B, n, H, W)
    rows, ids = torch.from_numpy(rows).cuda(), torch.from_numpy(ids).cuda()
    counts = torch.full((B,), n, dtype=torch.int32, device='cuda')
    names = ops.draw_names(['class%d' % i for i in range(20)], 'cuda')
    palette = ops.draw_palette(64, 'cuda')
    o = ops.DrawOptions(label=label, show_id=True, fill_alpha=fill_alpha)
    kw = dict(names=names, ids=ids, palette=palette, inplace=True)
    solid = ops.DrawOptions(label=label, show_id=True, fill_alpha=255 if fill_alpha else 0)            # same pixels, no blend
    black = ops.draw_detections(torch.zeros((B, H, W, 3), dtype=torch.uint8, device='cuda'), rows, counts, options=solid, **kw)
    white = ops.draw_detections(torch.full((B, H, W, 3), 255, dtype=torch.uint8, device='cuda'), rows, counts, options=solid, **kw)
    touched = int((black == white).all(dim=3).sum())
    del black, white
    frames = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device='cuda')
    ops.draw_detections(frames, rows, counts, options=o, **kw)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.draw_detections(frames, rows, counts, options=o, **kw)
    for _ in range(warmup):
        graph.replay()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        graph.replay()
    end.record()
    torch.cuda.synchronize()
    us = start.elapsed_time(end) / reps * 1e3
    moved = touched * 3 * (2 if fill_alpha else 1)
    return {'what': 'draw_detections alone, captured, event-timed', 'frames': B, 'H': H, 'W': W, 'rows_per_frame': n, 'label': label,
            'fill_alpha': fill_alpha, 'reps': reps, 'us_per_call': round(us, 2), 'pixels_under_a_primitive': touched,
            'share_of_all_pixels': round(touched / float(B * H * W), 4), 'bytes_the_rule_moves': moved,
            'implied_GB_per_s': round(moved / us / 1e3, 2), 'frame_bytes': B * H * W * 3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int)
    ap.add_argument('--size', type=int, nargs=2, metavar=('H', 'W'))
    ap.add_argument('--rows', type=int)
    ap.add_argument('--no-label', action='store_true')
    ap.add_argument('--fill-alpha', type=int, default=0)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--reps', type=int, default=2000)
    a = ap.parse_args()
    import torch
    from efficientdet.pytorch_amd import ops
    assert torch.cuda.is_available(), 'the renderer needs a GPU'
    if a.frames or a.size or a.rows:
        cases = [(a.frames or 32, (a.size or (512, 512))[0], (a.size or (512, 512))[1], a.rows or 100, not a.no_label)]
    else:
        cases = [(32, 512, 512, 100, True), (32, 512, 512, 100, False), (8, 1080, 1920, 256, True), (8, 1080, 1920, 256, False)]
    for B, H, W, n, label in cases:
        print(json.dumps(one(torch, ops, B, H, W, n, label, a.fill_alpha, a.warmup, a.reps)), flush=True)


if __name__ == '__main__':
    main()
