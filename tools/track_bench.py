"""Time ops.track_step alone: by default B = 32 streams, 100 detections per stream (a 10 x 10 grid of objects that drift a little every
frame, scores spread over the high and the low band), max_tracks = 128.  Ten eager frames bring the trackers to a steady state; the
step is then captured once in a graph and replayed --reps times between two events after --warmup replays.  Prints one JSON line with
the time per step and its share of one detection batch (--detect-ms-per-img, by default the committed D0 B = 32 inference time of
profiles/r06_bench_line.json).  --assignment optimal times the tracker with TrackOptions(assignment='optimal') (include/effdet_assign.h);
--dense replaces the grid by the adversarial scene for that solver: every box of a stream overlaps every other, so each association is
one dense component and the augmenting-path searches are as long as they get.

  python tools/track_bench.py
  python tools/track_bench.py --assignment optimal --dets 128 --max-tracks 256 --dense
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def frames(B, n, F, seed=0, dense=False):
    """[F, B, n, 6] float32: n objects per stream on a grid in a 512 x 512 frame, drifting by up to a pixel per frame; dense: all of
    them within 40 px of the centre and 100-140 px wide and high, every box overlapping every other"""
    rng = np.random.RandomState(seed)
    side = int(np.ceil(np.sqrt(n)))
    cell = 512.0 / side
    k = np.arange(n)
    cx = np.tile((k % side + 0.5) * cell, (B, 1)) + rng.uniform(-3, 3, (B, n))
    cy = np.tile((k // side + 0.5) * cell, (B, 1)) + rng.uniform(-3, 3, (B, n))
    w, h = rng.uniform(0.5, 0.8, (B, n)) * cell, rng.uniform(0.6, 0.9, (B, n)) * cell
    if dense:
        cx, cy = 256 + rng.uniform(-40, 40, (B, n)), 256 + rng.uniform(-40, 40, (B, n))
        w, h = rng.uniform(100, 140, (B, n)), rng.uniform(100, 140, (B, n))
    score = -np.sort(-rng.uniform(0.15, 0.95, (B, n)), axis=1)                    # score-descending rows, as finalize_dets writes them
    label = rng.randint(0, 20, (B, n)).astype(np.float64)
    out = np.zeros((F, B, n, 6), dtype=np.float32)
    for f in range(F):
        cx, cy = cx + rng.uniform(-1, 1, (B, n)), cy + rng.uniform(-1, 1, (B, n))
        out[f] = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2, score, label], axis=-1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--streams', type=int, default=32)
    ap.add_argument('--dets', type=int, default=100)
    ap.add_argument('--max-tracks', type=int, default=128)
    ap.add_argument('--frames', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--detect-ms-per-img', type=float, default=0.378)
    ap.add_argument('--assignment', choices=('greedy', 'optimal'), default='greedy')
    ap.add_argument('--dense', action='store_true')
    a = ap.parse_args()
    import torch
    from efficientdet.pytorch_amd import ops
    assert torch.cuda.is_available(), 'the tracker needs a GPU'
    B = a.streams
    seq = torch.from_numpy(frames(B, a.dets, a.frames + 1, dense=a.dense)).cuda()
    counts = torch.full((B,), a.dets, dtype=torch.int32, device='cuda')
    o = ops.TrackOptions(max_tracks=a.max_tracks) if a.assignment == 'greedy' else ops.TrackOptions(max_tracks=a.max_tracks, assignment=a.assignment)
    state = ops.track_state(B, a.max_tracks, 'cuda')
    out = None
    for f in range(a.frames):
        out = ops.track_step(seq[f], counts, state, o, out=out)
    torch.cuda.synchronize()
    tracked = int(out[2].sum())
    static = seq[a.frames].clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.track_step(static, counts, state, o, out=out)
    for _ in range(a.warmup):
        graph.replay()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(a.reps):
        graph.replay()
    end.record()
    torch.cuda.synchronize()
    ms = start.elapsed_time(end) / a.reps
    batch_ms = a.detect_ms_per_img * B
    print(json.dumps({'what': 'track_step alone, captured, event-timed', 'streams': B, 'dets_per_stream': a.dets, 'max_tracks': a.max_tracks,
                      'assignment': a.assignment, 'scene': 'dense' if a.dense else 'grid',
                      'steady_state_frames': a.frames, 'reps': a.reps, 'tracked_per_stream': round(tracked / B, 1),
                      'tracked_after': round(int(out[2].sum()) / B, 1), 'overflow': int(ops.track_overflow(state).sum()),
                      'step_ms': round(ms, 5), 'detect_batch_ms': round(batch_ms, 3), 'share_of_detect_batch': round(ms / batch_ms, 5)}))


if __name__ == '__main__':
    main()
