"""Time the device COCO metric (evaluate.COCOMeanAP) on a synthetic val2017-sized run: 5 000 images, 80 categories, about 7 GTs per
image (about 1 % crowd), up to 100 kept detections per image; `add` per batch of 32 and one `compute`.  Prints one JSON line
(device-event times).

  python tools/coco_map_bench.py                # GPU: add / compute times (profile with rocprofv3 --kernel-trace --stats for kernel times)
  python tools/coco_map_bench.py --cpu-ref      # CPU only: the NumPy restatement of COCOeval (tests/coco_eval_restated.py) on the same data
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic(n_img=5000, K=80, slots=100, seed=0):
    """-> (dets [n, slots, 6] fp32 (x, y, w, h, score, category index; score-descending, label -1 past counts), counts [n],
    gts: per image [g, 7] (x, y, w, h, category index, iscrowd, area), image ids (shuffled, val2017-like magnitudes))."""
    rng = np.random.RandomState(seed)
    ids = np.sort(rng.choice(np.arange(1, 600000), n_img, replace=False))[rng.permutation(n_img)]
    dets = np.zeros((n_img, slots, 6), dtype=np.float32)
    dets[:, :, 5] = -1
    counts = rng.randint(slots // 2, slots + 1, n_img).astype(np.int32)
    gts = []
    for i in range(n_img):
        ng = max(1, rng.poisson(7))
        wh = np.exp(rng.uniform(np.log(4), np.log(400), (ng, 2)))
        xy = rng.uniform(0, 640, (ng, 2))
        cat = rng.randint(0, K, ng)
        g = np.concatenate([xy, wh, cat[:, None], (rng.rand(ng) < 0.01)[:, None], (wh[:, 0] * wh[:, 1] * 0.8)[:, None]], 1)
        gts.append(g)
        k = counts[i]
        gi = g[rng.randint(0, ng, k)]
        near = rng.rand(k) < 0.5
        rnd = np.concatenate([rng.uniform(0, 640, (k, 2)), np.exp(rng.uniform(np.log(4), np.log(300), (k, 2)))], 1)
        box = np.where(near[:, None], gi[:, :4] + rng.normal(0, 0.1, (k, 4)) * np.concatenate([gi[:, 2:4]] * 2, 1), rnd)
        box[:, 2:] = np.maximum(box[:, 2:], 0.5)
        dets[i, :k, :4] = box
        dets[i, :k, 4] = np.sort(rng.uniform(0.05, 1.0, k).astype(np.float32))[::-1]
        dets[i, :k, 5] = np.where(near & (rng.rand(k) < 0.9), gi[:, 4], rng.randint(0, K, k))
    return dets, counts, gts, ids.astype(np.int64)


def cpu_reference(dets, counts, gts, ids, K):
    from tests import coco_eval_restated as R
    gt = {'annotations': [], 'categories': [{'id': c} for c in range(K)]}
    dt = []
    aid = 1
    for d, n, g, iid in zip(dets, counts, gts, ids):
        for r in g:
            gt['annotations'].append({'id': aid, 'image_id': int(iid), 'category_id': int(r[4]), 'bbox': [float(v) for v in r[:4]],
                                      'iscrowd': int(r[5]), 'area': float(r[6])})
            aid += 1
        for r in d[:int(n)]:
            dt.append({'image_id': int(iid), 'category_id': int(r[5]), 'bbox': [float(v) for v in r[:4]], 'score': float(r[4])})
    return R.coco_eval(gt, dt, [int(i) for i in ids])[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=5000)
    ap.add_argument('--categories', type=int, default=80)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--cpu-ref', action='store_true')
    a = ap.parse_args()
    dets, counts, gts, ids = synthetic(a.images, a.categories)
    if a.cpu_ref:
        t = time.perf_counter()
        stats = cpu_reference(dets, counts, gts, ids, a.categories)
        print(json.dumps({'what': 'cpu restatement of COCOeval (evaluate + accumulate + summarize)', 'images': a.images,
                          'detections': int(counts.sum()), 'seconds': round(time.perf_counter() - t, 3), 'AP': float(stats[0])}))
        return
    import torch
    from efficientdet.pytorch_amd.evaluate import COCOMeanAP
    assert torch.cuda.is_available(), 'the device metric needs a GPU'
    dd, cd = torch.from_numpy(dets).cuda(), torch.from_numpy(counts).cuda()
    gpu_gts = []                                                   # the GT of every batch staged once, so add() times the device work
    for i in range(0, a.images, a.batch):
        g = gts[i:i + a.batch]
        G = max(len(x) for x in g)
        h = np.zeros((len(g), G, 7)); h[:, :, 4] = -1
        for j, x in enumerate(g):
            h[j, :len(x)] = x
        gpu_gts.append(torch.from_numpy(h).cuda())
    add_ms, compute_ms = [], []
    for rep in range(a.reps + 1):                                  # rep 0: warm-up
        m = COCOMeanAP(a.categories)
        m._reserve(a.images * dets.shape[1])                       # (growth measured separately: not part of the per-batch time)
        torch.cuda.synchronize()
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        for k, i in enumerate(range(0, a.images, a.batch)):
            m.add(dd[i:i + a.batch], cd[i:i + a.batch], ids[i:i + a.batch], gpu_gts[k])
        e1.record()
        stats = m.compute()
        e2.record()
        torch.cuda.synchronize()
        if rep:
            add_ms.append(e0.elapsed_time(e1) / len(gpu_gts)); compute_ms.append(e1.elapsed_time(e2))
    print(json.dumps({'what': 'device COCO metric', 'images': a.images, 'categories': a.categories, 'records': m.num_records,
                      'detections': int(counts.sum()), 'add_ms_per_batch_of_%d' % a.batch: round(float(np.median(add_ms)), 4),
                      'compute_ms': round(float(np.median(compute_ms)), 4), 'AP': float(stats[0])}))


if __name__ == '__main__':
    main()
