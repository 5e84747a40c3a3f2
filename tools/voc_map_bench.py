"""Time the device VOC metric (evaluate.VOCMeanAP) on a synthetic VOC07-test-sized run: 4 952 images x 100 detection slots, 20 classes,
`add` per batch of 32 and one `compute` over the 495 200 records.  Prints one JSON line (device-event times).

  python tools/voc_map_bench.py                 # GPU: add / compute times (profile with rocprofv3 --kernel-trace --stats for kernel times)
  python tools/voc_map_bench.py --cpu-ref       # CPU only: the reference's per-detection loop (eval.py:198-241 restated) on the same data
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic(n_img=4952, C=20, slots=100, seed=0):
    rng = np.random.RandomState(seed)
    dets = np.zeros((n_img, slots, 6), dtype=np.float32)
    dets[:, :, 5] = -1
    counts = np.full(n_img, slots, dtype=np.int32)
    gts = []
    for i in range(n_img):
        ng = rng.randint(1, 9)
        x1 = rng.uniform(0, 400, ng); y1 = rng.uniform(0, 400, ng)
        g = np.stack([x1, y1, x1 + rng.uniform(10, 200, ng), y1 + rng.uniform(10, 200, ng), rng.randint(0, C, ng)], 1)
        gts.append(g)
        gi = g[rng.randint(0, ng, slots)]
        near = rng.rand(slots) < 0.5
        wh = np.concatenate([gi[:, 2:4] - gi[:, 0:2]] * 2, 1)
        rnd = rng.uniform(0, 400, (slots, 2))
        box = np.where(near[:, None], gi[:, :4] + rng.normal(0, 0.12, (slots, 4)) * wh,
                       np.concatenate([rnd, rnd + rng.uniform(5, 150, (slots, 2))], 1))
        dets[i, :, :4] = box
        dets[i, :, 4] = np.sort(rng.uniform(0.05, 1.0, slots).astype(np.float32))[::-1]
        dets[i, :, 5] = np.where(near, gi[:, 4], rng.randint(0, C, slots))
    return dets, counts, gts


def reference_loop(dets, counts, gts, C, iou_threshold=0.5):
    """eval.py:198-241 as the reference runs it: per class, per image, per detection compute_overlap + np.append."""
    def overlap(a, b):
        area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        iw = np.minimum(np.expand_dims(a[:, 2], 1), b[:, 2]) - np.maximum(np.expand_dims(a[:, 0], 1), b[:, 0])
        ih = np.minimum(np.expand_dims(a[:, 3], 1), b[:, 3]) - np.maximum(np.expand_dims(a[:, 1], 1), b[:, 1])
        iw = np.maximum(iw, 0); ih = np.maximum(ih, 0)
        ua = np.maximum(np.expand_dims((a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]), 1) + area - iw * ih, np.finfo(float).eps)
        return iw * ih / ua
    rows = [d[:n].astype(np.float64) for d, n in zip(dets, counts)]
    aps = []
    for label in range(C):
        fp, tp, scores, nann = np.zeros((0,)), np.zeros((0,)), np.zeros((0,)), 0.0
        for d, g in zip(rows, gts):
            det = d[d[:, 5] == label, :5]
            ann = g[g[:, 4] == label, :4]
            nann += ann.shape[0]
            taken = []
            for x in det:
                scores = np.append(scores, x[4])
                if ann.shape[0] == 0:
                    fp = np.append(fp, 1); tp = np.append(tp, 0)
                    continue
                ov = overlap(np.expand_dims(x, 0), ann)
                a = np.argmax(ov, axis=1)
                if ov[0, a] >= iou_threshold and a not in taken:
                    fp = np.append(fp, 0); tp = np.append(tp, 1); taken.append(a)
                else:
                    fp = np.append(fp, 1); tp = np.append(tp, 0)
        if nann == 0:
            aps.append(0)
            continue
        o = np.argsort(-scores)
        tp, fp = np.cumsum(tp[o]), np.cumsum(fp[o])
        r, p = tp / nann, tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
        mrec = np.concatenate(([0.], r, [1.])); mpre = np.concatenate(([0.], p, [0.]))
        for i in range(mpre.size - 1, 0, -1):
            mpre[i - 1] = np.maximum(mpre[i - 1], mpre[i])
        i = np.where(mrec[1:] != mrec[:-1])[0]
        aps.append(np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1]))
    return aps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=4952)
    ap.add_argument('--classes', type=int, default=20)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--cpu-ref', action='store_true')
    a = ap.parse_args()
    dets, counts, gts = synthetic(a.images, a.classes)
    if a.cpu_ref:
        t = time.perf_counter()
        aps = reference_loop(dets, counts, gts, a.classes)
        print(json.dumps({'what': 'cpu reference loop', 'records': int(counts.sum()), 'seconds': round(time.perf_counter() - t, 3),
                          'mean_ap': float(np.mean(aps))}))
        return
    import torch
    from efficientdet.pytorch_amd.evaluate import VOCMeanAP
    assert torch.cuda.is_available(), 'the device metric needs a GPU'
    dd, cd = torch.from_numpy(dets).cuda(), torch.from_numpy(counts).cuda()
    gpu_gts = []                                                   # the GT of every batch staged once, so add() times the device work
    for i in range(0, a.images, a.batch):
        g = gts[i:i + a.batch]
        G = max(len(x) for x in g)
        hb = np.zeros((len(g), G, 4)); hl = np.full((len(g), G), -1, dtype=np.int32)
        for j, x in enumerate(g):
            hb[j, :len(x)] = x[:, :4]; hl[j, :len(x)] = x[:, 4]
        gpu_gts.append((torch.from_numpy(hb).cuda(), torch.from_numpy(hl).cuda()))
    add_ms, compute_ms = [], []
    for rep in range(a.reps + 1):                                  # rep 0: warm-up
        m = VOCMeanAP(a.classes)
        m._reserve(a.images * dets.shape[1])                       # (growth measured separately: not part of the per-batch time)
        torch.cuda.synchronize()
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        for k, i in enumerate(range(0, a.images, a.batch)):
            m.add(dd[i:i + a.batch], cd[i:i + a.batch], gpu_gts[k])
        e1.record()
        out = m.compute()
        e2.record()
        torch.cuda.synchronize()
        if rep:
            add_ms.append(e0.elapsed_time(e1) / len(gpu_gts)); compute_ms.append(e1.elapsed_time(e2))
    print(json.dumps({'what': 'device VOC metric', 'images': a.images, 'classes': a.classes, 'records': m.num_records,
                      'add_ms_per_batch_of_%d' % a.batch: round(float(np.median(add_ms)), 4),
                      'compute_ms': round(float(np.median(compute_ms)), 4), 'mean_ap': float(out[0])}))


if __name__ == '__main__':
    main()
