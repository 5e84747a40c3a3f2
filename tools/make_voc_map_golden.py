"""Generate tests/golden/voc_map.npz: the reference's VOC metric (eval.py:165-257 `evaluate`, with `_get_detections`,
`_get_annotations`, `compute_overlap` and `_compute_ap`) executed FROM ITS OWN SOURCE TEXT on a stub dataset / model that replays
seeded detection lists.  BUILD CONTAINER ONLY (reads the reference through oracle/make_golden.reference_source_objects).

`_compute_ap` is wrapped in the namespace to record the sorted recall / precision arrays `evaluate` hands it, per class.

Contents: 48 images, 20 classes, 0-160 raw detections per image (the top-100 cap bites), images without detections and with (0, 5)
ground truth, a class without ground truth (19: AP 0 in the mean), a class with ground truth but no detections (18), IoU exactly 0.5
and one ulp below it, duplicate detections of one GT, a detection whose best GT is taken while another qualifying GT is free, an
exact IoU tie between two GTs, a zero-area GT, non-trivial scales.  Scores are distinct within each class (asserted).

Usage:  python tools/make_voc_map_golden.py      (writes tests/golden/voc_map.npz; deterministic)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.make_golden import reference_source_objects  # noqa: E402

NC, NIMG = 20, 48
OUT = os.path.join(ROOT, 'tests', 'golden', 'voc_map.npz')


def crafted():
    """(image -> (scale, [(box, label)] detections in score order, gt [n, 5])) of the corner cases; boxes AFTER the division."""
    det = np.array([10, 10, 30, 20], dtype=np.float64)
    y1 = 10.0
    for _ in range(8):                             # a GT y1 a few ulps above 10: IoU = the double just below 0.5
        y1 = np.nextafter(y1, np.inf)
        area = (30.0 - 10.0) * (30.0 - y1)
        ih = min(det[3], 30.0) - max(det[1], y1)
        if 20.0 * ih / ((det[2] - det[0]) * (det[3] - det[1]) + area - 20.0 * ih) == np.nextafter(0.5, 0.0):
            break
    else:
        raise AssertionError('no GT one ulp off')
    return {
        # IoU exactly 0.5 (TP) and one ulp below (FP), class 0
        0: (1.0, [([10, 10, 30, 20], 0), ([110, 10, 130, 20], 0)],
            np.array([[10, 10, 30, 30, 0], [110, y1, 130, 30, 0]], dtype=np.float64)),
        # duplicates of one GT (TP, FP, FP), class 1; scale 2 (exact division)
        1: (2.0, [([20, 20, 60, 60], 1), ([20, 20, 60, 61], 1), ([21, 20, 60, 60], 1)],
            np.array([[20, 20, 60, 60, 1]], dtype=np.float64)),
        # best GT taken while another qualifying GT is free (TP, FP), class 2
        2: (0.5, [([0, 0, 100, 100], 2), ([0, 0, 100, 98], 2)],
            np.array([[0, 0, 100, 100, 2], [0, 0, 100, 90, 2]], dtype=np.float64)),
        # exact IoU tie between two GTs (0.6 each: argmax takes the first; the second detection is FP), class 3,
        # plus a zero-area GT of class 4 and a detection on it (IoU 0: FP)
        3: (1.0, [([5, 0, 25, 20], 3), ([5, 0, 25, 20], 3), ([50, 50, 50, 60], 4)],
            np.array([[0, 0, 20, 20, 3], [10, 0, 30, 20, 3], [50, 50, 50, 60, 4]], dtype=np.float64)),
    }


def make_inputs():
    rng = np.random.RandomState(20261015)
    pool = rng.permutation(np.linspace(0.001, 0.999, 9000).astype(np.float32))     # distinct fp32 scores, dataset-wide
    assert len(np.unique(pool)) == len(pool)
    take = iter(pool.tolist())
    special = crafted()
    scales = rng.choice([0.37, 0.5, 0.8, 1.25, 1.6, 2.0], NIMG).tolist()
    nraw = rng.choice([0, 3, 12, 40, 70, 105, 130, 160], NIMG).tolist()
    for i in (5, 17, 30):
        nraw[i] = 0                                                            # images with no detections
    det_labels = [c for c in range(NC) if c != 18]                             # 18: GT, never detected
    gt_labels = list(range(19))                                                # 19: detected, never GT
    images = []
    for i in range(NIMG):
        if i in special:
            scale, rows, gt = special[i]
            sc = np.array(sorted([next(take) for _ in rows], reverse=True), dtype=np.float32)
            boxes = np.array([b for b, _ in rows], dtype=np.float32) * np.float32(scale)
            labels = np.array([l for _, l in rows], dtype=np.int64)
            images.append((scale, sc, labels, boxes, gt))
            continue
        scale = float(scales[i])
        ng = 0 if i in (7, 17, 29, 40) else int(rng.randint(1, 7))             # (0, 5) ground truth on some images
        x1 = rng.uniform(0, 300, ng); y1 = rng.uniform(0, 300, ng)
        gt = np.stack([x1, y1, x1 + rng.uniform(8, 150, ng), y1 + rng.uniform(8, 150, ng),
                       rng.choice(gt_labels, ng).astype(np.float64)], 1) if ng else np.zeros((0, 5))
        n = int(nraw[i])
        sc = np.sort(np.array([next(take) for _ in range(n)], dtype=np.float32))[::-1].copy()
        boxes = np.zeros((n, 4), dtype=np.float64)
        labels = np.zeros(n, dtype=np.int64)
        for k in range(n):
            if ng and rng.rand() < 0.6:                                          # near a GT: TPs, duplicates, near misses
                g = gt[rng.randint(ng)]
                w, h = g[2] - g[0], g[3] - g[1]
                j = rng.normal(0, 0.15, 4) * np.array([w, h, w, h])
                boxes[k] = g[:4] + j
                labels[k] = int(g[4]) if rng.rand() < 0.8 else rng.choice(det_labels)
            else:
                bx, by = rng.uniform(0, 350, 2)
                boxes[k] = [bx, by, bx + rng.uniform(4, 120), by + rng.uniform(4, 120)]
                labels[k] = rng.choice(det_labels)
        labels[labels == 18] = 17
        boxes = (boxes * scale).astype(np.float32)                             # what the model emits (the metric divides by scale)
        images.append((scale, sc, labels, boxes, gt))
    return images


def main():
    torch.Tensor.cuda = lambda self, *a, **k: self
    images = make_inputs()

    class DS:
        def __len__(self): return len(images)
        def num_classes(self): return NC
        def label_to_name(self, l): return 'class%d' % l
        def __getitem__(self, i): return {'img': torch.zeros(4, 4, 3), 'scale': images[i][0]}
        def load_annotations(self, i): return images[i][4].copy()

    class Model:
        def __init__(self): self.i = 0
        def eval(self): pass

        def __call__(self, x):
            _, s, l, b, _ = images[self.i]; self.i += 1
            return torch.from_numpy(s.copy()), torch.from_numpy(l.copy()), torch.from_numpy(b.copy())

    ns = reference_source_objects('eval.py', ['compute_overlap', '_compute_ap', '_get_detections', '_get_annotations', 'evaluate'],
                                  {'np': np, 'torch': torch})
    recorded = []
    inner = ns['_compute_ap']

    def recording_compute_ap(recall, precision):
        recorded.append((np.array(recall, dtype=np.float64), np.array(precision, dtype=np.float64)))
        return inner(recall, precision)
    ns['_compute_ap'] = recording_compute_ap
    all_det = ns['_get_detections'](DS(), Model(), score_threshold=0.05, max_detections=100)
    for c in range(NC):                                                         # the documented tie rule is not exercised here
        s = np.concatenate([all_det[i][c][:, 4] for i in range(NIMG)])
        assert len(np.unique(s)) == len(s), c
    mean, aps = ns['evaluate'](DS(), Model(), iou_threshold=0.5, score_threshold=0.05, max_detections=100)
    with_gt = [c for c in range(NC) if aps[c][1] != 0]
    assert len(recorded) == len(with_gt)
    assert aps[19] == (0, 0) and 18 in with_gt and len(recorded[with_gt.index(18)][0]) == 0
    assert max(sum(len(all_det[i][c]) for c in range(NC)) for i in range(NIMG)) == 100
    d = {'num_classes': NC, 'iou_threshold': 0.5, 'score_threshold': 0.05, 'max_detections': 100,
         'scales': np.array([im[0] for im in images], dtype=np.float64), 'mean_ap': np.float64(mean),
         'ap': np.array([aps[c][0] for c in range(NC)], dtype=np.float64),
         'num_annotations': np.array([aps[c][1] for c in range(NC)], dtype=np.float64),
         'curve_classes': np.array(with_gt, dtype=np.int64)}
    for i, (_, s, l, b, gt) in enumerate(images):
        d[f'in{i}_scores'], d[f'in{i}_labels'], d[f'in{i}_boxes'], d[f'gt{i}'] = s, l, b, gt
    for c, (r, p) in zip(with_gt, recorded):
        d[f'recall{c}'], d[f'precision{c}'] = r, p
    np.savez_compressed(OUT, **d)
    print('\nvoc_map: mean AP %.6f, %d kept detections, %d GT rows, %d bytes' % (
        mean, sum(len(all_det[i][c]) for i in range(NIMG) for c in range(NC)), int(d['num_annotations'].sum()), os.path.getsize(OUT)))


if __name__ == '__main__':
    main()
