"""Time evaluate.OperatingPoint.compute() next to evaluate.VOCMeanAP.compute() on the same records, in one process: by default 5 000
images x 100 detection slots, 80 classes, the default grid of 1 001 thresholds.  Both times span the call (launches, the device work and
the read-back of the tables each returns), host clock between device synchronisations, median of --reps.  Prints one JSON line.

  python tools/op_point_bench.py
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=5000)
    ap.add_argument('--classes', type=int, default=80)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--reps', type=int, default=5)
    a = ap.parse_args()
    import torch
    from voc_map_bench import synthetic
    from efficientdet.pytorch_amd.evaluate import OperatingPoint, VOCMeanAP
    assert torch.cuda.is_available(), 'the device metrics need a GPU'
    dets, counts, gts = synthetic(a.images, a.classes)
    dd, cd = torch.from_numpy(dets).cuda(), torch.from_numpy(counts).cuda()
    voc, op = VOCMeanAP(a.classes), OperatingPoint(a.classes)
    t0 = time.perf_counter()
    for i in range(0, a.images, a.batch):
        voc.add(dd[i:i + a.batch], cd[i:i + a.batch], gts[i:i + a.batch])
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    for i in range(0, a.images, a.batch):
        op.add(dd[i:i + a.batch], cd[i:i + a.batch], gts[i:i + a.batch])
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    times = {'voc': [], 'op': []}
    for rep in range(a.reps + 1):                                  # rep 0: warm-up
        for name, meter in (('voc', voc), ('op', op)):
            torch.cuda.synchronize()
            t = time.perf_counter()
            out = meter.compute()
            torch.cuda.synchronize()
            if rep:
                times[name].append((time.perf_counter() - t) * 1e3)
    assert out['mean_ap'] == voc.compute()[0]
    print(json.dumps({'what': 'operating point vs VOC metric', 'images': a.images, 'classes': a.classes, 'records': op.num_records,
                      'thresholds': int(len(op.thresholds)),
                      'voc_compute_ms': round(float(np.median(times['voc'])), 4), 'op_compute_ms': round(float(np.median(times['op'])), 4),
                      'voc_add_ms_per_batch_of_%d' % a.batch: round((t1 - t0) * 1e3 / ((a.images + a.batch - 1) // a.batch), 4),
                      'op_add_ms_per_batch_of_%d' % a.batch: round((t2 - t1) * 1e3 / ((a.images + a.batch - 1) // a.batch), 4),
                      'overall': [float(v) for v in out['overall']], 'mean_ap': float(out['mean_ap'])}))


if __name__ == '__main__':
    main()
