"""Time the JPEG decode path (data.decode_jpeg_batch) on a batch of 32 streams.  Not an acceptance gate; bench.py is untouched.

  python tools/jpeg_bench.py [--dir DIR_OF_JPG] [--batch 32] [--reps 30] [--out FILE] [--no-profile]

The batch: the .jpg files of --dir; else, when Pillow imports, 500 x 375 4:2:0 streams built at run time by tiling the PIXELS of the
golden 33 x 47 cases (tests/golden/jpeg_cases.npz) and re-encoding them; else the golden streams themselves, repeated (a toy size:
that line measures overheads and says so).  One JSON line per measurement, each with median / min / max over --reps repetitions
after warm-up:

  host_entropy     effdet_jpeg_entropy_batch alone (host, no GPU) at threads = 1, 8, 16, ms per batch;
  kernels          the two kernels' times from `rocprofv3 --kernel-trace --stats` over a child process of their own that runs
                   ops.jpeg_reconstruct on pre-uploaded coefficients (us per launch; skipped when rocprofv3 is not on PATH);
  end_to_end       decode_jpeg_batch from bytes to pixels on the device, host clock around a device synchronise, images / s;
  pillow           Image.open().convert('RGB') over the same streams on a pool of the same thread count (when Pillow imports).
"""
import argparse
import concurrent.futures as cf
import csv
import glob
import io
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'jpeg_cases.npz')
KERNELS = ('jpeg_idct_kernel', 'jpeg_rgb_kernel')


def make_streams(directory, batch):
    """-> (list of bytes, description of where they came from)."""
    if directory:
        files = sorted(glob.glob(os.path.join(directory, '*.jpg')) + glob.glob(os.path.join(directory, '*.jpeg')))
        if not files:
            raise SystemExit('no .jpg files in %s' % directory)
        return [open(files[i % len(files)], 'rb').read() for i in range(batch)], 'files of %s' % directory
    g = np.load(GOLDEN)
    try:
        from PIL import Image
    except ImportError:
        names = [str(n) for n in g['names'] if str(n).startswith('33x47')]
        return [g[names[i % len(names)] + '/jpg'].tobytes() for i in range(batch)], 'golden 33x47 streams repeated (toy size: overheads only)'
    tiles = [g[str(n) + '/rgb'] for n in g['names'] if str(n).startswith('33x47')]
    out = []
    for i in range(batch):
        t = tiles[i % len(tiles)]
        img = np.roll(np.tile(t, (375 // t.shape[0] + 1, 500 // t.shape[1] + 1, 1))[:375, :500], i, axis=1)
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(img)).save(buf, 'JPEG', quality=85, subsampling=2, progressive=False)
        out.append(buf.getvalue())
    return out, '500x375 4:2:0 q85, golden 33x47 pixels tiled and re-encoded'


def stats(xs):
    return {'median': round(float(np.median(xs)), 4), 'min': round(float(np.min(xs)), 4), 'max': round(float(np.max(xs)), 4), 'reps': len(xs)}


def host_stage(streams):
    from efficientdet.pytorch_amd import ops
    infos = [ops.jpeg_probe(s)[1] for s in streams]
    off = np.concatenate([[0], np.cumsum([i.coef_bytes for i in infos])]).astype(np.int64)
    coef = np.zeros(int(off[-1]), dtype=np.uint8)
    desc = np.zeros(len(streams) * ops.JPEG_DESC_BYTES, dtype=np.uint8)
    return infos, off, coef, desc


def time_host_entropy(streams, reps, emit):
    from efficientdet.pytorch_amd import ops
    _, off, coef, desc = host_stage(streams)
    for threads in (1, 8, 16):
        ms = []
        for r in range(reps + 3):
            t0 = time.perf_counter()
            status, _ = ops.jpeg_entropy_batch(streams, coef, off[:-1], desc, threads)
            if r >= 3:
                ms.append((time.perf_counter() - t0) * 1e3)
            assert status == 0
        emit({'measure': 'host_entropy', 'threads': threads, 'ms_per_batch': stats(ms)})


def reconstruct_loop(streams, iters):
    """The child under rocprofv3: only ops.jpeg_reconstruct launches, coefficients uploaded once."""
    import torch
    from efficientdet.pytorch_amd import ops
    infos, off, coef, desc = host_stage(streams)
    status, wgs = ops.jpeg_entropy_batch(streams, coef, off[:-1], desc, 8)
    assert status == 0
    sizes = np.array([(i.width * i.height * 3 + 15) // 16 * 16 for i in infos], dtype=np.int64)
    dst_off = np.concatenate([[0], np.cumsum(sizes)])
    dev = 'cuda'
    args = (torch.from_numpy(coef).to(dev), torch.from_numpy(desc).to(dev), len(streams), wgs,
            torch.empty(int(off[-1]) // 2, dtype=torch.uint8, device=dev), torch.from_numpy(off[:-1] // 2).to(dev),
            torch.empty(int(dst_off[-1]), dtype=torch.uint8, device=dev), torch.from_numpy(dst_off[:-1].copy()).to(dev))
    for _ in range(iters):
        ops.jpeg_reconstruct(*args)
    torch.cuda.synchronize()


def profile_kernels(argv, iters, out_dir, emit):
    if shutil.which('rocprofv3') is None:
        emit({'measure': 'kernels', 'skipped': 'rocprofv3 not on PATH'})
        return
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '-d', out_dir, '-o', 'jpeg', '--output-format', 'csv', '--',
           sys.executable, os.path.abspath(__file__), '--child', '--iters', str(iters)] + argv
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    files = glob.glob(os.path.join(out_dir, '**', '*kernel_stats.csv'), recursive=True)
    if r.returncode != 0 or not files:
        emit({'measure': 'kernels', 'failed': (r.stderr or r.stdout)[-400:]})
        return
    for row in csv.DictReader(open(files[0])):
        for k in KERNELS:
            if k in row['Name']:
                emit({'measure': 'kernels', 'kernel': k, 'calls': int(row['Calls']), 'average_us': round(float(row['AverageNs']) / 1e3, 2),
                      'min_us': round(float(row['MinNs']) / 1e3, 2), 'max_us': round(float(row['MaxNs']) / 1e3, 2)})


def time_end_to_end(streams, reps, threads, emit):
    import torch
    from efficientdet.pytorch_amd import data as D
    sec = []
    for r in range(reps + 5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        D.decode_jpeg_batch(streams, 'cuda', threads=threads)
        torch.cuda.synchronize()
        if r >= 5:
            sec.append(time.perf_counter() - t0)
    emit({'measure': 'end_to_end', 'threads': threads, 'ms_per_batch': stats(np.array(sec) * 1e3),
          'images_per_s_median': round(len(streams) / float(np.median(sec)), 1)})


def time_pillow(streams, reps, threads, emit):
    try:
        from PIL import Image
    except ImportError:
        emit({'measure': 'pillow', 'skipped': 'Pillow does not import'})
        return
    def one(s):
        return np.asarray(Image.open(io.BytesIO(s)).convert('RGB'))
    sec = []
    with cf.ThreadPoolExecutor(max_workers=threads) as ex:
        for r in range(reps + 3):
            t0 = time.perf_counter()
            list(ex.map(one, streams))
            if r >= 3:
                sec.append(time.perf_counter() - t0)
    emit({'measure': 'pillow', 'threads': threads, 'ms_per_batch': stats(np.array(sec) * 1e3),
          'images_per_s_median': round(len(streams) / float(np.median(sec)), 1)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dir', default=None)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--iters', type=int, default=200, help='launch pairs in the profiled child')
    ap.add_argument('--threads', type=int, default=8)
    ap.add_argument('--out', default=None)
    ap.add_argument('--profile-dir', default=None, help='where rocprofv3 writes (default: a fresh temporary directory)')
    ap.add_argument('--no-profile', action='store_true')
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    a = ap.parse_args()
    from efficientdet.pytorch_amd import build
    build.build(verbose=False)
    streams, origin = make_streams(a.dir, a.batch)
    if a.child:
        reconstruct_loop(streams, a.iters)
        return
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)
    emit({'measure': 'batch', 'images': len(streams), 'source': origin, 'stream_bytes_mean': int(np.mean([len(s) for s in streams]))})
    time_host_entropy(streams, a.reps, emit)                       # host only: the GPU is not open yet ...
    if not a.no_profile:                                           # ... so the profiled child is the only process on it
        passthrough = ['--batch', str(a.batch)] + (['--dir', a.dir] if a.dir else [])
        profile_kernels(passthrough, a.iters, a.profile_dir or tempfile.mkdtemp(prefix='jpeg_rocprof_'), emit)
    time_end_to_end(streams, a.reps, a.threads, emit)
    time_pillow(streams, a.reps, a.threads, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
