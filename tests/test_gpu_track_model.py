"""evaluate.TrackedDetector on a real detector: D0 at 128 x 128, B = 2, the seeded weights of the separated-detections fixture
(tests/golden/d0_128_dets_separated.npz: 18 detections per image, scores 0.93-0.95, kept boxes overlapping by at most the NMS limit)."""
import os

import numpy as np
import pytest
import torch

from oracle import effdet_oracle as O

pytestmark = pytest.mark.gpu
_SHARED = {}


def _setup(golden_dir):
    """(model, images, the three frames of one TrackedDetector on the same batch, detect() before and after), built once and shared"""
    if not _SHARED:
        from efficientdet.pytorch_amd import EfficientDet, EFFICIENTDET, evaluate
        g = np.load(os.path.join(golden_dir, 'd0_128_dets_separated.npz'), allow_pickle=False)
        net, nc = str(g['network']), int(g['num_classes'])
        c = EFFICIENTDET[net]
        sd = O.golden_state_dict(g)
        sd['bbox_head.retina_cls.weight'] = sd['bbox_head.retina_cls.weight'] * float(g['gain'])
        m = EfficientDet(nc, network=net, W_bifpn=c['W_bifpn'], D_bifpn=c['D_bifpn'], D_class=c['D_class'], is_training=False,
                         threshold=float(g['threshold']), compute_dtype=torch.float32, f32_arith='f32')
        m.load_state_dict(sd); m = m.cuda().eval()
        img, _ = O.synthetic_batch(int(g['B']), int(g['S']), seed=1, num_classes=nc)
        img = img.cuda()
        before = m.detect(img)
        tracker = evaluate.TrackedDetector(m)
        frames = [tuple(t.clone() for t in tracker.update(img)) for _ in range(3)]
        after = m.detect(img)
        _SHARED.update(m=m, img=img, tracker=tracker, frames=frames, before=before, after=after, B=int(g['B']))
    return _SHARED


def test_three_frames_of_the_same_batch(golden_dir):
    s = _setup(golden_dir)
    assert s['B'] == 2 and tuple(s['img'].shape[2:]) == (128, 128)
    o = s['tracker'].options
    dets, counts = s['tracker'].detections_device(s['img'])
    rows, ids, count = s['frames'][0]
    for b in range(2):
        n = int(counts[b])
        start = [r for r in range(n) if float(dets[b, r, 4]) >= o.new_thr]
        assert len(start) == n >= 5 and int(count[b]) == n                          # every row of the fixture scores above new_thr
        assert ids[b, :n].tolist() == list(range(1, n + 1))                         # ids 1..n in row order
        assert torch.equal(rows[b, :n, 4:6], dets[b, :n, 4:6]) and torch.allclose(rows[b, :n, :4], dets[b, :n, :4], atol=1e-4, rtol=0)
        assert not rows[b, n:].any() and bool((ids[b, n:] == -1).all())
    for f in (1, 2):                                                               # zero innovation: the same ids and box bits
        r, i, c = s['frames'][f]
        assert torch.equal(i, ids) and torch.equal(c, count) and torch.equal(r[:, :, :6], rows[:, :, :6])
        for b in range(2):
            n = int(count[b])
            assert r[b, :n, 6].tolist() == [float(f)] * n and r[b, :n, 7].tolist() == [float(f)] * n


def test_update_is_track_step_on_finalize_device(golden_dir):
    from efficientdet.pytorch_amd import evaluate, ops
    s = _setup(golden_dir)
    img, m = s['img'], s['m']
    with torch.no_grad():
        sc, lb, bx, cnt = ops.model_detections(m, img, 128, 128)
    dets, counts = evaluate.finalize_device(sc, lb, bx, cnt, [1.0, 1.0], s['tracker'].options.low_thr, 100)
    state = ops.track_state(2, s['tracker'].options.max_tracks, 'cuda')
    for f in range(3):
        out = ops.track_step(dets, counts, state, s['tracker'].options)
        assert all(torch.equal(a, b) for a, b in zip(out, s['frames'][f])), f
    assert torch.equal(state.buf, s['tracker'].state.buf)


def test_the_wrapper_leaves_detect_alone(golden_dir):
    s = _setup(golden_dir)
    assert len(s['before']) == len(s['after']) == 2
    for a, b in zip(s['before'], s['after']):
        assert all(torch.equal(x, y) for x, y in zip(a, b)) and len(a[0]) >= 5


def test_reset_restarts_only_the_listed_stream_and_tracks_reads_back(golden_dir):
    from efficientdet.pytorch_amd import evaluate
    s = _setup(golden_dir)
    t = evaluate.TrackedDetector(s['m'])
    first = t.tracks(s['img'])
    t.update(s['img'])
    t.reset((1,))
    rows, ids, count = t.update(s['img'])
    ref = s['frames']
    assert torch.equal(rows[0], ref[2][0][0]) and torch.equal(ids[0], ref[2][1][0])        # stream 0: its third frame
    assert torch.equal(rows[1], ref[0][0][1]) and torch.equal(ids[1], ref[0][1][1])        # stream 1: a first frame again
    assert torch.equal(count, ref[0][2])
    for b, (i, sc, lb, bx) in enumerate(first):
        n = int(ref[0][2][b])
        assert i.dtype == lb.dtype == torch.int64 and i.tolist() == list(range(1, n + 1)) and tuple(bx.shape) == (n, 4)
        assert torch.equal(sc, ref[0][0][b, :n, 4]) and torch.equal(lb, s['before'][b][1][:n])
    with pytest.raises(ValueError):
        t.update(s['img'][:1])                                                     # another batch size
    with pytest.raises(ValueError):
        t.reset((2,))
    t.reset()
    assert all(torch.equal(a, b) for a, b in zip(t.update(s['img']), ref[0]))


def test_the_wrapper_takes_an_ensemble(golden_dir):
    from efficientdet.pytorch_amd import evaluate
    s = _setup(golden_dir)
    ens = evaluate.EnsembleDetector([s['m'], s['m']])
    t = evaluate.TrackedDetector(ens, max_detections=64)
    rows, ids, count = t.update(s['img'])
    dets, counts = t.detections_device(s['img'])
    for b in range(2):
        n = int(count[b])
        fresh = int((dets[b, :int(counts[b]), 4] >= t.options.new_thr).sum())
        assert n == fresh >= 1 and ids[b, :n].tolist() == list(range(1, n + 1)) and tuple(rows.shape) == (2, 128, 8)
    r2, i2, c2 = t.update(s['img'])
    assert torch.equal(i2, ids) and torch.equal(c2, count) and torch.equal(r2[:, :, :6], rows[:, :, :6])


def test_update_captured_by_the_caller_replays_the_eager_frames(golden_dir):
    """TrackedDetector.update captured in a torch.cuda.graph by the class docstring's recipe (two warm-up updates on a side stream,
    reset, capture over a static image buffer) and replayed over three different frames: outputs and final state bit-equal to a fresh
    eager tracker on the same frames."""
    from efficientdet.pytorch_amd import evaluate
    s = _setup(golden_dir)
    img = s['img']
    seq = [img, img.flip(3).contiguous(), img]
    eager = evaluate.TrackedDetector(s['m'])
    want = [tuple(t.clone() for t in eager.update(f)) for f in seq]
    assert not torch.equal(want[0][0], want[1][0])                                 # the middle frame does change the tracks
    tracker = evaluate.TrackedDetector(s['m'])
    static = torch.zeros_like(img)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        tracker.update(static); tracker.update(static)
    torch.cuda.current_stream().wait_stream(side)
    tracker.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = tracker.update(static)
    for f, frame in enumerate(seq):
        static.copy_(frame)
        graph.replay()
        assert all(torch.equal(a, b) for a, b in zip(out, want[f])), f
    assert torch.equal(tracker.state.buf, eager.state.buf)
    assert all(torch.equal(x, y) for a, b in zip(s['before'], s['m'].detect(img)) for x, y in zip(a, b))
