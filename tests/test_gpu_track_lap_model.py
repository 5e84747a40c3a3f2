"""evaluate.TrackedDetector with TrackOptions(assignment='optimal') on a real detector: D0 at 128 x 128, B = 2, the seeded weights of the
separated-detections fixture (tests/golden/d0_128_dets_separated.npz), as tests/test_gpu_track_model.py runs the default tracker."""
import os

import numpy as np
import pytest
import torch

from oracle import effdet_oracle as O

pytestmark = pytest.mark.gpu
_SHARED = {}


def _setup(golden_dir):
    """(model, frames of an optimal and of a default TrackedDetector over three different images, detect() before and after), once"""
    if not _SHARED:
        from efficientdet.pytorch_amd import EfficientDet, EFFICIENTDET, evaluate, ops
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
        seq = [img, img.flip(3).contiguous(), img]
        before = m.detect(img)
        optimal = evaluate.TrackedDetector(m, ops.TrackOptions(assignment='optimal'))
        default = evaluate.TrackedDetector(m)
        frames = [tuple(t.clone() for t in optimal.update(f)) for f in seq]
        plain = [tuple(t.clone() for t in default.update(f)) for f in seq]
        after = m.detect(img)
        _SHARED.update(m=m, seq=seq, optimal=optimal, default=default, frames=frames, plain=plain, before=before, after=after)
    return _SHARED


def test_update_is_the_optimal_track_step_on_finalize_device(golden_dir):
    from efficientdet.pytorch_amd import evaluate, ops
    s = _setup(golden_dir)
    o = s['optimal'].options
    assert o.assignment == 'optimal' and tuple(s['seq'][0].shape) == (2, 3, 128, 128)
    state = ops.track_state(2, o.max_tracks, 'cuda')
    for f, img in enumerate(s['seq']):
        with torch.no_grad():
            sc, lb, bx, cnt = ops.model_detections(s['m'], img, 128, 128)
        dets, counts = evaluate.finalize_device(sc, lb, bx, cnt, [1.0, 1.0], o.low_thr, 100)
        out = ops.track_step(dets, counts, state, o)
        assert all(torch.equal(a, b) for a, b in zip(out, s['frames'][f])), f
        assert int(out[2].min()) >= 5
    assert torch.equal(state.buf, s['optimal'].state.buf)


def test_detect_is_untouched_and_the_default_tracker_unchanged(golden_dir):
    from efficientdet.pytorch_amd import evaluate, ops
    s = _setup(golden_dir)
    for a, b in zip(s['before'], s['after']):
        assert all(torch.equal(x, y) for x, y in zip(a, b)) and len(a[0]) >= 5
    d = s['default'].options
    assert d.assignment == 'greedy' and d == ops.TrackOptions() and len(d.key()) == 10
    state = ops.track_state(2, d.max_tracks, 'cuda')                                # the default wrapper is track_step without the option
    named = evaluate.TrackedDetector(s['m'], ops.TrackOptions(assignment='greedy'))
    for f, img in enumerate(s['seq']):
        dets, counts = s['default'].detections_device(img)
        assert all(torch.equal(a, b) for a, b in zip(ops.track_step(dets, counts, state), s['plain'][f])), f
        assert all(torch.equal(a, b) for a, b in zip(named.update(img), s['plain'][f])), f
    assert torch.equal(state.buf, s['default'].state.buf) and torch.equal(named.state.buf, s['default'].state.buf)
