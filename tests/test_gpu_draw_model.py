"""evaluate.Annotator behind a real detector: D0 at 128 x 128, B = 2 (the seeded weights of tests/golden/d0_128_dets_separated.npz, 18
detections per image), two TrackedDetector updates, then the tracks painted into uint8 frames of 96 x 160 with a box_scale -- the
painted frames equal the restatement (tests/draw_restated.py) run on the read-back rows; the same through finalize_device's rows."""
import os

import numpy as np
import pytest
import torch

from oracle import effdet_oracle as O
from tests import draw_restated as R

pytestmark = pytest.mark.gpu
_SHARED = {}
H, W = 96, 160
NAMES = ['class%d' % i for i in range(12)]                                          # fewer names than classes: the rest print as numbers


def _setup(golden_dir):
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
        tracker = evaluate.TrackedDetector(m)
        tracker.update(img)
        tracks = tracker.update(img)
        dets = tracker.detections_device(img)
        frames = torch.from_numpy(np.random.RandomState(5).randint(0, 256, (img.shape[0], H, W, 3)).astype(np.uint8)).cuda()
        scale = torch.tensor([[W / 128.0, H / 128.0]] * img.shape[0], dtype=torch.float32, device=img.device)
        _SHARED.update(tracks=tracks, dets=dets, frames=frames, scale=scale, S=int(g['S']))
    return _SHARED


def _restate(frames, rows, counts, ids, scale, palette, options):
    f, r, n, s = frames.cpu().numpy(), rows.cpu().numpy(), counts.cpu().numpy(), scale.cpu().numpy()
    i = None if ids is None else ids.cpu().numpy()
    names = [x.encode() for x in NAMES]
    return np.stack([R.paint(f[b].copy(), r[b], n[b], None if i is None else i[b], s[b], names, palette, **dict(zip(
        ('thickness', 'fill_alpha', 'label', 'show_score', 'show_id', 'text_scale', 'color_by'), options.key()))) for b in range(len(f))])


def test_tracks_painted_by_the_annotator(golden_dir):
    from efficientdet.pytorch_amd import evaluate, ops
    s = _setup(golden_dir)
    rows, ids, count = s['tracks']
    assert s['S'] == 128 and tuple(rows.shape[2:]) == (8,) and int(count.min()) >= 5
    o = ops.DrawOptions(thickness=2, fill_alpha=64, show_id=True, text_scale=1, color_by='id')
    annotator = evaluate.Annotator(NAMES, o)
    keep = s['frames'].clone()
    out = annotator(s['frames'], rows, count, ids, s['scale'])
    assert out is not s['frames'] and torch.equal(s['frames'], keep)
    want = _restate(keep, rows, count, ids, s['scale'], ops.draw_palette_host(64), o)
    assert np.array_equal(out.cpu().numpy(), want) and not np.array_equal(want, keep.cpu().numpy())
    again = annotator(s['frames'].clone(), rows, count, ids, s['scale'], inplace=True)
    assert torch.equal(again, out)


def test_detections_painted_without_ids(golden_dir):
    from efficientdet.pytorch_amd import evaluate, ops
    s = _setup(golden_dir)
    dets, counts = s['dets']
    assert tuple(dets.shape[2:]) == (6,) and int(counts.min()) >= 5
    pal = np.array([[10, 20, 30], [240, 230, 50], [0, 200, 0]], dtype=np.uint8)
    annotator = evaluate.Annotator(NAMES, palette=pal)                              # the default options
    out = annotator(s['frames'], dets, counts, box_scale=s['scale'])
    want = _restate(s['frames'], dets, counts, None, s['scale'], pal, ops.DrawOptions())
    assert np.array_equal(out.cpu().numpy(), want)
    with pytest.raises(ValueError):
        evaluate.Annotator(NAMES, ops.DrawOptions(show_id=True))(s['frames'], dets, counts)
