"""GPU parity of the Mosaic / MixUp stage (csrc/mosaic.hip, ops.mosaic_compose / ops.mosaic_boxes, DeviceAugmentation(mosaic=...))
with the NumPy restatement tests/mosaic_restated.py on the cases of tests/mosaic_cases.py: every canvas byte equal, the kept boxes the
same rows in the same order with coordinates within 1e-4 px (the chain's bound), and the chain behind the stage bit for bit what
tests/augment_restated.py gives on the restated canvases."""
import os

import numpy as np
import pytest
import torch

from efficientdet.pytorch_amd import data as D
from efficientdet.pytorch_amd import ops
from tests import augment_restated as A
from tests import mosaic_restated as R
from tests.mosaic_cases import CASES, _row

pytestmark = pytest.mark.gpu
BY_NAME = {c['name']: c for c in CASES}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'jpeg_cases.npz')


def _upload(imgs):
    """The uint8 source layout of the chain: (src, src_off [B] int64, src_hw [B, 2] int32) on the device, images 16-byte aligned."""
    offs = np.concatenate([[0], np.cumsum([(im.size + 15) // 16 * 16 for im in imgs])]).astype(np.int64)
    buf = np.zeros(int(offs[-1]), dtype=np.uint8)
    for im, o in zip(imgs, offs[:-1]):
        buf[o:o + im.size] = im.reshape(-1)
    hw = np.array([im.shape[:2] for im in imgs], dtype=np.int32)
    return torch.from_numpy(buf).cuda(), torch.from_numpy(offs[:-1].copy()).cuda(), torch.from_numpy(hw).cuda()


def _restated(c):
    if 'want' not in c:                                                # computed once per case, shared, never changed
        hws = [im.shape[:2] for im in c['imgs']]
        c['want'] = ([R.compose(c['imgs'], row, c['S'], c['fill'], b) for b, row in enumerate(c['table'])],
                     [R.boxes(c['annots'], hws, row, c['S'], c['min_area'], c['min_visibility'], b) for b, row in enumerate(c['table'])])
    return c['want']


def _check_rows(got_all, want, b, bound=1e-4):
    got = got_all[got_all[:, 4] != -1]
    assert (got_all[len(got):] == -1).all(), ('-1 rows follow the kept ones', b)
    assert len(got) == len(want) and got[:, 4].tolist() == want[:, 4].tolist(), (b, len(got), len(want))
    err = float(np.abs(got[:, :4] - want[:, :4]).max(initial=0))
    assert err <= bound, (b, err)
    return err


@pytest.mark.parametrize('name', [c['name'] for c in CASES])
def test_compose_equals_the_restatement(name):
    c = BY_NAME[name]
    src, off, hw = _upload(c['imgs'])
    out = ops.mosaic_compose(src, off, hw, torch.from_numpy(c['table']).cuda(), c['S'], c['fill'])
    assert out.dtype == torch.uint8 and tuple(out.shape) == (len(c['imgs']), c['S'], c['S'], 3)
    got = out.cpu().numpy()
    for b, want in enumerate(_restated(c)[0]):
        diff = got[b] != want
        assert not diff.any(), (name, b, int(diff.sum()), np.argwhere(diff)[:4].tolist())


@pytest.mark.parametrize('name', [c['name'] for c in CASES])
def test_boxes_equal_the_restatement(name):
    c = BY_NAME[name]
    B, M = c['annots'].shape[:2]
    _, _, hw = _upload(c['imgs'])
    out, counts = ops.mosaic_boxes(hw, torch.from_numpy(c['table']).cuda(), c['S'], torch.from_numpy(c['annots']).cuda(), c['min_area'],
                                   c['min_visibility'])
    assert tuple(out.shape) == (B, 5 * M, 5) and counts.dtype == torch.int32
    out, counts = out.cpu().numpy(), counts.cpu().numpy()
    worst = 0.0
    for b, want in enumerate(_restated(c)[1]):
        assert counts[b] == len(want), (name, b, int(counts[b]), len(want))
        worst = max(worst, _check_rows(out[b], want, b))
    print('%s: counts %s, largest coordinate error %.3g px' % (name, counts.tolist(), worst))


def test_determinism():
    c = BY_NAME['many_boxes']
    src, off, hw = _upload(c['imgs'])
    t, ann = torch.from_numpy(c['table']).cuda(), torch.from_numpy(c['annots']).cuda()
    a, b = (ops.mosaic_compose(src, off, hw, t, c['S'], c['fill']) for _ in range(2))
    assert torch.equal(a, b)
    (o1, n1), (o2, n2) = (ops.mosaic_boxes(hw, t, c['S'], ann, c['min_area'], c['min_visibility']) for _ in range(2))
    assert torch.equal(o1, o2) and torch.equal(n1, n2)


# ------------------------------------------------------------------------------------------------ through DeviceAugmentation
def _aug_row(**kw):
    r = np.zeros(len(D.AUG_COLUMNS), dtype=np.float32)
    for k, v in kw.items():
        r[D.AUG[k]] = v
    return r


AUG_ROWS = [_aug_row(rrc=1, crop_y=5, crop_x=11, crop_h=40, crop_w=33, flip=1, flip_code=-1, clahe=1, clip_limit=2.5),
            _aug_row(transpose=1, color=1, alpha=1.2, beta=-0.1, hflip=1),
            _aug_row(shift=2, hue_shift=-3.5, sat_shift=2.5, val_shift=9, vflip=1, flip=1, flip_code=1)]
MOSAIC_ROWS = [_row(cx=30, cy=35, src=(0, 1, 2, 1), side=(40, 64, 30, 50), mix=1, mix_src=1, lam=0.3),
               _row(on=0),
               _row(cx=40, cy=21, src=(2, 0, 0, 1), side=(21, 45, 64, 33))]


def _samples(c):
    return [{'img': im, 'annot': a[a[:, 4] != -1]} for im, a in zip(c['imgs'], c['annots'])]


def _final(images):
    return images.map.tensor()[..., :3].cpu()


def test_the_chain_runs_on_the_mosaic_as_on_dataset_images():
    c = BY_NAME['mixup_lam_0.3']
    S, samples = 64, _samples(c)
    mt, at = np.stack(MOSAIC_ROWS), np.stack(AUG_ROWS)
    opts = D.MosaicOptions(fill=99)
    aug = D.DeviceAugmentation(phase='train', width=S, height=S, dtype=torch.float32, min_area=3.0, min_visibility=0.2, mosaic=opts)
    stages = {}
    images, ann, params = aug(samples, table=at, stages=stages, mosaic_table=mt)
    torch.cuda.synchronize()
    hws = [im.shape[:2] for im in c['imgs']]
    assert torch.equal(stages['mosaic_table'].cpu(), torch.from_numpy(mt)) and torch.equal(params.cpu(), torch.from_numpy(at))
    got_m, got = stages['mosaic'].cpu().numpy(), _final(images)
    assert got_m.shape == (3, S, S, 3) and got_m.dtype == np.uint8
    kept = []
    for b in range(3):
        want_m = R.compose(c['imgs'], mt[b], S, 99, b)
        assert np.array_equal(got_m[b], want_m), ('mosaic', b)
        ref = A.train_stages(want_m, at[b], S)
        assert np.array_equal(stages['a'][b].cpu().numpy()[..., :3], want_m), ('the chain copies an S x S source', b)
        assert torch.equal(got[b], torch.from_numpy(ref['out'])), ('out', b)
        boxes_m = R.boxes(c['annots'], hws, mt[b], S, float(np.float32(3.0)), float(np.float32(0.2)), b)
        kept.append(A.boxes(boxes_m, (S, S), at[b], S, S, min_area=3.0, min_visibility=0.2))
    ann = ann.cpu().numpy()
    assert ann.shape[1] == max(1, max(len(k) for k in kept)) and sum(len(k) for k in kept) > 6
    for b in range(3):
        _check_rows(ann[b], kept[b], b)
    # trim=False keeps the 5 M rows and reads nothing back
    aug2 = D.DeviceAugmentation(phase='train', width=S, height=S, dtype=torch.float32, min_area=3.0, min_visibility=0.2, mosaic=opts, trim=False)
    images2, ann2, _ = aug2(samples, table=at, mosaic_table=torch.from_numpy(mt))
    assert ann2.shape[1] == 5 * c['annots'].shape[1] and torch.equal(_final(images2), got)
    assert np.array_equal(ann2.cpu().numpy()[:, :ann.shape[1]], ann) and (ann2.cpu().numpy()[:, ann.shape[1]:] == -1).all()
    # a table from the device, or one that fails the check, is refused before the stage runs
    with pytest.raises(ValueError, match='host'):
        aug(samples, table=at, mosaic_table=torch.from_numpy(mt).cuda())
    bad = mt.copy(); bad[2, D.MOSAIC['src1']] = 3
    with pytest.raises(ValueError, match='row 2'):
        aug(samples, table=at, mosaic_table=bad)


def test_all_rows_off_is_the_path_without_mosaic():
    c = BY_NAME['centres_at_quarters']
    S, samples = 64, _samples(c)
    at = np.stack([AUG_ROWS[b % 3] for b in range(5)])
    off = np.stack([_row(on=0)] * 5)
    # thresholds at their defaults: with others the two paths may differ by design, because the stage filters too and the chain then
    # measures a box's visibility against what the stage left of it
    kw = dict(phase='train', width=S, height=S, dtype=torch.float32)
    sa, sb = {}, {}
    ia, aa, _ = D.DeviceAugmentation(mosaic=D.MosaicOptions(), **kw)(samples, table=at, mosaic_table=off, stages=sa)
    ib, ab, _ = D.DeviceAugmentation(mosaic=None, **kw)(samples, table=at, stages=sb)
    assert torch.equal(ia.map.tensor(), ib.map.tensor()) and torch.equal(sa['a'], sb['a']) and torch.equal(sa['b'], sb['b'])
    assert torch.equal(sa['mosaic'], sb['a'][..., :3])
    aa, ab = aa.cpu().numpy(), ab.cpu().numpy()
    assert aa.shape == ab.shape and (ab[..., 4] != -1).sum() > 5
    for b in range(5):
        _check_rows(aa[b], ab[b][ab[b][:, 4] != -1], b)


def test_without_the_option_nothing_new_is_called(monkeypatch):
    calls = {'compose': 0, 'boxes': 0}
    real = (ops.mosaic_compose, ops.mosaic_boxes)

    def compose(*a, **k):
        calls['compose'] += 1
        return real[0](*a, **k)

    def boxes(*a, **k):
        calls['boxes'] += 1
        return real[1](*a, **k)
    monkeypatch.setattr(ops, 'mosaic_compose', compose)
    monkeypatch.setattr(ops, 'mosaic_boxes', boxes)
    c = BY_NAME['mixup_lam_0.3']
    S, samples = 64, _samples(c)
    aug = D.DeviceAugmentation(phase='train', width=S, height=S, dtype=torch.float32, seed=5, mosaic=D.MosaicOptions(mixup_p=0.5))
    aug.mosaic = None                                                  # the plain attribute: the last epochs of a schedule
    stages = {}
    images, ann, params = aug(samples, stages=stages)
    assert calls == {'compose': 0, 'boxes': 0} and 'mosaic' not in stages
    # the seed draws what it drew before the option existed, and the output is the chain's own
    table = D.sample_augment_table(np.random.RandomState(5), 3, S)
    assert np.array_equal(params.cpu().numpy(), table)
    for b, s in enumerate(samples):
        assert torch.equal(_final(images)[b], torch.from_numpy(A.train_stages(s['img'], table[b], S)['out'])), b
        _check_rows(ann.cpu().numpy()[b], A.boxes(s['annot'], s['img'].shape[:2], table[b], S, S), b)
    aug.mosaic = D.MosaicOptions(mixup_p=0.5)
    stages = {}
    aug(samples, stages=stages)
    assert calls == {'compose': 1, 'boxes': 1} and tuple(stages['mosaic'].shape) == (3, S, S, 3)
    assert tuple(stages['mosaic_table'].shape) == (3, len(D.MOSAIC_COLUMNS))


def test_jpeg_samples_give_the_same_mosaic():
    g = np.load(GOLDEN)
    ns = [str(n) for n in g['names']]
    ns = [ns[i] for i in np.random.RandomState(2).permutation(len(ns))[:4]]
    ann = np.array([[0, 0, 1, 1, 0]], dtype=np.float32)
    S = 64
    hw = np.array([g[n + '/rgb'].shape[:2] for n in ns])
    mt = np.stack([_row(cx=20, cy=40, src=(0, 1, 2, 3), side=(64, 33, 48, 64), mix=1, mix_src=3, lam=0.6), _row(on=0),
                   _row(cx=48, cy=16, src=(3, 2, 1, 0), side=(50, 64, 64, 40)), _row(cx=32, cy=32, src=(3, 3, 0, 1), side=(64, 64, 64, 64))])
    D.check_mosaic_table(mt, 4, S, hw)
    at = np.stack([AUG_ROWS[b % 3] for b in range(4)])
    outs = []
    for key in ('jpeg', 'img'):
        samples = [{key: g[n + '/jpg'].tobytes() if key == 'jpeg' else g[n + '/rgb'], 'annot': ann} for n in ns]
        stages = {}
        images, boxes, _ = D.DeviceAugmentation(phase='train', width=S, height=S, dtype=torch.float32, mosaic=D.MosaicOptions())(
            samples, table=at, stages=stages, mosaic_table=mt)
        outs.append((stages['mosaic'].clone(), images.map.tensor().clone(), boxes.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    for b in range(4):
        assert np.array_equal(outs[0][0][b].cpu().numpy(), R.compose([g[n + '/rgb'] for n in ns], mt[b], S, 114, b)), b


def test_a_mosaic_batch_with_padding_rows_trains():
    """D0 at 128 x 128, B = 2: the 5 M-row annotations of trim=False, -1 rows included, give the losses of the same tensors trimmed."""
    from efficientdet.pytorch_amd import EfficientDet, EFFICIENTDET
    from oracle import effdet_oracle as O
    net, nc = 'efficientdet-d0', 20
    cfg = EFFICIENTDET[net]
    m = EfficientDet(nc, network=net, W_bifpn=cfg['W_bifpn'], D_bifpn=cfg['D_bifpn'], D_class=cfg['D_class'], compute_dtype=torch.float32)
    m.load_state_dict(O.make_state_dict(net, nc, seed=0)); m.backbone.drop_connect_rate = 0.0
    m = m.cuda(); m.train(); m.is_training = True; m.freeze_bn()
    rng = np.random.RandomState(9)
    samples = []
    for h, w in ((200, 150), (90, 300)):
        x1, y1 = rng.uniform(0, w * 0.6, 4), rng.uniform(0, h * 0.6, 4)
        samples.append({'img': rng.randint(0, 256, (h, w, 3)).astype(np.uint8),
                        'annot': np.stack([x1, y1, x1 + rng.uniform(20, w * 0.4, 4), y1 + rng.uniform(20, h * 0.4, 4), rng.randint(0, nc, 4)], 1).astype(np.float32)})
    aug = D.DeviceAugmentation(phase='train', width=128, height=128, dtype=torch.float32, seed=1, trim=False,
                               mosaic=D.MosaicOptions(mixup_p=1.0))
    images, ann, _ = aug(samples)
    assert ann.shape[1] == 20
    n = int((ann[..., 4] != -1).sum(1).max())
    assert 0 < n < 20 and bool((ann[:, n:] == -1).all())
    cl, rl = m([images, ann])
    cl2, rl2 = m([images, ann[:, :n].contiguous()])
    torch.cuda.synchronize()
    print('losses %r %r, trimmed %r %r' % (float(cl.detach()), float(rl.detach()), float(cl2.detach()), float(rl2.detach())))
    assert bool(torch.isfinite(cl).all()) and bool(torch.isfinite(rl).all())
    assert torch.equal(cl, cl2) and torch.equal(rl, rl2)
