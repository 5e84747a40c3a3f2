"""GPU parity of the device-side get_augumentation (csrc/augment.hip, data.DeviceAugmentation) with the NumPy restatement
tests/augment_restated.py: uint8 stages bit for bit, the fp32 output bit for bit, bf16 equal to the restatement cast, kept box
sets identical with coordinates within 1e-4 px."""
import numpy as np
import pytest
import torch

from efficientdet.pytorch_amd import data as D
from tests import augment_restated as R

pytestmark = pytest.mark.gpu


def _samples(shapes, seed, nbox=5):
    rng = np.random.RandomState(seed)
    out = []
    for h, w in shapes:
        img = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        x1 = rng.uniform(0, w * 0.8, nbox); y1 = rng.uniform(0, h * 0.8, nbox)
        x2 = np.minimum(x1 + rng.uniform(0.5, w * 0.5 + 1, nbox), w); y2 = np.minimum(y1 + rng.uniform(0.5, h * 0.5 + 1, nbox), h)
        out.append({'img': img, 'annot': np.stack([x1, y1, x2, y2, rng.randint(0, 20, nbox)], 1).astype(np.float32)})
    return out


def _row(**kw):
    r = np.zeros(len(D.AUG_COLUMNS), dtype=np.float32)
    for k, v in kw.items():
        r[D.AUG[k]] = v
    return r


def _check_pixels(images, stages, ref, dtype, train=True):
    m = images.map.tensor().cpu()
    assert (m[..., 3:].float() == 0).all()
    for b, r in enumerate(ref):
        sa = stages['a'][b].cpu().numpy()
        assert (sa[..., :3] == r['a']).all(), ('stage a', b)
        if train:
            sb = stages['b'][b].cpu().numpy()
            assert (sb[..., :3] == r['b']).all(), ('stage b', b)
            assert (sb[..., 3] == r['L']).all(), ('L', b)
        want = torch.from_numpy(r['out'])
        got = m[b, ..., :3]
        if dtype == torch.float32:
            assert torch.equal(got, want), ('out', b, float((got - want).abs().max()))
        else:
            assert torch.equal(got, want.to(torch.bfloat16)), ('out', b)


def _check_boxes(ann, samples, rows, H, W, **kw):
    ann = ann.cpu().numpy()
    for b, s in enumerate(samples):
        want = R.boxes(s['annot'], s['img'].shape[:2], None if rows is None else rows[b], H, W, **kw)
        got = ann[b][ann[b][:, 4] != -1]
        assert (ann[b][len(got):] == -1).all()
        assert got[:, 4].tolist() == want[:, 4].tolist(), (b, got, want)
        assert np.abs(got[:, :4] - want[:, :4]).max(initial=0) <= 1e-4, b
    assert ann.shape[1] == max(1, max(len(R.boxes(s['annot'], s['img'].shape[:2], None if rows is None else rows[b], H, W, **kw))
                                       for b, s in enumerate(samples)))


def _train(samples, table, S, dtype, **kw):
    aug = D.DeviceAugmentation('train', width=S, height=S, dtype=dtype, **kw)
    stages = {}
    images, ann, params = aug(samples, table=table, stages=stages)
    torch.cuda.synchronize()
    ref = [R.train_stages(s['img'], table[b], S) for b, s in enumerate(samples)]
    return images, ann, params, stages, ref


SINGLE = [_row(), _row(rrc=1, crop_y=7, crop_x=20, crop_h=61, crop_w=37), _row(flip=1, flip_code=-1), _row(flip=1, flip_code=0),
          _row(flip=1, flip_code=1), _row(transpose=1), _row(color=1, alpha=1.3, beta=-0.2), _row(color=2, gamma=0.63),
          _row(color=3), _row(shift=1, r_shift=-17.5, g_shift=9.25, b_shift=3), _row(shift=2, hue_shift=-4.5, sat_shift=3.7, val_shift=-13),
          _row(clahe=1, clip_limit=2.7), _row(hflip=1), _row(vflip=1)]


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_each_transform_alone(dtype):
    S = 100                                                                   # not a multiple of 8: CLAHE's reflect-101 tiles
    shapes = [(120, 80), (60, 150), (100, 100), (33, 47), (1, 90), (90, 1), (200, 200), (64, 64), (75, 130), (100, 61),
              (150, 150), (81, 99), (100, 7), (45, 100)]
    samples = _samples(shapes, seed=1)
    table = np.stack(SINGLE)
    images, ann, params, stages, ref = _train(samples, table, S, dtype)
    _check_pixels(images, stages, ref, dtype)
    _check_boxes(ann, samples, table, S, S)
    assert torch.equal(params.cpu(), torch.from_numpy(table))


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_train_chain_mixed_sizes(dtype):
    S = 512
    samples = _samples([(700, 300), (200, 900), (100, 140), (1, 300), (512, 512), (333, 1000), (50, 1), (640, 480)], seed=2, nbox=7)
    table = D.sample_augment_table(np.random.RandomState(5), len(samples), S)
    table[::2, D.AUG['clahe']] = 1; table[::2, D.AUG['clip_limit']] = 3.1
    table[1, D.AUG['rrc']:D.AUG['crop_w'] + 1] = (1, 100, 0, 300, 200)       # at least two crops, one that cuts boxes
    table[3, D.AUG['rrc']:D.AUG['crop_w'] + 1] = (1, 0, 256, 256, 256)
    images, ann, params, stages, ref = _train(samples, table, S, dtype)
    _check_pixels(images, stages, ref, dtype)
    _check_boxes(ann, samples, table, S, S)


def test_train_chain_filters_boxes():
    S = 128
    samples = _samples([(128, 128)] * 4, seed=3, nbox=9)
    table = np.stack([_row(rrc=1, crop_y=30, crop_x=40, crop_h=50, crop_w=60), _row(rrc=1, crop_y=0, crop_x=0, crop_h=20, crop_w=128),
                      _row(rrc=1, crop_y=100, crop_x=100, crop_h=28, crop_w=28, transpose=1), _row(hflip=1)])
    for kw in ({'min_area': 150.0}, {'min_visibility': 0.6}, {}):
        images, ann, params, stages, ref = _train(samples, table, S, torch.float32, **kw)
        _check_boxes(ann, samples, table, S, S, **kw)
    aug = D.DeviceAugmentation('train', width=S, height=S, dtype=torch.float32, trim=False)
    _, ann_full, _ = aug(samples, table=table)
    assert ann_full.shape[1] == 9 and torch.equal(ann_full[:, :ann.shape[1]], ann)


def test_d7_size_clahe_reflect_padding():
    S = 1636                                                                  # 1636 % 8 = 4: tiles of 205 over a 1640 extension
    samples = _samples([(1636, 1200), (900, 1700)], seed=4)
    table = np.stack([_row(clahe=1, clip_limit=3.5, hflip=1), _row(clahe=1, clip_limit=1.2, vflip=1, transpose=1)])
    images, ann, params, stages, ref = _train(samples, table, S, torch.float32)
    _check_pixels(images, stages, ref, torch.float32)
    for b in range(2):
        L = ref[b]['L']
        luts, th, tw = R.clahe_luts(L, table[b, D.AUG['clip_limit']])
        assert th == 205 and (stages['lut'][b].cpu().numpy().reshape(8, 8, 256) == luts).all()


@pytest.mark.parametrize('phase', ['valid', 'test'])
def test_valid_and_test_phases(phase):
    H, W = 96, 160
    samples = _samples([(300, 200), (50, 400), (96, 160), (1, 5)], seed=5)
    for dtype in (torch.float32, torch.bfloat16):
        aug = D.DeviceAugmentation(phase, width=W, height=H, dtype=dtype)
        stages = {}
        images, ann, params = aug(samples, stages=stages)
        torch.cuda.synchronize()
        assert images.shape == (4, 3, H, W)
        _check_pixels(images, stages, [R.valid_stages(s['img'], H, W) for s in samples], dtype, train=False)
        hw = np.array([s['img'].shape[:2] for s in samples], np.float64)
        assert torch.equal(params.cpu(), torch.from_numpy(np.stack([W / hw[:, 1], H / hw[:, 0]], 1).astype(np.float32)))
        if phase == 'test':
            assert ann is None
        else:
            _check_boxes(ann, samples, None, H, W)


def test_two_runs_are_bitwise_equal():
    S = 256
    samples = _samples([(300, 200), (120, 500), (256, 256), (77, 3)], seed=6)
    table = D.sample_augment_table(np.random.RandomState(9), 4, S)
    table[:, D.AUG['clahe']] = 1; table[:, D.AUG['clip_limit']] = 2.0
    outs = []
    for _ in range(2):
        aug = D.DeviceAugmentation('train', width=S, height=S, dtype=torch.bfloat16)
        images, ann, _ = aug(samples, table=torch.from_numpy(table).cuda())
        outs.append((images.map.tensor().clone(), ann.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    # the seeded sampler: same seed, same batch
    a = D.DeviceAugmentation('train', width=S, height=S, dtype=torch.float32, seed=3)
    b = D.DeviceAugmentation('train', width=S, height=S, dtype=torch.float32, seed=3)
    ia, aa, pa = a(samples); ib, ab, pb = b(samples)
    assert torch.equal(pa, pb) and torch.equal(ia.map.tensor(), ib.map.tensor()) and torch.equal(aa, ab)


def test_output_feeds_the_model():
    from efficientdet.pytorch_amd import EfficientDet, EFFICIENTDET
    from oracle import effdet_oracle as O
    net, nc = 'efficientdet-d0', 20
    c = EFFICIENTDET[net]
    m = EfficientDet(nc, network=net, W_bifpn=c['W_bifpn'], D_bifpn=c['D_bifpn'], D_class=c['D_class'], compute_dtype=torch.float32)
    m.load_state_dict(O.make_state_dict(net, nc, seed=0))
    m = m.cuda(); m.train(); m.is_training = True; m.freeze_bn()
    aug = D.DeviceAugmentation('train', width=128, height=128, dtype=torch.float32, seed=1)
    images, ann, _ = aug(_samples([(200, 150), (90, 300)], seed=7))
    cl, rl = m([images, ann])
    (cl.mean() + rl.mean()).backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(cl).all()) and bool(torch.isfinite(rl).all())
