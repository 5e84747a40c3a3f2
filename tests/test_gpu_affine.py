"""GPU parity of the affine / perspective warp (csrc/affine.hip, ops.affine_warp / ops.affine_boxes, DeviceAugmentation(affine=...))
with the NumPy restatement tests/affine_restated.py on the cases of tests/affine_cases.py: every output byte equal, the kept boxes the
same rows in the same order with coordinates within 1e-4 px (the chain's bound; both sides are fp64, so the error printed is expected
to be 0), and the chain behind the stage bit for bit what tests/augment_restated.py gives on the restated images."""
import numpy as np
import pytest
import torch

from efficientdet.pytorch_amd import data as D
from efficientdet.pytorch_amd import ops
from tests import affine_restated as R
from tests import augment_restated as A
from tests import mosaic_restated as MR
from tests.affine_cases import CASES, _row, generic
from tests.mosaic_cases import CASES as MOSAIC_CASES
from tests.mosaic_cases import _row as mosaic_row

pytestmark = pytest.mark.gpu
BY_NAME = {c['name']: c for c in CASES}
MIX = {c['name']: c for c in MOSAIC_CASES}['mixup_lam_0.3']             # three sources of 30 x 45, 64 x 64 and 21 x 13 with boxes


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
        c['want'] = ([R.warp(c['imgs'][b], row, c['S'], c['fill']) for b, row in enumerate(c['table'])],
                     [R.boxes(c['annots'][b], c['imgs'][b].shape[:2], row, c['S'], c['wh_thr'], c['ar_thr'], c['area_thr'])
                      for b, row in enumerate(c['table'])])
    return c['want']


def _check_rows(got_all, want, b, bound=1e-4):
    got = got_all[got_all[:, 4] != -1]
    assert (got_all[len(got):] == -1).all(), ('-1 rows follow the kept ones', b)
    assert len(got) == len(want) and got[:, 4].tolist() == want[:, 4].tolist(), (b, len(got), len(want))
    err = float(np.abs(got[:, :4] - want[:, :4]).max(initial=0))
    assert err <= bound, (b, err)
    return err


def _run(c):
    src, off, hw = _upload(c['imgs'])
    t = torch.from_numpy(c['table']).cuda()
    out = ops.affine_warp(src, off, hw, t, c['S'], c['fill'])
    bx, counts = ops.affine_boxes(hw, t, c['S'], torch.from_numpy(c['annots']).cuda(), c['wh_thr'], c['ar_thr'], c['area_thr'])
    return out, bx, counts


@pytest.mark.parametrize('name', [c['name'] for c in CASES])
def test_warp_and_boxes_equal_the_restatement(name):
    c = BY_NAME[name]
    B, M = c['annots'].shape[:2]
    (out, bx, counts), (out2, bx2, counts2) = _run(c), _run(c)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (B, c['S'], c['S'], 3)
    assert tuple(bx.shape) == (B, M, 5) and bx.dtype == torch.float32 and counts.dtype == torch.int32
    assert torch.equal(out, out2) and torch.equal(bx, bx2) and torch.equal(counts, counts2)          # two runs
    got, bx, counts = out.cpu().numpy(), bx.cpu().numpy(), counts.cpu().numpy()
    want_px, want_bx = _restated(c)
    worst = 0.0
    for b in range(B):
        diff = got[b] != want_px[b]
        assert not diff.any(), (name, b, int(diff.sum()), np.argwhere(diff)[:4].tolist())
        assert counts[b] == len(want_bx[b]), (name, b, int(counts[b]), len(want_bx[b]))
        worst = max(worst, _check_rows(bx[b], want_bx[b], b))
    print('%s: counts %s, largest coordinate error %.3g px' % (name, counts.tolist(), worst))


def test_einval_raises_and_launches_nothing():
    c = BY_NAME['identity']
    src, off, hw = _upload(c['imgs'])
    t, ann = torch.from_numpy(c['table']).cuda(), torch.from_numpy(c['annots']).cuda()
    torch.cuda.synchronize()
    for side, fill in ((7, 114), (0, 114), (32, 256), (32, -1)):
        with pytest.raises(RuntimeError, match='EFFDET_EINVAL'):
            ops.affine_warp(src, off, hw, t, side, fill)
    with pytest.raises(RuntimeError, match='EFFDET_EINVAL'):
        ops.affine_boxes(hw, t, 7, ann)
    with pytest.raises(RuntimeError, match='EFFDET_EINVAL'):
        ops.affine_boxes(hw, t, 32, ann[:, :0].contiguous())           # M = 0
    torch.cuda.synchronize()                                           # nothing was enqueued that could fail later
    assert np.array_equal(ops.affine_warp(src, off, hw, t, 32, 114).cpu().numpy()[0], c['imgs'][0])


# ------------------------------------------------------------------------------------------------ through DeviceAugmentation, S = 32
S = 32


def _aug_row(**kw):
    r = np.zeros(len(D.AUG_COLUMNS), dtype=np.float32)
    for k, v in kw.items():
        r[D.AUG[k]] = v
    return r


AUG_ROWS = [_aug_row(rrc=1, crop_y=3, crop_x=5, crop_h=20, crop_w=17, flip=1, flip_code=-1, clahe=1, clip_limit=2.5),
            _aug_row(transpose=1, color=1, alpha=1.2, beta=-0.1, hflip=1),
            _aug_row(shift=2, hue_shift=-3.5, sat_shift=2.5, val_shift=9, vflip=1, flip=1, flip_code=1)]


def _samples(imgs, annots):
    return [{'img': im, 'annot': a[a[:, 4] != -1]} for im, a in zip(imgs, annots)]


def _final(images):
    return images.map.tensor()[..., :3].cpu()


def _count_calls(monkeypatch):
    calls = {'warp': 0, 'boxes': 0}
    real = (ops.affine_warp, ops.affine_boxes)

    def warp(*a, **k):
        calls['warp'] += 1
        return real[0](*a, **k)

    def boxes(*a, **k):
        calls['boxes'] += 1
        return real[1](*a, **k)
    monkeypatch.setattr(ops, 'affine_warp', warp)
    monkeypatch.setattr(ops, 'affine_boxes', boxes)
    return calls


def test_without_the_option_nothing_new_is_called(monkeypatch):
    calls = _count_calls(monkeypatch)
    samples = _samples(MIX['imgs'], MIX['annots'])
    kw = dict(phase='train', width=S, height=S, dtype=torch.float32, seed=5)
    for mosaic in (None, D.MosaicOptions(mixup_p=0.5)):
        aug = D.DeviceAugmentation(mosaic=mosaic, affine=D.AffineOptions(degrees=10.0), **kw)
        aug.affine = None                                              # the plain attribute
        plain = D.DeviceAugmentation(mosaic=mosaic, **kw)              # built without the argument
        sa, sb = {}, {}
        ia, aa, pa = aug(samples, stages=sa)
        ib, ab, pb = plain(samples, stages=sb)
        assert calls == {'warp': 0, 'boxes': 0} and 'affine' not in sa and 'affine_table' not in sa
        assert torch.equal(ia.map.tensor(), ib.map.tensor()) and torch.equal(aa, ab) and torch.equal(pa, pb)
        assert aug.rng.rand() == plain.rng.rand()                      # no random number was drawn for the stage
    # and what the seed draws is what it drew before the option existed
    assert np.array_equal(pb.cpu().numpy(), D.sample_augment_table(np.random.RandomState(5), 3, S))
    aug.affine = D.AffineOptions(degrees=10.0)
    stages = {}
    aug(samples, stages=stages)
    assert calls == {'warp': 1, 'boxes': 1} and tuple(stages['affine'].shape) == (3, S, S, 3) and stages['affine'].dtype == torch.uint8
    assert tuple(stages['affine_table'].shape) == (3, len(D.AFFINE_COLUMNS)) and stages['affine_table'].dtype == torch.float64
    assert tuple(stages['mosaic'].shape) == (3, S, S, 3)               # canvas = 1: the mosaic keeps its side


def test_all_rows_off_is_the_path_without_affine():
    c = BY_NAME['generic']
    samples = _samples(c['imgs'], c['annots'])
    at = np.stack([AUG_ROWS[b % 3] for b in range(5)])
    off = np.stack([_row(on=0)] * 5)
    kw = dict(phase='train', width=S, height=S, dtype=torch.float32)  # min_area = min_visibility = 0
    sa, sb = {}, {}
    ia, aa, _ = D.DeviceAugmentation(affine=D.AffineOptions(), **kw)(samples, table=at, affine_table=off, stages=sa)
    ib, ab, _ = D.DeviceAugmentation(affine=None, **kw)(samples, table=at, stages=sb)
    assert torch.equal(ia.map.tensor(), ib.map.tensor()) and torch.equal(sa['a'], sb['a']) and torch.equal(sa['b'], sb['b'])
    assert torch.equal(sa['affine'], sb['a'][..., :3])
    aa, ab = aa.cpu().numpy(), ab.cpu().numpy()
    assert aa.shape == ab.shape and (ab[..., 4] != -1).sum() > 100
    worst = max(_check_rows(aa[b], ab[b][ab[b][:, 4] != -1], b) for b in range(5))
    print('all rows off: largest coordinate error %.3g px' % worst)


def test_the_chain_runs_on_the_warped_images_as_on_dataset_images():
    c = BY_NAME['generic']
    imgs, annots = c['imgs'][:3], c['annots'][:3]
    samples = _samples(imgs, annots)
    rng = np.random.RandomState(8)
    wt = np.stack([generic(rng, 90, 70, S, perspective=0.001), _row(on=0), generic(rng, 1, 17, S)])
    at = np.stack(AUG_ROWS)
    opts = D.AffineOptions(fill=99, wh_thr=1.5, ar_thr=20.0, area_thr=0.15)
    aug = D.DeviceAugmentation(phase='train', width=S, height=S, dtype=torch.float32, min_area=1.0, min_visibility=0.2, affine=opts)
    stages = {}
    images, ann, params = aug(samples, table=at, stages=stages, affine_table=wt)
    torch.cuda.synchronize()
    assert torch.equal(stages['affine_table'].cpu(), torch.from_numpy(wt)) and torch.equal(params.cpu(), torch.from_numpy(at))
    got_w, got = stages['affine'].cpu().numpy(), _final(images)
    kept = []
    for b in range(3):
        want_w = R.warp(imgs[b], wt[b], S, 99)
        assert np.array_equal(got_w[b], want_w), ('affine', b)
        ref = A.train_stages(want_w, at[b], S)
        assert np.array_equal(stages['a'][b].cpu().numpy()[..., :3], want_w), ('the chain copies an S x S source', b)
        assert torch.equal(got[b], torch.from_numpy(ref['out'])), ('out', b)
        kept.append(A.boxes(R.boxes(annots[b], imgs[b].shape[:2], wt[b], S, 1.5, 20.0, 0.15), (S, S), at[b], S, S, min_area=1.0, min_visibility=0.2))
    ann = ann.cpu().numpy()
    assert ann.shape[1] == max(1, max(len(k) for k in kept)) and sum(len(k) for k in kept) > 50
    for b in range(3):
        _check_rows(ann[b], kept[b], b)
    # a table from the device, or one that fails the check, is refused before the stage runs
    with pytest.raises(ValueError, match='host'):
        aug(samples, table=at, affine_table=torch.from_numpy(wt).cuda())
    bad = wt.copy(); bad[2, D.AFFINE['g0']] += 1e-3
    with pytest.raises(ValueError, match='row 2'):
        aug(samples, table=at, affine_table=bad)
    # a CPU tensor is a host table too
    images2, _, _ = aug(samples, table=at, affine_table=torch.from_numpy(wt))
    assert torch.equal(_final(images2), got)


def test_a_mosaic_of_twice_the_side_warped_down():
    """canvas = 2: the mosaic is composed at 2 S with its table checked at that side, the warp brings it to S, the chain follows."""
    samples = _samples(MIX['imgs'], MIX['annots'])
    hws = [im.shape[:2] for im in MIX['imgs']]
    mt = np.stack([mosaic_row(cx=30, cy=35, src=(0, 1, 2, 1), side=(40, 64, 30, 50), mix=1, mix_src=1, lam=0.3), mosaic_row(on=0),
                   mosaic_row(cx=40, cy=21, src=(2, 0, 0, 1), side=(21, 45, 64, 33))])         # centres and sides beyond S = 32
    rng = np.random.RandomState(9)
    wt = np.stack([generic(rng, 64, 64, S, scale=(0.8, 1.2)), generic(rng, 64, 64, S, perspective=0.001), _row(on=0)])
    at = np.stack(AUG_ROWS)
    opts = D.AffineOptions(canvas=2, fill=50)
    aug = D.DeviceAugmentation(phase='train', width=S, height=S, dtype=torch.float32, min_area=1.0, min_visibility=0.1,
                               mosaic=D.MosaicOptions(fill=99), affine=opts)
    stages = {}
    images, ann, _ = aug(samples, table=at, stages=stages, mosaic_table=mt, affine_table=wt)
    assert tuple(stages['mosaic'].shape) == (3, 2 * S, 2 * S, 3) and tuple(stages['affine'].shape) == (3, S, S, 3)
    got_m, got_w, got = stages['mosaic'].cpu().numpy(), stages['affine'].cpu().numpy(), _final(images)
    kept = []
    for b in range(3):
        want_m = MR.compose(MIX['imgs'], mt[b], 2 * S, 99, b)
        assert np.array_equal(got_m[b], want_m), ('mosaic', b)
        want_w = R.warp(want_m, wt[b], S, 50)
        assert np.array_equal(got_w[b], want_w), ('affine', b)
        assert torch.equal(got[b], torch.from_numpy(A.train_stages(want_w, at[b], S)['out'])), ('out', b)
        bm = MR.boxes(MIX['annots'], hws, mt[b], 2 * S, 1.0, float(np.float32(0.1)), b)
        bw = R.boxes(bm, (2 * S, 2 * S), wt[b], S, opts.wh_thr, opts.ar_thr, opts.area_thr)
        kept.append(A.boxes(bw, (S, S), at[b], S, S, min_area=1.0, min_visibility=0.1))
    ann = ann.cpu().numpy()
    assert sum(len(k) for k in kept) > 3 and ann.shape[1] == max(1, max(len(k) for k in kept))
    worst = max(_check_rows(ann[b], kept[b], b) for b in range(3))
    print('canvas = 2: kept %s, largest coordinate error %.3g px' % ([len(k) for k in kept], worst))
    # a mosaic table that is only valid at S is refused at 2 S's check the other way round: a centre beyond 2 S
    bad = mt.copy(); bad[0, D.MOSAIC['cx']] = 2 * S + 1
    with pytest.raises(ValueError, match='row 0'):
        aug(samples, table=at, mosaic_table=bad, affine_table=wt)
    # sampled tables: the mosaic's at 2 S, then the warp's with the canvases as its sources
    aug2 = D.DeviceAugmentation(phase='train', width=S, height=S, dtype=torch.float32, seed=3, mosaic=D.MosaicOptions(), affine=opts)
    st = {}
    aug2(samples, stages=st)
    r = np.random.RandomState(3)
    D.sample_augment_table(r, 3, S)
    assert np.array_equal(st['mosaic_table'].cpu().numpy(), D.sample_mosaic_table(r, 3, 2 * S, D.MosaicOptions()))
    assert np.array_equal(st['affine_table'].cpu().numpy(), D.sample_affine_table(r, 3, S, np.full((3, 2), 2 * S), opts))
