"""GPU tier: the device half of the JPEG decoder (effdet_jpeg_reconstruct through data.decode_jpeg_batch and the two collaters)
against the goldens of tools/make_jpeg_golden.py -- the pixels of Pillow / libjpeg-turbo.  Every comparison is exact.  The device
only ever sees streams the host stage accepted."""
import os

import numpy as np
import pytest
import torch

from efficientdet.pytorch_amd import data as D
from efficientdet.pytorch_amd import ops

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'jpeg_cases.npz')


@pytest.fixture(scope='module')
def G():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


def names(G):
    return [str(n) for n in G['names']]


def stream(G, name):
    return G[name + '/jpg'].tobytes()


def assert_batch_equals_golden(G, ns, out):
    src, off, hw = out
    assert src.dtype == torch.uint8 and off.dtype == torch.int64 and hw.dtype == torch.int32
    src, off, hw = src.cpu().numpy(), off.cpu().numpy(), hw.cpu().numpy()
    assert off.shape == (len(ns),) and hw.shape == (len(ns), 2) and not (off % 16).any()
    spans = []
    for b, n in enumerate(ns):
        want = G[n + '/rgb']
        assert tuple(hw[b]) == want.shape[:2], n
        got = src[off[b]:off[b] + want.size].reshape(want.shape)
        assert np.array_equal(got, want), (n, int((got != want).sum()))
        spans.append((int(off[b]), int(off[b]) + want.size))
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))     # no two images overlap


def test_one_batch_everything_mixed(G):
    ns = names(G)
    order = np.random.RandomState(5).permutation(len(ns))
    ns = [ns[i] for i in order]                                    # all sampling classes, grey, restart intervals and sizes in one batch
    assert_batch_equals_golden(G, ns, D.decode_jpeg_batch([stream(G, n) for n in ns], 'cuda', threads=4))


@pytest.mark.parametrize('name', ['1x1_s0', '33x47_s2'])
def test_batch_of_one(G, name):
    assert_batch_equals_golden(G, [name], D.decode_jpeg_batch([stream(G, name)], 'cuda'))


def staged(G, ns, gap=48):
    """Host stage by hand -> device tensors for ops.jpeg_reconstruct, with `gap` bytes between the images of dst."""
    streams = [stream(G, n) for n in ns]
    infos = [ops.jpeg_probe(s)[1] for s in streams]
    coef_off = np.concatenate([[0], np.cumsum([i.coef_bytes for i in infos])]).astype(np.int64)
    coef = np.zeros(int(coef_off[-1]), dtype=np.uint8)
    desc = np.zeros(len(ns) * ops.JPEG_DESC_BYTES, dtype=np.uint8)
    status, wgs = ops.jpeg_entropy_batch(streams, coef, coef_off[:-1], desc, 2)
    assert status == 0
    sizes = [i.width * i.height * 3 for i in infos]
    dst_off, end = [], 16
    for n in sizes:
        dst_off.append(end)
        end = (end + n + gap + 15) // 16 * 16
    dev = 'cuda'
    return dict(coef=torch.from_numpy(coef).to(dev), desc=torch.from_numpy(desc).to(dev), B=len(ns), wgs=wgs,
                planes=torch.empty(int(coef_off[-1]) // 2, dtype=torch.uint8, device=dev),
                planes_off=torch.from_numpy(coef_off[:-1] // 2).to(dev), dst_off=torch.tensor(dst_off, dtype=torch.int64, device=dev)), \
        dst_off, sizes, end


def test_gap_bytes_are_untouched(G):
    ns = names(G)
    args, dst_off, sizes, end = staged(G, ns)
    pattern = (np.arange(end) * 7 + 3).astype(np.uint8)
    dst = torch.from_numpy(pattern.copy()).cuda()
    ops.jpeg_reconstruct(dst=dst, **args)
    got = dst.cpu().numpy()
    gaps = np.ones(end, dtype=bool)
    for n, o, sz in zip(ns, dst_off, sizes):
        assert np.array_equal(got[o:o + sz], G[n + '/rgb'].reshape(-1)), n
        gaps[o:o + sz] = False
    assert gaps.sum() >= 16 * len(ns) and np.array_equal(got[gaps], pattern[gaps])


def test_reconstruct_under_graph_capture(G):
    ns = ['33x47_s2_rst2', '17x9_s1', '9x20_grey', '1x1_s2', '33x47_s0']
    args, dst_off, sizes, end = staged(G, ns)
    eager = torch.zeros(end, dtype=torch.uint8, device='cuda')
    ops.jpeg_reconstruct(dst=eager, **args)
    torch.cuda.synchronize()
    dst = torch.zeros(end, dtype=torch.uint8, device='cuda')
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.jpeg_reconstruct(dst=dst, **args)                      # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                  # one linear chain: the two launches
        ops.jpeg_reconstruct(dst=dst, **args)
    for _ in range(2):
        dst.zero_()
        args['planes'].zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(dst, eager)
    for n, o, sz in zip(ns, dst_off, sizes):
        assert np.array_equal(eager[o:o + sz].cpu().numpy(), G[n + '/rgb'].reshape(-1)), n


def samples_pair(G, ns):
    rng = np.random.RandomState(2)
    jpeg, img = [], []
    for n in ns:
        px = G[n + '/rgb']
        h, w = px.shape[:2]
        k = rng.randint(0, 3)
        x1, y1 = rng.uniform(0, w / 2, k), rng.uniform(0, h / 2, k)
        ann = np.stack([x1, y1, x1 + rng.uniform(1, w / 2, k), y1 + rng.uniform(1, h / 2, k), rng.randint(0, 20, k)], 1)
        jpeg.append({'jpeg': stream(G, n), 'annot': ann})
        img.append({'img': px, 'annot': ann})
    return jpeg, img


COLLATE = ['33x47_s2', '19x16_s1', '16x16_grey', '17x9_s0', '33x47_s2_q5', '8x8_s2']


def test_collater_identity(G):
    jpeg, img = samples_pair(G, COLLATE)
    outs = []
    for samples in (jpeg, img):
        col = D.DeviceCollater(common_size=64, dtype=torch.float32, flip_x=0.5, seed=3)
        packed, ann, scale = col(samples)
        outs.append((packed.map.tensor().clone(), ann.clone(), scale.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize('phase', ['valid', 'train'])
def test_augmentation_identity(G, phase):
    jpeg, img = samples_pair(G, COLLATE)
    table = D.sample_augment_table(np.random.RandomState(9), len(COLLATE), 64) if phase == 'train' else None
    outs = []
    for samples in (jpeg, img):
        aug = D.DeviceAugmentation(phase, width=64, height=64, dtype=torch.float32)
        packed, ann, params = aug(samples, table=table) if phase == 'train' else aug(samples)
        outs.append((packed.map.tensor().clone(), ann.clone(), params.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_mixed_sample_kinds_are_refused(G):
    jpeg, img = samples_pair(G, COLLATE[:2])
    with pytest.raises(ValueError, match='not a mix'):
        D.DeviceCollater(common_size=64)([jpeg[0], img[1]])


def test_fallback_and_refusals(G, monkeypatch):
    ns = ['17x9_s2', '33x47_s1', '16x16_grey']
    fixed = (np.arange(5 * 7 * 3) * 11 % 251).astype(np.uint8).reshape(5, 7, 3)        # independent of every golden
    streams = [stream(G, ns[0]), stream(G, 'progressive'), stream(G, ns[1]), stream(G, ns[2])]
    seen = []

    def fallback(b):
        seen.append(b)
        return fixed
    src, off, hw = D.decode_jpeg_batch(streams, 'cuda', fallback=fallback)
    assert seen == [streams[1]]
    src, off, hw = src.cpu().numpy(), off.cpu().numpy(), hw.cpu().numpy()
    assert not (off % 16).any() and tuple(hw[1]) == (5, 7)
    assert np.array_equal(src[off[1]:off[1] + fixed.size], fixed.reshape(-1))
    for b, n in ((0, ns[0]), (2, ns[1]), (3, ns[2])):
        want = G[n + '/rgb']
        assert tuple(hw[b]) == want.shape[:2] and np.array_equal(src[off[b]:off[b] + want.size], want.reshape(-1)), n
    # the same through a collater
    ann = np.zeros((0, 5))
    col = D.DeviceCollater(common_size=32, dtype=torch.float32, decode_fallback=fallback)
    a = col([{'jpeg': s, 'annot': ann} for s in streams])
    pixels = [G[ns[0] + '/rgb'], fixed, G[ns[1] + '/rgb'], G[ns[2] + '/rgb']]
    b = D.DeviceCollater(common_size=32, dtype=torch.float32)([{'img': p, 'annot': ann} for p in pixels])
    assert torch.equal(a[0].map.tensor(), b[0].map.tensor()) and torch.equal(a[2], b[2])

    # refusals: raised on the host, before any launch
    launches = []
    real = ops.jpeg_reconstruct
    monkeypatch.setattr(ops, 'jpeg_reconstruct', lambda *a, **k: (launches.append(1), real(*a, **k))[1])
    with pytest.raises(D.UnsupportedJPEG, match='JPEG 1 of the batch.*progressive') as e:
        D.decode_jpeg_batch(streams, 'cuda')
    assert e.value.index == 1 and e.value.reason == 1
    bad = [stream(G, ns[0]), stream(G, ns[1]), stream(G, 'truncated_scan')]
    with pytest.raises(ValueError, match='JPEG 2 of the batch is corrupt'):
        D.DeviceCollater(common_size=32)([{'jpeg': s, 'annot': ann} for s in bad])
    with pytest.raises(ValueError, match='JPEG 0 of the batch is corrupt'):
        D.decode_jpeg_batch([stream(G, 'truncated_header')], 'cuda')
    assert not launches
    # ... and the next valid batch still decodes
    assert_batch_equals_golden(G, ns, D.decode_jpeg_batch([stream(G, n) for n in ns], 'cuda'))
    assert launches == [1]
