"""GPU, op level: ops.slice_images against torch indexing and ops.merge_slices against the NumPy restatement of include/effdet_slices.h
(tests/slices_restated.py), bit for bit.

Slicer: B = 2 images of 37 x 53, tiles of 5 x 7 and 16 x 8 at all four edges, inside, and at two origins outside the image (the
edge-clamp expectation), every kind of source (NCHW fp32; NHWC fp32 / bf16 with 4 / 8 channels; arena slices, strided, aligned and
not), tile ranges that start inside image 0 and end inside image 1, an Inf and a NaN pixel; the output lies between two guard regions
of a sentinel that must be untouched, and its pad channels must be +0 by bits.

Merge: every case of tests/slices_cases.CASES equals the restatement in score bits, labels, box bits and counts; refusals leave
pre-filled outputs alone; a captured call replays bit-equal.  One test prints single measured durations (no threshold)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import slices_restated as R
from tests.slices_cases import CASES

pytestmark = pytest.mark.gpu
GUARD = 1024                     # bytes of sentinel on either side of the output
SENTINEL = 0xA5
H, W, B = 37, 53, 2
BY_NAME = {c['name']: c for c in CASES}
# name -> (dtype, channels, ld, off, gap between images) in elements; None: the NCHW tensor
SOURCES = {'nchw_f32': None, 'f32_c4': ('f32', 4, 4, 0, 0), 'bf16_c8': ('bf16', 8, 8, 0, 0), 'f32_arena_aligned': ('f32', 4, 8, 4, 16),
           'f32_arena_c3_unaligned': ('f32', 3, 5, 1, 3), 'bf16_arena_aligned': ('bf16', 4, 12, 8, 4), 'bf16_arena_unaligned': ('bf16', 8, 9, 1, 5)}


def _table(h, w):
    """(y0, x0) at the four corners, inside, partly outside (above and past the right edge) and far outside."""
    return [(y0, x0, h, w, 1.0, 1.0) for y0, x0 in ((0, 0), (0, W - w), (H - h, 0), (H - h, W - w), (11, 17), (-3, W - 3), (1000, -1000))]


def _bits(seed, isz):
    """[B][H][W][3] element bits with an Inf, a -Inf and two NaNs (one with a payload) among them, at an edge and inside."""
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 1, (B, H, W, 3)).astype(np.float32)
    x[0, 0, 0, 0], x[0, H - 1, W - 1, 1], x[1, 12, 18, 2], x[1, 0, W - 1, 0] = np.inf, np.nan, -np.inf, np.nan
    bits = x.view(np.uint32).copy()
    bits[1, 0, W - 1, 0] = 0x7fc12345                                  # a NaN payload survives a bit copy
    return bits if isz == 4 else (bits >> 16).astype(np.uint16)


def _device_source(name, bits):
    from efficientdet.pytorch_amd import PackedImages, ops
    lay = SOURCES[name]
    if lay is None:
        return torch.from_numpy(np.ascontiguousarray(bits.view(np.float32).transpose(0, 3, 1, 2))).cuda()
    kind, Cc, ld, off, gap = lay
    bstride = H * W * ld + gap
    host = np.full(off + B * bstride + 8, 0x4111 if kind == 'bf16' else 0x41100000, dtype=bits.dtype)     # (9.0 between the pixels)
    for b in range(B):
        img = host[off + b * bstride: off + b * bstride + H * W * ld].reshape(H * W, ld)
        img[:, :Cc] = 0x40e0 if kind == 'bf16' else 0x40e00000         # 7.0 in the channels past the third: never copied
        img[:, :3] = bits[b].reshape(H * W, 3)
    arena = torch.from_numpy(host.view(np.int16)).view(torch.bfloat16) if kind == 'bf16' else torch.from_numpy(host.view(np.float32))
    return PackedImages(ops.Map(arena.cuda(), B, H, W, Cc, ld=ld, bstride=bstride, off=off))


def _want(bits, table, t0, t1, ce):
    """torch indexing on the bits: [t1 - t0][h][w][ce]."""
    src = torch.from_numpy(bits.astype(np.int64))
    T, h, w = len(table), table[0][2], table[0][3]
    out = torch.zeros((t1 - t0, h, w, ce), dtype=torch.int64)
    for t in range(t0, t1):
        b, j = divmod(t, T)
        ys = (table[j][0] + torch.arange(h)).clamp(0, H - 1)
        xs = (table[j][1] + torch.arange(w)).clamp(0, W - 1)
        out[t - t0, :, :, :3] = src[b][ys][:, xs]
    return out.numpy()


@pytest.mark.parametrize('hw', [(5, 7), (16, 8)], ids=['5x7', '16x8'])
@pytest.mark.parametrize('name', list(SOURCES))
def test_slicer_equals_torch_indexing_bit_for_bit(name, hw):
    from efficientdet.pytorch_amd import ops
    bf16 = SOURCES[name] is not None and SOURCES[name][0] == 'bf16'
    dtype, ce, isz = (torch.bfloat16, 8, 2) if bf16 else (torch.float32, 4, 4)
    bits = _bits(3, isz)
    src = _device_source(name, bits)
    h, w = hw
    table = _table(h, w)
    T = len(table)
    dev_table = ops.slice_table(table, 'cuda')
    for t0, t1, tab in ((0, B * T, table), (3, T + 3, dev_table), (T - 1, T + 1, dev_table), (B * T - 1, B * T, table)):
        n = (t1 - t0) * h * w * ce
        raw = torch.full((2 * GUARD + n * isz,), SENTINEL, dtype=torch.uint8, device='cuda')
        out = ops.Map(raw.view(dtype), t1 - t0, h, w, ce, off=GUARD // isz)
        res = ops.slice_images(src, tab, (h, w), t0, t1, out=out)
        torch.cuda.synchronize()
        host = raw.cpu().numpy()
        assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + n * isz:] == SENTINEL).all(), 'a guard region was written'
        assert res.map is out and tuple(res.shape) == (t1 - t0, 3, h, w) and res.dtype == dtype
        got = host[GUARD:GUARD + n * isz].view(np.uint16 if isz == 2 else np.uint32).reshape(t1 - t0, h, w, ce)
        assert not got[..., 3:].any()                                  # pad channels: +0, bit for bit
        want = _want(bits, table, t0, t1, ce)
        assert np.array_equal(got.astype(np.int64), want), (name, t0, t1, np.argwhere(got.astype(np.int64) != want)[:1].tolist())
        assert np.array_equal(want, R.slice_images(bits, table, t0, t1, ce).astype(np.int64))
    # the far-outside record is the clamped corner everywhere; an allocated output is the dense stem layout
    res = ops.slice_images(src, table, (h, w), T - 1, T)
    m = res.map
    assert (m.B, m.H, m.W, m.C, m.ld, m.bstride, m.off) == (1, h, w, ce, ce, h * w * ce, 0) and m.t.data_ptr() % 16 == 0
    got = m.t.view(torch.int16 if bf16 else torch.int32).cpu().numpy().view(np.uint16 if bf16 else np.uint32)
    assert (got[..., :3] == bits[0, H - 1, 0]).all() and not got[..., 3:].any()


def test_slicer_python_level_refusals():
    from efficientdet.pytorch_amd import ops
    img = torch.zeros(2, 3, 40, 40, device='cuda')
    tab = [(0, 0, 8, 8, 1.0, 1.0)] * 3
    for t0, t1 in ((-1, 2), (2, 2), (0, 7), (6, 7)):
        with pytest.raises(ValueError, match='tile range'):
            ops.slice_images(img, tab, (8, 8), t0, t1)
    with pytest.raises(TypeError, match='float32'):
        ops.slice_images(img.half(), tab, (8, 8), 0, 1)
    with pytest.raises(ValueError, match='contiguous'):
        ops.slice_images(torch.zeros(2, 40, 40, 3, device='cuda').permute(0, 3, 1, 2), tab, (8, 8), 0, 1)
    with pytest.raises(ValueError, match='out must be'):
        ops.slice_images(img, tab, (8, 8), 0, 2, out=ops.Map.new(1, 8, 8, 4, torch.float32, 'cuda'))
    with pytest.raises(ValueError, match='tile table'):
        ops.slice_images(img, torch.zeros(3, 4, device='cuda'), (8, 8), 0, 1)


def _run_merge(c):
    from efficientdet.pytorch_amd import ops
    o = ops.SliceMergeOptions(max_det=c['max_det'], top_n=c['score'].shape[2], **c['opts'])
    lists = tuple(torch.from_numpy(c[k]).cuda() for k in ('score', 'label', 'boxes', 'count'))
    out = ops.merge_slices(lists, c['table'], c['H'], c['W'], o)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _assert_equal(got, want, name):
    gs, gl, gb, gc = got
    ws, wl, wb, wc = want[:4]
    assert gc.tolist() == wc.tolist(), (name, gc.tolist(), wc.tolist())
    assert np.array_equal(gl, wl), name
    assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32)), name
    bad = gb.view(np.uint32) != wb.view(np.uint32)
    assert not bad.any(), '%s: %d box elements differ, first at %s' % (name, bad.sum(), np.argwhere(bad)[0].tolist())


@pytest.mark.parametrize('c', CASES, ids=[c['name'] for c in CASES])
def test_merge_equals_the_restatement_bit_for_bit(c):
    K = min(c['max_det'], c['score'].shape[1] * c['score'].shape[2])
    want = R.merge_batch(c['score'], c['label'], c['boxes'], c['count'], c['table'], c['W'], c['H'], K, **c['opts'])
    got = _run_merge(c)
    assert got[0].shape == (len(c['score']), K) and got[2].shape == (len(c['score']), K, 4) and got[1].dtype == np.int64 and got[3].dtype == np.int32
    _assert_equal(got, want, c['name'])
    if c['name'] == 'chain':
        assert got[3].tolist() == [3] and got[2][0, :3].tolist() == [[0, 0, 12, 10], [0, 0, 12, 3.5], [40, 40, 48, 48]]
    if c['name'] == 'batch3_one_empty':
        assert got[3][1] == 0 and not got[0][1].any() and not got[2][1].any()


def test_merged_rows_go_through_finalize_dets_as_they_are():
    from efficientdet.pytorch_amd import ops
    c = BY_NAME['nmm_ios_aware']
    o = ops.SliceMergeOptions(max_det=c['max_det'], top_n=64, **c['opts'])
    s, l, b, n = ops.merge_slices(tuple(torch.from_numpy(c[k]).cuda() for k in ('score', 'label', 'boxes', 'count')), c['table'], c['H'], c['W'], o)
    out, oc = ops.finalize_dets(s, l, b, n, torch.ones(1, device='cuda'), 0.0, 100, False)
    k = int(oc[0])
    assert k == min(int(n[0]), 100) and torch.equal(out[0, :k, 4], s[0, :k]) and torch.equal(out[0, :k, :4], b[0, :k])


def test_refusals_launch_nothing_and_leave_the_outputs_alone():
    from efficientdet.pytorch_amd import _lib, ops
    L = _lib.require('effdet_slice_merge', 'effdet_slice_merge_workspace_bytes')
    for kw in (dict(TPI=8193, R=1), dict(TPI=1, R=8193), dict(max_det=0), dict(thr=1.5)):
        v = dict(TPI=4, R=8, max_det=8, thr=0.5)
        v.update(kw)
        TPI, Rr, K = v['TPI'], v['R'], max(v['max_det'], 1)
        s = torch.rand(1, TPI, Rr, device='cuda'); l = torch.zeros(1, TPI, Rr, dtype=torch.int64, device='cuda')
        b = torch.rand(1, TPI, Rr, 4, device='cuda'); n = torch.full((1, TPI), Rr, dtype=torch.int32, device='cuda')
        table = ops.slice_table([(0, 0, 128, 128, 1.0, 1.0)] * min(TPI, 1024), 'cuda')
        outs = [torch.full((1, K), -7.0, device='cuda'), torch.full((1, K), -7, dtype=torch.int64, device='cuda'),
                torch.full((1, K, 4), -7.0, device='cuda'), torch.full((1,), -7, dtype=torch.int32, device='cuda')]
        ws = torch.full((1 << 20,), SENTINEL, dtype=torch.uint8, device='cuda')
        d = _lib.SliceMerge()
        d.score, d.label, d.boxes, d.count, d.tiles = (_lib.ptr(t) for t in (s, l, b, n, table))
        d.out_score, d.out_label, d.out_boxes, d.out_count = (_lib.ptr(t) for t in outs)
        d.B, d.TPI, d.R, d.method, d.metric, d.class_aware, d.max_det, d.W, d.H, d.thr, d.skip_thr = 1, TPI, Rr, 1, 1, 1, v['max_det'], 128.0, 128.0, v['thr'], 0.0
        assert L.effdet_slice_merge(C.byref(d), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()) == -3, kw
        torch.cuda.synchronize()
        assert all(bool((t == -7).all()) for t in outs) and bool((ws == SENTINEL).all()), kw
    with pytest.raises(ValueError, match=r'TPI \* R <= 8192'):
        ops.merge_slices((torch.zeros(1, 1, 8193, device='cuda'), torch.zeros(1, 1, 8193, dtype=torch.int64, device='cuda'),
                          torch.zeros(1, 1, 8193, 4, device='cuda'), torch.zeros(1, 1, dtype=torch.int32, device='cuda')),
                         [(0, 0, 128, 128, 1.0, 1.0)], 128, 128)
    with pytest.raises(ValueError, match='2 lists per image but 3 tiles'):
        ops.merge_slices((torch.zeros(1, 2, 8, device='cuda'), torch.zeros(1, 2, 8, dtype=torch.int64, device='cuda'),
                          torch.zeros(1, 2, 8, 4, device='cuda'), torch.zeros(1, 2, dtype=torch.int32, device='cuda')),
                         [(0, 0, 128, 128, 1.0, 1.0)] * 3, 128, 128)


def test_captured_merge_replays_bit_equal():
    from efficientdet.pytorch_amd import ops
    c = BY_NAME['nmm_ios_aware']
    o = ops.SliceMergeOptions(max_det=c['max_det'], top_n=64, **c['opts'])
    lists = tuple(torch.from_numpy(c[k]).cuda() for k in ('score', 'label', 'boxes', 'count'))
    eager = [t.clone() for t in ops.merge_slices(lists, c['table'], c['H'], c['W'], o)]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = ops.merge_slices(lists, c['table'], c['H'], c['W'], o)
    for _ in range(2):
        for t in res:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, e) for a, e in zip(res, eager))


def test_single_measurements_of_the_cap_and_the_slicer():
    """Prints (no threshold): the merge of the 8192-candidate case at max_det = 1000, the slicer at 64 x 512 x 512 fp32 tiles from a
    2048 x 2048 source, and resample_images at the same output size in the same run for comparison."""
    from efficientdet.pytorch_amd import ops
    c = BY_NAME['n8192']
    assert c['max_det'] == 1000 and c['score'].shape[1:] == (32, 256)
    o = ops.SliceMergeOptions(max_det=1000, top_n=256, **c['opts'])
    lists = tuple(torch.from_numpy(c[k]).cuda() for k in ('score', 'label', 'boxes', 'count'))
    img = torch.rand(1, 3, 2048, 2048, device='cuda')
    at = [int(v) for v in np.linspace(0, 2048 - 512, 8)]
    table = ops.slice_table([(y, x, 512, 512, 1.0, 1.0) for y in at for x in at], 'cuda')
    small = torch.rand(64, 3, 256, 256, device='cuda')
    out = ops.Map.new(64, 512, 512, 4, torch.float32, 'cuda')

    def calls():
        ops.merge_slices(lists, c['table'], c['H'], c['W'], o)
        ops.slice_images(img, table, (512, 512), 0, 64, out=out)
        ops.resample_images(small, (512, 512), out=out)
    calls()                                                             # (warm: code objects loaded, workspace allocated)
    torch.cuda.synchronize()
    prev, ops.PROFILE = ops.PROFILE, ops.LaunchProfile()
    try:
        calls()
        summ = ops.PROFILE.summary()
    finally:
        ops.PROFILE = prev
    assert len(summ) == 3
    for name, d in sorted(summ.items()):
        print('%-60s %8.3f ms  %8.1f GB/s (algorithmic bytes)' % (name, d['ms'], d['flops'] / (d['ms'] * 1e-3) / 1e9))
