"""Weight gradients of one layer of both RetinaHead towers as one launch (include/effdet_wgrad_pair.h; functional.HEAD_PAIR_WGRAD).

ops.conv2d_wgrad_pair runs a dense problem a and a (flagged) problem b of the same geometry in one grid, each planned as on its own.
Checked here: slabs and bias partial rows of both problems bit for bit against the two separate launches, for flag patterns that take
every branch of the flag walk (first / last step of a range, ranges without a live step, every flag set, no flags at all), with a grid
of less than one round of workgroups and one of more; the refusals; and the whole model with the switch on and off."""
import ctypes as C

import pytest
import torch

from tests.test_gpu_sparse_reg_grad import ALL, B3, LD, POINTS, SIZES, _model, _poff, _split_pyramid, _targets

pytestmark = pytest.mark.gpu

PATTERNS = {'ends': [(0, 0, 0, 0), (0, 1, 15, 15), (0, 2, 0, 0), (0, 2, 15, 15)], 'level1_only': [(1, 1, 2, 3), (1, 2, 7, 7)],
            'scattered': POINTS, 'all': ALL, 'none': []}
BIG_B, BIG_SIZES = 4, [(32, 32), (16, 16), (8, 8)]


def _problem(B, sizes, cin, pts, gen, x=None):
    """-> (x maps, dz maps, live32 of radius 0): a 3x3 cin -> 256 problem in the split layout whose dz is random on the pixels
    pts = [(level, b, h, w)] and an exact zero elsewhere (pts None: random everywhere)"""
    from efficientdet.pytorch_amd import ops
    poff, apix = _poff(sizes)
    nzpix = torch.zeros(B, apix, dtype=torch.bool)
    if pts is None:
        nzpix[:] = True
    for (l, b, h, w) in pts or []:
        nzpix[b, poff[l] + h * sizes[l][1] + w] = True
    if x is None:
        x = _split_pyramid([torch.randn(B, cin, h, w, generator=gen) for (h, w) in sizes], B, sizes, cin)
    dzs = []
    for l, (h, w) in enumerate(sizes):
        m = nzpix[:, poff[l]:poff[l] + h * w].reshape(B, 1, h, w)
        dzs.append(torch.randn(B, 256, h, w, generator=gen) * m)
    flagsrc = torch.zeros(B, apix, LD)
    flagsrc[..., 0] = nzpix.float()
    l32, _ = ops.live_tiles(flagsrc.cuda(), B, sizes, LD, False)
    return x, _split_pyramid(dzs, B, sizes, 256), l32[0].contiguous()


def _check_pair(B, sizes, cin, pts_b, gen, flags='own', shared_x=False):
    """the paired launch against the two separate ones; flags: 'own' (b's radius-0 flags), 'ones' (every flag set), None (both dense)"""
    from efficientdet.pytorch_amd import ops
    xa, za, _ = _problem(B, sizes, cin, None, gen)
    xb, zb, l32 = _problem(B, sizes, cin, pts_b, gen, x=xa if shared_x else None)
    live = {'own': l32, 'ones': torch.ones_like(l32), None: None}[flags]
    kw = dict(Cin=cin, Cout=256, KH=3, KW=3, pad_t=1, pad_l=1)
    Ga, ba = ops.conv2d_wgrad(xa, za, split=True, **kw)
    Gb, bb = ops.conv2d_wgrad(xb, zb, split=True, live32=live, **kw)
    (Pa, pa), (Pb, pb) = ops.conv2d_wgrad_pair(xa, za, xb, zb, live32_b=live, **kw)
    torch.cuda.synchronize()
    assert Pa.shape == Ga.shape and Pb.shape == Gb.shape and pa.shape == ba.shape and pb.shape == bb.shape
    for got, want in ((Pa, Ga), (pa, ba), (Pb, Gb), (pb, bb)):
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert bool(Ga.any()) and bool(ba.any())
    if pts_b is None or len(pts_b):
        assert bool(Gb.any()) and bool(bb.any())
    else:
        assert not bool(Gb.any()) and not bool(bb.any())
    return l32, Ga.shape[0] + Gb.shape[0]


@pytest.mark.parametrize('cin', [256, 64])
@pytest.mark.parametrize('pattern', ['ends', 'level1_only', 'scattered', 'all', 'none'])
def test_paired_launch_equals_the_two_separate_launches(cin, pattern):
    """B = 3, levels 16x16, 8x8, 4x4 (split ranges of 512 pixels, a level that is no multiple of the range, 4-wide rows): a dense, b flagged.
    64 -> 256: both problems read the same x, as layer 0 of the towers reads the pyramid."""
    l32, _ = _check_pair(B3, SIZES, cin, PATTERNS[pattern], torch.Generator().manual_seed(cin + len(pattern)), shared_x=cin == 64)
    if pattern == 'all':
        assert bool(l32.all())
    else:
        assert bool((l32 == 0).any())
    if pattern == 'none':
        assert not bool(l32.any())


@pytest.mark.parametrize('flags', [None, 'ones'])
def test_both_dense_and_every_flag_set(flags):
    """live32_b = None: both halves run the dense body; every flag set on a sparse dz: the flag walk visits every step."""
    _check_pair(B3, SIZES, 256, POINTS, torch.Generator().manual_seed(3), flags=flags)


def test_a_grid_of_more_than_one_round():
    """More blocks than the 512 resident workgroups: the order of the blocks matters and a second round exists."""
    from efficientdet.pytorch_amd import _lib as L
    from tests.host_util import wgrad_desc
    d = wgrad_desc(L.F32_SPLIT, BIG_B, 256, 256, BIG_SIZES, k=3, pad=1)
    splits = int(L.lib().effdet_conv2d_wgrad_splits(C.byref(d)))
    tiles = 2 * 18                                   # 256 output channels / 128 x 2304 (tap, channel) columns / 128
    assert splits >= 1 and 2 * splits * tiles > 512, splits
    pts = [(0, 0, 0, 0), (0, 3, 31, 31), (0, 1, 16, 5), (1, 2, 7, 7), (2, 0, 3, 3), (2, 3, 0, 7)]
    l32, nslab = _check_pair(BIG_B, BIG_SIZES, 256, pts, torch.Generator().manual_seed(9))
    assert nslab == 2 * splits and bool((l32 == 0).any()) and bool(l32.any())


def test_refusals_launch_nothing():
    """Different Cout, and a dtype that does not plan to the split-layout kernel: the unsupported status, the workspace untouched."""
    from efficientdet.pytorch_amd import ops, _lib as L
    gen = torch.Generator().manual_seed(4)
    xa, za, _ = _problem(B3, SIZES, 256, None, gen)
    lib = L.require('effdet_conv2d_wgrad_pair')

    def desc(cout, split=True):
        return ops._wgrad_desc(xa, za, None, None, 256, cout, 3, 3, 1, 1, 1, True, split, False)
    good = desc(256)
    need = int(lib.effdet_conv2d_wgrad_workspace_bytes(C.byref(good)))
    assert need > 0
    ws = torch.full((2 * need // 4,), float('nan'), device='cuda')
    for a, b in ((good, desc(128)), (desc(128), good), (desc(256, split=False), desc(256, split=False)), (good, desc(256, split=False))):
        rc = int(lib.effdet_conv2d_wgrad_pair(C.byref(a), C.byref(b), L.ptr(ws), ws.numel() * 4, None, L.stream_ptr()))
        assert L._ERR[rc] == 'EFFDET_EUNSUPPORTED', rc
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws).all())
    assert int(lib.effdet_conv2d_wgrad_pair(C.byref(good), C.byref(good), L.ptr(ws), 2 * need - 4, None, L.stream_ptr())) == -1      # short workspace
    assert int(lib.effdet_conv2d_wgrad_pair(C.byref(good), C.byref(good), L.ptr(ws), 2 * need, None, L.stream_ptr())) == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(ws).any())


# ----------------------------------------------------------------------------------------------------------- whole model
def _step(m, img, ann):
    m.zero_grad(set_to_none=True)
    cl, rl = m([img, ann])
    (cl.mean() + rl.mean()).backward()
    torch.cuda.synchronize()
    return cl.detach().clone(), rl.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}


def _on_off(arith, targets, sparse):
    from efficientdet.pytorch_amd import ops, functional as Fn
    from oracle import effdet_oracle as O
    m = _model(arith)
    img = O.synthetic_batch(2, 512, seed=2, num_classes=8)[0].cuda()
    ann = _targets(targets).cuda()
    calls, real = [], ops.conv2d_wgrad_pair

    def counting(*a, **kw):
        calls.append(kw.get('live32_b') is not None)
        return real(*a, **kw)
    old = Fn.HEAD_PAIR_WGRAD, Fn.HEAD_SPARSE_REG
    outs = []
    try:
        ops.conv2d_wgrad_pair = counting
        Fn.HEAD_SPARSE_REG = sparse
        for on in (False, True):
            Fn.HEAD_PAIR_WGRAD = on
            n0 = len(calls)
            outs.append(_step(m, img, ann))
            # the paired head (the f16x3 forward) pairs its four tower layers when the switch is on; nothing else ever does
            assert len(calls) - n0 == (4 if on and arith == 'f32_hf16x3_bwd_bf16x3' else 0)
        assert all(f == sparse for f in calls)
    finally:
        ops.conv2d_wgrad_pair = real
        Fn.HEAD_PAIR_WGRAD, Fn.HEAD_SPARSE_REG = old
    a, b = outs
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert a[2].keys() == b[2].keys() and len(a[2]) == 274
    bad = [k for k in a[2] if not torch.equal(a[2][k], b[2][k])]
    assert not bad, bad[:8]


@pytest.mark.parametrize('arith', ['f32_hf16x3_bwd_bf16x3', 'bf16x3'])
@pytest.mark.parametrize('targets', ['one_small_box', 'empty_and_eight', 'every_tile_live'])
def test_model_gradients_equal_with_the_switch_on_and_off(arith, targets):
    """D0 @512, B = 2: both losses and every parameter gradient torch.equal with functional.HEAD_PAIR_WGRAD off and on -- the paired head
    (f32_hf16x3_bwd_bf16x3), which the switch changes, and the unpaired one (bf16x3), which it must leave alone."""
    _on_off(arith, targets, True)


def test_model_gradients_equal_without_the_flags():
    """HEAD_SPARSE_REG off: both halves of every paired launch are dense."""
    _on_off('f32_hf16x3_bwd_bf16x3', 'empty_and_eight', False)
