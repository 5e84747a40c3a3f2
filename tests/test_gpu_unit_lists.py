"""Gathered 32-pixel units of the regression tower's flagged launches, op level (include/effdet_unit_lists.h).

The compacted lists against the numpy restatement (tools/unit_count.py), and the gathered form of the f16x3 forward launches (needed
flags) and of the split-layout data-gradient launches (live flags) against the DENSE launch: the rows of every flagged unit hold the
dense launch's bytes in all output streams, every other flagged-segment row is zero bytes (under the in-place add: unchanged).  Every
comparison is exact.

Geometry: B = 2 with levels 32x32, 16x16, 8x8 -> 64 + 16 + 4 units of 32 pixels (one / two / four image rows), 16 + 4 + 1 tiles."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import unit_count as U          # noqa: E402

pytestmark = pytest.mark.gpu

B = 2
SIZES = [(32, 32), (16, 16), (8, 8)]
STEP0 = [0, 64, 80]              # first unit of each level; image 1 starts at unit 32 / 72 / 82
NSTEP, NTILE, ROWS = 84, 21, 2688
NAN_BITS = 0x7fc07fc0            # NaN as fp32 and as either 16-bit half: a row nobody wrote shows

PATTERNS = {
    'none': [],
    'all': list(range(NSTEP)),
    'seven': [3, 4, 40, 41, 42, 70, 83],                      # a count not divisible by 4, the last unit of the pyramid in the short tile
    'image_edges': [0, 31, 32, 63, 64, 71, 72, 79, 80, 83],   # the first and last row(s) of both images on every level
    'mixed_tile': [31, 32, 71, 72],                           # ONE gathered tile: two images of level 0, two images of level 1
}


# ------------------------------------------------------------------------------------------------------- the lists
def _map(kind):
    n = B * sum(h * w for h, w in SIZES)
    pm = np.zeros(n, dtype=np.uint8)
    if kind == 'full':
        pm[:] = 1
    elif kind == 'corner':
        pm[1023] = 1                                          # image 0, level 0, (31, 31)
    elif kind == 'straddle':
        pm[2046:2050] = 3                                     # the last two pixels of level 0 and the first two of level 1
    elif kind == 'scattered':
        pm[np.random.RandomState(3).permutation(n)[:9]] = 1
    return pm


@pytest.mark.parametrize('kind', ['empty', 'full', 'corner', 'straddle', 'scattered'])
def test_lists_and_counts_equal_the_numpy_restatement(kind):
    from efficientdet.pytorch_amd import ops
    pm = _map(kind)
    l32, l128 = ops.live_tiles_from_map(torch.from_numpy(pm).cuda(), B, SIZES)
    ul = ops.UnitLists(l32, l128)
    torch.cuda.synchronize()
    f32, f128 = U.unit_flags(pm, B, SIZES, 32), U.unit_flags(pm, B, SIZES, 128)
    assert np.array_equal(l32.cpu().numpy(), f32) and np.array_equal(l128.cpu().numpy(), f128)
    units, n = U.unit_lists(f32)
    counts = ul.counts.cpu().numpy()
    got = ul.units.cpu().numpy()
    for r in range(6):
        n128 = int(f128[r].sum())
        assert counts[r].tolist() == [n[r], n128, int(16 * ((n[r] + 3) // 4) <= 15 * n128), 0], (kind, r, counts[r])
        assert np.array_equal(got[r, :n[r]], units[r]), (kind, r)
    if kind == 'corner':
        assert counts[:, 2].tolist() == [0] * 6               # 1 .. 6 units of ONE tile gather into one or two tiles: nothing saved
    if kind in ('empty', 'full'):
        assert counts[:, 2].tolist() == [1 if kind == 'empty' else 0] * 6


def test_lists_beyond_one_scan_run():
    """more than 2048 flags per radius (the kernel walks runs of 256 threads x 8 flags) and a count that is no multiple of 8"""
    from efficientdet.pytorch_amd import ops
    S, T = 5001, 1251
    g = torch.Generator().manual_seed(4)
    l32 = (torch.rand(6, S, generator=g) < 0.3).to(torch.uint8)
    l128 = (torch.rand(6, T, generator=g) < 0.5).to(torch.uint8)
    ul = ops.UnitLists(l32.cuda(), l128.cuda())
    torch.cuda.synchronize()
    for r in range(6):
        want = torch.nonzero(l32[r]).reshape(-1).to(torch.int32)
        n = int(ul.counts[r, 0])
        assert n == want.numel() and int(ul.counts[r, 1]) == int(l128[r].sum())
        assert torch.equal(ul.units[r, :n].cpu(), want)


# ------------------------------------------------------------------------------------------------------- flags of a hand-made pattern
def _flag_set(pattern, gather=1):
    """-> (tile flags [21], (unit flags [84], list [84] with a poisoned tail, counts [4]), kept rows [2688] bool) on the device"""
    units = PATTERNS[pattern]
    f32 = torch.zeros(NSTEP, dtype=torch.uint8)
    f32[units] = 1
    f128 = torch.zeros(NTILE, dtype=torch.uint8)
    keep = torch.zeros(ROWS, dtype=torch.bool)
    tile0 = [0, 16, 20]
    for u in units:
        l = 2 if u >= 80 else (1 if u >= 64 else 0)
        f128[tile0[l] + (u - STEP0[l]) // 4] = 1
        keep[32 * u:32 * u + 32] = True                      # (every level is whole units: row = 32 * unit in the level-major buffer)
    lst = torch.full((NSTEP,), 0x7fffffff, dtype=torch.int32)
    lst[:len(units)] = torch.tensor(units, dtype=torch.int32)
    counts = torch.tensor([len(units), int(f128.sum()), gather, 0], dtype=torch.int32)
    return f128.cuda(), (f32.cuda(), lst.cuda(), counts.cuda()), keep.cuda()


def _hsplit_pair(C, gen, relu=True):
    """two random pyramids in the H-split layout, pairwise in one buffer"""
    from efficientdet.pytorch_amd import ops, functional as Fn
    _, xa, xb = Fn.pyramid_alloc_pair(B, SIZES, C, torch.float32, 'cuda')
    for m in xa + xb:
        src = torch.randn(m.B, m.H, m.W, C, generator=gen)
        ops.to_split2((torch.relu(src) if relu else src).cuda(), None, m.addr(), src.numel(), None)
    return xa, xb


def _split_pair(C, gen, relu=False):
    """two random pyramids in the split layout, pairwise in one buffer -> (flat, maps a, maps b)"""
    from efficientdet.pytorch_amd import ops, functional as Fn
    flat, xa, xb = Fn.pyramid_alloc_pair(B, SIZES, C, torch.float32, 'cuda')
    for m in xa + xb:
        src = torch.randn(m.B, m.H, m.W, C, generator=gen)
        ops.to_split2((torch.relu(src) if relu else src).cuda(), m.addr(), None, src.numel(), None)
    return flat, xa, xb


def _expect(dense, keep, first_rows=0):
    """the dense launch's rows where kept (and in the dense first tower), zero bytes elsewhere"""
    k = torch.cat([torch.ones(first_rows, dtype=torch.bool, device=keep.device), keep]).unsqueeze(1)
    return torch.where(k, dense, torch.zeros_like(dense))


# ------------------------------------------------------------------------------------------------------- forward: needed flags, f16x3
_FWD = {}


def _fwd_case(cin):
    from efficientdet.pytorch_amd import ops
    if cin not in _FWD:
        g = torch.Generator().manual_seed(300 + cin)
        xa, xb = _hsplit_pair(cin, g)
        ws = [ops.pack_weight((torch.randn(256, cin, 3, 3, generator=g) / (9 * cin) ** 0.5).cuda(), torch.float32, h3=True) for _ in range(2)]
        bs = [(torch.randn(256, generator=g) * 0.1).cuda() for _ in range(2)]
        case = dict(x=xa + xb, w=ws, b=bs)
        case['dense'] = _run_fwd(case, None, None)
        _FWD[cin] = case
    return _FWD[cin]


def _run_fwd(case, needed, units):
    """the paired tower layer: classification tower dense in front (tile0 = 21), the regression tower flagged -> (y, ysplit) as int32 rows"""
    from efficientdet.pytorch_amd import ops, functional as Fn
    cin = case['x'][0].C
    yf, ya, yb = Fn.pyramid_alloc_pair(B, SIZES, 256, torch.float32, 'cuda')
    sf, sa, sb = Fn.pyramid_alloc_pair(B, SIZES, 256, torch.float32, 'cuda')
    yf.view(torch.int32).fill_(NAN_BITS); sf.view(torch.int32).fill_(NAN_BITS)
    n = len(SIZES)
    ops.conv2d(case['x'], case['w'][0], ya + yb, Cin=cin, Cout=256, KH=3, KW=3, pad_t=1, pad_l=1, shift=case['b'][0], act=ops.ACT_RELU,
               hsplit=True, ysplit=sa + sb, seg_w=[case['w'][0]] * n + [case['w'][1]] * n, seg_shift=[case['b'][0]] * n + [case['b'][1]] * n,
               needed=needed, needed_tile0=NTILE if needed is not None else 0, units=units)
    torch.cuda.synchronize()
    return yf.view(torch.int32).view(-1, 256), sf.view(torch.int32).view(-1, 256)


@pytest.mark.parametrize('cin', [256, 64])
@pytest.mark.parametrize('pattern', list(PATTERNS))
def test_forward_paired_launch_gathers_the_needed_units(cin, pattern):
    case = _fwd_case(cin)
    f128, units, keep = _flag_set(pattern)
    got = _run_fwd(case, f128, units)
    for name, d, y in zip(('y', 'ysplit'), case['dense'], got):
        assert not bool((d == NAN_BITS).any()) and bool((d[ROWS:] != 0).any(dim=1).all()), name
        assert torch.equal(y, _expect(d, keep, ROWS)), (name, pattern)


def test_forward_falls_back_to_the_tile_flags_on_the_devices_word():
    """counts[2] == 0, read on the device: the launch with the tile flags alone -- whole tiles computed, never a dense launch"""
    case = _fwd_case(64)
    f128, units, _ = _flag_set('seven', gather=0)
    got = _run_fwd(case, f128, units)
    keep = f128.bool().repeat_interleave(128)
    for d, y in zip(case['dense'], got):
        assert torch.equal(y, _expect(d, keep, ROWS))


_FINAL = {}


def _run_final(case, needed, units):
    from efficientdet.pytorch_amd import ops, functional as Fn
    apix = sum(h * w for h, w in SIZES)
    reg = torch.empty(B, apix * 9, 4, device='cuda')
    reg.view(torch.int32).fill_(NAN_BITS)
    ops.conv2d(case['x'], case['w'], Fn.head_out_maps(reg, B, SIZES, 4), Cin=256, Cout=36, KH=3, KW=3, pad_t=1, pad_l=1, shift=case['b'],
               out_f32=True, hsplit=True, needed=needed, units=units)
    torch.cuda.synchronize()
    return reg.view(torch.int32).view(B, apix, 36)


def _image_major(keep):
    """kept rows of the level-major buffer -> [B][pixels of an image] as retina_reg's fp32 rows are laid out"""
    out, o = [], 0
    for h, w in SIZES:
        out.append(keep[o:o + B * h * w].view(B, h * w)); o += B * h * w
    return torch.cat(out, dim=1)


@pytest.mark.parametrize('pattern', list(PATTERNS))
def test_forward_final_layer_fp32_rows(pattern):
    """256 -> 36 with bias into the [B, A, 4] buffer (image-major fp32 rows of 36, the 64-channel tile), tile0 = 0"""
    from efficientdet.pytorch_amd import ops
    if not _FINAL:
        g = torch.Generator().manual_seed(9)
        _FINAL.update(x=_hsplit_pair(256, g)[0], b=(torch.randn(36, generator=g) * 0.1 + 1.0).cuda(),
                      w=ops.pack_weight((torch.randn(36, 256, 3, 3, generator=g) / 48.0).cuda(), torch.float32, h3=True))
        _FINAL['dense'] = _run_final(_FINAL, None, None)
    f128, units, keep = _flag_set(pattern)
    got = _run_final(_FINAL, f128, units)
    dense = _FINAL['dense']
    assert not bool((dense == NAN_BITS).any()) and bool((dense != 0).any(dim=2).all())
    k = _image_major(keep).unsqueeze(2)
    assert torch.equal(got, torch.where(k, dense, torch.zeros_like(dense))), pattern


# ------------------------------------------------------------------------------------------------------- backward: live flags, split layout
_BWD = {}


def _bwd_case(cin):
    """the paired data gradient cin -> 256 with the ReLU mask of the producing layer: dz and mask random, own weights per tower"""
    from efficientdet.pytorch_amd import ops
    if cin not in _BWD:
        g = torch.Generator().manual_seed(500 + cin)
        _, xa, xb = _split_pair(cin, g)
        _, ra, rb = _split_pair(256, g, relu=True)
        ws = [ops.pack_weight((torch.randn(256, cin, 3, 3, generator=g) / (9 * cin) ** 0.5).cuda(), torch.float32, x3=True) for _ in range(2)]
        case = dict(x=xa + xb, w=ws, res=ra + rb)
        case['dense'] = _run_bwd(case, None, None)
        _BWD[cin] = case
    return _BWD[cin]


def _run_bwd(case, live, units):
    from efficientdet.pytorch_amd import ops, functional as Fn
    cin = case['x'][0].C
    yf, ya, yb = Fn.pyramid_alloc_pair(B, SIZES, 256, torch.float32, 'cuda')
    yf.view(torch.int32).fill_(NAN_BITS)
    n = len(SIZES)
    ops.conv2d(case['x'], case['w'][0], ya + yb, Cin=cin, Cout=256, KH=3, KW=3, pad_t=1, pad_l=1, split=True, res=case['res'],
               res_mode=ops.RES_RELU_MASK, seg_w=[case['w'][0]] * n + [case['w'][1]] * n, live=live, live_tile0=NTILE if live is not None else 0,
               units=units)
    torch.cuda.synchronize()
    return yf.view(torch.int32).view(-1, 256)


@pytest.mark.parametrize('cin', [256, 64])
@pytest.mark.parametrize('pattern', list(PATTERNS))
def test_backward_paired_relu_mask_launch_gathers_the_live_units(cin, pattern):
    case = _bwd_case(cin)
    f128, units, keep = _flag_set(pattern)
    got = _run_bwd(case, f128, units)
    d = case['dense']
    assert not bool((d == NAN_BITS).any()) and bool((d[ROWS:] != 0).any(dim=1).all())
    assert torch.equal(got, _expect(d, keep, ROWS)), pattern


_ADD = {}


def _run_add(case, live, units):
    """256 -> 64 back to the neck: plain fp32 rows, added in place onto what the other tower left there"""
    from efficientdet.pytorch_amd import ops, functional as Fn
    flat, maps = Fn.pyramid_alloc(B, SIZES, 64, torch.float32, 'cuda')
    flat.copy_(case['before'])
    ops.conv2d(case['x'], case['w'], maps, Cin=256, Cout=64, KH=3, KW=3, pad_t=1, pad_l=1, res=maps, res_mode=ops.RES_ADD, split=True,
               out_f32=True, live=live, units=units)
    torch.cuda.synchronize()
    return flat.view(torch.int32).view(-1, 64)


@pytest.mark.parametrize('pattern', list(PATTERNS))
def test_backward_in_place_add_touches_the_live_units_only(pattern):
    from efficientdet.pytorch_amd import ops
    if not _ADD:
        g = torch.Generator().manual_seed(11)
        _ADD.update(x=_split_pair(256, g)[1], before=torch.randn(ROWS * 64, generator=g).cuda(),
                    w=ops.pack_weight((torch.randn(64, 256, 3, 3, generator=g) / 48.0).cuda(), torch.float32, x3=True))
        _ADD['dense'] = _run_add(_ADD, None, None)
    f128, units, keep = _flag_set(pattern)
    got = _run_add(_ADD, f128, units)
    before = _ADD['before'].view(torch.int32).view(-1, 64)
    assert bool((_ADD['dense'] != before).any(dim=1).all())
    assert torch.equal(got, torch.where(keep.unsqueeze(1), _ADD['dense'], before)), pattern


def test_a_launch_that_takes_no_flags_is_refused():
    """the gathered entry points never fall back to a dense launch: an exact-fp32 conv (no flagged kernel) raises"""
    from efficientdet.pytorch_amd import ops, functional as Fn
    _, xs = Fn.pyramid_alloc(B, SIZES, 64, torch.float32, 'cuda')
    _, ys = Fn.pyramid_alloc(B, SIZES, 64, torch.float32, 'cuda')
    w = ops.pack_weight(torch.randn(64, 64, 3, 3).cuda(), torch.float32)
    f128, units, _ = _flag_set('seven')
    with pytest.raises(RuntimeError):
        ops.conv2d(xs, w, ys, Cin=64, Cout=64, KH=3, KW=3, pad_t=1, pad_l=1, live=f128, units=units)


def test_partial_units_of_small_levels():
    """B = 3 with levels 16x16 .. 1x1: M = 768, 192, 48, 12, 3 pixels -> 24 + 6 + 2 + 1 + 1 units, the last unit of the three coarse levels
    partial (16, 12 and 3 pixels), 11 tiles.  The paired forward layer with five units flagged, the partial ones among them: their rows
    hold the dense bytes, every other row of the tower is zero bytes, and nothing is written past a level's last pixel (the next level's
    rows follow it in the buffer)."""
    from efficientdet.pytorch_amd import ops, functional as Fn
    b3, sizes = 3, [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]
    M = [b3 * h * w for h, w in sizes]
    step0, row0, tile0 = [0, 24, 30, 32, 33], [0, 768, 960, 1008, 1020], [0, 6, 8, 9, 10]
    rows, nstep, ntile = sum(M), 34, 11
    units = [5, 29, 31, 32, 33]
    f32 = torch.zeros(nstep, dtype=torch.uint8); f32[units] = 1
    f128 = torch.zeros(ntile, dtype=torch.uint8)
    keep = torch.zeros(rows, dtype=torch.bool)
    for u in units:
        l = max(i for i in range(5) if u >= step0[i])
        f128[tile0[l] + (u - step0[l]) // 4] = 1
        lo = 32 * (u - step0[l])
        keep[row0[l] + lo:row0[l] + min(lo + 32, M[l])] = True
    lst = torch.full((nstep,), 0x7fffffff, dtype=torch.int32); lst[:5] = torch.tensor(units, dtype=torch.int32)
    counts = torch.tensor([5, int(f128.sum()), 1, 0], dtype=torch.int32)
    g = torch.Generator().manual_seed(77)
    _, xa, xb = Fn.pyramid_alloc_pair(b3, sizes, 64, torch.float32, 'cuda')
    for m in xa + xb:
        src = torch.relu(torch.randn(m.B, m.H, m.W, 64, generator=g)).cuda()
        ops.to_split2(src, None, m.addr(), src.numel(), None)
    ws = [ops.pack_weight((torch.randn(256, 64, 3, 3, generator=g) / 24.0).cuda(), torch.float32, h3=True) for _ in range(2)]
    bs = [(torch.randn(256, generator=g) * 0.1).cuda() for _ in range(2)]

    def run(**kw):
        yf, ya, yb = Fn.pyramid_alloc_pair(b3, sizes, 256, torch.float32, 'cuda')
        sf, sa, sb = Fn.pyramid_alloc_pair(b3, sizes, 256, torch.float32, 'cuda')
        yf.view(torch.int32).fill_(NAN_BITS); sf.view(torch.int32).fill_(NAN_BITS)
        ops.conv2d(xa + xb, ws[0], ya + yb, Cin=64, Cout=256, KH=3, KW=3, pad_t=1, pad_l=1, shift=bs[0], act=ops.ACT_RELU, hsplit=True,
                   ysplit=sa + sb, seg_w=[ws[0]] * 5 + [ws[1]] * 5, seg_shift=[bs[0]] * 5 + [bs[1]] * 5, **kw)
        torch.cuda.synchronize()
        return yf.view(torch.int32).view(-1, 256), sf.view(torch.int32).view(-1, 256)
    dense = run()
    got = run(needed=f128.cuda(), needed_tile0=ntile, units=(f32.cuda(), lst.cuda(), counts.cuda()))
    k = torch.cat([torch.ones(rows, dtype=torch.bool), keep]).cuda().unsqueeze(1)
    for d, y in zip(dense, got):
        assert not bool((d == NAN_BITS).any())
        assert torch.equal(y, torch.where(k, d, torch.zeros_like(d)))
