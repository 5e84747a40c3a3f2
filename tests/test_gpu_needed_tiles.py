"""Sparse forward pass of the RetinaHead's regression tower, op level (include/effdet_needed_tiles.h).

Three entry points: the positive-pixel map of the default matcher (against the codes the loss's own assign pass leaves in its
workspace), the flags derived from such a map (against ops.live_tiles on a d(reg) that is non-zero exactly there), and the f16x3 conv
launch that skips the tiles nobody reads (needed tiles: the dense launch's bytes; every other tile: zero bytes in every output stream).
Every comparison is exact.

Small geometry: B = 3 with levels 16x16, 8x8, 4x4 -> 6 + 2 + 1 tiles of 128 pixels, the last tile of each coarse level partial; the
ten-segment launches add 2x2 and 1x1 levels (two more partial tiles)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B3 = 3
SIZES = [(16, 16), (8, 8), (4, 4)]
SIZES5 = SIZES + [(2, 2), (1, 1)]
NAN_BITS = 0x7fc07fc0            # NaN as fp32 and as either 16-bit half: a row nobody wrote shows


def _poff(sizes):
    out, o = [], 0
    for (h, w) in sizes:
        out.append(o); o += h * w
    return out, o


# ------------------------------------------------------------------------------------------------------- positive-pixel map
def _anchors3():
    """the anchor table of a 128 x 128 image cut to its first three levels (16x16, 8x8, 4x4) -> [1, A, 4] on the device"""
    from efficientdet.pytorch_amd import ops
    _, apix = _poff(SIZES)
    return ops.anchors(128, 128, 'cuda')[:, :9 * apix].contiguous()


def _iou32(an, box):
    """assign_iou restated in separately rounded fp32 steps (host)"""
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    ax1, ay1, ax2, ay2 = [f(float(v)) for v in an]
    bx1, by1, bx2, by2 = [f(float(v)) for v in box]
    aarea = (ax2 - ax1) * (ay2 - ay1); barea = (bx2 - bx1) * (by2 - by1)
    iw = (torch.minimum(ax2, bx2) - torch.maximum(ax1, bx1)).clamp(min=0); ih = (torch.minimum(ay2, by2) - torch.maximum(ay1, by1)).clamp(min=0)
    ua = (aarea + barea - iw * ih).clamp(min=1e-8)
    return float(iw * ih / ua)


def _annots(case, anc):
    """-> ([3, N, 5] annotations, anchors that must come out positive as (image, anchor index))"""
    g = torch.Generator().manual_seed(21)
    a = anc[0].cpu()
    must = []
    if case == 'few_boxes':
        ann = torch.full((B3, 4, 5), -1.0)
        for b in range(B3):
            for n in range(3):
                x1, y1 = (torch.rand(2, generator=g) * 70).tolist()
                w, h = (14 + torch.rand(2, generator=g) * 50).tolist()
                ann[b, n + (b == 1)] = torch.tensor([x1, y1, min(x1 + w, 127.0), min(y1 + h, 127.0), float(n)])      # (image 1: the pad row first)
    elif case == 'padding_image':
        ann = torch.full((B3, 3, 5), -1.0)
        ann[0, 0] = torch.tensor([10.0, 20.0, 60.0, 70.0, 1.0]); ann[2, 2] = torch.tensor([64.0, 64.0, 127.0, 127.0, 0.0])
        ann[1, :, :4] = torch.tensor([10.0, 20.0, 60.0, 70.0])                   # image 1: boxes that would match, every label -1
    elif case == 'box_is_an_anchor':
        ann = torch.full((B3, 2, 5), -1.0)
        for b, k in enumerate((9 * 100 + 4, 9 * (256 + 20) + 1, 9 * (256 + 64 + 5) + 8)):
            ann[b, 1, :4] = a[k]; ann[b, 1, 4] = 2.0
            must.append((b, k))
    elif case == 'iou_exactly_half':
        # the upper half of an anchor: intersection = the box, union = the anchor.  Taken from the anchors for which the restated fp32
        # arithmetic gives exactly 0.5 (power-of-two sizes do)
        ann = torch.full((B3, 1, 5), -1.0)
        found = None
        for k in range(9 * 120, 9 * 136):
            x1, y1, x2, y2 = a[k].tolist()
            box = [x1, y1, x2, y1 + (y2 - y1) / 2]
            if min(x1, y1) >= 0 and _iou32(a[k], torch.tensor(box)) == 0.5:
                found = (k, box); break
        assert found is not None
        ann[1, 0] = torch.tensor(found[1] + [3.0])
        must.append((1, found[0]))
    else:
        assert case == 'second_chunk'
        ann = torch.full((B3, 70, 5), -1.0)
        xy = torch.rand(70, 2, generator=g) * 90; wh = 10 + torch.rand(70, 2, generator=g) * 36
        ann[0, :, :2] = xy; ann[0, :, 2:4] = (xy + wh).clamp(max=127.0); ann[0, :, 4] = (torch.arange(70) % 8).float()
        k = 9 * 77 + 4
        ann[1, 68, :4] = a[k]; ann[1, 68, 4] = 5.0                               # image 1: its only valid row sits in the second chunk
        ann[2, 3] = ann[0, 3]; ann[2, 66] = ann[0, 66]
        must.append((1, k))
    return ann, must


@pytest.mark.parametrize('case', ['few_boxes', 'padding_image', 'box_is_an_anchor', 'iou_exactly_half', 'second_chunk'])
def test_positive_pixel_map_equals_the_assign_pass(case):
    from efficientdet.pytorch_amd import ops
    anc = _anchors3()
    A = anc.shape[1]
    ann, must = _annots(case, anc)
    ann = ann.cuda()
    g = torch.Generator().manual_seed(1)
    cls = torch.rand(B3, A, 8, generator=g).clamp(1e-3, 1 - 1e-3).cuda()
    reg = (torch.randn(B3, A, 4, generator=g) * 0.3).cuda()
    _, ws = ops.focal_loss_fwd(cls, reg, anc, ann)
    pm = ops.positive_pixel_map(anc, ann, SIZES)
    torch.cuda.synchronize()
    assign = ws[:B3 * A * 4].view(torch.int32).view(B3, A)                       # the codes of the assign pass: >= 0 positive
    for b, k in must:
        assert int(assign[b, k]) >= 0, (case, b, k)
    poff, _ = _poff(SIZES)
    want = torch.cat([(assign[:, 9 * poff[l]:9 * (poff[l] + h * w)] >= 0).view(B3, h * w, 9).any(dim=2).reshape(-1)
                      for l, (h, w) in enumerate(SIZES)]).to(torch.uint8)
    assert torch.equal(pm, want), case
    if case == 'padding_image':
        assert not bool(pm.view(-1)[256:512].any()) and bool(pm.any())           # level 0 of image 1
    else:
        assert bool(pm.any()) and not bool(pm.all())


# ------------------------------------------------------------------------------------------------------- flags from a map
def _map_to_rows(pm, ld=64):
    """level-major byte map -> [B][sum H*W][ld] fp32 rows, non-zero (one channel) exactly at the map's pixels"""
    poff, apix = _poff(SIZES)
    d = torch.zeros(B3, apix, ld, device=pm.device)
    o = 0
    for l, (h, w) in enumerate(SIZES):
        d[:, poff[l]:poff[l] + h * w, (5 * l) % 36] = pm[o:o + B3 * h * w].view(B3, h * w).float() * -1.5
        o += B3 * h * w
    return d


@pytest.mark.parametrize('src', ['boxes', 'corners', 'none', 'all'])
def test_flags_from_a_map_equal_the_flags_from_dreg(src):
    from efficientdet.pytorch_amd import ops
    _, apix = _poff(SIZES)
    if src == 'boxes':
        anc = _anchors3()
        pm = ops.positive_pixel_map(anc, _annots('few_boxes', anc)[0].cuda(), SIZES)
    else:
        pm = torch.full((B3 * apix,), 1 if src == 'all' else 0, dtype=torch.uint8)
        if src == 'corners':
            pm[0] = 7; pm[7 * 16 + 15] = 1; pm[256 + 255] = 255; pm[3 * 256 + 63] = 1; pm[3 * 256 + 3 * 64 + 47] = 1      # (any non-zero byte counts)
        pm = pm.cuda()
    l32, l128 = ops.live_tiles_from_map(pm, B3, SIZES)
    d = _map_to_rows(pm)
    for split in (False, True):
        r32, r128 = ops.live_tiles(ops.to_split(d) if split else d, B3, SIZES, 64, split)
        torch.cuda.synchronize()
        assert torch.equal(l32, r32) and torch.equal(l128, r128), (src, split)
    if src == 'boxes':                                                           # the two calls in one
        assert torch.equal(ops.needed_tiles(anc, _annots('few_boxes', anc)[0].cuda(), B3, SIZES), l128)
    if src in ('boxes', 'corners'):
        assert bool((l128[0] == 0).any()) and bool(l128[0].any())


# ------------------------------------------------------------------------------------------------------- needed-tile conv launches
def _tile_rows(sizes):
    """[(first pixel row, rows)] of every 128-pixel tile of a level-major buffer, levels in order"""
    out, row0 = [], 0
    for (h, w) in sizes:
        M = B3 * h * w
        out += [(row0 + t, min(128, M - t)) for t in range(0, M, 128)]
        row0 += M
    return out, row0


def _patterns(sizes):
    tiles, _ = _tile_rows(sizes)
    n = len(tiles)
    partial = torch.tensor([1 if r < 128 else 0 for _, r in tiles], dtype=torch.uint8)
    assert 0 < int(partial.sum()) < n
    return {'all': torch.ones(n, dtype=torch.uint8), 'none': torch.zeros(n, dtype=torch.uint8),
            'alternating': (torch.arange(n) % 2).to(torch.uint8), 'partial_only': partial}


def _hsplit_pair(sizes, C, gen):
    """two random pyramids (relu-like: half the values zero) in the H-split layout, pairwise in one buffer"""
    from efficientdet.pytorch_amd import ops, functional as Fn
    _, xa, xb = Fn.pyramid_alloc_pair(B3, sizes, C, torch.float32, 'cuda')
    for m in xa + xb:
        src = torch.relu(torch.randn(m.B, m.H, m.W, C, generator=gen)).cuda()
        ops.to_split2(src, None, m.addr(), src.numel(), None)
    return xa, xb


_PAIRED = {}


def _paired_case(cin):
    """operands and the DENSE outputs of the ten-segment launch (two towers x five levels, own weights and bias each), computed once"""
    from efficientdet.pytorch_amd import ops, functional as Fn
    if cin not in _PAIRED:
        g = torch.Generator().manual_seed(100 + cin)
        xa, xb = _hsplit_pair(SIZES5, cin, g)
        ws = [ops.pack_weight((torch.randn(256, cin, 3, 3, generator=g) / (9 * cin) ** 0.5).cuda(), torch.float32, h3=True) for _ in range(2)]
        bs = [(torch.randn(256, generator=g) * 0.1).cuda() for _ in range(2)]
        case = dict(x=xa + xb, w=ws, b=bs)
        case['dense'] = _run_paired(case, None)
        _PAIRED[cin] = case
    return _PAIRED[cin]


def _run_paired(case, needed):
    from efficientdet.pytorch_amd import ops, functional as Fn
    cin = case['x'][0].C
    ntile = len(_tile_rows(SIZES5)[0])
    yf, ya, yb = Fn.pyramid_alloc_pair(B3, SIZES5, 256, torch.float32, 'cuda')
    sf, sa, sb = Fn.pyramid_alloc_pair(B3, SIZES5, 256, torch.float32, 'cuda')
    yf.view(torch.int32).fill_(NAN_BITS); sf.view(torch.int32).fill_(NAN_BITS)
    ops.conv2d(case['x'], case['w'][0], ya + yb, Cin=cin, Cout=256, KH=3, KW=3, pad_t=1, pad_l=1, shift=case['b'][0], act=ops.ACT_RELU,
               hsplit=True, ysplit=sa + sb, seg_w=[case['w'][0]] * 5 + [case['w'][1]] * 5, seg_shift=[case['b'][0]] * 5 + [case['b'][1]] * 5,
               needed=needed, needed_tile0=ntile if needed is not None else 0)
    torch.cuda.synchronize()
    return yf.view(torch.int32).view(-1, 256), sf.view(torch.int32).view(-1, 256)      # one row per pixel: tower A's levels, then tower B's


@pytest.mark.parametrize('cin', [256, 64])
@pytest.mark.parametrize('pattern', ['all', 'none', 'alternating', 'partial_only'])
def test_paired_launch_computes_the_needed_tiles_and_zeroes_the_rest(cin, pattern):
    """Both output streams (H-split y, split twin), row by row: the first tower (below needed_tile0) and the needed tiles of the second
    hold the dense launch's bytes, every other row of the second tower is zero bytes."""
    case = _paired_case(cin)
    flags = _patterns(SIZES5)[pattern]
    tiles, rows = _tile_rows(SIZES5)
    got = _run_paired(case, flags.cuda())
    keep = torch.ones(2 * rows, dtype=torch.bool)
    for (r0, n), f in zip(tiles, flags.tolist()):
        keep[rows + r0:rows + r0 + n] = bool(f)
    keep = keep.cuda().unsqueeze(1)
    for name, d, y in zip(('y', 'ysplit'), case['dense'], got):
        assert not bool((d == NAN_BITS).any()), name                           # the dense launch wrote every row
        assert bool((d[rows:] != 0).any(dim=1).all()), name                    # ... and no row of it is all zero (bias + ReLU of 256 channels)
        assert torch.equal(y, torch.where(keep, d, torch.zeros_like(d))), (name, pattern)


_FINAL = {}


def _run_final(case, needed):
    from efficientdet.pytorch_amd import ops, functional as Fn
    _, apix = _poff(SIZES)
    reg = torch.empty(B3, apix * 9, 4, device='cuda')
    reg.view(torch.int32).fill_(NAN_BITS)
    ops.conv2d(case['x'], case['w'], Fn.head_out_maps(reg, B3, SIZES, 4), Cin=256, Cout=36, KH=3, KW=3, pad_t=1, pad_l=1, shift=case['b'],
               out_f32=True, hsplit=True, needed=needed)
    torch.cuda.synchronize()
    return reg.view(torch.int32).view(B3, apix, 36)


@pytest.mark.parametrize('pattern', ['all', 'none', 'alternating', 'partial_only'])
def test_final_layer_fp32_rows(pattern):
    """256 -> 36 with bias into the [B, A, 4] buffer (image-major fp32 rows of 36, the 64-channel tile): needed tiles equal the dense
    launch, the rows of every other tile are zeros, tile0 = 0."""
    from efficientdet.pytorch_amd import ops
    if not _FINAL:
        g = torch.Generator().manual_seed(7)
        _FINAL.update(x=_hsplit_pair(SIZES, 256, g)[0], b=(torch.randn(36, generator=g) * 0.1 + 1.0).cuda(),
                      w=ops.pack_weight((torch.randn(36, 256, 3, 3, generator=g) / 48.0).cuda(), torch.float32, h3=True))
        _FINAL['dense'] = _run_final(_FINAL, None)
    flags = _patterns(SIZES)[pattern]
    got = _run_final(_FINAL, flags.cuda())
    dense = _FINAL['dense']
    poff, apix = _poff(SIZES)
    keep = torch.zeros(B3, apix, dtype=torch.bool)
    fl = flags.tolist()
    for l, (h, w) in enumerate(SIZES):
        M = B3 * h * w
        lv = torch.zeros(M, dtype=torch.bool)
        for t in range(0, M, 128):
            lv[t:t + 128] = bool(fl.pop(0))
        keep[:, poff[l]:poff[l] + h * w] = lv.view(B3, h * w)
    assert not fl
    keep = keep.cuda().unsqueeze(2)
    assert not bool((dense == NAN_BITS).any()) and bool((dense != 0).any(dim=2).all())
    assert torch.equal(got, torch.where(keep, dense, torch.zeros_like(dense))), pattern
