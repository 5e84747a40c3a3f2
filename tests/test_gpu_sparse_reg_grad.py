"""Sparse backward pass of the RetinaHead's regression tower (include/effdet_live_tiles.h; functional.HEAD_SPARSE_REG).

d(reg) is an exact zero away from the positive anchors; ops.live_tiles turns it into byte flags per 32-pixel step and 128-pixel tile for
dilation radii 0..5, and the split-layout data- and weight-gradient kernels skip the units whose flag is 0.  Checked here: the flags
against a torch restatement (per-image max_pool2d dilation, OR over each unit), flagged launches against unflagged ones bit for bit
(outputs pre-filled with NaN, so a dead tile nobody wrote shows), the reach of a chain of five 3x3 convs against the flags of its
radius, and the whole model with the switch on and off.

Small geometry: B = 3 with levels 16x16, 8x8, 4x4 -> M = 768 (six 128-pixel tiles), 192 (one and a half), 48 (one partial tile that
spans all three images); the ten-segment launch adds 2x2 and 1x1 levels."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

B3 = 3
SIZES = [(16, 16), (8, 8), (4, 4)]
LD = 64
RADII = 6


def _poff(sizes):
    out, o = [], 0
    for (h, w) in sizes:
        out.append(o); o += h * w
    return out, o


def _dreg(B, sizes, points, value=1.0, fill=0.0):
    """[B][sum H*W][LD] fp32 rows, `fill` everywhere but channel (7 * i) % 36 of the pixels points[i] = (level, b, h, w)."""
    poff, apix = _poff(sizes)
    d = torch.full((B, apix, LD), fill)
    for i, (l, b, h, w) in enumerate(points):
        d[b, poff[l] + h * sizes[l][1] + w, (7 * i) % 36] = value
    return d


def _nz_maps(d, B, sizes):
    """per level the [B, H, W] map of pixels with a word that has a bit outside the sign bit"""
    poff, _ = _poff(sizes)
    bits = d.contiguous().view(torch.int32) & 0x7fffffff
    px = (bits != 0).any(dim=2)
    return [px[:, poff[l]:poff[l] + h * w].reshape(B, h, w) for l, (h, w) in enumerate(sizes)]


def _ref_flags(nz, B, sizes):
    """torch reference: per radius, dilate every image with max_pool2d, then OR over each 32-pixel step / 128-pixel tile of the level's
    (b, h, w) pixel index -> (live32 [6][steps], live128 [6][tiles]) uint8"""
    r32, r128 = [], []
    for r in range(RADII):
        s32, s128 = [], []
        for m in nz:
            dil = F.max_pool2d(m.float().unsqueeze(1), 2 * r + 1, 1, r).reshape(-1) > 0
            for unit, dst in ((32, s32), (128, s128)):
                n = (dil.numel() + unit - 1) // unit
                pad = torch.zeros(n * unit, dtype=torch.bool); pad[:dil.numel()] = dil
                dst.append(pad.view(n, unit).any(dim=1))
        r32.append(torch.cat(s32)); r128.append(torch.cat(s128))
    return torch.stack(r32).to(torch.uint8), torch.stack(r128).to(torch.uint8)


CORNER = [(0, 1, 0, 0)]
TILE_END = [(0, 0, 7, 15)]            # level 0: the last column of the row that ends tile 0 -> tile 1 is live from radius 1 on
IMAGE_END = [(1, 0, 7, 7), (2, 1, 3, 3)]     # last pixel of an image that shares its tile with the next image
ALL = [(l, b, h, w) for l, (H, W) in enumerate(SIZES) for b in range(B3) for h in range(H) for w in range(W)]


@pytest.mark.parametrize('split', [False, True])
@pytest.mark.parametrize('name,points', [('corner', CORNER), ('tile_end', TILE_END), ('image_end', IMAGE_END), ('none', []), ('all', ALL),
                                         ('mixed', CORNER + TILE_END + IMAGE_END + [(0, 2, 9, 4), (1, 2, 0, 5)])])
def test_flags_match_the_torch_reference(name, points, split):
    from efficientdet.pytorch_amd import ops
    assert ops.wgrad_split_supported(B3, SIZES, 256, 256, 256) and ops.wgrad_split_supported(B3, SIZES, 256, 64, 64)
    d = _dreg(B3, SIZES, points, value=0.37)
    dev = ops.to_split(d.cuda()) if split else d.cuda()
    l32, l128 = ops.live_tiles(dev, B3, SIZES, LD, split)
    torch.cuda.synchronize()
    w32, w128 = _ref_flags(_nz_maps(d, B3, SIZES), B3, SIZES)
    assert l32.shape == w32.shape == (RADII, 24 + 6 + 2) and l128.shape == w128.shape == (RADII, 6 + 2 + 1)
    # (the kernel clips its window to the image, so it equals the reference everywhere -- which is also the superset the skip needs)
    assert torch.equal(l32.cpu(), w32), (name, (l32.cpu() != w32).nonzero().tolist())
    assert torch.equal(l128.cpu(), w128), (name, (l128.cpu() != w128).nonzero().tolist())
    if name == 'tile_end':
        assert l128[:, 1].tolist() == [0, 1, 1, 1, 1, 1]
    if name == 'none':
        assert not bool(l32.any()) and not bool(l128.any())
    if name == 'all':
        assert bool(l32.all()) and bool(l128.all())


@pytest.mark.parametrize('split', [False, True])
def test_nan_is_live_and_negative_zero_is_dead(split):
    from efficientdet.pytorch_amd import ops
    d = _dreg(B3, SIZES, [(0, 2, 15, 15)], value=float('nan'), fill=-0.0)
    assert bool((d.view(torch.int32) != 0).all())                         # every word has its sign bit set
    dev = ops.to_split(d.cuda()) if split else d.cuda()
    l32, l128 = ops.live_tiles(dev, B3, SIZES, LD, split)
    torch.cuda.synchronize()
    want = torch.zeros(B3, 16, 16, dtype=torch.bool); want[2, 15, 15] = True
    zero = [torch.zeros(B3, h, w, dtype=torch.bool) for (h, w) in SIZES[1:]]
    w32, w128 = _ref_flags([want] + zero, B3, SIZES)
    assert torch.equal(l32.cpu(), w32) and torch.equal(l128.cpu(), w128)
    assert int(l32[0].sum()) == 1 and int(l32[0, 23]) == 1 and int(l128[0, 5]) == 1


# ----------------------------------------------------------------------------------------------------------- flagged launches
def _sparse_rows(B, sizes, points, gen):
    """d(reg)-like rows: random values in the first 36 channels of the given pixels, exact zeros elsewhere"""
    poff, apix = _poff(sizes)
    d = torch.zeros(B, apix, LD)
    for (l, b, h, w) in points:
        d[b, poff[l] + h * sizes[l][1] + w, :36] = torch.randn(36, generator=gen)
    return d


def _row_maps(t, B, sizes):
    """the levels of a [B][sum H*W][LD] buffer as Maps (image-major: what head_bwd hands retina_reg's gradient launches)"""
    from efficientdet.pytorch_amd.ops import Map
    poff, apix = _poff(sizes)
    return [Map(t, B, h, w, LD, ld=LD, bstride=apix * LD, off=poff[l] * LD) for l, (h, w) in enumerate(sizes)]


def _split_pyramid(ts, B, sizes, C):
    """per-level NCHW host tensors -> level-major split-layout Maps"""
    from efficientdet.pytorch_amd import ops, functional as Fn
    _, maps = Fn.pyramid_alloc(B, sizes, C, torch.float32, 'cuda')
    for t, m in zip(ts, maps):
        Fn.level_tensor(m).copy_(ops.to_split(t.permute(0, 2, 3, 1).contiguous().cuda()))
    return maps


def _nan_pyramid(B, sizes, C):
    from efficientdet.pytorch_amd import functional as Fn
    flat, maps = Fn.pyramid_alloc(B, sizes, C, torch.float32, 'cuda')
    flat.view(torch.int32).fill_(0x7fc07fc0)          # NaN as fp32 and as bf16 hi | lo halves
    return flat, maps


def _support(flat, B, sizes, C):
    """per level the pixels of a level-major buffer (fp32 or split: same zero test) with a non-zero word -> unit flags like _ref_flags"""
    px, off = [], 0
    for (h, w) in sizes:
        n = B * h * w
        px.append(((flat[off * C:(off + n) * C].view(torch.int32) & 0x7fff7fff) != 0).view(n, C).any(dim=1).cpu())
        off += n
    out = []
    for unit in (32, 128):
        parts = []
        for p in px:
            n = (p.numel() + unit - 1) // unit
            pad = torch.zeros(n * unit, dtype=torch.bool); pad[:p.numel()] = p
            parts.append(pad.view(n, unit).any(dim=1))
        out.append(torch.cat(parts))
    return out


POINTS = [(0, 0, 0, 0), (0, 0, 7, 15), (0, 1, 15, 15), (1, 0, 7, 7), (1, 2, 3, 0), (2, 1, 3, 3)]


def test_data_gradient_chain_flagged_equals_dense_and_stays_inside_the_flags():
    """The five data gradients of the regression tower through ops with random weights and ReLU masks: 64 -> 256 (ReLU mask, flags of
    radius 1), three 256 -> 256 (radii 2, 3, 4; split in, split out, ReLU mask), 256 -> 64 added in place onto an fp32 map (radius 5).
    Every flagged launch writes into a NaN-filled buffer and must equal the unflagged one bit for bit; the measured support of every
    map lies inside the flags of its radius."""
    from efficientdet.pytorch_amd import ops, functional as Fn
    g = torch.Generator().manual_seed(11)
    d = _sparse_rows(B3, SIZES, POINTS, g)
    dz_rows = ops.to_split(d.cuda())
    l32, l128 = ops.live_tiles(dz_rows, B3, SIZES, LD, True)
    ops.set_f32_arith('bf16x3')
    try:
        cur = {False: _row_maps(dz_rows, B3, SIZES), True: _row_maps(dz_rows, B3, SIZES)}
        cin = LD
        for r in range(1, 5):
            w = torch.randn(256, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
            wp = ops.pack_weight(w.cuda(), torch.float32, x3=True)
            mask = _split_pyramid([F.relu(torch.randn(B3, 256, h, ww, generator=g)) for (h, ww) in SIZES], B3, SIZES, 256)
            outs = {}
            for flagged in (False, True):
                flat, ym = _nan_pyramid(B3, SIZES, 256)
                ops.conv2d(cur[flagged], wp, ym, Cin=cin, Cout=256, KH=3, KW=3, pad_t=1, pad_l=1, res=mask, res_mode=ops.RES_RELU_MASK,
                           split=True, live=l128[r] if flagged else None)
                outs[flagged] = (flat, ym)
            torch.cuda.synchronize()
            assert torch.equal(outs[True][0].view(torch.int32), outs[False][0].view(torch.int32)), 'radius %d' % r
            s32, s128 = _support(outs[False][0], B3, SIZES, 256)
            assert bool(s32.any()) and not bool((s32 & (l32[r].cpu() == 0)).any()) and not bool((s128 & (l128[r].cpu() == 0)).any()), r
            cur = {k: v[1] for k, v in outs.items()}
            cin = 256
        # back to a 64-channel fp32 map: dense without residual (the support), then added in place with and without flags
        w = torch.randn(64, 256, 3, 3, generator=g) / (256 * 9) ** 0.5
        wp = ops.pack_weight(w.cuda(), torch.float32, x3=True)
        kw = dict(Cin=256, Cout=64, KH=3, KW=3, pad_t=1, pad_l=1, split=True, out_f32=True)
        pflat, pm = _nan_pyramid(B3, SIZES, 64)
        ops.conv2d(cur[False], wp, pm, live=l128[5], **kw)                 # no residual: dead tiles are written as fp32 zeros
        dflat, dm = _nan_pyramid(B3, SIZES, 64)
        ops.conv2d(cur[False], wp, dm, **kw)
        base = torch.randn(pflat.numel(), generator=g).cuda()
        acc = {}
        for flagged in (False, True):
            flat, ym = Fn.pyramid_alloc(B3, SIZES, 64, torch.float32, 'cuda')
            flat.copy_(base)
            ops.conv2d(cur[flagged], wp, ym, res=ym, res_mode=ops.RES_ADD, live=l128[5] if flagged else None, **kw)
            acc[flagged] = flat
        torch.cuda.synchronize()
        assert torch.equal(pflat.view(torch.int32), dflat.view(torch.int32))
        assert torch.equal(acc[True].view(torch.int32), acc[False].view(torch.int32))
        s32, s128 = _support(dflat, B3, SIZES, 64)
        assert not bool((s128 & (l128[5].cpu() == 0)).any()) and bool((l128[5] == 0).any())
    finally:
        ops.set_f32_arith('f32')


def test_paired_launch_flags_only_the_second_tower():
    """Ten segments (two towers x five levels) in one launch, flags from the sixth segment on: the first tower's input is dense and its
    tiles carry no flag; the second tower's is sparse."""
    from efficientdet.pytorch_amd import ops, functional as Fn
    sizes = SIZES + [(2, 2), (1, 1)]
    g = torch.Generator().manual_seed(12)
    d = _sparse_rows(B3, sizes, POINTS + [(3, 1, 1, 1)], g)
    l32, l128 = ops.live_tiles(ops.to_split(d.cuda()), B3, sizes, LD, True)
    ntile = sum((B3 * h * w + 127) // 128 for (h, w) in sizes)
    assert l128.shape[1] == ntile == 11
    # second tower's input: random values on the pixels within distance 1 of the points (the flags of radius 2 then cover its taps)
    nz = _nz_maps(d, B3, sizes)
    ops.set_f32_arith('bf16x3')
    try:
        _, xa, xb = Fn.pyramid_alloc_pair(B3, sizes, 256, torch.float32, 'cuda')
        _, ra, rb = Fn.pyramid_alloc_pair(B3, sizes, 256, torch.float32, 'cuda')
        for l, (h, w) in enumerate(sizes):
            dense = torch.randn(B3, h, w, 256, generator=g)
            near = F.max_pool2d(nz[l].float().unsqueeze(1), 3, 1, 1).squeeze(1) > 0
            sparse = torch.randn(B3, h, w, 256, generator=g) * near.unsqueeze(-1)
            Fn.level_tensor(xa[l]).copy_(ops.to_split(dense.cuda())); Fn.level_tensor(xb[l]).copy_(ops.to_split(sparse.cuda()))
            for m in (ra[l], rb[l]):
                Fn.level_tensor(m).copy_(ops.to_split(F.relu(torch.randn(B3, h, w, 256, generator=g)).cuda()))
        ws = [ops.pack_weight((torch.randn(256, 256, 3, 3, generator=g) / 48.0).cuda(), torch.float32, x3=True) for _ in range(2)]
        outs = {}
        for flagged in (False, True):
            flat, ya, yb = Fn.pyramid_alloc_pair(B3, sizes, 256, torch.float32, 'cuda')
            flat.view(torch.int32).fill_(0x7fc07fc0)
            ops.conv2d(xa + xb, ws[0], ya + yb, Cin=256, Cout=256, KH=3, KW=3, pad_t=1, pad_l=1, res=ra + rb, res_mode=ops.RES_RELU_MASK,
                       split=True, seg_w=[ws[0]] * 5 + [ws[1]] * 5, live=l128[2] if flagged else None, live_tile0=ntile if flagged else 0)
            outs[flagged] = flat
        torch.cuda.synchronize()
    finally:
        ops.set_f32_arith('f32')
    assert bool((l128[2] == 0).any())
    assert torch.equal(outs[True].view(torch.int32), outs[False].view(torch.int32))
    assert not bool(torch.isnan(outs[False]).any())


@pytest.mark.parametrize('cout,lddz', [(36, 64), (256, 256)])
@pytest.mark.parametrize('pattern', ['ends', 'level1_only', 'scattered', 'all'])
def test_weight_gradient_flagged_equals_dense(cout, lddz, pattern):
    """Slabs and bias partial rows, bit for bit.  'ends': level 0 is non-zero only in the first and last step of each of its split-K
    ranges (steps 0, 15, 16, 23 for the 512-pixel chunks the planner gives this size, and robust to others); 'level1_only': every
    split of levels 0 and 2 has no live step and takes the zero-slab branch."""
    from efficientdet.pytorch_amd import ops
    g = torch.Generator().manual_seed(cout)
    pts = {'ends': [(0, 0, 0, 0), (0, 1, 15, 15), (0, 2, 0, 0), (0, 2, 15, 15)], 'level1_only': [(1, 1, 2, 3), (1, 2, 7, 7)],
           'scattered': POINTS, 'all': ALL}[pattern]
    poff, apix = _poff(SIZES)
    nzpix = torch.zeros(B3, apix, dtype=torch.bool)
    for (l, b, h, w) in pts:
        nzpix[b, poff[l] + h * SIZES[l][1] + w] = True
    xs = _split_pyramid([torch.randn(B3, 256, h, w, generator=g) for (h, w) in SIZES], B3, SIZES, 256)
    dzs, flagsrc = [], torch.zeros(B3, apix, LD)
    for l, (h, w) in enumerate(SIZES):
        m = nzpix[:, poff[l]:poff[l] + h * w].reshape(B3, 1, h, w)
        dz = torch.zeros(B3, lddz, h, w)
        dz[:, :cout] = torch.randn(B3, cout, h, w, generator=g) * m
        dzs.append(dz)
    flagsrc[..., 0] = nzpix.float()
    l32, _ = ops.live_tiles(flagsrc.cuda(), B3, SIZES, LD, False)
    zmaps = _split_pyramid(dzs, B3, SIZES, lddz)
    kw = dict(Cin=256, Cout=cout, KH=3, KW=3, pad_t=1, pad_l=1, split=True)
    G0, b0 = ops.conv2d_wgrad(xs, zmaps, **kw)
    G1, b1 = ops.conv2d_wgrad(xs, zmaps, live32=l32[0], **kw)
    G2, b2 = ops.conv2d_wgrad(xs, zmaps, live32=torch.ones_like(l32[0]), **kw)          # every step live: the dense walk
    torch.cuda.synchronize()
    for G, b in ((G1, b1), (G2, b2)):
        assert torch.equal(G.view(torch.int32), G0.view(torch.int32)), pattern
        assert torch.equal(b.view(torch.int32), b0.view(torch.int32)), pattern
    if pattern != 'all':
        assert bool((l32[0] == 0).any())
    assert bool(G0.any()) and bool(b0.any())


# ----------------------------------------------------------------------------------------------------------- whole model
_MODELS = {}


def _model(arith):
    from efficientdet.pytorch_amd import EfficientDet, EFFICIENTDET
    from oracle import effdet_oracle as O
    if arith not in _MODELS:
        net, nc = 'efficientdet-d0', 8
        c = EFFICIENTDET[net]
        m = EfficientDet(nc, network=net, W_bifpn=c['W_bifpn'], D_bifpn=c['D_bifpn'], D_class=c['D_class'], compute_dtype=torch.float32,
                         f32_arith=arith)
        m.load_state_dict(O.make_state_dict(net, nc, seed=3)); m.backbone.drop_connect_rate = 0.0
        m = m.cuda(); m.train(); m.is_training = True; m.freeze_bn()
        _MODELS[arith] = m
    return _MODELS[arith]


def _targets(name):
    S = 512
    if name == 'one_small_box':
        ann = torch.full((2, 1, 5), -1.0)
        ann[:, 0] = torch.tensor([100.0, 140.0, 120.0, 160.0, 3.0])
    elif name == 'empty_and_eight':
        g = torch.Generator().manual_seed(5)
        ann = torch.full((2, 8, 5), -1.0)
        x1 = torch.rand(8, generator=g) * 0.7 * S; y1 = torch.rand(8, generator=g) * 0.7 * S
        wh = 16 + torch.rand(8, 2, generator=g) * 0.3 * S
        ann[1, :, 0], ann[1, :, 1], ann[1, :, 2], ann[1, :, 3] = x1, y1, (x1 + wh[:, 0]).clamp(max=S - 1), (y1 + wh[:, 1]).clamp(max=S - 1)
        ann[1, :, 4] = torch.arange(8).float() % 8
    else:
        # every 128-pixel tile of every level holds a positive anchor: square boxes of each level's base anchor size (32 .. 512), one
        # per tile of that level's maps (64x64: two rows per tile, ..., 8x8 and 4x4: whole images)
        boxes = []
        for size, step in ((32, 16), (64, 64), (128, 256), (256, 512), (512, 512)):
            for i, cy in enumerate(range(step // 2, S, step)):
                cx = min(max(size // 2, 96 + 104 * (i % 4)), S - size // 2)
                cy = min(max(cy, size // 2), S - size // 2)
                boxes.append([cx - size / 2, cy - size / 2, cx + size / 2 - 1, cy + size / 2 - 1, float(i % 8)])
        ann = torch.tensor(boxes).unsqueeze(0).repeat(2, 1, 1)
    return ann


@pytest.mark.parametrize('arith', ['f32_hf16x3_bwd_bf16x3', 'bf16x3', 'f32_bwd_bf16x3'])
@pytest.mark.parametrize('targets', ['one_small_box', 'empty_and_eight', 'every_tile_live'])
def test_model_gradients_equal_with_the_switch_on_and_off(arith, targets):
    """D0 @512, B = 2, the paired head (f32_hf16x3_bwd_bf16x3), the unpaired head whose forward itself runs in the split layout (bf16x3: bench.py's
    f32_bf16x3) and the unpaired head fed by the exact forward's split copies (f32_bwd_bf16x3): losses and every parameter gradient
    torch.equal with functional.HEAD_SPARSE_REG on and off."""
    from efficientdet.pytorch_amd import ops, functional as Fn
    from oracle import effdet_oracle as O
    m = _model(arith)
    img = O.synthetic_batch(2, 512, seed=2, num_classes=8)[0].cuda()
    ann = _targets(targets).cuda()
    if targets == 'every_tile_live':
        sizes = [(64 >> i, 64 >> i) for i in range(5)]
        anc = ops.anchors(512, 512, 'cuda')
        A = anc.shape[1]
        g = torch.Generator().manual_seed(1)
        cls = torch.rand(2, A, 8, generator=g).clamp(1e-3, 1 - 1e-3).cuda()
        reg = (torch.randn(2, A, 4, generator=g) * 0.3).cuda()
        _, ws = ops.focal_loss_fwd(cls, reg, anc, ann)
        dreg = ops.focal_loss_bwd_reg(reg, anc, ann, torch.ones(2, device='cuda'), ws, torch.float32, reg_ld=64, split=True)
        l32, l128 = ops.live_tiles(dreg, 2, sizes, 64, True)
        assert bool(l128[0].all()), (l128[0] == 0).nonzero().flatten().tolist()
    outs = []
    old = Fn.HEAD_SPARSE_REG
    try:
        for on in (False, True):
            Fn.HEAD_SPARSE_REG = on
            m.zero_grad(set_to_none=True)
            cl, rl = m([img, ann])
            (cl.mean() + rl.mean()).backward()
            torch.cuda.synchronize()
            outs.append((cl.detach().clone(), rl.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}))
    finally:
        Fn.HEAD_SPARSE_REG = old
    a, b = outs
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert a[2].keys() == b[2].keys() and len(a[2]) == 274
    bad = [k for k in a[2] if not torch.equal(a[2][k], b[2][k])]
    assert not bad, bad[:8]
