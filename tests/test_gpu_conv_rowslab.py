"""Row-slab activation staging of the split-layout 3x3 convs (csrc/conv_igemm.hip, tuning knob TUNE_ROWSLAB): per 32-channel group and
kernel row the 128-pixel tile's image rows are staged ONCE, with a halo column on each side, and serve the three taps of that row.  Every
case runs the launch with the knob on and off and asks for (a) the same bits -- the per-tap form is the code the slab replaces, and each
matrix instruction is fed the same operands in the same order -- and (b) the float64 convolution of the same inputs under the rules of
tests/test_gpu_hsplit.py (f16x3: at most twice the exact-fp32 kernel's distance, 3e-6 of the tensor's scale, 1e-4 per element) and
tests/test_gpu_split.py (bf16x3: 1e-3 per element).  Shapes are the smallest at which a slab can go wrong: tiles of two, four, eight and
sixteen image rows, a tile that straddles two images, a half-filled last tile, one to three channel groups, both tile widths, slab and
per-tap segments (W = 4) in one launch.  Inputs carry a distinct factor per (image, row, column, channel group), so a shifted or leaked
row cannot cancel."""
import pytest
import torch
import torch.nn.functional as F

from tests.gpu_util import assert_close
from tests.test_gpu_hsplit import _err, from_hsplit, from_split

gpu = pytest.mark.gpu
TOL_SPLIT = 1e-3                 # tests/test_gpu_split.py


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous().cuda()


def _input(g, B, C, H, W, signed):
    """[B, C, H, W]: a distinct factor per (image, row, column, channel group) times a value in [0.5, 1.5) (random sign if signed)."""
    b = torch.arange(B).view(B, 1, 1, 1).float()
    c = (torch.arange(C) // 32).view(1, C, 1, 1).float()
    h = torch.arange(H).view(1, 1, H, 1).float()
    w = torch.arange(W).view(1, 1, 1, W).float()
    x = (1.0 + 0.37 * b + 0.11 * h + 0.013 * w + 0.0041 * c) * (torch.rand(B, C, H, W, generator=g) + 0.5)
    if signed:
        x = x * (torch.randint(0, 2, (B, C, H, W), generator=g).float() * 2.0 - 1.0)
    return x


def _both(launch):
    """launch() -> list of output tensors, with the slab staging on and off -> (on, off) and the bits compared."""
    from efficientdet.pytorch_amd import ops, _lib as L
    out = {}
    old = ops.tuning_set(L.TUNE_ROWSLAB, 1)
    try:
        for sw in (1, 0):
            ops.tuning_set(L.TUNE_ROWSLAB, sw)
            out[sw] = [t.clone() for t in launch()]
            torch.cuda.synchronize()
    finally:
        ops.tuning_set(L.TUNE_ROWSLAB, old)
    for a, b in zip(out[1], out[0]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), 'slab staging changed the bits'
    return out[1]


def _fill(maps, xs, h):
    """NCHW host tensors -> the Maps, in the H-split (h) or the bf16 split layout."""
    from efficientdet.pytorch_amd import ops
    for x, m in zip(xs, maps):
        src = _nhwc(x)
        ops.to_split2(src, None if h else m.addr(), m.addr() if h else None, src.numel(), ops.range_flag(src.device) if h else None)


def _exact(xs, w, shift, act):
    """The exact-fp32 kernel on the same inputs: the yardstick of the f16x3 rule."""
    from efficientdet.pytorch_amd import ops
    from efficientdet.pytorch_amd.ops import Map
    ops.set_f32_arith('f32')
    out = []
    for x in xs:
        B, Cin, H, W = x.shape
        ym = Map.new(B, H, W, w.shape[0], torch.float32, 'cuda')
        ops.conv2d(Map.of(_nhwc(x)), ops.pack_weight(w.cuda(), torch.float32), ym, Cin=Cin, Cout=w.shape[0], KH=3, KW=3, pad_t=1, pad_l=1,
                   shift=shift.cuda() if shift is not None else None, act=act)
        out.append(ym.tensor().cpu().double().permute(0, 3, 1, 2))
    torch.cuda.synchronize()
    return out


def _ref64(x, w, shift, act):
    r = F.conv2d(x.double(), w.double(), shift.double() if shift is not None else None, padding=1)
    return F.relu(r) if act == 1 else r


def _check_h(got, ref, exact, out_f32, what):
    """tests/test_gpu_hsplit.py::test_conv_f16x3_is_fp32_equivalent's three assertions."""
    e_h, e_x = _err(got, ref), _err(exact, ref)
    print('%s: e_h %.3g e_x %.3g' % (what, e_h, e_x))
    assert e_h <= 2.0 * e_x + (0.0 if out_f32 else 2.5e-7), (what, e_h, e_x)
    assert e_h <= 3e-6, (what, e_h)
    assert_close(got.float(), ref.float(), 1e-4, what)


def _levels(B, sizes, Cin, Cout, hs, out_f32, g, act=1, bias=True):
    """One grouped launch over `sizes` in either arithmetic, on / off compared -> (inputs, weights, bias, decoded outputs per level)."""
    from efficientdet.pytorch_amd import ops, functional as Fn
    xs = [_input(g, B, Cin, h, w, signed=not hs) for (h, w) in sizes]
    wt = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    shift = torch.randn(Cout, generator=g) * 0.3 if bias else None
    _, xm = Fn.pyramid_alloc(B, sizes, Cin, torch.float32, 'cuda')
    _fill(xm, xs, hs)
    wp = ops.pack_weight(wt.cuda(), torch.float32, h3=True) if hs else ops.pack_weight(wt.cuda(), torch.float32, x3=True)
    fy, ym = Fn.pyramid_alloc(B, sizes, Cout, torch.float32, 'cuda')
    fs, sm = Fn.pyramid_alloc(B, sizes, Cout, torch.float32, 'cuda')
    twin = hs and not out_f32

    def launch():
        fy.fill_(7.0); fs.fill_(7.0)
        ops.set_f32_arith('f32' if hs else 'bf16x3')
        try:
            ops.conv2d(xm, wp, ym, Cin=Cin, Cout=Cout, KH=3, KW=3, pad_t=1, pad_l=1, shift=shift.cuda() if bias else None, act=act,
                       out_f32=out_f32, hsplit=hs, split=not hs, ysplit=sm if twin else None)
        finally:
            ops.set_f32_arith('f32')
        return [fy, fs]
    y, s = _both(launch)
    got, twins, off = [], [], 0
    for (h, w) in sizes:                       # (the flat buffers are level-major)
        nel = B * h * w * Cout
        t = y[off:off + nel].view(B, h, w, Cout)
        got.append((t.cpu().double() if out_f32 else from_hsplit(t)[0] if hs else from_split(t).double()).permute(0, 3, 1, 2))
        if twin:
            twins.append(from_split(s[off:off + nel].view(B, h, w, Cout)).double().permute(0, 3, 1, 2))
        off += nel
    return xs, wt, shift, got, twins


SINGLE = [
    # B, H, W, Cin, Cout
    (1, 4, 64, 32, 128),         # tiles of two image rows; one channel group
    (1, 8, 32, 64, 256),         # four rows per tile, two tiles, two channel tiles
    (3, 4, 16, 96, 128),         # the second tile straddles images 1 and 2: the row above an image's first row is halo, not the image
                                 # before it; M = 192: the last tile is half filled; three groups
    (2, 8, 8, 64, 256),          # sixteen rows per tile = two whole images
]


@gpu
@pytest.mark.parametrize('cfg', SINGLE)
def test_f16x3_single_map(cfg):
    B, H, W, Cin, Cout = cfg
    g = torch.Generator().manual_seed(sum(cfg) + 3)
    xs, wt, shift, got, twins = _levels(B, [(H, W)], Cin, Cout, True, False, g)
    ref = _ref64(xs[0], wt, shift, 1)
    _check_h(got[0], ref, _exact(xs, wt, shift, 1)[0], False, 'f16x3 %s' % (cfg,))
    assert float((twins[0] - got[0]).abs().max()) <= 2.0 ** -15 * float(got[0].abs().max())        # the bf16 split twin: the same values


@gpu
@pytest.mark.parametrize('cfg', SINGLE)
def test_bf16x3_single_map(cfg):
    B, H, W, Cin, Cout = cfg
    g = torch.Generator().manual_seed(sum(cfg) + 4)
    xs, wt, shift, got, _ = _levels(B, [(H, W)], Cin, Cout, False, False, g, act=0)
    assert_close(got[0].float(), _ref64(xs[0], wt, shift, 0).float(), TOL_SPLIT, 'bf16x3 %s' % (cfg,))


@gpu
@pytest.mark.parametrize('hs', [True, False])
def test_five_levels_slab_and_per_tap_segments_in_one_launch(hs):
    sizes = [(2, 64), (4, 32), (4, 16), (8, 8), (4, 4)]          # W = 4 keeps the per-tap staging
    g = torch.Generator().manual_seed(17 + hs)
    xs, wt, shift, got, _ = _levels(2, sizes, 64, 256, hs, False, g, act=1 if hs else 0)
    exact = _exact(xs, wt, shift, 1) if hs else None
    for i, x in enumerate(xs):
        ref = _ref64(x, wt, shift, 1 if hs else 0)
        if hs:
            _check_h(got[i], ref, exact[i], False, 'f16x3 level %s' % (sizes[i],))
        else:
            assert_close(got[i].float(), ref.float(), TOL_SPLIT, 'bf16x3 level %s' % (sizes[i],))


@gpu
@pytest.mark.parametrize('Cout', [72, 36])
def test_f16x3_plain_fp32_rows(Cout):
    """out_f32 with rows off the 128-channel grid: 72 channels on the 128-wide tile, 36 on the 64-wide one (which keeps W = 8 per tap)."""
    g = torch.Generator().manual_seed(Cout)
    sizes = [(8, 16), (8, 8)]
    xs, wt, shift, got, _ = _levels(2, sizes, 64, Cout, True, True, g, act=0)
    exact = _exact(xs, wt, shift, 0)
    for i, x in enumerate(xs):
        _check_h(got[i], _ref64(x, wt, shift, 0), exact[i], True, 'f16x3 fp32 rows Cout %d level %s' % (Cout, sizes[i]))


@gpu
def test_f16x3_two_towers_with_needed_flags():
    """The head's paired forward layer: two segment groups with their own weights and bias, the bf16 split twin, and flags on the second
    group that mix needed and unneeded tiles."""
    from efficientdet.pytorch_amd import ops, functional as Fn
    g = torch.Generator().manual_seed(29)
    B, sizes, Cin, Cout = 2, [(4, 32), (8, 16), (8, 8), (4, 4)], 64, 256
    ws = [torch.randn(Cout, Cin, 3, 3, generator=g) / 24.0 for _ in range(2)]
    bs = [torch.randn(Cout, generator=g) * 0.1 for _ in range(2)]
    wps = [ops.pack_weight(w.cuda(), torch.float32, h3=True) for w in ws]
    bd = [b.cuda() for b in bs]
    xs = [[_input(g, B, Cin, h, w, False) for (h, w) in sizes] for _ in range(2)]
    _, xa, xb = Fn.pyramid_alloc_pair(B, sizes, Cin, torch.float32, 'cuda')
    _fill(xa, xs[0], True); _fill(xb, xs[1], True)
    fy, ya, yb = Fn.pyramid_alloc_pair(B, sizes, Cout, torch.float32, 'cuda')
    fs, sa, sb = Fn.pyramid_alloc_pair(B, sizes, Cout, torch.float32, 'cuda')
    n = len(sizes)
    ntile = sum((B * h * w + 127) // 128 for (h, w) in sizes)            # 2 + 2 + 1 + 1
    flags = torch.tensor([1, 0, 0, 1, 1, 0], dtype=torch.uint8, device='cuda')
    assert flags.numel() == ntile

    def launch(needed):
        fy.fill_(7.0); fs.fill_(7.0)
        ops.conv2d(xa + xb, wps[0], ya + yb, Cin=Cin, Cout=Cout, KH=3, KW=3, pad_t=1, pad_l=1, shift=bd[0], act=ops.ACT_RELU, hsplit=True,
                   ysplit=sa + sb, seg_w=[wps[0]] * n + [wps[1]] * n, seg_shift=[bd[0]] * n + [bd[1]] * n, needed=needed,
                   needed_tile0=ntile if needed is not None else 0)
        return [fy, fs]
    dy, ds = _both(lambda: launch(None))
    ny, ns = _both(lambda: launch(flags))
    half = dy.numel() // 2
    assert torch.equal(ny[:half].view(torch.int32), dy[:half].view(torch.int32)) and torch.equal(ns[:half].view(torch.int32), ds[:half].view(torch.int32))
    off = half
    t = 0
    for (h, w) in sizes:                      # the flagged group: needed tiles hold the dense values, the others zero bytes
        for m0 in range(0, B * h * w, 128):
            rows = min(128, B * h * w - m0)
            a, b_ = off + m0 * Cout, off + (m0 + rows) * Cout
            for full, part in ((dy, ny), (ds, ns)):
                want = full[a:b_] if int(flags[t]) else torch.zeros_like(full[a:b_])
                assert torch.equal(part[a:b_].view(torch.int32), want.view(torch.int32)), (h, w, m0)
            t += 1
        off += B * h * w * Cout
    off = 0
    for tw in range(2):                       # the dense launch against float64, tower by tower
        exact = _exact(xs[tw], ws[tw], bs[tw], 1)
        for i, (h, w) in enumerate(sizes):
            nel = B * h * w * Cout
            got = from_hsplit(dy[off:off + nel].view(B, h, w, Cout))[0].permute(0, 3, 1, 2)
            _check_h(got, _ref64(xs[tw][i], ws[tw], bs[tw], 1), exact[i], False, 'tower %d level %s' % (tw, (h, w)))
            off += nel


@gpu
def test_bf16x3_relu_mask_and_rowscale():
    """The tower's data gradient: split-layout output under the ReLU mask of the forward activation, scaled per image."""
    from efficientdet.pytorch_amd import ops, functional as Fn
    g = torch.Generator().manual_seed(31)
    B, sizes, C = 3, [(4, 32), (4, 16), (8, 8), (4, 4)], 64
    Cout = 128
    xs = [_input(g, B, C, h, w, True) for (h, w) in sizes]
    rs_ = [F.relu(torch.randn(B, Cout, h, w, generator=g)) for (h, w) in sizes]
    wt = torch.randn(Cout, C, 3, 3, generator=g) / 24.0
    rs = torch.rand(B, generator=g) + 0.5
    _, xm = Fn.pyramid_alloc(B, sizes, C, torch.float32, 'cuda')
    _, rm = Fn.pyramid_alloc(B, sizes, Cout, torch.float32, 'cuda')
    fy, ym = Fn.pyramid_alloc(B, sizes, Cout, torch.float32, 'cuda')
    _fill(xm, xs, False); _fill(rm, rs_, False)
    wp = ops.pack_weight(wt.cuda(), torch.float32, x3=True)
    rsd = rs.cuda()

    def launch():
        fy.fill_(7.0)
        ops.set_f32_arith('bf16x3')
        try:
            ops.conv2d(xm, wp, ym, Cin=C, Cout=Cout, KH=3, KW=3, pad_t=1, pad_l=1, res=rm, res_mode=ops.RES_RELU_MASK, rowscale=rsd, split=True)
        finally:
            ops.set_f32_arith('f32')
        return [fy]
    y, = _both(launch)
    off = 0
    for x, r, (h, w) in zip(xs, rs_, sizes):
        nel = B * h * w * Cout
        got = from_split(y[off:off + nel].view(B, h, w, Cout)).permute(0, 3, 1, 2)
        ref = _ref64(x, wt, None, 0) * rs.double().view(-1, 1, 1, 1)
        ref = torch.where(r > 0, ref, torch.zeros_like(ref))
        assert_close(got, ref.float(), TOL_SPLIT, 'masked gradient level %s' % ((h, w),))
        off += nel


@gpu
@pytest.mark.parametrize('Cout', [128, 64])
def test_bf16x3_in_place_add_with_live_flags(Cout):
    """Plain fp32 rows accumulated in place (the second tower onto the first one's gradient), with liveness flags: image 1 is all zeros, so
    the tile it fills is dead and keeps its value."""
    from efficientdet.pytorch_amd import ops
    from efficientdet.pytorch_amd.ops import Map
    g = torch.Generator().manual_seed(37 + Cout)
    B, H, W, C = 3, 8, 16, 64                       # one 128-pixel tile per image
    x = _input(g, B, C, H, W, True)
    x[1] = 0.0
    base = torch.randn(B, Cout, H, W, generator=g)
    wt = torch.randn(Cout, C, 3, 3, generator=g) / 24.0
    xm = Map.new(B, H, W, C, torch.float32, 'cuda')
    _fill([xm], [x], False)
    wp = ops.pack_weight(wt.cuda(), torch.float32, x3=True)
    y = _nhwc(base)
    ym = Map.of(y)
    live = torch.tensor([1, 0, 1], dtype=torch.uint8, device='cuda')
    b0 = _nhwc(base)

    def launch():
        y.copy_(b0)
        ops.set_f32_arith('bf16x3')
        try:
            ops.conv2d(xm, wp, ym, Cin=C, Cout=Cout, KH=3, KW=3, pad_t=1, pad_l=1, res=ym, res_mode=ops.RES_ADD, out_f32=True, split=True, live=live)
        finally:
            ops.set_f32_arith('f32')
        return [y]
    got, = _both(launch)
    assert torch.equal(got[1], b0[1])
    assert_close(got.cpu().permute(0, 3, 1, 2), (_ref64(x, wt, None, 0) + base.double()).float(), TOL_SPLIT, 'in-place add Cout %d' % Cout)
