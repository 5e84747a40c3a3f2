"""The squeeze-excite gate applied in the project conv's operand registers (include/effdet_gate_operand.h; functional.GATE_IN_OPERAND).

ops.conv2d(z, w, ..., a_gate=gate, a_act=act) and ops.conv2d_wgrad(z, dy, ..., image_splits=True, a_gate=gate, a_act=act) against the
same launches on ops.channel_scale(z, gate, act): the kernels form act(v) * gate[b][c] with channel_scale's two statements between the
LDS read and the matrix-core instruction, so every comparison here is BITWISE (through int32 views: NaNs compare too) -- outputs, slabs,
bias partial rows, and at model level both losses and all 274 parameter gradients of a D0 train step."""
import pytest
import torch

from oracle import effdet_oracle as O

pytestmark = pytest.mark.gpu

DEV = 'cuda'
ACT_NONE, ACT_SWISH = 0, 2


@pytest.fixture(autouse=True)
def _plain_state():
    """no model's parameter arena, exact-fp32 arithmetic: whatever an earlier test of the session left is put back afterwards"""
    from efficientdet.pytorch_amd import ops
    old = (ops.get_prep(), ops.F32_ARITH, ops.F32_ARITH_BWD, ops.F32_ARITH_HEAD)
    ops.set_prep(None); ops.set_model_arith('f32')
    yield
    ops.set_prep(old[0])
    ops.F32_ARITH, ops.F32_ARITH_BWD, ops.F32_ARITH_HEAD = old[1:]


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _guarded_gate(B, C, g):
    """gate [B][C] at the head of one allocation whose remainder is NaN: a read past B * C floats (the K padding of the last K-step)
    would poison the tile.  One entry is exactly 0."""
    buf = torch.full((B * C + 4096,), float('nan'), device=DEV)
    gate = buf[:B * C].view(B, C)
    gate.copy_(torch.rand(B, C, generator=g).to(DEV) * 1.5 + 0.01)
    gate[B - 1, C - 1] = 0.0
    gate[0, 1] = 0.0
    return gate, buf


def _z(B, H, W, C, g, inf=True):
    """depthwise pre-activation: N(0, 2) with -100 (Swish lands in the denormal range) and, if asked, two +inf: one under a gate of
    exactly 0 (_guarded_gate: inf * 0, a NaN operand) and one under an ordinary gate (an inf operand) -- the same outputs leave the
    finite range on both sides"""
    z = (torch.randn(B, H, W, C, generator=g) * 2.0).to(DEV)
    z[0, 0, 1, 0] = -100.0
    z[B - 1, H - 1, W - 1, C - 1] = -100.0
    z[0, 0, 2, 1] = -87.5
    if inf:
        z[0, 1, 0, 1] = float('inf')
        z[B - 1, H // 2, W // 2, C // 2] = float('inf')
    return z


FWD_SHAPES = [(2, 8, 16), (3, 16, 16)]              # one 128-pixel tile per image (image boundary = tile boundary) | two tiles per image
FWD_CH = [(32, 16), (96, 24), (144, 24), (144, 40)]  # 144: the last K-step is half padding


@pytest.mark.parametrize('B,H,W', FWD_SHAPES)
@pytest.mark.parametrize('Cin,Cout', FWD_CH)
@pytest.mark.parametrize('act', [ACT_SWISH, ACT_NONE])
def test_forward_is_bitwise_channel_scale_then_conv(B, H, W, Cin, Cout, act):
    from efficientdet.pytorch_amd import ops
    from efficientdet.pytorch_amd.ops import Map
    g = torch.Generator().manual_seed(100 * Cin + Cout + H)
    z = _z(B, H, W, Cin, g)
    x = Map.of(z if act == ACT_SWISH else ops.channel_scale(Map.of(z), torch.ones(B, Cin, device=DEV), ACT_SWISH).t)   # ACT_NONE: on a Swish output
    gate, buf = _guarded_gate(B, Cin, g)
    w = (torch.randn(Cout, Cin, 1, 1, generator=g) * 0.2).to(DEV)
    wp = ops.pack_weight(w, torch.float32)
    s = (torch.rand(Cout, generator=g) + 0.5).to(DEV); t = torch.randn(Cout, generator=g).to(DEV)
    variants = [dict(scale=s, shift=t)]
    if (Cin, Cout) == (144, 24):
        res = Map.of(torch.randn(B, H, W, Cout, generator=g).to(DEV))
        rs = torch.tensor([0.0, 1.25, 1.25][:B], device=DEV)
        variants.append(dict(scale=s, shift=t, res=res, res_mode=ops.RES_ADD, rowscale=rs))
    for kw in variants:
        kw = dict(kw, Cin=Cin, Cout=Cout, KH=1, KW=1)
        ref = Map.new(B, H, W, Cout, torch.float32, DEV)
        ops.conv2d(ops.channel_scale(x, gate, act), wp, ref, **kw)
        got = Map.new(B, H, W, Cout, torch.float32, DEV)
        assert ops.conv2d_gated_ok(x, wp, got, gate, act, **kw)
        n0 = ops.GATE_OPERAND_LAUNCHES[0]
        ops.conv2d(x, wp, got, a_gate=gate, a_act=act, **kw)
        assert ops.GATE_OPERAND_LAUNCHES[0] == n0 + 1
        assert _bits_equal(got.t, ref.t), (int((got.t.view(torch.int32) != ref.t.view(torch.int32)).sum()), got.t.numel())
        assert bool(torch.isnan(ref.t).any()) and bool(torch.isfinite(ref.t).any())          # the infs reached some outputs, not all
    assert bool(torch.isnan(buf[B * Cin:]).all())


def _block(cin=24, cout=24, k=3):
    from efficientdet.pytorch_amd.config import Block
    return Block(k=k, stride=1, expand=6, cin=cin, cout=cout, cexp=6 * cin, cse=max(1, cin // 4), pad=(1, 1), skip=cin == cout, stage_end=False)


def _block_params(blk, g):
    r = lambda *s, sc=0.2: torch.nn.Parameter((torch.randn(*s, generator=g) * sc).to(DEV))
    P = {'expand.weight': r(blk.cexp, blk.cin, 1, 1), 'dw.weight': r(blk.cexp, 1, blk.k, blk.k), 'project.weight': r(blk.cout, blk.cexp, 1, 1),
         'se_reduce.weight': r(blk.cse, blk.cexp, 1, 1), 'se_reduce.bias': r(blk.cse), 'se_expand.weight': r(blk.cexp, blk.cse, 1, 1),
         'se_expand.bias': r(blk.cexp)}
    for n, c in (('bn0', blk.cexp), ('bn1', blk.cexp), ('bn2', blk.cout)):
        P[n + '.weight'] = torch.nn.Parameter((torch.rand(c, generator=g) + 0.5).to(DEV)); P[n + '.bias'] = r(c)
        P[n + '.running_mean'] = (torch.randn(c, generator=g) * 0.1).to(DEV); P[n + '.running_var'] = (torch.rand(c, generator=g) + 0.5).to(DEV)
    return P


def _mbconv_step(blk, P, x, dy, rs, on_fwd, on_bwd):
    """mbconv_fwd + mbconv_bwd with the switch as given for each half -> (y, dx, grads, gated launches [forward, weight gradient])"""
    from efficientdet.pytorch_amd import ops, functional as Fn
    from efficientdet.pytorch_amd.ops import Map
    old, old_hw, n0 = Fn.GATE_IN_OPERAND, Fn.GATE_OPERAND_MIN_HW, list(ops.GATE_OPERAND_LAUNCHES)
    try:
        Fn.GATE_OPERAND_MIN_HW = 128                              # (every map the planners accept, whatever the measured default)
        with torch.no_grad():
            Fn.GATE_IN_OPERAND = on_fwd
            y, sv = Fn.mbconv_fwd(Map.of(x), blk, P, torch.float32, True, rs)
            kept = sv.xs is not None
            Fn.GATE_IN_OPERAND = on_bwd
            dx, gr = Fn.mbconv_bwd(sv, Map.of(dy))
        torch.cuda.synchronize()
    finally:
        Fn.GATE_IN_OPERAND, Fn.GATE_OPERAND_MIN_HW = old, old_hw
    return y.t, dx.t, gr, [a - b for a, b in zip(ops.GATE_OPERAND_LAUNCHES, n0)], kept


def test_a_map_that_is_no_whole_number_of_tiles_falls_back():
    """6 x 6: Ho*Wo % 128 != 0, the planner refuses the form (and conv2d with a_gate raises instead of launching on ungated data);
    mbconv_fwd runs channel_scale as before and the counters do not move."""
    from efficientdet.pytorch_amd import ops
    from efficientdet.pytorch_amd.ops import Map
    g = torch.Generator().manual_seed(7)
    blk = _block()
    P = _block_params(blk, g)
    z = Map.of(_z(2, 6, 6, blk.cexp, g, inf=False))
    gate, _ = _guarded_gate(2, blk.cexp, g)
    y = Map.new(2, 6, 6, blk.cout, torch.float32, DEV)
    wp = ops.pack_weight(P['project.weight'], torch.float32)
    kw = dict(Cin=blk.cexp, Cout=blk.cout, KH=1, KW=1)
    assert not ops.conv2d_gated_ok(z, wp, y, gate, ACT_SWISH, **kw)
    with pytest.raises(RuntimeError, match='EFFDET_EUNSUPPORTED'):
        ops.conv2d(z, wp, y, a_gate=gate, a_act=ACT_SWISH, **kw)
    x = torch.randn(2, 6, 6, blk.cin, generator=g).to(DEV); dy = torch.randn(2, 6, 6, blk.cout, generator=g).to(DEV)
    rs = torch.tensor([1.25, 0.0], device=DEV)
    n0 = list(ops.GATE_OPERAND_LAUNCHES)
    on = _mbconv_step(blk, P, x, dy, rs, True, True)
    assert on[3] == [0, 0] and on[4] and [a - b for a, b in zip(ops.GATE_OPERAND_LAUNCHES, n0)] == [0, 0]
    off = _mbconv_step(blk, P, x, dy, rs, False, False)
    assert _bits_equal(on[0], off[0]) and _bits_equal(on[1], off[1])


@pytest.mark.parametrize('on_bwd', [True, False])
def test_one_block_forward_and_backward(on_bwd):
    """One MBConv block on a 16 x 16 map (two tiles per image), drop_connect scale on the branch: output, input gradient and every
    parameter gradient equal the channel_scale path's; xs is not kept; with the switch flipped between forward and backward the
    backward materialises xs itself."""
    g = torch.Generator().manual_seed(11)
    blk = _block()
    P = _block_params(blk, g)
    x = torch.randn(2, 16, 16, blk.cin, generator=g).to(DEV); dy = torch.randn(2, 16, 16, blk.cout, generator=g).to(DEV)
    rs = torch.tensor([1.25, 0.0], device=DEV)
    off = _mbconv_step(blk, P, x, dy, rs, False, False)
    on = _mbconv_step(blk, P, x, dy, rs, True, on_bwd)
    assert off[3] == [0, 0] and off[4]
    assert on[3] == [1, 1 if on_bwd else 0] and not on[4]
    assert _bits_equal(on[0], off[0]) and _bits_equal(on[1], off[1])
    assert on[2].keys() == off[2].keys()
    bad = [k for k in on[2] if not _bits_equal(on[2][k], off[2][k])]
    assert not bad, bad


def test_gate_in_weights_forward_then_chain_backward():
    """The gate in per-image weights in the forward (GATE_IN_WEIGHTS_TRAIN), the fused squeeze-excite backward switched off before the
    backward: mbconv_bwd materialises xs = channel_scale(xd, gate) and runs the chain.  Against DW_SAVE_Y on and SE_FUSED off throughout:
    both backwards run the chain on the same xd, zd, gate, mid, pool, the same xs and the same dy, so dx and every parameter gradient are
    torch.equal (the outputs y differ in rounding -- W diag(gate) against gate x -- and are not compared)."""
    from efficientdet.pytorch_amd import functional as Fn
    from efficientdet.pytorch_amd.ops import Map
    g = torch.Generator().manual_seed(11)
    blk = _block()
    P = _block_params(blk, g)
    x = torch.randn(2, 16, 16, blk.cin, generator=g).to(DEV); dy = torch.randn(2, 16, 16, blk.cout, generator=g).to(DEV)
    rs = torch.tensor([1.25, 0.0], device=DEV)
    names = ('GATE_IN_WEIGHTS_TRAIN', 'SE_FUSED', 'DW_SAVE_Y')
    old = {k: getattr(Fn, k) for k in names}

    def step(fwd, bwd):
        try:
            with torch.no_grad():
                for k in names:
                    setattr(Fn, k, fwd.get(k, old[k]))
                y, sv = Fn.mbconv_fwd(Map.of(x), blk, P, torch.float32, True, rs)
                for k in names:
                    setattr(Fn, k, bwd.get(k, old[k]))
                dx, gr = Fn.mbconv_bwd(sv, Map.of(dy))
            torch.cuda.synchronize()
        finally:
            for k in names:
                setattr(Fn, k, old[k])
        return dx.t, gr, sv.path.gate
    a_dx, a, a_form = step({'GATE_IN_WEIGHTS_TRAIN': True, 'SE_FUSED': True}, {'GATE_IN_WEIGHTS_TRAIN': True, 'SE_FUSED': False})
    b_dx, b, b_form = step({'DW_SAVE_Y': True, 'SE_FUSED': False}, {'DW_SAVE_Y': True, 'SE_FUSED': False})
    assert a_form == Fn.GATE_WEIGHTS and b_form == Fn.GATE_XS_FROM_XD
    assert _bits_equal(a_dx, b_dx)
    assert a.keys() == b.keys() and len(a) == 13
    bad = [k for k in a if not _bits_equal(a[k], b[k])]
    assert not bad, bad


# (Cout, Cin) at B = 2, 128 x 128 = 32768 pixels, the thin kernel's threshold: its <1,2>, <2,6>, <2,9> and <3,9> tile shapes
THIN = [(16, 32), (24, 96), (24, 144), (40, 144),
        (96, 16), (144, 24), (16, 16), (32, 16), (16, 48), (32, 32)]      # the table's other shapes: <6,1>, <9,2>, <1,1>, <2,1>, <1,3>, <2,2>
# at B = 2, 16 x 16: the DMA-staged fp32 kernel, exact and bf16x3
TILED = [(40, 240), (80, 240)]


def _wgrad_case(B, H, W, Cout, Cin, arith, kernel_id):
    from efficientdet.pytorch_amd import ops
    from efficientdet.pytorch_amd.ops import Map
    g = torch.Generator().manual_seed(Cout * 1000 + Cin)
    x = Map.of(_z(B, H, W, Cin, g))
    dz = Map.of(torch.randn(B, H, W, Cout, generator=g).to(DEV))
    gate, buf = _guarded_gate(B, Cin, g)
    old = (ops.F32_ARITH, ops.F32_ARITH_BWD)
    try:
        ops.set_f32_arith(arith)
        kw = dict(Cin=Cin, Cout=Cout, KH=1, KW=1)
        assert ops.conv2d_wgrad_kernel_id(x, dz, image_splits=True, **kw) == kernel_id
        assert ops.conv2d_wgrad_kernel_id(x, dz, image_splits=True, a_gate=gate, a_act=ACT_SWISH, **kw) == kernel_id
        assert ops.conv2d_wgrad_kernel_id(x, dz, image_splits=False, a_gate=gate, a_act=ACT_SWISH, **kw) == -3      # only per-image splits
        for act in (ACT_SWISH, ACT_NONE):
            ref_s, ref_p = ops.conv2d_wgrad(ops.channel_scale(x, gate, act), dz, image_splits=True, **kw)
            n0 = ops.GATE_OPERAND_LAUNCHES[1]
            got_s, got_p = ops.conv2d_wgrad(x, dz, image_splits=True, a_gate=gate, a_act=act, **kw)
            assert ops.GATE_OPERAND_LAUNCHES[1] == n0 + 1
            assert _bits_equal(got_s, ref_s), (act, int((got_s.view(torch.int32) != ref_s.view(torch.int32)).sum()), got_s.numel())
            assert _bits_equal(got_p, ref_p), act
            assert got_s.shape[0] % B == 0 and bool(torch.isnan(ref_s).any()) and bool(torch.isfinite(ref_s).any())   # the infs reached some slabs, not all
    finally:
        ops.F32_ARITH, ops.F32_ARITH_BWD = old
    assert bool(torch.isnan(buf[B * Cin:]).all())


@pytest.mark.parametrize('Cout,Cin', THIN)
def test_weight_gradient_thin_kernel(Cout, Cin):
    _wgrad_case(2, 128, 128, Cout, Cin, 'f32', 1)


@pytest.mark.parametrize('arith', ['f32', 'bf16x3'])
@pytest.mark.parametrize('Cout,Cin', TILED)
def test_weight_gradient_dma_kernel(Cout, Cin, arith):
    _wgrad_case(2, 16, 16, Cout, Cin, arith, 0)


def test_weight_gradient_thin_kernel_ragged_last_stage():
    """Sixteen 96 x 96 images: 32 splits per image of 288 pixels against the thin kernel's 128-pixel stages -- the last stage of a split
    is zero filled past the split's end, and those rows must stay +0 whatever the gate."""
    from efficientdet.pytorch_amd import ops
    from efficientdet.pytorch_amd.ops import Map
    B, H, W, Cout, Cin = 16, 96, 96, 16, 32
    g = torch.Generator().manual_seed(3)
    x = Map.of(_z(B, H, W, Cin, g, inf=False))
    dz = Map.of(torch.randn(B, H, W, Cout, generator=g).to(DEV))
    gate, _ = _guarded_gate(B, Cin, g)
    kw = dict(Cin=Cin, Cout=Cout, KH=1, KW=1)
    assert ops.conv2d_wgrad_kernel_id(x, dz, image_splits=True, a_gate=gate, a_act=ACT_SWISH, **kw) == 1
    ref_s, ref_p = ops.conv2d_wgrad(ops.channel_scale(x, gate, ACT_SWISH), dz, image_splits=True, **kw)
    got_s, got_p = ops.conv2d_wgrad(x, dz, image_splits=True, a_gate=gate, a_act=ACT_SWISH, **kw)
    assert (H * W // (got_s.shape[0] // B)) % 128 != 0                # (what the case is for: a split is no whole number of stages)
    assert _bits_equal(got_s, ref_s) and _bits_equal(got_p, ref_p)
    assert bool(torch.isfinite(got_s).all())


# ------------------------------------------------------------------------------------------------------------------ model
_MODELS = {}


def _model(arith):
    from efficientdet.pytorch_amd import EfficientDet, EFFICIENTDET
    if arith not in _MODELS:
        net, nc = 'efficientdet-d0', 8
        c = EFFICIENTDET[net]
        torch.manual_seed(5)                                     # (the drop_connect seed is one draw from the default generator)
        m = EfficientDet(nc, network=net, W_bifpn=c['W_bifpn'], D_bifpn=c['D_bifpn'], D_class=c['D_class'], compute_dtype=torch.float32,
                         f32_arith=arith)
        m.load_state_dict(O.make_state_dict(net, nc, seed=3))
        m = m.cuda(); m.train(); m.is_training = True; m.freeze_bn()
        _MODELS[arith] = m
    return _MODELS[arith]


def _dc_counters(m):
    return [v for k, v in m._dc.items() if isinstance(k, tuple) and k[0] == 'step_dev']


def _train_step(m, img, ann, on_fwd, on_bwd):
    from efficientdet.pytorch_amd import ops, functional as Fn
    old, n0 = Fn.GATE_IN_OPERAND, list(ops.GATE_OPERAND_LAUNCHES)
    try:
        m.zero_grad(set_to_none=True)
        Fn.GATE_IN_OPERAND = on_fwd
        cl, rl = m([img, ann])
        Fn.GATE_IN_OPERAND = on_bwd
        (cl.mean() + rl.mean()).backward()
        torch.cuda.synchronize()
    finally:
        Fn.GATE_IN_OPERAND = old
    return (cl.detach().clone(), rl.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None},
            [a - b for a, b in zip(ops.GATE_OPERAND_LAUNCHES, n0)])


@pytest.mark.parametrize('arith', ['f32_hf16x3_bwd_bf16x3', 'f32'])
def test_model_step_equals_the_channel_scale_path(arith):
    """D0, B = 2 @256, drop_connect active: one train step with the switch off, on, and on in the forward only, each from the same
    weights and the same drop_connect counter.  @256 the blocks' maps are 128^2, 64^2 (x2), 32^2 (x2), 16^2 (x3), 8^2 (x3), 4^2 (x4)
    and 2^2: the eight blocks whose images are whole 128-pixel tiles take the form in forward and backward, the others fall back."""
    from efficientdet.pytorch_amd import functional as Fn
    m = _model(arith)
    img, ann = O.synthetic_batch(2, 256, seed=2, num_classes=8)
    img, ann = img.cuda(), ann.cuda()
    if not _dc_counters(m):
        _train_step(m, img, ann, False, False)                    # (the first forward draws the seed and creates the device counter)
    saved = [t.clone() for t in _dc_counters(m)]
    outs = []
    old = Fn.GATE_OPERAND_MIN_HW
    try:
        Fn.GATE_OPERAND_MIN_HW = 128                              # (every block the planners accept, whatever the measured default)
        for on_fwd, on_bwd in ((False, False), (True, True), (True, False)):
            for t, s in zip(_dc_counters(m), saved):
                t.copy_(s)
            outs.append(_train_step(m, img, ann, on_fwd, on_bwd))
    finally:
        Fn.GATE_OPERAND_MIN_HW = old
    off, on, flipped = outs
    side, n = 128, 0
    for blk in m.backbone.plan:
        side = (side + blk.stride - 1) // blk.stride
        n += (side * side) % 128 == 0
    assert n == 8
    assert off[3] == [0, 0] and on[3] == [n, n] and flipped[3] == [n, 0], (off[3], on[3], flipped[3])
    assert float(off[1]) > 0 and len(off[2]) == 274 and all(bool(torch.isfinite(v).all()) for v in off[2].values())
    for other in (on, flipped):
        assert torch.equal(off[0], other[0]) and torch.equal(off[1], other[1]), (off[0], other[0], off[1], other[1])
        assert off[2].keys() == other[2].keys()
        bad = [k for k in off[2] if not torch.equal(off[2][k], other[2][k])]
        assert not bad, bad[:8]
