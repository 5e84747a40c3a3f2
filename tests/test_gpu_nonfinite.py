"""GPU non-finite parity: every kernel that restates a torch op keeps NaN and inf where that op keeps them.

fmaxf / fminf (llvm.maxnum, v_max_f32) return the operand that is NOT NaN, while torch's relu, clamp, max_pool2d and max(dim) keep the
NaN: a diverged value would come out of such a kernel as a plausible number (a ReLU'd 0, a clamp bound, a skipped class).  Each case
below plants NaN (both signs), +inf and -inf at chosen positions of finite random data and compares one op with the same op in float64
torch on the CPU (the loss: oracle autograd in fp32, as in tests/test_gpu_post_loss.py), through tests.gpu_util.assert_nonfinite_match."""
import struct

import pytest
import torch
import torch.nn.functional as F

from oracle import effdet_oracle as O
from tests.gpu_util import assert_close, assert_nonfinite_match
from tests.test_gpu_hsplit import from_hsplit, from_split, to_split2

pytestmark = pytest.mark.gpu

NAN, INF = float('nan'), float('inf')
NEG_NAN = struct.unpack('<f', struct.pack('<I', 0xffc00000))[0]       # a quiet NaN with the sign bit set


@pytest.fixture(autouse=True)
def _arith_and_watch():
    """Cases here switch the process-wide conv arithmetic and feed the fp16 range watch on purpose: put both back."""
    from efficientdet.pytorch_amd import ops
    old = (ops.F32_ARITH, ops.F32_ARITH_BWD)
    yield
    ops.set_f32_arith(*old)
    for t in ops._range_flags.values():
        t.zero_()


def _nhwc(x, dtype=torch.float32):
    return x.permute(0, 2, 3, 1).contiguous().to('cuda', dtype)


def _nchw(t):
    return t.detach().float().cpu().permute(0, 3, 1, 2)


def test_negative_nan_constant_has_its_sign_bit():
    t = torch.tensor([NEG_NAN], dtype=torch.float32)
    assert bool(torch.isnan(t)) and int(t.view(torch.int32)) == -4194304          # 0xffc00000


# ----------------------------------------------------------------------------- conv2d ACT_RELU (head towers)
def _operands(where, seed=0, B=2, Cin=64, Cout=256, H=8, W=8, exact=True):
    """x, w, bias with non-finite values planted in `where` ('x', 'w' or 'b').  exact=False (the x3 split forms): no inf in the operands
    of the product -- an inf is split into (inf, inf - inf = NaN), and a NaN cannot be ReLU'd to the 0 that torch makes of a -inf sum;
    the bias is added in fp32 after the products, so it carries the infs there."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.3
    if where == 'x':
        x[0, 5, 2, 3] = NAN; x[1, 11, 7, 7] = NEG_NAN; x[0, 9, 0, 0] = NAN
        if exact:
            x[1, 7, 4, 4] = INF; x[1, 20, 1, 6] = -INF
    elif where == 'w':
        w[3, 10, 1, 1] = NAN; w[40, 2, 0, 2] = NEG_NAN
        if exact:
            w[7, 2, 0, 2] = INF; w[100, 33, 2, 0] = -INF
    else:
        b[0] = NAN; b[5] = NEG_NAN; b[6] = INF; b[7] = -INF; b[255] = INF
    return x, w, b


def _relu_ref(x, w, b):
    return F.relu(F.conv2d(x.double(), w.double(), b.double(), padding=1))


@pytest.mark.parametrize('where', ['x', 'w', 'b'])
@pytest.mark.parametrize('form', ['f32', 'bf16', 'bf16x3'])
def test_conv_relu_epilogue_keeps_nonfinite(form, where):
    from efficientdet.pytorch_amd import ops
    from efficientdet.pytorch_amd.ops import Map
    exact = form != 'bf16x3'
    x, w, b = _operands(where, exact=exact)
    ops.set_f32_arith('bf16x3' if form == 'bf16x3' else 'f32')
    dt = torch.bfloat16 if form == 'bf16' else torch.float32
    if dt == torch.bfloat16:
        x, w = x.bfloat16().float(), w.bfloat16().float()
    B, Cin, H, W = x.shape
    ym = Map.new(B, H, W, 256, dt, 'cuda')
    ops.conv2d(Map.of(_nhwc(x, dt)), ops.pack_weight(w.cuda(), dt), ym, Cin=Cin, Cout=256, KH=3, KW=3, pad_t=1, pad_l=1,
               shift=b.cuda(), act=ops.ACT_RELU)
    torch.cuda.synchronize()
    tol = {'f32': 2e-4, 'bf16': 2e-2, 'bf16x3': 1e-3}[form]
    assert_nonfinite_match(_nchw(ym.tensor()), _relu_ref(x, w, b), tol, exact=exact, what='relu conv %s %s' % (form, where))


@pytest.mark.parametrize('where', ['x', 'w', 'b'])
def test_conv_relu_epilogue_keeps_nonfinite_persistent_split(where):
    """The persistent 256 x 256 form of the split-layout kernel (long-K head convs: Cin = 256)."""
    from efficientdet.pytorch_amd import ops, _lib as L
    from efficientdet.pytorch_amd.ops import Map
    x, w, b = _operands(where, Cin=256, exact=False)
    old = ops.tuning_set(L.TUNE_SPLIT_PERS, 1), ops.tuning_set(L.TUNE_IGEMM_BIG_MIN_M, 0)
    try:
        B, Cin, H, W = x.shape
        ym = Map.new(B, H, W, 256, torch.float32, 'cuda')
        ops.conv2d(Map.of(ops.to_split(_nhwc(x))), ops.pack_weight(w.cuda(), torch.float32, x3=True), ym, Cin=Cin, Cout=256, KH=3, KW=3,
                   pad_t=1, pad_l=1, shift=b.cuda(), act=ops.ACT_RELU, split=True)
        torch.cuda.synchronize()
    finally:
        ops.tuning_set(L.TUNE_SPLIT_PERS, old[0]); ops.tuning_set(L.TUNE_IGEMM_BIG_MIN_M, old[1])
    assert_nonfinite_match(from_split(ym.tensor()).permute(0, 3, 1, 2), _relu_ref(x, w, b), 1e-3, exact=False, what='persistent ' + where)


@pytest.mark.parametrize('where', ['x', 'w', 'b'])
@pytest.mark.parametrize('out_f32', [True, False])
def test_conv_relu_epilogue_keeps_nonfinite_hsplit(where, out_f32):
    """f16x3 (H-split operands): plain fp32 output, and the H-split output with its bf16 split copy (the backward's ReLU mask)."""
    from efficientdet.pytorch_amd import ops
    from efficientdet.pytorch_amd.ops import Map
    x, w, b = _operands(where, exact=False)
    B, Cin, H, W = x.shape
    ym = Map.new(B, H, W, 256, torch.float32, 'cuda')
    ys = None if out_f32 else Map.new(B, H, W, 256, torch.float32, 'cuda')
    ops.conv2d(Map.of(to_split2(_nhwc(x), bf=False)[1]), ops.pack_weight(w.cuda(), torch.float32, h3=True), ym, Cin=Cin, Cout=256, KH=3,
               KW=3, pad_t=1, pad_l=1, shift=b.cuda(), act=ops.ACT_RELU, out_f32=out_f32, hsplit=True, ysplit=ys)
    torch.cuda.synchronize()
    ref = _relu_ref(x, w, b)
    if out_f32:
        assert_nonfinite_match(_nchw(ym.tensor()), ref, 1e-4, exact=False, what='hsplit relu ' + where)
    else:
        assert_nonfinite_match(from_hsplit(ym.tensor())[0].permute(0, 3, 1, 2), ref, 1e-4, exact=False, what='hsplit relu ' + where)
        assert_nonfinite_match(from_split(ys.tensor()).permute(0, 3, 1, 2), ref, 1e-4, exact=False, what='hsplit relu copy ' + where)


@pytest.mark.parametrize('paired', [False, True])
def test_conv_relu_hsplit_grouped_levels_and_paired_towers(paired):
    """The head's level-grouped launch (and both towers in one launch) with a NaN in one level's input and non-finite bias entries."""
    from efficientdet.pytorch_amd import ops, functional as Fn
    g = torch.Generator().manual_seed(7)
    B, sizes, Cin, Cout = 2, [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)], 64, 256
    ntw = 2 if paired else 1
    ws = [torch.randn(Cout, Cin, 3, 3, generator=g) / 24.0 for _ in range(ntw)]
    bs = [torch.randn(Cout, generator=g) * 0.1 for _ in range(ntw)]
    bs[-1][3] = NAN; bs[-1][4] = -INF; bs[-1][9] = INF; bs[0][200] = NEG_NAN
    xs_all, hs = [], []
    for t in range(ntw):
        xs = [F.relu(torch.randn(B, Cin, h, w_, generator=g)) for (h, w_) in sizes]
        xs[1 + t][1, 17, 2, 3] = NAN
        xs_all.append(xs)
        hs.append(Fn._pyramid_to_split([ops.Map.of(_nhwc(x)) for x in xs], B, sizes, Cin, torch.float32, 'cuda', bf=False, h=True)[1])
    wps = [ops.pack_weight(w.cuda(), torch.float32, h3=True) for w in ws]
    kw = dict(Cin=Cin, Cout=Cout, KH=3, KW=3, pad_t=1, pad_l=1, act=ops.ACT_RELU, hsplit=True)
    if paired:
        _, ya, yb = Fn.pyramid_alloc_pair(B, sizes, Cout, torch.float32, 'cuda')
        ops.conv2d(hs[0] + hs[1], wps[0], ya + yb, shift=bs[0].cuda(), seg_w=[wps[0]] * 5 + [wps[1]] * 5,
                   seg_shift=[bs[0].cuda()] * 5 + [bs[1].cuda()] * 5, **kw)
        ys = [ya, yb]
    else:
        _, ym = Fn.pyramid_alloc(B, sizes, Cout, torch.float32, 'cuda')
        ops.conv2d(hs[0], wps[0], ym, shift=bs[0].cuda(), **kw)
        ys = [ym]
    torch.cuda.synchronize()
    for t in range(ntw):
        for x, m in zip(xs_all[t], ys[t]):
            got = from_hsplit(Fn.level_tensor(m))[0].permute(0, 3, 1, 2)
            assert_nonfinite_match(got, _relu_ref(x, ws[t], bs[t]), 1e-4, exact=False, what='tower %d level %s' % (t, tuple(x.shape)))


# ----------------------------------------------------------------------------- RES_RELU_MASK (data gradient through a ReLU)
def _mask_case(seed=3, B=2, Cin=256, Cout=256, H=8, W=8):
    """dz (finite gradient), w, and the forward activation q the mask is read from: zeros of both signs, negatives, NaN of both signs,
    +inf and -inf.  torch's threshold_backward drops the gradient where q <= 0 and passes it everywhere else, a NaN included."""
    g = torch.Generator().manual_seed(seed)
    dz = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    q = F.relu(torch.randn(B, Cout, H, W, generator=g))
    q[0, :, 0, 0] = NAN; q[0, :, 1, 1] = NEG_NAN; q[1, :, 2, 2] = INF; q[1, :, 3, 3] = -INF; q[0, :, 4, 4] = -0.0
    q[1, ::3, 5, 5] = NAN; q[1, 1::3, 5, 5] = NEG_NAN; q[0, ::2, 6, 6] = -1.5
    ref = F.conv2d(dz.double(), w.double(), padding=1)
    ref = torch.where(q.double() <= 0, torch.zeros_like(ref), ref)
    return dz, w, q, ref


@pytest.mark.parametrize('form', ['f32', 'bf16', 'bf16_big', 'split', 'split_pers'])
def test_relu_mask_passes_the_gradient_at_nan(form):
    """Every form of the fused ReLU mask -- the fp32 compare, the bf16 compare, the packed bf16 bit test of the wide big-tile epilogue
    (relu_mask2) and the split-layout bit test on hi (the activations saved by the bf16x3 / f16x3 forwards) -- agrees with torch."""
    from efficientdet.pytorch_amd import ops, _lib as L
    from efficientdet.pytorch_amd.ops import Map
    dz, w, q, ref = _mask_case()
    B, Cin, H, W = dz.shape
    knobs = []
    try:
        if form in ('bf16', 'bf16_big'):
            dz, w = dz.bfloat16().float(), w.bfloat16().float()
            ref = F.conv2d(dz.double(), w.double(), padding=1)
            ref = torch.where(q.double() <= 0, torch.zeros_like(ref), ref)
        if form == 'bf16_big':
            knobs = [(L.TUNE_IGEMM_BIG_MIN_M, ops.tuning_set(L.TUNE_IGEMM_BIG_MIN_M, 0)), (L.TUNE_IGEMM_BIG, ops.tuning_set(L.TUNE_IGEMM_BIG, 442))]
        if form == 'split_pers':
            knobs = [(L.TUNE_IGEMM_BIG_MIN_M, ops.tuning_set(L.TUNE_IGEMM_BIG_MIN_M, 0)), (L.TUNE_SPLIT_PERS, ops.tuning_set(L.TUNE_SPLIT_PERS, 1))]
        if form.startswith('split'):
            ym = Map.new(B, H, W, 256, torch.float32, 'cuda')
            ops.conv2d(Map.of(ops.to_split(_nhwc(dz))), ops.pack_weight(w.cuda(), torch.float32, x3=True), ym, Cin=Cin, Cout=256, KH=3,
                       KW=3, pad_t=1, pad_l=1, res=Map.of(ops.to_split(_nhwc(q))), res_mode=ops.RES_RELU_MASK, split=True)
            torch.cuda.synchronize()
            got = from_split(ym.tensor()).permute(0, 3, 1, 2)
            tol = 1e-3
        else:
            ops.set_f32_arith('f32')
            dt = torch.float32 if form == 'f32' else torch.bfloat16
            ym = Map.new(B, H, W, 256, dt, 'cuda')
            ops.conv2d(Map.of(_nhwc(dz, dt)), ops.pack_weight(w.cuda(), dt), ym, Cin=Cin, Cout=256, KH=3, KW=3, pad_t=1, pad_l=1,
                       res=Map.of(_nhwc(q, dt)), res_mode=ops.RES_RELU_MASK)
            torch.cuda.synchronize()
            got = _nchw(ym.tensor())
            tol = 2e-4 if dt == torch.float32 else 2e-2
    finally:
        for k, v in knobs:
            ops.tuning_set(k, v)
    assert_nonfinite_match(got, ref, tol, what='relu mask ' + form)
    # the masked positions are exactly zero, the NaN positions carry the gradient
    assert float(got[0, :, 4, 4].abs().max()) == 0.0 and float(got[0, ::2, 6, 6].abs().max()) == 0.0
    assert float(got[0, :, 0, 0].abs().max()) > 0.0 and float(got[0, :, 1, 1].abs().max()) > 0.0


# ----------------------------------------------------------------------------- BiFPN fusion node
def _fuse_ref(a, b, c, wraw, col, mode):
    eps = 1e-4
    wn = F.relu(wraw); wn = wn / (wn.sum(0) + eps)
    if mode == 0:
        return (wn[0, col] * a + wn[1, col] * F.interpolate(b, scale_factor=2, mode='nearest')) / (wn[0, col] + wn[1, col] + eps)
    if mode == 1:
        return (wn[0, col] * a + wn[1, col] * F.max_pool2d(b, 2) + wn[2, col] * c) / (wn[0, col] + wn[1, col] + wn[2, col] + eps)
    return (wn[0, col] * a + wn[1, col] * F.max_pool2d(b, 2)) / (wn[0, col] + wn[1, col] + eps)


@pytest.mark.parametrize('wcase', ['plain', 'negative_zero', 'nan_other_col', 'nan'])
@pytest.mark.parametrize('mode', [0, 1, 2])
def test_bifpn_fuse_keeps_nonfinite(mode, wcase):
    """A NaN at each of the 4 positions of a max-pool window (and two NaNs in one window: torch routes the gradient to the LAST),
    +-inf elsewhere; fusion weights negative / zero / NaN (in the node's own column or in another one).  Forward (plain and H-split
    output), the data gradients and the weight gradient against float64 autograd."""
    from efficientdet.pytorch_amd import ops
    from efficientdet.pytorch_amd.ops import Map
    g = torch.Generator().manual_seed(30 + mode)
    B, H, W, C = 2, 6, 8, 64
    rows, cols, col = (3, 3, 1) if mode == 1 else (2, 5, 2)
    wraw = 0.2 + torch.rand(rows, cols, generator=g)
    if wcase == 'negative_zero':
        wraw[0, col] = -0.3; wraw[1, col] = 0.0
    elif wcase == 'nan_other_col':
        wraw[1, col - 1] = NAN
    elif wcase == 'nan':
        wraw[1, col] = NAN
    a = torch.randn(B, C, H, W, generator=g)
    bshape = (B, C, H // 2, W // 2) if mode == 0 else (B, C, 2 * H, 2 * W)
    b = torch.randn(bshape, generator=g)
    c = torch.randn(B, C, H, W, generator=g) if mode == 1 else None
    if mode == 0:
        b[0, 3, 1, 1] = NAN; b[1, 4, 2, 3] = INF; b[1, 5, 0, 0] = -INF; b[0, 8, 2, 2] = NEG_NAN
    else:
        for qd in range(4):                              # window (2, qd + 1) of channel 3 + qd: NaN at position qd
            b[0, 3 + qd, 4 + (qd >> 1), 2 * (qd + 1) + (qd & 1)] = NAN
        b[1, 9, 6, 6] = NEG_NAN; b[1, 9, 7, 7] = NAN                       # two NaNs in one window
        b[1, 10, 0, 0] = INF; b[1, 11, 3, 2] = -INF
        b[0, 12, 8, 8] = -INF; b[0, 12, 8, 9] = -INF; b[0, 12, 9, 8] = -INF; b[0, 12, 9, 9] = -INF
    a[1, 0, 1, 1] = NAN; a[0, 2, 3, 3] = INF
    wd = wraw.double().requires_grad_(True)
    ad, bd = a.double().requires_grad_(True), b.double().requires_grad_(True)
    cd = c.double().requires_grad_(True) if c is not None else None
    out = _fuse_ref(ad, bd, cd, wd, col, mode)
    dout = torch.randn(out.shape, generator=g)
    out.backward(dout.double())
    am, bm = Map.of(_nhwc(a)), Map.of(_nhwc(b))
    cm = Map.of(_nhwc(c)) if c is not None else None
    wdev = wraw.cuda()
    om, oh = ops.bifpn_fuse_fwd(am, bm, cm, wdev, col, mode, plain=True, hsplit=True)
    da = Map.new(B, H, W, C, torch.float32, 'cuda'); db = Map.new(bm.B, bm.H, bm.W, C, torch.float32, 'cuda')
    dc = Map.new(B, H, W, C, torch.float32, 'cuda') if mode == 1 else None
    dn = torch.zeros(ops.fuse_dn_floats(cols), device='cuda')
    ops.bifpn_fuse_bwd(Map.of(_nhwc(dout)), am, bm, cm, da, db, dc, False, False, False, wdev, dn, col, mode)
    dw = torch.zeros(rows, cols, device='cuda')
    ops.bifpn_weight_bwd(wdev, dn, dw)
    torch.cuda.synchronize()
    what = 'fuse mode %d %s' % (mode, wcase)
    assert_nonfinite_match(_nchw(om.tensor()), out, 2e-4, what=what + ' fwd')
    assert_nonfinite_match(from_hsplit(oh.tensor())[0].permute(0, 3, 1, 2), out, 2e-4, exact=False, what=what + ' fwd hsplit')
    assert_nonfinite_match(_nchw(da.tensor()), ad.grad, 2e-4, what=what + ' da')
    assert_nonfinite_match(_nchw(db.tensor()), bd.grad, 2e-4, what=what + ' db')
    if mode == 1:
        assert_nonfinite_match(_nchw(dc.tensor()), cd.grad, 2e-4, what=what + ' dc')
    # (dwraw: only the node's own column -- the kernel writes its column's partial sums; other columns' dn is from other nodes)
    assert_nonfinite_match(dw.cpu()[:, col], wd.grad[:, col], 2e-3, what=what + ' dw')


# ----------------------------------------------------------------------------- focal loss
def _loss_case(nc=20, S=128, B=3, seed=4):
    """Probabilities with NaN at a positive, a negative and an ignored anchor of image 0, a NaN everywhere in image 1's first anchor,
    image 2 without annotations (with a NaN); NaN regression at a positive and at a negative anchor; clamp-edge probabilities."""
    g = torch.Generator().manual_seed(seed)
    anc = O.anchors_for_image(S, S)
    A = anc.shape[1]
    _, ann = O.synthetic_batch(B, S, seed=5, num_classes=nc)
    ann[2] = -1.0
    cls = torch.sigmoid(torch.randn(B, A, nc, generator=g) * 2.0)
    reg = torch.randn(B, A, 4, generator=g) * 0.5
    info = {}
    for j in range(2):
        a_ = ann[j][ann[j][:, 4] != -1]
        iou = O.calc_iou(anc[0], a_[:, :4]).max(dim=1)[0]
        pos = torch.nonzero(iou >= 0.5).reshape(-1); neg = torch.nonzero(iou < 0.4).reshape(-1)
        ign = torch.nonzero((iou >= 0.4) & (iou < 0.5)).reshape(-1)
        assert len(pos) >= 2 and len(neg) >= 2 and len(ign) >= 1, (j, len(pos), len(neg), len(ign))
        info[j] = (pos, neg, ign)
    pos, neg, ign = info[0]
    cls[0, pos[0], 3] = NAN; cls[0, neg[0], 0] = NAN; cls[0, ign[0], 5] = NAN
    reg[0, pos[1], 2] = NAN; reg[0, neg[1], 0] = NAN
    cls[2, 7, 1] = NAN
    # the clamp's gradient edge: exactly at 1e-4 / 1 - 1e-4 and one ulp either side (image 1, negatives and the positive's row)
    p1, n1, _ = info[1]
    lo = torch.tensor(1e-4, dtype=torch.float32); hi = torch.tensor(1.0 - 1e-4, dtype=torch.float32)
    edge = [lo, torch.nextafter(lo, torch.tensor(0.0)), torch.nextafter(lo, torch.tensor(1.0)),
            hi, torch.nextafter(hi, torch.tensor(0.0)), torch.nextafter(hi, torch.tensor(1.0))]
    for i, e in enumerate(edge):
        cls[1, n1[i % len(n1)], i] = e
        cls[1, p1[0], i] = e
    return cls, reg, anc, ann


def _loss_ref(cls, reg, anc, ann, gs):
    c = cls.clone().requires_grad_(True); r = reg.clone().requires_grad_(True)
    cl, rl = O.focal_loss(c, r, anc, ann)
    (gs[0] * cl.sum() + gs[1] * rl.sum()).backward()
    # d/d(logit) through the sigmoid that produced the probabilities: autograd multiplies even a zero gradient by p (1 - p)
    return torch.cat([cl.detach(), rl.detach()]), c.grad * cls * (1 - cls), r.grad


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_focal_loss_keeps_nonfinite(dtype):
    from efficientdet.pytorch_amd import ops
    nc = 20
    cls, reg, anc, ann = _loss_case(nc)
    B, A, _ = cls.shape
    gs = torch.tensor([0.7, 1.3])
    ref_l, ref_dl, ref_dr = _loss_ref(cls, reg, anc, ann, gs)
    assert bool(torch.isnan(ref_l).all())                                    # (the NaNs reach both losses)
    tol = 1e-3 if dtype == torch.float32 else 1e-2
    cu, ru, au, nu, gu = cls.cuda(), reg.cuda(), anc.cuda(), ann.cuda(), gs.cuda()
    losses, ws = ops.focal_loss_fwd(cu, ru, au, nu)
    assert_nonfinite_match(losses.cpu(), ref_l, 2e-4, what='losses')
    dcls, dreg = ops.focal_loss_bwd(cu, ru, au, nu, gu, ws, dtype)
    assert_nonfinite_match(dcls.float().cpu(), ref_dl, tol, what='dcls')
    assert_nonfinite_match(dreg.float().cpu(), ref_dr, tol, what='dreg')
    dld = (9 * nc + 63) // 64 * 64
    dpix, dreg2 = ops.focal_loss_bwd_pix(cu, ru, au, nu, gu, ws, dtype, dld)
    assert_nonfinite_match(dpix[:, :, :9 * nc].reshape(B, A, nc).float().cpu(), ref_dl, tol, what='dcls pix')
    assert_nonfinite_match(dreg2.float().cpu(), ref_dr, tol, what='dreg (bwd_pix)')
    assert float(dpix[:, :, 9 * nc:].float().abs().max()) == 0.0
    losses2, ws2, dpix1 = ops.focal_loss_fwd_grad(cu, ru, au, nu, dtype, dld)
    assert_nonfinite_match(losses2.cpu(), ref_l, 2e-4, what='losses (fwd_grad)')
    assert_nonfinite_match(dpix1[:, :, :9 * nc].reshape(B, A, nc).float().cpu() * float(gs[0]), ref_dl, tol, what='dcls (fwd_grad)')
    dreg3 = ops.focal_loss_bwd_reg(ru, au, nu, gu, ws2, dtype)
    assert_nonfinite_match(dreg3.float().cpu(), ref_dr, tol, what='dreg (bwd_reg)')


def test_focal_loss_ignored_and_empty_images_stay_finite():
    """NaN only where the reference's loss does not look (an ignored anchor, an image without annotations): finite losses, like the
    reference, and a NaN gradient only at those elements (sigmoid's backward of a NaN probability)."""
    from efficientdet.pytorch_amd import ops
    nc = 20
    cls, reg, anc, ann = _loss_case(nc)
    keep = torch.isnan(cls)
    cls = torch.where(keep, torch.full_like(cls, 0.3), cls)
    a_ = ann[0][ann[0][:, 4] != -1]
    iou = O.calc_iou(anc[0], a_[:, :4]).max(dim=1)[0]
    ign = torch.nonzero((iou >= 0.4) & (iou < 0.5)).reshape(-1)
    cls[0, ign[0], :] = NAN
    cls[2, 11, 4] = NAN
    reg = torch.nan_to_num(reg)
    gs = torch.tensor([1.0, 1.0])
    ref_l, ref_dl, ref_dr = _loss_ref(cls, reg, anc, ann, gs)
    assert bool(torch.isfinite(ref_l).all())
    losses, ws = ops.focal_loss_fwd(cls.cuda(), reg.cuda(), anc.cuda(), ann.cuda())
    assert_nonfinite_match(losses.cpu(), ref_l, 2e-4, what='losses')
    dld = (9 * nc + 63) // 64 * 64
    losses2, ws2, dpix1 = ops.focal_loss_fwd_grad(cls.cuda(), reg.cuda(), anc.cuda(), ann.cuda(), torch.float32, dld)
    assert_nonfinite_match(losses2.cpu(), ref_l, 2e-4, what='losses (fwd_grad)')
    B, A, _ = cls.shape
    assert_nonfinite_match(dpix1[:, :, :9 * nc].reshape(B, A, nc).cpu(), ref_dl, 1e-3, what='dcls (fwd_grad)')


# ----------------------------------------------------------------------------- decode + class max
def test_decode_score_keeps_nonfinite():
    from efficientdet.pytorch_amd import ops
    g = torch.Generator().manual_seed(2)
    H, W, B, nc = 256, 128, 2, 20
    anc = O.anchors_for_image(H, W)
    A = anc.shape[1]
    assert (B * A) % 64 != 0                                     # the last 64-anchor block is partial
    reg = torch.randn(B, A, 4, generator=g)
    cls = torch.rand(B, A, nc, generator=g)
    cls[0, 10, 0] = NAN; cls[0, 11, 9] = NAN; cls[0, 12, nc - 1] = NAN; cls[0, 13, 4] = NEG_NAN; cls[0, 13, 15] = NAN
    cls[1, A - 1, 7] = NAN; cls[1, A - 2, nc - 1] = NAN                   # inside the partial block
    reg[0, 20, 0] = NAN; reg[0, 21, 1] = INF; reg[0, 22, 2] = NAN; reg[0, 23, 3] = -INF
    reg[0, 24, 2] = 500.0; reg[0, 25, 3] = 500.0; reg[1, A - 1, 2] = INF; reg[1, A - 3, 0] = -INF   # expf overflows
    ref = O.decode_clip(anc.double(), reg.double(), H, W)
    boxes, score, label = ops.decode_score(anc.cuda(), reg.cuda(), cls.cuda(), H, W)
    torch.cuda.synchronize()
    assert_nonfinite_match(boxes.cpu(), ref, 1e-5, what='boxes')
    ms, ml = cls.max(dim=2)
    assert_nonfinite_match(score.cpu(), ms, 0.0, what='score')
    assert torch.equal(label.cpu().long(), ml)                       # (a NaN row: the index of its first NaN, like torch.max)
    assert bool(torch.isnan(boxes[0, 20]).any()) and bool(torch.isnan(score[0, 12]))


# ----------------------------------------------------------------------------- ClipAdamW
@pytest.mark.parametrize('bad', [NAN, INF])
@pytest.mark.parametrize('max_norm', [0.1, 0.0])
def test_clip_adamw_keeps_nonfinite(max_norm, bad):
    """One non-finite gradient element against clip_grad_norm_ + torch.optim.AdamW (test_clip_adamw_matches_torch's setup): a NaN norm
    turns every gradient into NaN, an inf norm zeroes the finite ones (and makes the inf one NaN)."""
    import math
    from efficientdet.pytorch_amd.optim import ClipAdamW
    g = torch.Generator().manual_seed(22)
    shapes = [(64, 32, 3, 3), (17,), (4097,), (3, 5, 7), (1,)]
    pa = [torch.randn(s, generator=g).cuda().requires_grad_(True) for s in shapes]
    pb = [p.detach().clone().requires_grad_(True) for p in pa]
    oa = ClipAdamW(pa, lr=1e-2, weight_decay=0.01, max_norm=max_norm)
    ob = torch.optim.AdamW(pb, lr=1e-2, weight_decay=0.01)
    for it in range(3):
        for i, (a, b) in enumerate(zip(pa, pb)):
            gr = torch.randn(a.shape, generator=g).cuda()
            if it == 1 and i == 2:
                gr[100] = bad
            a.grad = gr; b.grad = gr.clone()
        ref_norm = torch.nn.utils.clip_grad_norm_(pb, max_norm) if max_norm else None
        oa.step(); ob.step()
        torch.cuda.synchronize()
        if max_norm:
            n, r = float(oa.grad_norm()), float(ref_norm)
            assert (math.isnan(n), math.isinf(n)) == (math.isnan(r), math.isinf(r)), (it, n, r)
            if math.isfinite(r):
                assert abs(n - r) <= 2e-6 * r
        for a, b in zip(pa, pb):
            assert_nonfinite_match(a.detach().cpu(), b.detach().cpu(), 1e-5, what='param step %d' % it)


# ----------------------------------------------------------------------------- fp16 range watch
def _flag():
    from efficientdet.pytorch_amd import ops
    return ops.range_flag(torch.device('cuda', torch.cuda.current_device()))


@pytest.mark.parametrize('bad', [NAN, NEG_NAN, INF, -INF, 65520.0, 65504.0])
def test_range_watch_sees_one_bad_lane(bad):
    """One value fp16 cannot hold in ANY lane of a 4-channel quad, the rest finite, sets the watch in each H-split producer: the pyramid
    conversion, the BiFPN fusion output and the conv epilogue.  65504 (fp16's largest) does not."""
    from efficientdet.pytorch_amd import ops
    from efficientdet.pytorch_amd.ops import Map
    want = bad != 65504.0
    for lane in range(4):
        x = torch.full((1, 2, 2, 64), 0.5, device='cuda')
        x[0, 1, 0, 36 + lane] = bad
        _flag().zero_(); to_split2(x, bf=False); torch.cuda.synchronize()
        assert bool(_flag().item()) == want, ('to_split2', bad, lane)
        # fusion (mode 0, weights 1 / 0: the output is a)
        a = torch.full((1, 4, 4, 64), 0.25, device='cuda'); a[0, 2, 3, 8 + lane] = bad
        b = torch.full((1, 2, 2, 64), 0.25, device='cuda')
        wraw = torch.tensor([[1.0], [0.0]], device='cuda')
        _flag().zero_(); ops.bifpn_fuse_fwd(Map.of(a), Map.of(b), None, wraw, 0, 0, plain=False, hsplit=True); torch.cuda.synchronize()
        if bad != 65520.0:                    # (65520 * 1 / (1 + 1e-4) is back in range)
            assert bool(_flag().item()) == want, ('fuse', bad, lane)
        # conv H-split epilogue: x = 0, so the output is the bias
        bias = torch.full((256,), 0.1, device='cuda'); bias[100 + lane] = bad
        xm = Map.of(to_split2(torch.zeros(1, 4, 4, 64, device='cuda'), bf=False)[1])
        ym = Map.new(1, 4, 4, 256, torch.float32, 'cuda')
        _flag().zero_()
        ops.conv2d(xm, ops.pack_weight(torch.randn(256, 64, 3, 3, device='cuda'), torch.float32, h3=True), ym, Cin=64, Cout=256, KH=3,
                   KW=3, pad_t=1, pad_l=1, shift=bias, hsplit=True)
        torch.cuda.synchronize()
        assert bool(_flag().item()) == want, ('conv epilogue', bad, lane)
    _flag().zero_()


# ----------------------------------------------------------------------------- the watch reports the guarded call's own overflow
def test_detect_is_not_failed_by_an_earlier_overflow():
    """An overflow outside detect() (a diverged training forward sets the same device word) must not make the next detect() on clean
    input raise: detect() and GraphedDetect start with a clean watch.  An overflow inside them still raises (tests/test_gpu_hsplit.py)."""
    from efficientdet.pytorch_amd import EfficientDet, EFFICIENTDET
    from efficientdet.pytorch_amd.graph import GraphedDetect
    net, nc = 'efficientdet-d0', 20
    c = EFFICIENTDET[net]
    m = EfficientDet(nc, network=net, W_bifpn=c['W_bifpn'], D_bifpn=c['D_bifpn'], D_class=c['D_class'], compute_dtype=torch.float32,
                     f32_arith='f32_hf16x3_bwd_bf16x3')
    m.load_state_dict(O.make_state_dict(net, nc, seed=0)); m = m.cuda().eval(); m.is_training = False
    img, _ = O.synthetic_batch(2, 128, seed=1, num_classes=nc)
    img = img.cuda()
    clean = m.detect(img)
    to_split2(torch.full((1, 1, 1, 32), 7.0e4, device='cuda'), bf=False)            # an overflow that belongs to someone else
    for (s, l, b), (rs, rl, rb) in zip(m.detect(img), clean):
        assert torch.equal(l, rl) and torch.equal(s, rs) and torch.equal(b, rb)
    det = GraphedDetect(m, img)
    first = det()
    to_split2(torch.full((1, 1, 1, 32), 7.0e4, device='cuda'), bf=False)
    for (s, l, b), (rs, rl, rb) in zip(det(), first):
        assert torch.equal(l, rl) and torch.equal(s, rs) and torch.equal(b, rb)
