"""GPU parity: BiFPN fast-normalised fusion nodes forward/backward (incl. raw weight gradients)."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.gpu_util import assert_close
from tests.test_gpu_backbone_ops import nhwc, nchw, q_, TOL, DT

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('mode', [0, 1, 2])
def test_fuse_node(dtype, mode):
    from efficientdet.pytorch_amd import ops
    from efficientdet.pytorch_amd.ops import Map
    g = torch.Generator().manual_seed(10 + mode)
    q = q_(dtype)
    B, H, W, C = 2, 6, 8, 64
    rows, cols, col = (3, 3, 1) if mode == 1 else (2, 5, 2)
    wraw = (0.2 + torch.rand(rows, cols, generator=g))
    if mode == 0:
        wraw[1, 3] = -0.4
    wraw.requires_grad_(True)
    a = q(torch.randn(B, C, H, W, generator=g)).requires_grad_(True)
    bshape = (B, C, H // 2, W // 2) if mode == 0 else (B, C, 2 * H, 2 * W)
    b = q(torch.randn(bshape, generator=g)).requires_grad_(True)
    c = q(torch.randn(B, C, H, W, generator=g)).requires_grad_(True) if mode == 1 else None
    eps = 1e-4
    wn = F.relu(wraw); wn = wn / (wn.sum(0) + eps)
    if mode == 0:
        out = (wn[0, col] * a + wn[1, col] * F.interpolate(b, scale_factor=2, mode='nearest')) / (wn[0, col] + wn[1, col] + eps)
    elif mode == 1:
        out = (wn[0, col] * a + wn[1, col] * F.max_pool2d(b, 2) + wn[2, col] * c) / (wn[0, col] + wn[1, col] + wn[2, col] + eps)
    else:
        out = (wn[0, col] * a + wn[1, col] * F.max_pool2d(b, 2)) / (wn[0, col] + wn[1, col] + eps)
    dout = q(torch.randn(out.shape, generator=g))
    out.backward(dout)
    dev = 'cuda'
    am, bm = nhwc(a.detach(), dtype), nhwc(b.detach(), dtype)
    cm = nhwc(c.detach(), dtype) if c is not None else None
    wd = wraw.detach().to(dev)
    om = ops.bifpn_fuse_fwd(am, bm, cm, wd, col, mode)
    torch.cuda.synchronize()
    assert_close(nchw(om), out.detach(), TOL[dtype], 'fuse fwd')
    da = Map.new(am.B, am.H, am.W, C, dtype, dev); db = Map.new(bm.B, bm.H, bm.W, C, dtype, dev)
    dc = Map.new(am.B, am.H, am.W, C, dtype, dev) if mode == 1 else None
    dn = torch.zeros(ops.fuse_dn_floats(cols), device=dev)
    ops.bifpn_fuse_bwd(nhwc(dout, dtype), am, bm, cm, da, db, dc, False, False, False, wd, dn, col, mode)
    dw = torch.zeros(rows, cols, device=dev)
    ops.bifpn_weight_bwd(wd, dn, dw)
    torch.cuda.synchronize()
    assert_close(nchw(da), a.grad, TOL[dtype], 'fuse da'); assert_close(nchw(db), b.grad, TOL[dtype], 'fuse db')
    if mode == 1:
        assert_close(nchw(dc), c.grad, TOL[dtype], 'fuse dc')
    assert_close(dw.cpu(), wraw.grad, 3e-2 if dtype == torch.bfloat16 else 2e-3, 'fuse dw')
    # accumulate flags
    da2 = Map.of(da.tensor().clone())
    ops.bifpn_fuse_bwd(nhwc(dout, dtype), am, bm, cm, da2, db, dc, True, False, False, wd, dn, col, mode)
    assert_close(nchw(da2), q(2 * a.grad), 2 * TOL[dtype], 'fuse da accumulate')


# ----------------------------------------------------------------------------- edges: launch caps, weight tables, stale partial rows,
# accumulate flags, max-pool ties, small / odd shapes, refusals.  Reference: fp64 torch autograd.
EPS = 1e-4
DW_TOL = {torch.float32: 2e-3, torch.bfloat16: 3e-2}


def _node_ref(mode, wraw, col, a, b, c):
    """One fusion node in torch (fp64 when its inputs are)."""
    wn = F.relu(wraw); wn = wn / (wn.sum(0) + EPS)
    if mode == 0:
        return (wn[0, col] * a + wn[1, col] * F.interpolate(b, scale_factor=2, mode='nearest')) / (wn[0, col] + wn[1, col] + EPS)
    if mode == 1:
        return (wn[0, col] * a + wn[1, col] * F.max_pool2d(b, 2) + wn[2, col] * c) / (wn[0, col] + wn[1, col] + wn[2, col] + EPS)
    return (wn[0, col] * a + wn[1, col] * F.max_pool2d(b, 2)) / (wn[0, col] + wn[1, col] + EPS)


def _b_shape(mode, B, H, W, C):
    return (B, C, H // 2, W // 2) if mode == 0 else (B, C, 2 * H, 2 * W)


def _inputs(g, q, mode, B, H, W, C):
    """-> (a, b, c or None, dout) NCHW fp32, representable in the dtype q rounds to."""
    a = q(torch.randn(B, C, H, W, generator=g))
    b = q(torch.randn(_b_shape(mode, B, H, W, C), generator=g))
    c = q(torch.randn(B, C, H, W, generator=g)) if mode == 1 else None
    return a, b, c, q(torch.randn(B, C, H, W, generator=g))


def _ref_grads(mode, wraw, col, a, b, c, dout, dtype=torch.float64):
    """-> (out, da, db, dc or None, dwraw) of one node by autograd in dtype."""
    w = wraw.to(dtype).requires_grad_(True)
    t = [x.to(dtype).requires_grad_(True) if x is not None else None for x in (a, b, c)]
    out = _node_ref(mode, w, col, *t)
    out.backward(dout.to(dtype))
    return out.detach(), t[0].grad, t[1].grad, t[2].grad if t[2] is not None else None, w.grad


def _dev_fwd_bwd(dtype, mode, wraw, col, a, b, c, dout, dn=None, acc=(False, False, False), into=None):
    """Forward + backward of one node on the device.  dn: the table's partial-row scratch (fresh zeros when None); into: (da, db, dc)
    Maps to write / accumulate into (fresh ones when None).  -> (out, da, db, dc, dn) with the maps as NCHW fp32 CPU tensors."""
    from efficientdet.pytorch_amd import ops
    from efficientdet.pytorch_amd.ops import Map
    dev = 'cuda'
    am, bm = nhwc(a, dtype), nhwc(b, dtype)
    cm = nhwc(c, dtype) if c is not None else None
    wd = wraw.detach().float().to(dev)
    om = ops.bifpn_fuse_fwd(am, bm, cm, wd, col, mode)
    C = a.shape[1]
    if into is None:
        into = (Map.new(am.B, am.H, am.W, C, dtype, dev), Map.new(bm.B, bm.H, bm.W, C, dtype, dev),
                Map.new(am.B, am.H, am.W, C, dtype, dev) if mode == 1 else None)
    da, db, dc = into
    if dn is None:
        dn = torch.zeros(ops.fuse_dn_floats(wraw.shape[1]), device=dev)
    ops.bifpn_fuse_bwd(nhwc(dout, dtype), am, bm, cm, da, db, dc, acc[0], acc[1], acc[2], wd, dn, col, mode)
    torch.cuda.synchronize()
    return nchw(om), nchw(da), nchw(db), nchw(dc) if dc is not None else None, dn


def _dev_dw(wraw, dn):
    from efficientdet.pytorch_amd import ops
    dw = torch.zeros(wraw.shape, device='cuda')
    ops.bifpn_weight_bwd(wraw.detach().float().cuda(), dn, dw)
    torch.cuda.synchronize()
    return dw.cpu()


def _check_node(dtype, mode, wraw, col, tensors, ref, what):
    out, da, db, dc, dn = _dev_fwd_bwd(dtype, mode, wraw, col, *tensors)
    assert_close(out, ref[0], TOL[dtype], what + ' fwd')
    assert_close(da, ref[1], TOL[dtype], what + ' da'); assert_close(db, ref[2], TOL[dtype], what + ' db')
    if mode == 1:
        assert_close(dc, ref[3], TOL[dtype], what + ' dc')
    dw = _dev_dw(wraw, dn)
    other = torch.ones(wraw.shape[1], dtype=torch.bool); other[col] = False
    assert float(dw[:, other].abs().max()) == 0.0, what + ': a column that was never launched'
    assert_close(dw, ref[4], DW_TOL[dtype], what + ' dw')
    return dn


def _wraw(g, mode):
    rows, cols = (3, 3) if mode == 1 else (2, 5)
    return 0.2 + torch.rand(rows, cols, generator=g)


OVER_CAPS = {0: (2, 256, 320, 64, 1), 1: (2, 192, 192, 64, 2), 2: (2, 192, 192, 64, 4)}       # mode -> B, H, W (of a / out), C, column


@functools.lru_cache(maxsize=1)
def _over_caps_case(mode):
    """Inputs representable in bf16, so both dtypes share one fp64 reference (kept for the mode being tested only: ~0.5 GB)."""
    B, H, W, C, col = OVER_CAPS[mode]
    g = torch.Generator().manual_seed(40 + mode)
    wraw = _wraw(g, mode)
    t = _inputs(g, q_(torch.bfloat16), mode, B, H, W, C)
    ref = _ref_grads(mode, wraw, col, *t)
    return wraw, col, t, tuple(x.float() if x is not None and x.dim() == 4 else x for x in ref)      # dw stays fp64


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('mode', [0, 1, 2])
def test_fuse_node_over_the_launch_caps(dtype, mode):
    """More work than one pass of the capped grids: fp32 forward of modes 1/2 at 192 x 192 is 4608 workgroups' worth against the cap of
    4096; backward is 4608 (modes 1/2) and 2560 (mode 0, fine grid 256 x 320) against EFFDET_FUSE_MAX_WG = 2048 (bf16: half of each,
    still over the backward cap in modes 1/2).  Every launch writes 2048 partial rows: the weight-gradient kernel's w += 256 loop runs 8
    times.  dw sums ~10M terms (|dw| ~ 1e3): an fp32 torch autograd differs from the fp64 one at these shapes by 1.2e-7 .. 2.9e-7 of
    |dw|_max, so the op tolerances 2e-3 / 3e-2 hold here as they are."""
    from efficientdet.pytorch_amd import ops
    wraw, col, t, ref = _over_caps_case(mode)
    B, H, W, C, _ = OVER_CAPS[mode]
    ce = 4 if dtype == torch.float32 else 8
    coarse = B * (H // 2) * (W // 2) * (C // ce) if mode == 0 else B * H * W * (C // ce)
    if dtype == torch.float32:
        assert coarse > 2048 * 256 and (mode == 0 or coarse > 4096 * 256)
    dn = _check_node(dtype, mode, wraw, col, t, ref, 'over the caps, mode %d' % mode)
    base = col * ops.FUSE_COL_FLOATS
    assert float(dn[base]) == min(2048, (coarse + 255) // 256)


def _table_nodes(table):
    """-> [(mode, column, H, W)] of every node of a weight table, each at its own level size (B = 2, C = 64)."""
    if table == 'w1':      # [2, 5]: the top-down nodes (mode 0) on columns 0-3, the last bottom-up node (mode 2) on column 4
        return [(0, 0, 96, 96), (0, 1, 40, 40), (0, 2, 16, 24), (0, 3, 8, 8), (2, 4, 5, 5)]
    return [(1, 0, 40, 40), (1, 1, 12, 20), (1, 2, 3, 5)]      # w2 [3, 3]: the bottom-up nodes (mode 1)


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('table', ['w1', 'w2'])
def test_whole_weight_table(dtype, table):
    """Every column of a table filled by its own launch (different sizes -> different numbers of partial rows, 288 for the largest),
    then ONE bifpn_weight_bwd for the table, as bifpn_module_bwd does: the whole dw against autograd of the summed nodes, including
    the negative weight whose ReLU gradient is zero."""
    from efficientdet.pytorch_amd import ops
    g = torch.Generator().manual_seed(60 + len(table))
    q = q_(dtype)
    B, C = 2, 64
    wraw = 0.2 + torch.rand((2, 5) if table == 'w1' else (3, 3), generator=g)
    neg = (1, 3) if table == 'w1' else (2, 1)
    wraw[neg] = -0.4
    w64 = wraw.double().requires_grad_(True)
    dn = torch.zeros(ops.fuse_dn_floats(wraw.shape[1]), device='cuda')
    for mode, col, H, W in _table_nodes(table):
        t = _inputs(g, q, mode, B, H, W, C)
        _node_ref(mode, w64, col, *[x.double() if x is not None else None for x in t[:3]]).backward(t[3].double())
        _dev_fwd_bwd(dtype, mode, wraw, col, *t, dn=dn)
        chunks = (B * (H // 2) * (W // 2) if mode == 0 else B * H * W) * (C // (4 if dtype == torch.float32 else 8))
        assert float(dn[col * ops.FUSE_COL_FLOATS]) == (chunks + 255) // 256         # one partial row per workgroup
    dw = _dev_dw(wraw, dn)
    assert float(w64.grad[neg]) == 0.0 and float(dw[neg]) == 0.0
    assert int((w64.grad != 0).sum()) == wraw.numel() - 1
    assert_close(dw, w64.grad, DW_TOL[dtype], 'dw of the whole %s table' % table)


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('mode', [0, 1])
def test_stale_partial_rows_are_not_summed(dtype, mode):
    """A large launch, then a small one on the same column of the same dn: the rows the small launch did not rewrite still hold the
    large launch's partials.  dw must be bit-equal to the small launch on a zeroed dn."""
    from efficientdet.pytorch_amd import ops
    g = torch.Generator().manual_seed(70 + mode)
    q = q_(dtype)
    wraw = _wraw(g, mode)
    col = 1
    big = _inputs(g, q, mode, 2, 64, 64, 64)
    small = _inputs(g, q, mode, 1, 4, 6, 64)
    dn = _dev_fwd_bwd(dtype, mode, wraw, col, *big)[4]
    nbig = int(dn[col * ops.FUSE_COL_FLOATS])
    _dev_fwd_bwd(dtype, mode, wraw, col, *small, dn=dn)
    nsmall = int(dn[col * ops.FUSE_COL_FLOATS])
    assert nsmall < nbig
    rows = dn[col * ops.FUSE_COL_FLOATS + 4 + 3 * nsmall: col * ops.FUSE_COL_FLOATS + 4 + 3 * nbig]
    assert float(rows.abs().max()) > 0.0                             # the stale rows are really there
    fresh = _dev_fwd_bwd(dtype, mode, wraw, col, *small)[4]
    assert torch.equal(_dev_dw(wraw, dn), _dev_dw(wraw, fresh))
    assert_close(_dev_dw(wraw, dn), _ref_grads(mode, wraw, col, *small)[4], DW_TOL[dtype], 'dw after a larger launch')


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('mode,flag', [(0, 1), (1, 1), (1, 2), (2, 1)])
def test_accumulate_into_nonzero_buffers(dtype, mode, flag):
    """db_acc (flag 1; modes 0, 1 and 2) and dc_acc (flag 2) add to what the buffer holds; the other outputs are overwritten."""
    from efficientdet.pytorch_amd.ops import Map
    g = torch.Generator().manual_seed(80 + 3 * mode + flag)
    q = q_(dtype)
    B, H, W, C = 2, 6, 10, 64
    wraw = _wraw(g, mode)
    col = 2
    t = _inputs(g, q, mode, B, H, W, C)
    ref = _ref_grads(mode, wraw, col, *t)
    held = [q(torch.randn(B, C, H, W, generator=g)), q(torch.randn(_b_shape(mode, B, H, W, C), generator=g)),
            q(torch.randn(B, C, H, W, generator=g)) if mode == 1 else None]
    into = tuple(nhwc(x, dtype) if x is not None else None for x in held)
    acc = (False, flag == 1, flag == 2)
    _, da, db, dc, _ = _dev_fwd_bwd(dtype, mode, wraw, col, *t, acc=acc, into=into)
    assert_close(da, ref[1], TOL[dtype], 'da (overwritten)')
    assert_close(db, ref[2] + (held[1].double() if acc[1] else 0.0), TOL[dtype], 'db (accumulate %d)' % acc[1])
    if mode == 1:
        assert_close(dc, ref[3] + (held[2].double() if acc[2] else 0.0), TOL[dtype], 'dc (accumulate %d)' % acc[2])


def test_max_pool_tie_routing_of_the_reference():
    """What the ties test below compares with: torch sends the gradient of a tied 2x2 window to its FIRST maximum in row-major order."""
    for win, want in (([[1.0, 1.0], [1.0, 1.0]], 0), ([[0.0, 2.0], [2.0, 1.0]], 1), ([[0.0, 0.0], [0.0, 0.0]], 0)):
        x = torch.tensor(win, dtype=torch.float64).reshape(1, 1, 2, 2).requires_grad_(True)
        F.max_pool2d(x, 2).backward(torch.ones(1, 1, 1, 1, dtype=torch.float64))
        assert torch.nonzero(x.grad.reshape(-1)).reshape(-1).tolist() == [want]


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('mode', [1, 2])
def test_max_pool_ties_route_to_the_first_maximum(dtype, mode):
    """b in multiples of 0.5 (ties in most windows), an all-zero region (ties in every window), and two hand-made windows: db must be
    non-zero exactly where torch's is."""
    g = torch.Generator().manual_seed(90 + mode)
    B, H, W, C = 2, 9, 12, 64
    wraw = _wraw(g, mode)
    col = 0
    a, b, c, dout = _inputs(g, q_(dtype), mode, B, H, W, C)
    b = (b * 2).round().clamp(-2, 2) / 2                              # 9 values: exact in bf16
    b[:, :, 6:14, 4:16] = 0.0
    b[0, :, 0:2, 0:2] = torch.tensor([[1.0, 1.0], [1.0, 1.0]])        # constant window -> element 0
    b[0, :, 0:2, 2:4] = torch.tensor([[0.0, 2.0], [2.0, 1.0]])        # -> element 1
    dout = dout + 0.25 * dout.sign() + (dout == 0)                    # no zero upstream gradient: every window routes something
    dout = q_(dtype)(dout)
    ref = _ref_grads(mode, wraw, col, a, b, c, dout)
    win = F.unfold(b.reshape(-1, 1, 2 * H, 2 * W), 2, stride=2)
    tied = (win == win.max(dim=1, keepdim=True)[0]).sum(dim=1) > 1
    assert float(tied.float().mean()) > 0.5                          # most windows are tied
    _, _, db, _, _ = _dev_fwd_bwd(dtype, mode, wraw, col, a, b, c, dout)
    assert int((ref[2] != 0).sum()) == B * C * H * W                 # exactly one element per window
    assert torch.equal(db != 0, ref[2] != 0)
    assert bool((db[0, :, 0, 0] != 0).all()) and bool((db[0, :, 0, 3] != 0).all())
    assert_close(db, ref[2], TOL[dtype], 'db with ties')


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('mode', [1, 2])
@pytest.mark.parametrize('H,W', [(3, 5), (1, 7)])
def test_fuse_node_small_and_odd(dtype, mode, H, W):
    """Odd H and W, H = 1, at the narrowest channel count of the dtype (one 16-byte chunk per pixel: C = 4 in fp32, 8 in bf16)."""
    g = torch.Generator().manual_seed(100 + 10 * mode + H)
    C = 4 if dtype == torch.float32 else 8
    wraw = _wraw(g, mode)
    col = 1
    t = _inputs(g, q_(dtype), mode, 3, H, W, C)
    _check_node(dtype, mode, wraw, col, t, _ref_grads(mode, wraw, col, *t), 'mode %d at %dx%dx%d' % (mode, H, W, C))


@pytest.mark.parametrize('dtype', DT)
def test_fuse_refusals(dtype):
    """Mode 0 with an odd fine grid -> EFFDET_EUNSUPPORTED; a channel count that is no whole number of 16-byte chunks -> EFFDET_EINVAL;
    both from forward and backward, as errors of L.check."""
    g = torch.Generator().manual_seed(110)
    q = q_(dtype)
    ce = 4 if dtype == torch.float32 else 8

    def both(mode, B, H, W, C, hb, wb, code):
        from efficientdet.pytorch_amd import ops
        from efficientdet.pytorch_amd.ops import Map
        wraw = _wraw(g, mode).cuda()
        am = nhwc(q(torch.randn(B, C, H, W, generator=g)), dtype)
        bm = nhwc(q(torch.randn(B, C, hb, wb, generator=g)), dtype)
        with pytest.raises(RuntimeError, match=r'effdet_bifpn_fuse_fwd2 failed: %s' % code):
            ops.bifpn_fuse_fwd(am, bm, None, wraw, 0, mode)
        da, db = Map.new(B, H, W, C, dtype, 'cuda'), Map.new(B, hb, wb, C, dtype, 'cuda')
        dn = torch.zeros(ops.fuse_dn_floats(wraw.shape[1]), device='cuda')
        with pytest.raises(RuntimeError, match=r'effdet_bifpn_fuse_bwd failed: %s' % code):
            ops.bifpn_fuse_bwd(am, am, bm, None, da, db, None, False, False, False, wraw, dn, 0, mode)
        torch.cuda.synchronize()
        assert float(dn.abs().max()) == 0.0                          # refused before anything was launched

    both(0, 1, 5, 6, 2 * ce, 3, 3, 'EFFDET_EUNSUPPORTED')             # odd H (b sized generously: nothing may be read)
    both(0, 1, 6, 5, 2 * ce, 3, 3, 'EFFDET_EUNSUPPORTED')             # odd W
    both(0, 1, 4, 4, ce + ce // 2, 2, 2, 'EFFDET_EINVAL')
    both(2, 1, 3, 3, ce + ce // 2, 6, 6, 'EFFDET_EINVAL')
