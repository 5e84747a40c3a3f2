"""GPU parity of the depthwise kernels at MULTI-TILE workgroup runs (tests/dwconv_cases.py): a workgroup walks ppt > 1 tiles -- the
cur ^ 1 buffer alternation and the prefetch behind the barrier (nbuf = 2), the restage branch (nbuf = 1), Swish on the prefetched
buffer, squeeze-excite sums and weight-gradient accumulators carried across tiles, the ragged last run, the [B][groups][C] rows with
groups < tiles per image.  tests/test_gpu_backbone_ops.py keeps the single-tile paths; tests/test_dwconv_cases_host.py proves through
effdet_dwconv_plan_info which path every case here takes.

Reference: float64 on the CPU.  Forward z and the plain data gradient are held to a derived per-element bound (dwconv_cases.value_bound);
the rest to the tolerances of test_dwconv_fwd_bwd / test_dwconv_fused_data_and_weight_gradient / test_fused_expand_depthwise_forward.
Bitwise: an image of the batched launch equals that image launched alone (one tile per workgroup: the tap order of an output element does
not depend on the run), and two launches are equal.  Each value check prints its worst error / bound before it asserts."""
import types

import pytest
import torch
import torch.nn.functional as F

from tests import dwconv_cases as D
from tests.gpu_util import assert_close, assert_close_scale
from tests.test_gpu_backbone_ops import TOL, nchw, nhwc

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module', params=D.RUN_CASES + D.SINGLE_TILE_CASES, ids=D.case_id)
def run(request):
    """One case: its float64 reference (computed once, shared by the tests below, never written to) and its operands on the device."""
    from efficientdet.pytorch_amd import ops
    c = request.param
    ref = D.reference(c)
    r = types.SimpleNamespace(c=c, ref=ref, geo=D.geometry(c))
    r.xm, r.dzm, r.zpm = nhwc(ref.x, c.dtype), nhwc(ref.dz, c.dtype), nhwc(ref.zprev, c.dtype)
    r.wk = ops.dw_pack_weight(ref.w.to(DEV))
    r.scale, r.shift = ref.scale.to(DEV), ref.shift.to(DEV)
    yield r
    del r.xm, r.dzm, r.zpm
    torch.cuda.empty_cache()


def image(m, i):
    """Image i of a Map as a batch of one."""
    from efficientdet.pytorch_amd.ops import Map
    return Map.of(m.tensor()[i:i + 1])


def within_bound(c, got, ref, scale_abs, what):
    err = (got.double() - ref).abs()
    bound = D.value_bound(c, scale_abs, ref)
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print('%s %s: worst error / bound = %.4f' % (what, D.case_id(c), ratio))
    assert bool(torch.isfinite(got).all()) and bool((err <= bound).all()), \
        '%s: %d elements exceed the bound, worst error / bound %.3f' % (what, int((err > bound).sum()), ratio)


def check_rows(c, info, rows):
    """[B][groups][C] with the planner's groups, fewer than tiles (the cases with runs of tiles)."""
    assert tuple(rows.shape) == (c.B, info['groups'], c.C if hasattr(c, 'C') else 6 * c.Cin)
    assert info['groups'] < info['tpi'] or info['ppt'] == 1


def test_forward(run):
    from efficientdet.pytorch_amd import ops
    c, ref = run.c, run.ref
    _, _, _, k, s, pt, pl, Ho, Wo = run.geo
    q = lambda t: t.to(c.dtype).float()
    fwd = lambda x, **kw: ops.dwconv_fwd(x, run.wk, run.scale, run.shift, k, s, pt, pl, Ho, Wo, save_z=True, pool=True, **kw)
    ym, zm, pp = fwd(run.xm)
    torch.cuda.synchronize()
    within_bound(c, nchw(zm), ref.z, ref.z_abs, 'dw z')
    assert_close(nchw(ym), ref.y, TOL[c.dtype], 'dw y')
    check_rows(c, D.plan('fwd', c), pp)
    assert_close(pp.sum(dim=1).cpu(), q(ref.y).sum(dim=(2, 3)), 5 * TOL[c.dtype], 'se pool')
    assert torch.equal(fwd(run.xm)[2], pp)
    # z-only storage: same stored z, the pooled sum is that of Swish(stored z)
    y2, z2, pp2 = fwd(run.xm, save_y=False)
    assert y2 is None and torch.equal(z2.tensor(), zm.tensor())
    zs = nchw(z2).double()
    assert_close(pp2.sum(dim=1).cpu(), D.swish64(zs).sum(dim=(2, 3)), 5 * TOL[c.dtype], 'se pool (z-only)')
    # an image of the batch == that image alone (one tile per workgroup, see the host test)
    for i in sorted({0, c.B - 1}):
        y1, z1, _ = fwd(image(run.xm, i))
        assert torch.equal(z1.tensor()[0], zm.tensor()[i]) and torch.equal(y1.tensor()[0], ym.tensor()[i]), 'image %d' % i


def test_data_gradient(run):
    from efficientdet.pytorch_amd import ops
    c, ref = run.c, run.ref
    H, W, _, k, s, pt, pl, _, _ = run.geo
    dgrad = lambda dz, zp: ops.dwconv_dgrad(dz, run.wk, run.scale, zp, H, W, k, s, pt, pl)
    dxm = dgrad(run.dzm, None)
    dxm2 = dgrad(run.dzm, run.zpm)
    torch.cuda.synchronize()
    within_bound(c, nchw(dxm), ref.dx, ref.dx_abs, 'dw dgrad')
    assert_close(nchw(dxm2), ref.dx * D.swish_grad64(ref.zprev.double()), TOL[c.dtype], 'dw dgrad*swish')
    for i in sorted({0, c.B - 1}):
        assert torch.equal(dgrad(image(run.dzm, i), None).tensor()[0], dxm.tensor()[i]), 'image %d' % i
        assert torch.equal(dgrad(image(run.dzm, i), image(run.zpm, i)).tensor()[0], dxm2.tensor()[i]), 'image %d (zprev)' % i


def test_weight_gradient(run):
    from efficientdet.pytorch_amd import ops
    c, ref = run.c, run.ref
    _, _, _, k, s, pt, pl, _, _ = run.geo
    gk, dsum = ops.dwconv_wgrad(run.xm, run.dzm, k, s, pt, pl)
    gk2, dsum2 = ops.dwconv_wgrad(run.xm, run.dzm, k, s, pt, pl)
    assert torch.equal(gk, gk2) and torch.equal(dsum, dsum2)
    assert_close(gk.cpu(), ref.g, 5 * TOL[c.dtype], 'dw wgrad rows')
    assert_close(dsum.cpu(), ref.dsum, 5 * TOL[c.dtype], 'dw dsum')


@pytest.mark.parametrize('c', [c for c in D.RUN_CASES if c.pre], ids=D.case_id)
def test_forward_and_weight_gradient_from_the_pre_activation(c):
    """in_act = SWISH: handed the PRE-activation, the forward Swishes its staged tiles (the prefetched buffer of a run included) and the
    weight gradient its tile == the same kernels on the activated tensor."""
    from efficientdet.pytorch_amd import ops
    _, _, _, k, s, pt, pl, Ho, Wo = D.geometry(c)
    g = torch.Generator().manual_seed(7)
    q = lambda t: t.to(c.dtype).float()
    pre = q(torch.randn(c.B, c.C, c.H, c.W, generator=g))
    w = torch.randn(c.C, 1, k, k, generator=g) * (2.0 / (k * k)) ** 0.5
    scale, shift = (0.5 + torch.rand(c.C, generator=g)).to(DEV), (torch.randn(c.C, generator=g) * 0.2).to(DEV)
    dzm = nhwc(q(torch.randn(c.B, c.C, Ho, Wo, generator=g)), c.dtype)
    wk = ops.dw_pack_weight(w.to(DEV))
    am, pm = nhwc(q(pre * torch.sigmoid(pre)), c.dtype), nhwc(pre, c.dtype)
    fwd = lambda x, act: ops.dwconv_fwd(x, wk, scale, shift, k, s, pt, pl, Ho, Wo, save_z=True, pool=True, save_y=False, in_act=act)
    _, za, pa = fwd(am, ops.ACT_NONE)
    _, zb, pb = fwd(pm, ops.ACT_SWISH)
    assert_close_scale(nchw(zb), nchw(za), 2 * TOL[c.dtype], 'dw z from the pre-activation')
    assert_close_scale(pb.sum(dim=1).cpu(), pa.sum(dim=1).cpu(), 2 * TOL[c.dtype], 'se pool from the pre-activation')
    _, zb2, pb2 = fwd(pm, ops.ACT_SWISH)
    assert torch.equal(zb2.tensor(), zb.tensor()) and torch.equal(pb2, pb)
    for i in sorted({0, c.B - 1}):
        assert torch.equal(fwd(image(pm, i), ops.ACT_SWISH)[1].tensor()[0], zb.tensor()[i]), 'image %d' % i
    ga, da = ops.dwconv_wgrad(am, dzm, k, s, pt, pl)
    gb, dbb = ops.dwconv_wgrad(pm, dzm, k, s, pt, pl, in_act=ops.ACT_SWISH)
    assert_close_scale(gb.cpu(), ga.cpu(), 2 * TOL[c.dtype], 'dw wgrad from the pre-activation'); assert torch.equal(dbb, da)


@pytest.mark.parametrize('c', D.BWD_CASES, ids=D.case_id)
def test_fused_backward(c):
    """effdet_dwconv_bwd at runs of tiles vs float64 autograd of conv(swish(zprev)), vs the two separate kernels, twice."""
    from efficientdet.pytorch_amd import ops
    H, W, _, k, s, pt, pl, Ho, Wo = D.geometry(c)
    g = torch.Generator().manual_seed(5)
    zp32 = torch.randn(c.B, c.C, H, W, generator=g)
    w32 = torch.randn(c.C, 1, k, k, generator=g) * (2.0 / (k * k)) ** 0.5
    scale = 0.5 + torch.rand(c.C, generator=g)
    dz = torch.randn(c.B, c.C, Ho, Wo, generator=g)
    zp, w = zp32.double().requires_grad_(True), w32.double().requires_grad_(True)
    z = D.dwconv64(D.swish64(zp), w, k, s) * scale.double().view(1, -1, 1, 1)
    z.backward(dz.double())
    g_ref = (w.grad / scale.double().view(-1, 1, 1, 1)).reshape(c.C, k * k).t()
    wk = ops.dw_pack_weight(w32.to(DEV))
    zpm, dzm = nhwc(zp32, torch.float32), nhwc(dz, torch.float32)
    out = ops.dwconv_bwd(dzm, wk, scale.to(DEV), zpm, k, s, pt, pl)
    assert out is not None
    dxm, gk, dsum = out
    out2 = ops.dwconv_bwd(dzm, wk, scale.to(DEV), zpm, k, s, pt, pl)
    assert torch.equal(out2[0].tensor(), dxm.tensor()) and torch.equal(out2[1], gk) and torch.equal(out2[2], dsum)
    assert_close(nchw(dxm), zp.grad, 2e-4, 'fused dw dgrad*swish\'')
    assert_close(gk.cpu(), g_ref, 1e-3, 'fused dw wgrad rows')
    assert_close(dsum.cpu(), dz.double().sum(dim=(0, 2, 3)), 1e-3, 'fused dw dsum')
    dx_sep = ops.dwconv_dgrad(dzm, wk, scale.to(DEV), zpm, H, W, k, s, pt, pl)
    g_sep, ds_sep = ops.dwconv_wgrad(zpm, dzm, k, s, pt, pl, in_act=ops.ACT_SWISH)
    assert torch.equal(dx_sep.tensor(), dxm.tensor())
    assert_close_scale(gk.cpu(), g_sep.cpu(), 2e-5, 'fused vs separate dw wgrad'); assert_close_scale(dsum.cpu(), ds_sep.cpu(), 2e-5, 'fused vs separate dsum')


@pytest.mark.parametrize('c', D.EXPAND_CASES, ids=D.case_id)
def test_fused_expand_depthwise_forward(c):
    """effdet_mbconv_expand_dw_fwd at runs of tiles vs float64 and vs the expand conv + depthwise launches it replaces."""
    from efficientdet.pytorch_amd import ops
    from efficientdet.pytorch_amd.ops import Map
    H, W, Cexp, k, s, pt, pl, Ho, Wo = D.geometry(c)
    tol = TOL[torch.float32]
    g = torch.Generator().manual_seed(2)
    x = torch.randn(c.B, c.Cin, H, W, generator=g)
    we = torch.randn(Cexp, c.Cin, 1, 1, generator=g) / c.Cin ** 0.5
    s0 = 0.5 + torch.rand(Cexp, generator=g); t0 = torch.randn(Cexp, generator=g) * 0.5          # large shifts: padding pixels would show
    wd = torch.randn(Cexp, 1, k, k, generator=g) * (2.0 / (k * k)) ** 0.5
    s1 = 0.5 + torch.rand(Cexp, generator=g); t1 = torch.randn(Cexp, generator=g) * 0.2
    e = D.swish64(F.conv2d(x.double(), we.double()) * s0.double().view(1, -1, 1, 1) + t0.double().view(1, -1, 1, 1))
    y = D.swish64(D.dwconv64(e, wd.double(), k, s) * s1.double().view(1, -1, 1, 1) + t1.double().view(1, -1, 1, 1))
    del e
    xm, wk = nhwc(x, torch.float32), ops.dw_pack_weight(wd.to(DEV))
    dv = [t.to(DEV) for t in (we, s0, t0, s1, t1)]
    fused = lambda xin: ops.expand_dw_fwd(xin, dv[0], dv[1], dv[2], wk, dv[3], dv[4], k, s, pt, pl, Ho, Wo)
    ym, pp = fused(xm)
    torch.cuda.synchronize()
    assert_close(nchw(ym), y, tol, 'fused expand + depthwise y')
    check_rows(c, D.plan('expand_fwd', c), pp)
    assert_close(pp.sum(dim=1).cpu(), y.sum(dim=(2, 3)), 5 * tol, 'se pool')
    ym2, pp2 = fused(xm)
    assert torch.equal(ym2.tensor(), ym.tensor()) and torch.equal(pp2, pp)
    for i in sorted({0, c.B - 1}):
        assert torch.equal(fused(image(xm, i))[0].tensor()[0], ym.tensor()[i]), 'image %d' % i
    # the chain it replaces: 1x1 expand conv + BN + Swish, then the depthwise forward
    xe = Map.new(c.B, H, W, Cexp, torch.float32, DEV)
    ops.conv2d(xm, ops.pack_weight(dv[0], torch.float32), xe, Cin=c.Cin, Cout=Cexp, KH=1, KW=1, scale=dv[1], shift=dv[2], act=ops.ACT_SWISH)
    yc, _, pc = ops.dwconv_fwd(xe, wk, dv[3], dv[4], k, s, pt, pl, Ho, Wo, pool=True)
    torch.cuda.synchronize()
    assert_close(nchw(ym), nchw(yc), tol, 'fused vs expand conv + depthwise y')
    assert_close(pp.sum(dim=1).cpu(), pc.sum(dim=1).cpu(), 5 * tol, 'fused vs expand conv + depthwise se pool')
