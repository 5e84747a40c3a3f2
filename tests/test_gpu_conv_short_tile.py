"""The short-tile instances of the implicit-GEMM conv (csrc/conv_igemm.hip, TUNE_SHORT_TILE) against the 128-pixel-tile plans of the same
descriptors: ops.conv2d with the knob 0 and 1 on the same inputs -- the plan really switches, the outputs (and the pre-activation copies)
are torch.equal, both are within tests/test_gpu_conv.py's tolerance of a float64 reference, and nothing is written outside the output
rows (sentinel-filled buffers with a guard region behind them).  Shapes: the smallest at which the kernel can still go wrong -- partial
pixel and channel tiles, tiles straddling images, a K loop longer than the stage ring, a partial last K-step, a grouped launch whose
tile range changes level -- in exact fp32 and bf16x3, with every epilogue the small-map launches of the train step use."""
import pytest
import torch
import torch.nn.functional as F

from tests.gpu_util import assert_close
from tests.test_gpu_conv import TOL, TOL_X3

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = -7777.0, 4096
PYRAMID = [(8, 8), (4, 4), (2, 2), (1, 1), (1, 1)]

# name -> (B, levels, Cin, Cout, k, epilogue)
CASES = {
    '1x1 672->40 partial tiles, bias': (3, [(5, 7)], 672, 40, 1, 'bias'),
    '1x1 672->40 partial tiles, se backward': (3, [(5, 7)], 672, 40, 1, 'se_bwd'),
    '1x1 1152->192 ring wraps, affine swish zs': (2, [(8, 8)], 1152, 192, 1, 'swish_zs'),
    '1x1 520->64 partial last k-step, res add rowscale': (2, [(5, 7)], 520, 64, 1, 'res_add'),
    '3x3 64->64 five segments, bias': (2, PYRAMID, 64, 64, 3, 'bias'),
    '3x3 64->64 five segments, data gradient': (2, PYRAMID, 64, 64, 3, 'dgrad'),
}


def _swish_grad(z):
    s = torch.sigmoid(z)
    return s + z * s * (1 - s)


def _maps(buf, B, levels, C):
    """the levels back to back in one flat buffer"""
    from efficientdet.pytorch_amd.ops import Map
    out, off = [], 0
    for h, w in levels:
        out.append(Map(buf, B, h, w, C, off=off)); off += B * h * w * C
    return out


def _flat(ts):
    """per-level NCHW float64 -> the flat NHWC fp32 image of _maps"""
    return torch.cat([t.permute(0, 2, 3, 1).reshape(-1) for t in ts]).float()


def _case(name, arith):
    from efficientdet.pytorch_amd import ops, _lib as L
    B, levels, Cin, Cout, k, epi = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float().double()       # fp32-representable float64
    xs = [rnd(B, Cin, h, w) for h, w in levels]
    wt = rnd(Cout, Cin, k, k) / (Cin * k * k) ** 0.5
    wt = wt.float().double()
    scale, shift = (0.5 + torch.rand(Cout, generator=g)).double(), (rnd(Cout) * 0.3).float().double()
    rows = (torch.rand(B, generator=g) + 0.5).double()
    gate, dpool = torch.rand(B, Cout, generator=g).double(), (rnd(B, Cout) * 0.1).float().double()
    res = [rnd(B, Cout, h, w) for h, w in levels]
    pad = k // 2
    old_arith = ops.set_f32_arith(arith)
    try:
        dev = 'cuda'
        kw = dict(Cin=Cin, Cout=Cout, KH=k, KW=k, pad_t=pad, pad_l=pad)
        if epi == 'dgrad':
            # the forward conv is Cout -> Cin channels here (both 64); xs plays dz, the result is dx
            wfull = (wt.float() * scale.float().view(-1, 1, 1, 1)).double()
            ref = [F.conv_transpose2d(x, wfull, None, 1, pad) for x in xs]
            wp = ops.pack_weight(wt.float().to(dev), torch.float32, mode=1, scale=scale.float().to(dev))
            zref = None
        else:
            conv = [F.conv2d(x, wt, None, 1, pad) for x in xs]
            wp = ops.pack_weight(wt.float().to(dev), torch.float32)
            zref = None
            if epi == 'bias':
                ref = [c + shift.view(1, -1, 1, 1) for c in conv]
                kw.update(shift=shift.float().to(dev))
            elif epi == 'swish_zs':
                zref = [c * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1) for c in conv]
                ref = [z * torch.sigmoid(z) for z in zref]
                kw.update(scale=scale.float().to(dev), shift=shift.float().to(dev), act=ops.ACT_SWISH)
            elif epi == 'res_add':
                ref = [c * rows.view(-1, 1, 1, 1) + r for c, r in zip(conv, res)]
                kw.update(rowscale=rows.float().to(dev), res_mode=ops.RES_ADD)
            else:
                assert epi == 'se_bwd'
                ref = [((c * rows.view(-1, 1, 1, 1)) * gate.view(B, Cout, 1, 1) + dpool.view(B, Cout, 1, 1)) * _swish_grad(r) for c, r in zip(conv, res)]
                kw.update(rowscale=rows.float().to(dev), bc_scale=gate.float().to(dev).contiguous(), bc_shift=dpool.float().to(dev).contiguous(),
                          res_mode=ops.RES_SWISH_GRAD)
        n_out = sum(B * h * w * Cout for h, w in levels)
        xbuf = _flat(xs).to(dev)
        xm = _maps(xbuf, B, levels, Cin)
        if 'res_mode' in kw:
            rbuf = torch.cat([_flat(res), torch.zeros(GUARD)]).to(dev)
            kw['res'] = _maps(rbuf, B, levels, Cout)
        got = {}
        for on in (0, 1):
            ybuf = torch.full((n_out + GUARD,), SENTINEL, device=dev)
            zbuf = torch.full((n_out + GUARD,), SENTINEL, device=dev) if zref is not None else None
            ym = _maps(ybuf, B, levels, Cout)
            kk = dict(kw, zs=_maps(zbuf, B, levels, Cout)) if zref is not None else kw
            old = ops.tuning_set(L.TUNE_SHORT_TILE, on)
            try:
                info = ops.conv2d_plan_info(xm, wp, ym, **kk)
                ops.conv2d(xm, wp, ym, **kk)
                torch.cuda.synchronize()
            finally:
                ops.tuning_set(L.TUNE_SHORT_TILE, old)
            got[on] = (info, ybuf.cpu(), zbuf.cpu() if zbuf is not None else None)
        i0, i1 = got[0][0], got[1][0]
        # the plan really switched, to the form this arithmetic asks for (Cin = 520 is no whole [hi | lo] group: exact fp32 either way)
        x3 = arith == 'bf16x3' and (k * k * Cin) % 32 == 0
        assert i0['tile_m'] == 128 and i1['tile_m'] == 32 and i0['form'] == i1['form'] == ('bf16x3' if x3 else 'plain'), (i0, i1)
        assert i1['grid'] == i1['mtiles'] * i1['ntiles'] and i1['mtiles'] == sum(-(-B * h * w // 32) for h, w in levels)
        assert i1['ksteps'] == i0['ksteps'] == -(-(k * k * Cin // 4) // 8)
        tol = TOL_X3 if arith == 'bf16x3' else TOL[torch.float32]
        for which, want in ((1, ref), (2, zref)):
            if want is None:
                continue
            a, b = got[0][which], got[1][which]
            assert bool((a[n_out:] == SENTINEL).all()) and bool((b[n_out:] == SENTINEL).all()), 'guard region written'
            assert not bool((b[:n_out] == SENTINEL).any()), 'output rows left unwritten'
            assert torch.equal(a, b), '%s: %d elements differ between the 128- and the 32-pixel tile' % (name, int((a != b).sum()))
            assert_close(b[:n_out], _flat(want), tol, '%s %s' % (name, 'y' if which == 1 else 'z'))
        return i1
    finally:
        ops.set_f32_arith(old_arith)


@pytest.mark.parametrize('arith', ['f32', 'bf16x3'])
@pytest.mark.parametrize('name', list(CASES))
def test_short_tile_equals_the_128_pixel_tile(name, arith):
    i = _case(name, arith)
    B, levels, Cin, Cout, k, _ = CASES[name]
    M = sum(B * h * w for h, w in levels)
    if Cout == 40:
        assert M % 32 and M % 64 and (5 * 7) % 32 and i['ntiles'] == 2                  # partial pixel tile, tiles straddle images, partial channel tile
    if Cin == 1152:
        assert i['ksteps'] == 36 > i['stages'] == 8                                     # the stage ring wraps
    if Cin == 520:
        assert (Cin // 4) % 8 and i['ksteps'] == 17 > i['stages'] == 8                  # a partial last K-step
    if len(levels) == 5:
        assert i['mtiles'] == 8 and i['ksteps'] == 18 > i['stages'] == 8                # five segments, partial tiles on four of them
