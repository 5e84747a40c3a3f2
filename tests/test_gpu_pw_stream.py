"""GPU parity, op by op, of the two persistent MFMA streaming kernels of the MBConv backward: effdet_pw_bwd (csrc/pw_bwd.hip: data +
weight gradient of the expand conv, one slab and one dsum row per workgroup) and effdet_pw_dgrad_se (csrc/pw_dgrad.hip: project-conv
data gradient with the squeeze-excite backward and Swish' in the epilogue), at the case tables of tests/pw_stream_cases.py
(tests/test_pw_stream_cases_host.py proves what every case reaches).  tests/test_gpu_backbone_ops.py keeps the comparison with the
launches the kernels replace and the path through the unpack job.

EXACT: hashed small integers and powers of two -- fp32 arithmetic is exact in any order, so dx, EVERY raw slab, EVERY dsum row and dz_d
must be torch.equal to the float64 reference: a wrong lane, a dropped tail pixel or a tile summed into the wrong workgroup's slab fails
with zero tolerance.  The entry points are called through the C ABI on buffers the test owns: sentinel-filled outputs with guard
regions behind them (64 rows behind dx / dz_d, one slab and one dsum row behind the used ones) that must stay untouched.
FLOAT64: randn with per-channel magnitudes over 2^-6 .. 2^6, every element within the derived any-order bound
(pw_stream_cases.bwd_bounds / dgrad_bound); each check prints its worst error / bound first.  The references are evaluated in float64
on the device (plain torch matmuls and elementwise ops)."""
import pytest
import torch

from tests import pw_stream_cases as P

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENTINEL = -7777.25


def _lib():
    from efficientdet.pytorch_amd import _lib as L
    return L, L.require('effdet_pw_bwd_slabs', 'effdet_pw_bwd', 'effdet_pw_dgrad_se_supported', 'effdet_pw_dgrad_se')


def _filled(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.float32, device=DEV)


def _exact(got, ref64, what):
    """torch.equal with the float64 reference cast to fp32, which must lose nothing."""
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    r32 = ref64.float()
    assert torch.equal(r32.double(), ref64), what + ': the reference is not an fp32 number'
    bad = got != r32
    n = int(bad.sum())
    first = ''
    if n:
        k = int(torch.nonzero(bad.reshape(-1))[0])
        first = '  first at %d: got %r ref %r' % (k, float(got.reshape(-1)[k]), float(r32.reshape(-1)[k]))
    print('FIG %-64s mismatches %d of %d  ref max %g  (exact)%s' % (what, n, got.numel(), float(ref64.abs().max()), first))
    assert n == 0, '%s: %d of %d elements differ%s' % (what, n, got.numel(), first)


def _within(got, ref64, bound, what):
    """|got - ref| <= bound for every element; prints the worst error / bound."""
    assert got.shape == ref64.shape == bound.shape, (what, got.shape, ref64.shape, bound.shape)
    err = (got.double() - ref64).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    n = int((err > bound).sum())
    print('FIG %-64s worst error / bound %.4f  over %d of %d  ref max %.3e' % (what, ratio, n, got.numel(), float(ref64.abs().max())))
    assert bool(torch.isfinite(got).all()), what
    assert n == 0, '%s: %d of %d elements exceed the bound, worst error / bound %.3f' % (what, n, got.numel(), ratio)


def _untouched(guard, what):
    assert bool((guard == SENTINEL).all()), '%s: %d guard words were written' % (what, int((guard != SENTINEL).sum()))


# ----------------------------------------------------------------------------- effdet_pw_bwd
def _run_pw_bwd(c, i):
    """-> (dx [M + 64][Cin], slabs [nwg + 1][Cexp][Cin], dsum [nwg + 1][Cexp]) of one launch into sentinel-filled buffers."""
    L, lib = _lib()
    g = P.bwd_geometry(c)
    M, Ci, Ce, nwg = g['M'], c.Cin, g['Cexp'], g['nwg']
    assert int(lib.effdet_pw_bwd_slabs(M, Ci, Ce)) == nwg
    assert i.dz.shape == (M, Ce) and i.x.shape == (M, Ci) and i.w.shape == (Ce, Ci) and all(t is None or t.is_contiguous() for t in i)
    dx, slabs, dsum = _filled(M + P.TP, Ci), _filled(nwg + 1, Ce, Ci), _filled(nwg + 1, Ce)
    L.check(lib.effdet_pw_bwd(L.ptr(i.dz), L.ptr(i.x), L.ptr(i.w), L.ptr(i.scale), L.ptr(i.res), L.ptr(dx), L.ptr(slabs), L.ptr(dsum),
                              M, Ci, Ce, L.stream_ptr()), 'effdet_pw_bwd')
    torch.cuda.synchronize()
    return dx, slabs, dsum


def _check_pw_bwd_guards(c, out, what):
    g = P.bwd_geometry(c)
    dx, slabs, dsum = out
    _untouched(dx[g['M']:], what + ' rows behind dx')
    _untouched(slabs[g['nwg']:], what + ' slab behind the last workgroup\'s')
    _untouched(dsum[g['nwg']:], what + ' dsum row behind the last workgroup\'s')
    return dx[:g['M']], slabs[:g['nwg']], dsum[:g['nwg']]


@pytest.mark.parametrize('c', P.PW_BWD_CASES, ids=P.bwd_id)
def test_pw_bwd_exact_dx_slabs_and_dsum_rows(c):
    """Hashed integers: dx, every workgroup's slab (the sum over the tiles t = w mod nwg of dz_t^T x_t) and dsum row equal the float64
    reference bit for bit -- tile ownership, the tail tile, the Cin = 24 ones-column dsum, res on the tail; guards untouched; two
    launches bitwise equal."""
    what = 'pw_bwd ' + P.bwd_id(c)
    i = P.bwd_exact_inputs(c, DEV)
    out = _run_pw_bwd(c, i)
    dx, slabs, dsum = _check_pw_bwd_guards(c, out, what)
    ref = P.bwd_reference(i, P.bwd_geometry(c)['nwg'])
    assert float(ref.slabs.abs().max()) < 2 ** 22 and float(ref.dsum.abs().max()) < 2 ** 22
    _exact(dx, ref.dx, what + ' dx')
    _exact(slabs, ref.slabs, what + ' slabs')
    _exact(dsum, ref.dsum, what + ' dsum rows')
    again = _run_pw_bwd(c, i)
    assert all(torch.equal(a, b) for a, b in zip(out, again)), what + ': two launches differ'


@pytest.mark.parametrize('c', P.PW_BWD_CASES, ids=P.bwd_id)
def test_pw_bwd_float64_per_element_bound(c):
    """randn, channel magnitudes over 2^-6 .. 2^6: dx, every raw slab and every dsum row within gamma(n + 2) * sum |a_i b_i| of float64."""
    what = 'pw_bwd f64 ' + P.bwd_id(c)
    nwg = P.bwd_geometry(c)['nwg']
    i = P.bwd_random_inputs(c, DEV)
    out = _run_pw_bwd(c, i)
    dx, slabs, dsum = _check_pw_bwd_guards(c, out, what)
    ref = P.bwd_reference(i, nwg)
    bound = P.bwd_bounds(i, nwg, ref)
    _within(dx, ref.dx, bound.dx, what + ' dx')
    _within(slabs, ref.slabs, bound.slabs, what + ' slabs')
    _within(dsum, ref.dsum, bound.dsum, what + ' dsum rows')
    again = _run_pw_bwd(c, i)
    assert all(torch.equal(a, b) for a, b in zip(out, again)), what + ': two launches differ'


# ----------------------------------------------------------------------------- effdet_pw_dgrad_se
def _run_pw_dgrad(c, i):
    """-> dz_d [M + 64][Ce] of one launch into a sentinel-filled buffer."""
    L, lib = _lib()
    g = P.dgrad_geometry(c)
    M = g['M']
    assert int(lib.effdet_pw_dgrad_se_supported(M, c.Co, c.Ce)) == 1
    assert i.dy.shape == (M, c.Co) and i.zd.shape == (M, c.Ce) and i.w.shape == (c.Co, c.Ce) and i.gate.shape == i.dpool.shape == (c.B, c.Ce)
    assert all(t is None or t.is_contiguous() for t in i)
    out = _filled(M + P.TP, c.Ce)
    L.check(lib.effdet_pw_dgrad_se(L.ptr(i.dy), L.ptr(i.w), L.ptr(i.scale), L.ptr(i.rowscale), L.ptr(i.gate), L.ptr(i.dpool), L.ptr(i.zd),
                                   L.ptr(out), M, g['HW'], c.B, c.Co, c.Ce, L.stream_ptr()), 'effdet_pw_dgrad_se')
    torch.cuda.synchronize()
    return out


def _swish_grad_factor(z, dy=None):
    """dy * swish_gradf_(z) through effdet_act_bwd (se.hip), which shares the device function with pw_dgrad_se; z, dy: [n], n % 4096 == 0."""
    from efficientdet.pytorch_amd import ops
    from efficientdet.pytorch_amd.ops import Map
    shape = (1, z.numel() // 4096, 64, 64)
    dy = torch.ones_like(z) if dy is None else dy
    return ops.act_bwd(Map.of(dy.view(shape).contiguous()), Map.of(z.view(shape).contiguous()), ops.ACT_SWISH).tensor().view(-1)


def test_swish_grad_factor_is_exactly_one_and_zero_at_the_mask_values():
    """What the exact test of pw_dgrad_se rests on: swish_gradf_(40) == 1 and swish_gradf_(-100) == +-0 on the device."""
    z = P.hash_choice(4096, 4, P.Z_PASS, P.Z_BLOCK, 3, DEV).view(-1)
    dy = P.hash_ints(4096, 4, 4, 4, DEV).view(-1) + 0.5
    got = _swish_grad_factor(z, dy)
    torch.cuda.synchronize()
    print('FIG swish_gradf_(%g) in [%r, %r]   swish_gradf_(%g) in [%r, %r]' % (
        P.Z_PASS, float(got[z == P.Z_PASS].div(dy[z == P.Z_PASS]).min()), float(got[z == P.Z_PASS].div(dy[z == P.Z_PASS]).max()),
        P.Z_BLOCK, float(got[z == P.Z_BLOCK].min()), float(got[z == P.Z_BLOCK].max())))
    assert torch.equal(got, torch.where(z == P.Z_PASS, dy, torch.zeros_like(dy)))


def test_swish_grad_factor_error_is_within_the_constant():
    """SWISH_GRAD_E of tests/pw_stream_cases.py: |dy swish_gradf_(z) - dy swish'(z)| <= E dy m(z) over z in [-30, 30], measured against
    float64 on 2^22 points (a regular grid jittered by the hash); printed for dy = 1 (the factor alone) and dy in [1, 2)."""
    n = 1 << 22
    k = torch.arange(n, dtype=torch.float64, device=DEV)
    jitter = (P.hash32(n, 1, 9, DEV).view(-1) % 1024).double() / 1024
    z = ((k + jitter) * (60.0 / n) - 30.0).float()
    dy = 1 + (P.hash32(n, 1, 10, DEV).view(-1) % 4096).float() / 4096
    f, m = P.swish_grad64(z), P.swish_grad_magnitude(z)
    one = ((_swish_grad_factor(z).double() - f).abs() / m)
    rnd = ((_swish_grad_factor(z, dy).double() - dy.double() * f).abs() / (dy.double() * m))
    near = z.abs() <= 8
    print('FIG swish_gradf_ relative to m(z): dy = 1: %.3e (|z| <= 8: %.3e)   dy in [1, 2): %.3e (|z| <= 8: %.3e)   constant %.3e' % (
        float(one.max()), float(one[near].max()), float(rnd.max()), float(rnd[near].max()), P.SWISH_GRAD_E))
    assert float(rnd.max()) <= P.SWISH_GRAD_E and float(one.max()) <= P.SWISH_GRAD_E


@pytest.mark.parametrize('c', P.PW_DGRAD_CASES, ids=P.dgrad_id)
def test_pw_dgrad_se_exact_with_a_zero_one_swish_mask(c):
    """Hashed integers, power-of-two scales, z_d in {40, -100}: dz_d == ((acc rs) gate + dpool) * {1, 0} bit for bit -- every pixel's
    image index (rowscale, gate, dpool), every channel tile incl. the ones behind the wave-uniform break, and the mask shows that z_d
    was read from the right place; 64 rows behind dz_d untouched; two launches bitwise equal."""
    what = 'pw_dgrad_se ' + P.dgrad_id(c)
    g = P.dgrad_geometry(c)
    i = P.dgrad_exact_inputs(c, DEV)
    out = _run_pw_dgrad(c, i)
    _untouched(out[g['M']:], what + ' rows behind dz_d')
    ref = P.dgrad_exact_reference(i, c.B, g['HW'])
    frac = float((ref != 0).double().mean())
    assert 0.3 < frac < 0.7, frac
    _exact(out[:g['M']], ref, what)
    assert torch.equal(_run_pw_dgrad(c, i), out), what + ': two launches differ'


@pytest.mark.parametrize('c', P.PW_DGRAD_CASES, ids=P.dgrad_id)
def test_pw_dgrad_se_float64_per_element_bound(c):
    """randn operands (dy channels and weight rows over 2^-6 .. 2^6), z_d ~ 2 randn: every element within dgrad_bound of float64."""
    what = 'pw_dgrad_se f64 ' + P.dgrad_id(c)
    g = P.dgrad_geometry(c)
    i = P.dgrad_random_inputs(c, DEV)
    out = _run_pw_dgrad(c, i)
    _untouched(out[g['M']:], what + ' rows behind dz_d')
    ref = P.dgrad_reference(i, c.B, g['HW'])
    _within(out[:g['M']], ref, P.dgrad_bound(i, c.B, g['HW'], ref), what)
    assert torch.equal(_run_pw_dgrad(c, i), out), what + ': two launches differ'
