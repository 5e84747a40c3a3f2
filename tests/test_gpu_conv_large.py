"""GPU parity of the dense conv at launches beyond one round of workgroups (tests/conv_plan_cases.py): the persistent kernels where a
workgroup walks 2-4 tiles -- the hand-over to the next tile issued ahead of the finished tile's epilogue, into another pyramid level
too -- the two- and four-stage instances of the 128-pixel-tile kernel in the steady state of an 18-72 step K loop, and the flagged
launch's round-robin deal past its first group.  tests/test_conv_plan_cases_host.py proves through effdet_conv2d_plan_info which instance
every case takes; here the plan is asked again of the very buffers that are launched.

Reference: float64 im2col x weights on the device, one image at a time (conv_plan_cases.conv64_unfold; the host test holds it against
nested loops), for the operands as stored.  Every output element is held to the derived bound conv_plan_cases.value_bound (the f16x3
form: to the criterion of tests/test_gpu_hsplit.py).  Outputs start as NaN, every launch runs twice and must repeat bit for bit, the
flagged launches equal the dense ones bit for bit.  Each case prints its plan, its walk on this device and worst error / bound."""
import types

import pytest
import torch
import torch.nn.functional as F

from tests import conv_plan_cases as P
from tests.test_gpu_conv import big_igemm  # noqa: F401  (the tuning fixture of the persistent bf16 variants)

pytestmark = pytest.mark.gpu
DEV = 'cuda'

_SHARED = {}          # one entry: operands + float64 reference of the last geometry (cases of one geometry are neighbours in the table)


def _operands(c):
    """Operands as stored (fp32 values; bf16 cases: already rounded) and the float64 pre-activation reference + bound scale S per level,
    computed once per geometry and never written to."""
    key = (c.B, tuple(c.sizes), c.Cin, c.Cout, c.arith == 'bf16', c.arith == 'hsplit', c.flagged, c.bias, c.mask)
    if key not in _SHARED:
        _SHARED.clear()
        torch.cuda.empty_cache()
        g = torch.Generator(device=DEV).manual_seed(c.B + c.Cin + c.Cout + len(c.sizes))
        q = (lambda t: t.bfloat16().float()) if c.arith == 'bf16' else (lambda t: t)
        o = types.SimpleNamespace(xs=[], rs=[], ref=[], S=[])
        o.w = q(torch.randn(c.Cout, c.Cin, 3, 3, generator=g, device=DEV) / (9 * c.Cin) ** 0.5)
        o.bias = torch.randn(c.Cout, generator=g, device=DEV) * 0.3 if c.bias else None
        live = [m.to(DEV) for m in P.live_pixels(c)] if c.flagged else None
        for lvl, (h, w) in enumerate(c.sizes):
            x = torch.randn(c.B, h, w, c.Cin, generator=g, device=DEV)
            if c.arith == 'hsplit':
                x = F.relu(x) * 1.7                                      # (activations as the head sees them, tests/test_gpu_hsplit.py)
            if c.flagged:
                x = torch.where(live[lvl].unsqueeze(-1), x, torch.zeros_like(x))      # exact +0
            x = q(x)
            o.xs.append(x)
            if c.mask:
                r = F.relu(torch.randn(c.B, h, w, c.Cout, generator=g, device=DEV))
                r[0, 0, 0, :] = 0.0                                      # exact zeros must mask
                o.rs.append(r)
            ref, S = P.conv64_unfold(x.double(), o.w.double(), o.bias.double() if c.bias else None)
            o.ref.append(ref); o.S.append(S)
        _SHARED[key] = o
    return _SHARED[key]


@pytest.fixture(scope='module', autouse=True)
def _free_shared():
    yield
    _SHARED.clear()
    torch.cuda.empty_cache()


def _nan_pyramid(c):
    from efficientdet.pytorch_amd import functional as Fn
    flat, maps = Fn.pyramid_alloc(c.B, c.sizes, c.Cout, P.out_dtype(c), DEV)
    if flat.dtype == torch.bfloat16:
        flat.view(torch.int16).fill_(0x7fc0)
    else:
        flat.view(torch.int32).fill_({'f32': 0x7fc00000, 'split': 0x7fc07fc0, 'hsplit': 0x7e007e00}[P.out_kind(c)])
    return flat, maps


def _bits(flat):
    return flat.view(torch.int16 if flat.dtype == torch.bfloat16 else torch.int32)


def _stage(c, o):
    """-> (input maps, packed weights, ReLU-mask maps or None) of a case in the layout its arithmetic reads."""
    from efficientdet.pytorch_amd import ops, functional as Fn
    if c.arith == 'hsplit':
        xm = Fn._pyramid_to_split([ops.Map.of(x) for x in o.xs], c.B, c.sizes, c.Cin, torch.float32, DEV, bf=False, h=True)[1]
    else:
        _, xm = Fn.pyramid_alloc(c.B, c.sizes, c.Cin, P.storage_dtype(c), DEV)
        for x, m in zip(o.xs, xm):
            Fn.level_tensor(m).copy_(ops.to_split(x) if c.arith == 'split' else x)
    wp = ops.pack_weight(o.w, P.storage_dtype(c), x3=c.arith == 'split', h3=c.arith == 'hsplit')
    rm = None
    if c.mask:
        _, rm = Fn.pyramid_alloc(c.B, c.sizes, c.Cout, torch.float32, DEV)
        for r, m in zip(o.rs, rm):
            Fn.level_tensor(m).copy_(ops.to_split(r))
    return xm, wp, rm


def _reference(c, o, lvl):
    ref = o.ref[lvl]
    if c.act == 1:
        ref = F.relu(ref)
    if c.mask:
        ref = torch.where(o.rs[lvl] > 0, ref, torch.zeros_like(ref))
    return ref


def _symbol(c, info):
    if not info['persistent']:
        return None
    if c.arith == 'split':
        return 'conv_igemm_pers_kernel<split,bf16x3>'
    return 'conv_igemm_pers_kernel<%s,%s,%s>' % tuple(str(info['id'] - 10))


@pytest.mark.parametrize('c', P.CASES, ids=P.case_id)
def test_large_launch_matches_float64(c, request):
    from efficientdet.pytorch_amd import ops, functional as Fn
    if c.big:
        request.getfixturevalue('big_igemm')(c.big)
    o = _operands(c)
    with P.tuned(c):
        xm, wp, rm = _stage(c, o)
        outs = [_nan_pyramid(c) for _ in range(2)]
        kw = P.conv_kwargs(c, o.bias, rm)
        info = ops.conv2d_plan_info(xm, wp, outs[0][1], **kw)
        assert P.reached(c, info) == c.expect and info['ksteps'] >= c.min_ksteps, info
        rounds = 1
        if info['persistent']:
            cus = torch.cuda.get_device_properties(0).multi_processor_count
            facts = P.walk_facts(c, info, cus)
            rounds = facts['rounds']
            assert rounds >= 2, 'no workgroup of this device (%d compute units) walks a second tile of the %d: the hand-over does not ' \
                                'run, size the case for this device' % (cus, info['grid'])
            print('%s: %d compute units, %s' % (c.name, cus, facts))
        ops.PROFILE = ops.LaunchProfile() if info['persistent'] else None
        try:
            for _, ym in outs:
                ops.conv2d(xm, wp, ym, **kw)
            torch.cuda.synchronize()
            if info['persistent']:
                assert [r[0] for r in ops.PROFILE.records] == [_symbol(c, info)] * 2, ops.PROFILE.records[0][0]
        finally:
            ops.PROFILE = None
        flat, ym = outs[0]
        assert torch.equal(_bits(flat), _bits(outs[1][0])), 'two launches differ'
        if c.flagged:
            live = P.tile_flags(c, P.live_pixels(c)).to(DEV)
            assert bool((live == 0).any()) and bool((live == 1).any())
            fflat, fym = _nan_pyramid(c)
            ops.conv2d(xm, wp, fym, **dict(kw, live=live))
            torch.cuda.synchronize()
            assert torch.equal(_bits(fflat), _bits(flat)), 'flagged launch differs from the dense one'
        exact = None
        if c.arith == 'hsplit':                                          # the exact-fp32 kernel on the same operands: the yardstick of the f16x3 criterion
            _, xe = Fn.pyramid_alloc(c.B, c.sizes, c.Cin, torch.float32, DEV)
            for x, m in zip(o.xs, xe):
                Fn.level_tensor(m).copy_(x)
            _, exact = Fn.pyramid_alloc(c.B, c.sizes, c.Cout, torch.float32, DEV)
            ops.conv2d(xe, ops.pack_weight(o.w, torch.float32), exact, Cin=c.Cin, Cout=c.Cout, KH=3, KW=3, pad_t=1, pad_l=1, shift=o.bias, act=c.act)
            torch.cuda.synchronize()
    worst, over, err_h, err_x, scale, bad = 0.0, 0, 0.0, 0.0, 0.0, 0
    for lvl in range(len(c.sizes)):
        got = P.decode(c, Fn.level_tensor(ym[lvl]))
        ref = _reference(c, o, lvl)
        assert got.shape == ref.shape and bool(torch.isfinite(got).all()), 'level %d: an element was never written (or is not finite)' % lvl
        err = (got - ref).abs()
        if c.arith == 'hsplit':
            err_h = max(err_h, float(err.max())); scale = max(scale, float(ref.abs().max()))
            err_x = max(err_x, float((Fn.level_tensor(exact[lvl]).double() - ref).abs().max()))
        else:
            bound = P.value_bound(c, o.S[lvl], ref)
            worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
            over += int((err > bound).sum())
    plan = 'id %d %s %dx%d/%d stages, %d x %d tiles, %d K-steps, %d round(s)' % (
        info['id'], info['form'], info['tile_m'], info['tile_n'], info['stages'], info['mtiles'], info['ntiles'], info['ksteps'], rounds)
    if c.arith == 'hsplit':
        e_h, e_x = err_h / scale, err_x / scale
        print('%s: %s; f16x3 error %.3g vs exact fp32 %.3g of the scale' % (c.name, plan, e_h, e_x))
        assert e_h <= P.HSPLIT_VS_EXACT * e_x + (P.HSPLIT_OUT_BITS if P.out_kind(c) == 'hsplit' else 0.0), (e_h, e_x)
        assert e_h <= P.HSPLIT_SCALE_CAP, e_h
        for lvl in range(len(c.sizes)):
            ref = _reference(c, o, lvl)
            tol = P.HSPLIT_ELEMENT_TOL * ref.abs().clamp_min(1e-2 * float(ref.abs().max()))
            bad += int(((P.decode(c, Fn.level_tensor(ym[lvl])) - ref).abs() > tol).sum())
        assert bad == 0, '%d elements beyond 1e-4' % bad
    else:
        print('%s: %s; worst error / bound = %.4f' % (c.name, plan, worst))
        assert over == 0, '%d elements exceed the bound, worst error / bound %.3f' % (over, worst)
