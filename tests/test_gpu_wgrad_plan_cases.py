"""Weight-gradient kernels at multi-range split-K plans against float64, slab by slab (csrc/conv_wgrad.hip; the case table, the reference
and the bounds: tests/wgrad_plan_cases.py, held against the planner by tests/test_wgrad_plan_cases_host.py).

One test per case and form.  The test owns the workspace: NaN before the launch (with a NaN guard behind it), so a slab or bias row no
workgroup wrote fails the finiteness check, and a write past the end shows in the guard.  Every slab is compared with the reference of
its own pixel range, every bias partial row likewise, then the unpacked gradient with the sum over all pixels.  Flagged launches get
flags built from the stored dz (a step is live when any of its 32 pixels holds a non-zero word), equal to ops.live_tiles' radius-0
answer; their slabs are held against float64 as well, and a range without a live step must be zero bit for bit.  The paired launches
run two problems with different data.  The float64 references are computed on the device, one image at a time, once per case."""
import pytest
import torch

from tests import wgrad_plan_cases as P

pytestmark = pytest.mark.gpu

DEV = 'cuda'
GUARD = 256                    # NaN floats behind the workspace the launch may use
_CACHE = {}                    # (case name, problem) -> problem; one case at a time


def _view(m):
    """[B, H, W, ld] view of a Map's storage (a level of a flat pyramid buffer, or a map of its own)"""
    n = m.B * m.H * m.W * m.ld
    return m.t.view(-1)[m.off:m.off + n].view(m.B, m.H, m.W, m.ld)


def _make(c, info, which):
    """Problem 'a' (random everywhere) or 'b' (other data; dz non-zero on live_pixel_masks' pixels only) of a case on the device, with
    the float64 reference of every slab: -> dict(xm, zm, masks, G, S, bias, Sb) with per level [count][Cout][k k][Cin] / [count][Cout]"""
    from efficientdet.pytorch_amd import ops
    gen = torch.Generator(device=DEV).manual_seed(1000 * (which == 'b') + len(c.name) + c.Cin + c.Cout)
    xm, zm = P.alloc(c, DEV)
    masks = [m.to(DEV) for m in P.live_pixel_masks(c, info)] if which == 'b' else None
    rng = P.ranges(c, info)
    out = dict(xm=xm, zm=zm, masks=masks, G=[], S=[], bias=[], Sb=[])
    for l, (h, w) in enumerate(c.sizes):
        x = torch.randn(c.B, h, w, c.Cin, device=DEV, generator=gen)
        dz = torch.zeros(c.B, h, w, c.lddz, device=DEV)
        dz[..., :c.Cout] = torch.randn(c.B, h, w, c.Cout, device=DEV, generator=gen)
        if masks is not None:
            dz = torch.where(masks[l].view(c.B, h, w, 1), dz, torch.zeros((), device=DEV))
        if c.kind == 'split':
            x, dz = ops.to_split(x), ops.to_split(dz)
        _view(xm[l]).copy_(x)
        _view(zm[l]).copy_(dz)
        mine = [(m0, m1) for (lv, m0, m1) in rng if lv == l]
        assert len(mine) == info['count'][l] and [rng[info['first'][l] + r][1:] for r in range(len(mine))] == mine
        G, S, bias, Sb = P.range_refs(P.stored64(c, _view(xm[l])), P.stored64(c, _view(zm[l]))[..., :c.Cout], c.k, mine)
        out['G'].append(G); out['S'].append(S); out['bias'].append(bias); out['Sb'].append(Sb)
    torch.cuda.synchronize()
    return out


def _problem(c, info, which):
    for key in [k for k in _CACHE if k[0] != c.name]:
        del _CACHE[key]
    if (c.name, which) not in _CACHE:
        _CACHE[(c.name, which)] = _make(c, info, which)
    return _CACHE[(c.name, which)]


def _flags(c, info, prob):
    """Problem b's step flags from the definition, on the stored dz: a step is live when any of its 32 pixels has a non-zero word (a bit
    outside the sign bits of the word's two halves).  Equal to the flags of the pixel pattern and to ops.live_tiles' radius-0 answer."""
    from efficientdet.pytorch_amd import ops
    px = [((_view(m).view(torch.int32) & 0x7fff7fff) != 0).view(-1, c.lddz).any(dim=1) for m in prob['zm']]
    flags = P.step_flags(px)
    assert torch.equal(flags.cpu(), P.step_flags(P.live_pixel_masks(c, info)))
    src = torch.zeros(c.B, sum(h * w for h, w in c.sizes), 64, device=DEV)
    src[..., 0] = torch.cat([p.view(c.B, -1) for p in px], dim=1).float()
    l32, _ = ops.live_tiles(src, c.B, c.sizes, 64, False)
    assert torch.equal(l32[0], flags)
    assert bool(flags.any()) and bool((flags == 0).any())
    return flags.contiguous()


def _workspace(nslabs, c):
    floats = nslabs * (c.Cout * c.k * c.k * c.Cin + c.Cout)
    return torch.full((floats + GUARD,), float('nan'), device=DEV), floats


def _worst(err, bound):
    """largest err / bound (0 / 0 = 0, x / 0 = inf): the figure a failing slab is reported with"""
    ratio = torch.where(err > 0, err / bound, torch.zeros_like(err))
    return float(ratio.max())


def _check(c, info, prob, slabs, parts, what, flagged):
    """every slab and bias partial row against its own range's reference, then the unpacked gradient against the sum over all pixels"""
    from efficientdet.pytorch_amd import ops
    kk, rng = c.k * c.k, P.ranges(c, info)
    assert slabs.shape == (info['splits'], c.Cout, kk, c.Cin) and parts.shape == (info['splits'], c.Cout)
    assert bool(torch.isfinite(slabs).all()) and bool(torch.isfinite(parts).all()), '%s: a slab or bias row holds NaN / Inf: not written' % what
    per = info['mchunk'] // 32
    live = P.live_steps(c, info) if flagged else None
    bad, worst = [], 0.0
    for l in range(len(c.sizes)):
        f0, cnt = info['first'][l], info['count'][l]
        n = torch.tensor([m1 - m0 for (_, m0, m1) in rng[f0:f0 + cnt]], dtype=torch.float64, device=DEV)
        eg = (slabs[f0:f0 + cnt].double() - prob['G'][l]).abs()
        bg = P.sum_bound(c, n.view(-1, 1, 1, 1), prob['S'][l])
        eb = (parts[f0:f0 + cnt].double() - prob['bias'][l]).abs()
        bb = P.sum_bound(c, n.view(-1, 1), prob['Sb'][l])
        for r in range(cnt):
            wg, wb = _worst(eg[r], bg[r]), _worst(eb[r], bb[r])
            worst = max(worst, wg, wb)
            if bool((eg[r] > bg[r]).any()) or bool((eb[r] > bb[r]).any()):
                bad.append((l, r, 'slab %.3g x bound, bias row %.3g x bound' % (wg, wb)))
            if flagged and not any(r * per <= s < (r + 1) * per for s in live[l]):       # no live step: zeros, bit for bit (+0 or -0)
                assert not bool((slabs[f0 + r].view(torch.int32) & 0x7fffffff).any()) and not bool((parts[f0 + r].view(torch.int32) & 0x7fffffff).any()), \
                    '%s: level %d range %d has no live step and is not zero' % (what, l, r)
    print('%s: %d slabs, worst error / bound %.3g' % (what, info['splits'], worst))
    assert not bad, '%s: (level, range) beyond the bound: %s' % (what, bad[:6])
    # the consumer: unpack_wgrad sums the slabs and the bias rows in slab order
    groups = [(info['first'][l], info['count'][l], [l]) for l in range(len(c.sizes))] if c.layout == 'group' else \
        [(0, info['splits'], list(range(len(c.sizes))))]
    for f0, cnt, levels in groups:
        dw = torch.full((c.Cout, c.Cin, c.k, c.k), float('nan'), device=DEV)
        db = ops.unpack_wgrad(slabs[f0:f0 + cnt], dw, dbias_part=parts[f0:f0 + cnt])
        M = sum(P.level_pixels(c)[l] for l in levels)
        Gt, St = sum(prob['G'][l].sum(0) for l in levels), sum(prob['S'][l].sum(0) for l in levels)
        bt, Sbt = sum(prob['bias'][l].sum(0) for l in levels), sum(prob['Sb'][l].sum(0) for l in levels)
        oihw = lambda t: t.view(c.Cout, c.k, c.k, c.Cin).permute(0, 3, 1, 2)
        ew, bw = (dw.double() - oihw(Gt)).abs(), P.sum_bound(c, M + cnt, oihw(St))
        ed, bd = (db.double() - bt).abs(), P.sum_bound(c, M + cnt, Sbt)
        print('%s: unpacked levels %s, worst error / bound: dw %.3g, db %.3g' % (what, levels, _worst(ew, bw), _worst(ed, bd)))
        assert bool(torch.isfinite(dw).all()) and bool(torch.isfinite(db).all())
        assert not bool((ew > bw).any()) and not bool((ed > bd).any()), '%s: unpacked gradient of levels %s beyond the bound' % (what, levels)


def _split_ws(ws, o, nslabs, c):
    n = c.Cout * c.k * c.k * c.Cin
    return ws[o:o + nslabs * n].view(nslabs, c.Cout, c.k * c.k, c.Cin), ws[o + nslabs * n:o + nslabs * (n + c.Cout)].view(nslabs, c.Cout)


@pytest.mark.parametrize('v', P.VARIANTS, ids=P.variant_id)
def test_every_slab_against_float64(v):
    from efficientdet.pytorch_amd import ops
    c, form = v
    with P.tuned(c):
        info = P.plan(c)
        assert P.holds(c.need, P.facts(c, info)) == [] and P.reached(c, info, form)[1:3] == ('split' if c.kind == 'split' else 'tiled', c.launches)
        kw = P.wgrad_kwargs(c)
        S = info['splits']
        if form in ('pair-dense', 'pair-flagged'):
            a, b = _problem(c, info, 'a'), _problem(c, info, 'b')
            flags = _flags(c, info, b) if form == 'pair-flagged' else None
            ws, floats = _workspace(2 * S, c)
            pkw = {k: kw[k] for k in ('Cin', 'Cout', 'KH', 'KW', 'pad_t', 'pad_l')}
            (Ga, pa), (Gb, pb) = ops.conv2d_wgrad_pair(a['xm'], a['zm'], b['xm'], b['zm'], live32_b=flags, ws=ws, **pkw)
            torch.cuda.synchronize()
            assert bool(torch.isnan(ws[floats:]).all())
            for (G, p), (wG, wp) in (((Ga, pa), _split_ws(ws, 0, S, c)), ((Gb, pb), _split_ws(ws, floats // 2, S, c))):
                assert G.data_ptr() == wG.data_ptr() and p.data_ptr() == wp.data_ptr() and G.shape == wG.shape and p.shape == wp.shape
            _check(c, info, a, Ga, pa, '%s %s problem a' % (c.name, form), False)
            _check(c, info, b, Gb, pb, '%s %s problem b' % (c.name, form), flags is not None)
            return
        prob = _problem(c, info, 'b' if form == 'flagged' else 'a')
        flags = _flags(c, info, prob) if form == 'flagged' else None
        ws, floats = _workspace(S, c)
        out = ops.conv2d_wgrad(prob['xm'], prob['zm'], live32=flags, group=c.layout == 'group', ws=ws, **kw)
        torch.cuda.synchronize()
        assert bool(torch.isnan(ws[floats:]).all())
        slabs, parts = _split_ws(ws, 0, S, c)
        if c.layout == 'group':              # one (slabs, rows) pair per level: the level's own range of the workspace
            assert len(out) == len(c.sizes)
            for l, (G, p) in enumerate(out):
                f0, cnt = info['first'][l], info['count'][l]
                assert G.data_ptr() == slabs[f0].data_ptr() and p.data_ptr() == parts[f0].data_ptr() and G.shape[0] == p.shape[0] == cnt
        else:
            assert out[0].data_ptr() == slabs.data_ptr() and out[1].data_ptr() == parts.data_ptr()
        _check(c, info, prob, slabs, parts, '%s %s' % (c.name, form), flags is not None)
