"""CPU tier of the streaming pointwise-backward tests: the tables of tests/pw_stream_cases.py are served by the library's own gates
(effdet_pw_bwd_slabs, effdet_pw_dgrad_se_supported: no device work), reach every class they are meant to reach -- asserted over the
tables, so that an edit cannot silently lose one -- the support boundaries are where the kernels' text puts them, and the float64
references are the gradients of the plain conv + BN scale (+ squeeze-excite + Swish) chain."""
import pytest
import torch
import torch.nn.functional as F

from tests import pw_stream_cases as P


def _lib():
    from efficientdet.pytorch_amd import _lib as L
    return L.require('effdet_pw_bwd_slabs', 'effdet_pw_bwd', 'effdet_pw_dgrad_se_supported', 'effdet_pw_dgrad_se')


# ----------------------------------------------------------------------------- the tables against the gates
@pytest.mark.parametrize('c', P.PW_BWD_CASES, ids=P.bwd_id)
def test_pw_bwd_case_is_served_with_the_geometry_restated_here(c):
    g = P.bwd_geometry(c)
    assert int(_lib().effdet_pw_bwd_slabs(g['M'], c.Cin, g['Cexp'])) == g['nwg'] == P.PWB_SLOTS[c.Cin]
    assert g['M'] >= P.PWB_MIN_M and g['ntiles'] == -(-g['M'] // 64) and g['tiles_min'] >= 2
    assert g['tiles_max'] - g['tiles_min'] == (1 if g['ntiles'] % g['nwg'] else 0)
    assert g['dz_bytes'] <= 110e6, 'keep the expanded gradient at ~100 MB'
    # exact inputs: the largest partial sum (the whole-M weight gradient of |dz|, |x| <= 4) stays far below 2^24
    assert 16 * g['M'] < 2 ** 22 and 4 * 2 * 4 * g['Cexp'] < 2 ** 22


@pytest.mark.parametrize('c', P.PW_DGRAD_CASES, ids=P.dgrad_id)
def test_pw_dgrad_case_is_served_with_the_geometry_restated_here(c):
    g = P.dgrad_geometry(c)
    assert int(_lib().effdet_pw_dgrad_se_supported(g['M'], c.Co, c.Ce)) == 1
    assert g['M'] >= P.PWD_MIN_M and g['nwg'] == P.PWD_SLOTS and (g['tiles_min'], g['tiles_max']) == (1, 2)        # already ragged
    assert g['lds'] <= P.PWD_LDS_BYTES and g['nj'] * 16 == c.Ce
    assert g['z_bytes'] <= 180e6
    assert (c.Co, c.Ce) in P.DGRAD_PAIRS and P.dgrad_classes(c)[0] in P.DGRAD_GEOMETRIES
    # exact inputs: |dy w s2| <= 32 in quarters, x rowscale (2^-3 .. 2) x gate (2^-2 .. 4) + dpool: multiples of 2^-7 below 2^15
    assert 32 * c.Co * 2 * 4 + 4 < 2 ** 15


def _bwd_coverage(cases):
    seen = {}
    for c in cases:
        seen.setdefault(c.Cin, set()).update(P.bwd_classes(c))
    return seen


def _bwd_missing(cases):
    seen = _bwd_coverage(cases)
    return sorted((cin, k) for cin in (16, 24, 32) for k in P.BWD_CLASSES if k not in seen.get(cin, ()))


def _dgrad_missing(cases):
    missing = []
    geo, pairs, opts = {}, set(), set()
    for c in cases:
        geo.setdefault(c.Co, set()).add(P.dgrad_classes(c)[0])
        pairs.add((c.Co, c.Ce)); opts |= P.dgrad_classes(c)[1]
    missing += [(co, k) for co in (16, 24, 40) for k in P.DGRAD_GEOMETRIES if k not in geo.get(co, ())]
    missing += [p for p in P.DGRAD_PAIRS if p not in pairs] + [o for o in P.DGRAD_OPTIONS if o not in opts]
    return missing


def test_pw_bwd_table_reaches_every_class_for_every_instance():
    """Per Cin (= per template instance): the threshold, the three tails, a tail with and one without the identity-skip gradient, unequal
    tile counts per workgroup, no BN scale.  Taking out a case that alone carries a class is noticed."""
    assert _bwd_missing(P.PW_BWD_CASES) == []
    assert len(P.PW_BWD_CASES) <= 13
    sole = [i for i in range(len(P.PW_BWD_CASES)) if _bwd_missing(P.PW_BWD_CASES[:i] + P.PW_BWD_CASES[i + 1:])]
    assert sole, 'no case alone carries a class: the table could be smaller'
    # the classes as the kernel sees them: live pixels of the last tile per wave
    for c in P.PW_BWD_CASES:
        t = P.bwd_geometry(c)['tail']
        live = [max(0, min(16, t - 16 * w)) for w in range(4)] if t else [16] * 4
        assert live == {0: [16] * 4, 1: [1, 0, 0, 0], 17: [16, 1, 0, 0], 63: [16, 16, 16, 15]}[t]
    # Cin = 24 / 32 at the threshold: every workgroup owns 4 tiles; the ragged case: 38 workgroups own 5
    g = P.bwd_geometry(P.PwBwdCase(1, 317, 421, 24, True, False))
    assert (g['ntiles'] % g['nwg'], g['tiles_min'], g['tiles_max']) == (38, 4, 5)
    assert P.bwd_geometry(P.PwBwdCase(2, 256, 256, 32, True, True))['tiles_max'] == 4


def test_pw_dgrad_table_reaches_every_class():
    """Every (Co, Ce) pair, the three image geometries for every Co, rowscale / scale absent and both given; what the pairs stand for."""
    assert _dgrad_missing(P.PW_DGRAD_CASES) == []
    sole = [i for i in range(len(P.PW_DGRAD_CASES)) if _dgrad_missing(P.PW_DGRAD_CASES[:i] + P.PW_DGRAD_CASES[i + 1:])]
    assert sole
    by_pair = {(c.Co, c.Ce): P.dgrad_geometry(c) for c in P.PW_DGRAD_CASES}
    assert {p: (g['nj_mod'], g['k_tail']) for p, g in by_pair.items()} == \
        {(16, 48): (0, 0), (16, 64): (1, 0), (24, 80): (2, 1), (40, 112): (1, 1), (40, 400): (1, 1), (24, 672): (0, 1)}
    assert by_pair[(40, 400)]['lds'] == 64640 and by_pair[(24, 672)]['lds'] == 64896
    for co, ce in ((40, 400), (24, 672)):
        assert P.dgrad_lds_bytes(co, ce + 16) > P.PWD_LDS_BYTES
    geo = {P.dgrad_classes(c)[0]: P.dgrad_geometry(c) for c in P.PW_DGRAD_CASES}
    assert geo['exact65536']['M'] == 65536 and geo['exact65536']['tail'] == 0
    assert (geo['straddle']['tail'], geo['straddle']['span_min'], geo['straddle']['span_max']) == (7, 1, 2)
    assert (geo['tiny_images']['HW'], geo['tiny_images']['span_min'], geo['tiny_images']['span_max']) == (9, 2, 3)


def test_support_boundaries():
    lib = _lib()
    slabs, sup = (lambda *a: int(lib.effdet_pw_bwd_slabs(*a))), (lambda *a: int(lib.effdet_pw_dgrad_se_supported(*a)))
    assert slabs(131072, 16, 96) == 768 and slabs(131072, 24, 144) == 512 and slabs(131072, 32, 192) == 512
    assert slabs(131071, 16, 96) == 0 and slabs(131071, 32, 192) == 0
    assert slabs(262144, 40, 240) == 0 and slabs(262144, 8, 48) == 0
    assert slabs(262144, 16, 64) == 0 and slabs(262144, 24, 96) == 0 and slabs(262144, 32, 96) == 0
    assert sup(65536, 16, 48) == 1 and sup(65535, 16, 48) == 0 and sup(65535, 40, 112) == 0
    assert sup(65536, 16, 32) == 0 and sup(65536, 16, 56) == 0 and sup(65536, 24, 56) == 0
    assert sup(65536, 40, 400) == 1 and sup(65536, 40, 416) == 0
    assert sup(65536, 24, 672) == 1 and sup(65536, 24, 688) == 0
    assert sup(65536, 16, 1008) == 1 and sup(65536, 16, 1024) == 0
    assert sup(65536, 32, 96) == 0 and sup(65536, 8, 96) == 0 and sup(65536, 48, 96) == 0


def test_maps_past_the_buffer_descriptor_are_refused_on_the_host():
    """M * C * 4 >= 0xFFFF0000: the 32-bit descriptors cannot cover the map -- slabs == 0 / unsupported, and the entry points answer
    EFFDET_EUNSUPPORTED before any launch (non-null placeholder addresses: nothing is dereferenced)."""
    lib = _lib()
    fake = 0x1000
    for cin in (16, 24, 32):
        ce = 6 * cin
        m = -(-P.DESCRIPTOR_LIMIT // (4 * ce))
        assert int(lib.effdet_pw_bwd_slabs(m, cin, ce)) == 0 and int(lib.effdet_pw_bwd_slabs(m - 1, cin, ce)) == P.PWB_SLOTS[cin]
        assert int(lib.effdet_pw_bwd(fake, fake, fake, None, None, fake, fake, fake, m, cin, ce, None)) == P.EUNSUPPORTED
    assert int(lib.effdet_pw_bwd(fake, fake, fake, None, None, fake, fake, fake, 131071, 16, 96, None)) == P.EUNSUPPORTED
    m = -(-P.DESCRIPTOR_LIMIT // (4 * 48))
    assert int(lib.effdet_pw_dgrad_se_supported(m, 16, 48)) == 0 and int(lib.effdet_pw_dgrad_se_supported(m - 1, 16, 48)) == 1
    assert int(lib.effdet_pw_dgrad_se(fake, fake, None, None, fake, fake, fake, fake, m, m, 1, 16, 48, None)) == P.EUNSUPPORTED
    assert int(lib.effdet_pw_dgrad_se(fake, fake, None, None, fake, fake, fake, fake, 65535, 65535, 1, 16, 48, None)) == P.EUNSUPPORTED


# ----------------------------------------------------------------------------- the exact inputs
def test_hashed_integers_depend_on_row_and_column_without_a_short_period():
    t = P.hash_ints(512, 192, 4, 1)
    assert t.dtype == torch.float32 and float(t.min()) == -4 and float(t.max()) == 4 and bool((t == t.round()).all())
    assert sorted(set(t.view(-1).tolist())) == list(range(-4, 5))
    for d in (1, 4, 16, 64):                      # no period in the channels, none in the pixels; not a function of one index alone
        assert float((t[:, d:] != t[:, :-d]).float().mean()) > 0.8
        assert float((t[d:] != t[:-d]).float().mean()) > 0.8
    assert not torch.equal(P.hash_ints(512, 192, 4, 2), t)                                  # the salt
    s = P.hash_pow2(192, 1, 4).view(-1)
    assert set(s.tolist()) == {0.25, 0.5, 1.0, 2.0, 4.0} and float((s[1:] != s[:-1]).float().mean()) > 0.6
    z = P.hash_choice(512, 192, P.Z_PASS, P.Z_BLOCK, 17)
    assert set(z.view(-1).tolist()) == {P.Z_PASS, P.Z_BLOCK} and 0.4 < float((z == P.Z_PASS).float().mean()) < 0.6
    for d in (4, 16):
        assert float((z[:, d:] != z[:, :-d]).float().mean()) > 0.4 and float((z[4 * d:] != z[:-4 * d]).float().mean()) > 0.4


def test_exact_inputs_keep_every_partial_sum_exact_in_fp32():
    """On a small M: the float64 references of the exact inputs are multiples of 2^-7 and cast to fp32 without loss."""
    c = P.PwBwdCase(1, 1, 1000, 24, True, True)
    i = P.bwd_exact_inputs(c)
    assert float(i.dz.abs().max()) <= 4 and float(i.x.abs().max()) <= 4 and float(i.w.abs().max()) <= 2
    assert bool((i.res * 4 == (i.res * 4).round()).all()) and bool((torch.log2(i.scale) == torch.log2(i.scale).round()).all())
    r = P.bwd_reference(i, 3)
    for t in r:
        assert torch.equal(t.float().double(), t) and bool((t * 4 == (t * 4).round()).all())
    d = P.PwDgradCase(7, 3, 5, 40, 112, True, True)
    j = P.dgrad_exact_inputs(d)
    assert float(j.dy.abs().max()) <= 4 and float(j.w.abs().max()) <= 2
    for t in (j.scale, j.rowscale, j.gate):
        assert bool((torch.log2(t) == torch.log2(t).round()).all()) and len(set(t.view(-1).tolist())) > 1
    assert bool((j.dpool * 4 == (j.dpool * 4).round()).all())
    r = P.dgrad_exact_reference(j, d.B, d.H * d.W)
    assert torch.equal(r.float().double(), r) and bool((r * 128 == (r * 128).round()).all())
    assert 0.3 < float((r == 0).double().mean()) < 0.7
    # the float64 Swish' at the two z_d values is 1 and 0 to 1e-15: the exact reference is the plain one
    full = P.dgrad_reference(j, d.B, d.H * d.W)
    assert float((full - r).abs().max()) <= 1e-12 * float(r.abs().max())


# ----------------------------------------------------------------------------- the references
def _swish(t):
    return t * torch.sigmoid(t)


@pytest.mark.parametrize('skip,scaled', [(True, True), (False, True), (True, False)])
def test_pw_bwd_reference_is_the_gradient_of_the_expand_conv(skip, scaled):
    """M = 203 (four tiles, the last of 11 pixels) over 3 workgroups: torch.autograd of the float64 1x1 conv + BN scale gives dx, the
    scale-free weight gradient and dsum; the per-slab reference is the explicit loop over tiles and sums to the whole-tensor one."""
    c = P.PwBwdCase(1, 7, 29, 16, skip, scaled)
    M, Ci, Ce, nwg = 203, 16, 96, 3
    i = P.bwd_random_inputs(c)
    if scaled:
        i = i._replace(scale=P.hash_pow2(Ce, 1, 4).view(-1))                  # powers of two: fl32(w * s) is w * s
    ref = P.bwd_reference(i, nwg)
    x = i.x.double().view(1, 7, 29, Ci).permute(0, 3, 1, 2).clone().requires_grad_(True)
    w = i.w.double().view(Ce, Ci, 1, 1).clone().requires_grad_(True)
    shift = torch.zeros(Ce, dtype=torch.float64, requires_grad=True)
    s = i.scale.double() if scaled else torch.ones(Ce, dtype=torch.float64)
    z = F.conv2d(x, w) * s.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    z.backward(i.dz.double().view(1, 7, 29, Ce).permute(0, 3, 1, 2))
    dx = x.grad.permute(0, 2, 3, 1).reshape(M, Ci) + (i.res.double() if skip else 0)
    tol = lambda t: 1e-13 * float(t.abs().max())
    assert float((ref.dx - dx).abs().max()) <= tol(dx)
    G = w.grad.view(Ce, Ci) / s.view(-1, 1)
    assert float((ref.slabs.sum(0) - G).abs().max()) <= tol(G)
    assert float((ref.dsum.sum(0) - shift.grad).abs().max()) <= tol(shift.grad)
    for wg in range(nwg):
        g, d = torch.zeros(Ce, Ci, dtype=torch.float64), torch.zeros(Ce, dtype=torch.float64)
        for t in range(wg, 4, nwg):
            g += i.dz.double()[64 * t:64 * t + 64].t() @ i.x.double()[64 * t:64 * t + 64]
            d += i.dz.double()[64 * t:64 * t + 64].sum(0)
        assert float((ref.slabs[wg] - g).abs().max()) <= tol(g) and float((ref.dsum[wg] - d).abs().max()) <= tol(d)
    assert P.owned_pixels(M, nwg).tolist() == [75.0, 64.0, 64.0]
    # the bounds: their scales dominate, and a plain fp32 evaluation in another order stays within them
    b = P.bwd_bounds(i, nwg, ref)
    ws32 = i.w * i.scale.view(-1, 1) if scaled else i.w
    dx32 = (i.dz @ ws32 + i.res) if skip else i.dz @ ws32
    assert bool(((dx32.double() - ref.dx).abs() <= b.dx).all())
    slab32 = torch.stack([sum(i.dz[64 * t:64 * t + 64].t() @ i.x[64 * t:64 * t + 64] for t in range(wg, 4, nwg)) for wg in range(nwg)])
    assert bool(((slab32.double() - ref.slabs).abs() <= b.slabs).all())
    assert float((b.dsum[0] / P.bwd_reference(i, nwg, absolute=True).dsum[0]).max()) == pytest.approx(P.gamma(77), rel=1e-12)


@pytest.mark.parametrize('B,H,W,rowscale,scaled', [(3, 8, 9, True, True), (23, 3, 3, False, True), (2, 10, 10, True, False)])
def test_pw_dgrad_reference_is_the_gradient_of_the_se_project_chain(B, H, W, rowscale, scaled):
    """torch.autograd of float64 Swish -> squeeze-excite gate -> 1x1 project conv -> BN scale -> per-image row scale, with the pooled
    path's gradient dpool flowing into every pixel of its image: d / d z_d is the reference."""
    c = P.PwDgradCase(B, H, W, 24, 80, rowscale, scaled)
    HW, Co, Ce = H * W, 24, 80
    i = P.dgrad_random_inputs(c)
    if scaled:
        i = i._replace(scale=P.hash_pow2(Co, 1, 13).view(-1))
    ref = P.dgrad_reference(i, B, HW)
    z = i.zd.double().view(B, H, W, Ce).permute(0, 3, 1, 2).clone().requires_grad_(True)
    a = _swish(z)
    y = F.conv2d(a * i.gate.double().view(B, Ce, 1, 1), i.w.double().view(Co, Ce, 1, 1))
    if scaled:
        y = y * i.scale.double().view(1, -1, 1, 1)
    if rowscale:
        y = y * i.rowscale.double().view(B, 1, 1, 1)
    loss = (y * i.dy.double().view(B, H, W, Co).permute(0, 3, 1, 2)).sum() + (a.sum(dim=(2, 3)) * i.dpool.double()).sum()
    loss.backward()
    got = z.grad.permute(0, 2, 3, 1).reshape(B * HW, Ce)
    assert float((ref - got).abs().max()) <= 1e-13 * float(got.abs().max())
    # the bound dominates a plain fp32 evaluation (torch's own sigmoid: its error is far inside E)
    v32 = i.dy @ (i.w * i.scale.view(-1, 1) if scaled else i.w)
    if rowscale:
        v32 = v32 * i.rowscale.repeat_interleave(HW).view(-1, 1)
    v32 = (v32.view(B, HW, Ce) * i.gate.view(B, 1, Ce) + i.dpool.view(B, 1, Ce)).view(B * HW, Ce)
    sg = torch.sigmoid(i.zd)
    out32 = v32 * (sg * (1 + i.zd * (1 - sg)))
    bound = P.dgrad_bound(i, B, HW, ref)
    assert bool(((out32.double() - ref).abs() <= bound).all())
    assert bool((P.swish_grad_magnitude(i.zd) >= P.swish_grad64(i.zd).abs() * (1 - 1e-15)).all())
    pos = i.zd >= 0
    assert torch.equal(P.swish_grad_magnitude(i.zd)[pos], P.swish_grad64(i.zd)[pos])


def test_error_constants():
    assert P.gamma(98) == 98 * 2.0 ** -24 / (1 - 98 * 2.0 ** -24)
    assert 1e-7 < P.SWISH_GRAD_E < 1e-5
    # Swish' crosses zero once, at z = -1.2785: there |ref| vanishes and only the magnitude m(z) scales an error
    z = torch.tensor([-1.27846454276107])
    assert abs(float(P.swish_grad64(z))) < 1e-7 and float(P.swish_grad_magnitude(z)) > 0.25
