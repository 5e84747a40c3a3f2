"""GPU parity, op by op, of the squeeze-excite forward and the small streaming helpers every MBConv block calls (csrc/se.hip,
csrc/pack.hip), at the sizes where their loops loop: (a) the pool reduction inside se_gate_fwd with more than four partial rows, in
both instantiations, counted exactly; (b) the gate MLP on many partial rows vs float64; (c) se_dgate across slab counts; (d) the
grid-stride elementwise kernels in their second round; (e) the layout converters beyond one round; (f) colsum, exact; (g) the
depthwise forward's partial rows handed straight to the gate.  The tables are tests/se_fwd_cases.py; tests/test_se_fwd_cases_host.py keeps
them from going shallow.

Two kinds of input.  EXACT: small integers (torch.randint(-3, 4), exact in bf16 too) for the pure reductions -- every product and
partial sum is an integer below 2^24 (asserted on the float64 reference of every case), so the fp32 result does not depend on the
summation order and must be torch.equal to the float64 reference: a dropped, double-counted or misattributed group, pixel or row fails
with zero tolerance.  RANDOM: seeded torch.Generator draws against float64 at the project's tolerances, fp32 storage 1e-4 per element
(assert_close), bf16 storage 2e-2 (x 5 for reductions); the pool rows are drawn positive (rand + 0.5): summing up to 144 positive fp32
terms errs by at most 143 * 2^-24 ~ 8.5e-6 relative, so 1e-4 on pool, mid and gate is a derived bound.  Loop ends additionally get a
PLANTED SPIKE (1024 x the rest) at the element only the last group / pixel / chunk reaches."""
import pytest
import torch

from tests import se_fwd_cases as S
from tests.dwconv_cases import dwconv64, swish64, swish_grad64, tf_same
from tests.gpu_util import assert_close

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F32, BF16 = S.F32, S.BF16
TOL = {F32: 1e-4, BF16: 2e-2}                               # per element, vs float64
RED = {F32: 1e-4, BF16: 5 * 2e-2}                           # reductions over pixels
SPIKE = 1024.0                                              # (a power of two: exact in bf16)
EXACT_BELOW = float(2 ** 24)


def _name(dtype):
    return 'bf16' if dtype == BF16 else 'f32'


def _q(dtype):
    return (lambda t: t.bfloat16().float()) if dtype == BF16 else (lambda t: t)


def _ints(g, *shape):
    return torch.randint(-3, 4, shape, generator=g).float()


def _check(got, ref, tol, what):
    """assert_close (per element), printing the measured figure first."""
    g, r = got.detach().double().cpu(), ref.detach().double().cpu()
    assert g.shape == r.shape, (what, g.shape, r.shape)
    print('FIG %-72s max abs err %.3e  ref max %.3e  tol %g' % (what, float((g - r).abs().max()), float(r.abs().max()), tol))
    assert_close(g, r, tol, what)


def _exact(got, ref64, what):
    """torch.equal with the float64 reference cast to float32; the reference must be an integer-valued tensor below 2^24."""
    g, r = got.detach().float().cpu(), ref64.detach().double().cpu()
    assert g.shape == r.shape, (what, g.shape, r.shape)
    assert float(r.abs().max()) < EXACT_BELOW and bool((r == r.round()).all()), what
    print('FIG %-72s mismatches %d of %d  ref max %.0f  (exact)' % (what, int((g.double() != r).sum()), r.numel(), float(r.abs().max())))
    assert torch.equal(g, r.float()), what


def _same(got, want, what):
    """Bitwise equality of two tensors of one type (a single rounding per element on both sides)."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    print('FIG %-72s mismatches %d of %d  (bitwise)' % (what, int((got != want).sum()), got.numel()))
    assert torch.equal(got, want), what


def _mlp(g, C, Cse):
    """(w1, b1, w2, b2) of a gate MLP, on the CPU."""
    return (torch.randn(Cse, C, generator=g) / C ** 0.5, torch.randn(Cse, generator=g) * 0.1,
            torch.randn(C, Cse, generator=g) / Cse ** 0.5, torch.randn(C, generator=g) * 0.1)


def _gate_fwd(part, mlp, inv_hw):
    from efficientdet.pytorch_amd import ops
    return ops.se_gate_fwd(part if part.is_cuda else part.to(DEV), *(t.to(DEV) for t in mlp), inv_hw, save_mid=True)


def _gate_ref(pool64, mlp, inv_hw):
    w1, b1, w2, b2 = (t.double() for t in mlp)
    mid = (pool64 * inv_hw) @ w1.t() + b1
    return mid, torch.sigmoid(swish64(mid) @ w2.t() + b2)


# ------------------------------------------------------------------------------------------ (a) the pool reduction, exact
@pytest.mark.parametrize('C', S.POOL_C)
@pytest.mark.parametrize('G', S.POOL_G)
def test_pool_sum_counts_every_group_exactly_once(G, C):
    """se_gate_fwd's pooled sum in both instantiations of pool_reduce (one workgroup per image: Cse 4, 16 slices; split: Cse 8, 4 slices).
    One group per image: G images, image b holds an integer row in group b and zeros elsewhere -- pool_out[b] must be that row, so one
    table shows each group counted exactly once (run in chunks of 16 images, the split form's limit).  All groups: B = 3, every group an
    integer row -- pool_out must equal the float64 sum, and two launches must agree bitwise."""
    g = torch.Generator().manual_seed(1000 * G + C)
    rows = _ints(g, G, C)
    rows[rows == 0] = 3.0                               # no zero entry: every element of a dropped group shows
    full = _ints(g, 3, G, C)
    rows_d = rows.to(DEV)
    for form, Cse in S.POOL_FORMS.items():
        mlp = _mlp(g, C, Cse)
        got = []
        for b0 in range(0, G, S.SPLIT_MAX_B):
            nb = min(S.SPLIT_MAX_B, G - b0)
            assert S.gate_form(nb, Cse) == form
            part = torch.zeros(nb, G, C, device=DEV)
            i = torch.arange(nb, device=DEV)
            part[i, b0 + i] = rows_d[b0:b0 + nb]
            got.append(_gate_fwd(part, mlp, 1.0 / 49)[2])
        _exact(torch.cat(got), rows.double(), 'pool, one group per image G%d C%d %s' % (G, C, form))
        gate, mid, pool = _gate_fwd(full, mlp, 1.0 / 49)
        _exact(pool, full.double().sum(1), 'pool, all groups G%d C%d %s' % (G, C, form))
        gate2, mid2, pool2 = _gate_fwd(full, mlp, 1.0 / 49)
        assert torch.equal(pool, pool2) and torch.equal(mid, mid2) and torch.equal(gate, gate2)
        assert bool(torch.isfinite(gate).all()) and bool(torch.isfinite(mid).all())


@pytest.mark.parametrize('C', S.POOL_C)
@pytest.mark.parametrize('G', S.POOL_G)
def test_pool_sum_is_added_in_the_fixed_order_the_kernel_documents(G, C):
    """On rows that do NOT add exactly (rand + 0.5) the pooled sum is bit for bit the restatement of pool_reduce's order
    (tests/se_fwd_cases.pool_reduce_restated: four chains and a tail per slice, (s0 + s1) + (s2 + s3), the slices in order) -- only
    additions, each rounded once, so the fixed pattern the kernel promises can be held to the bit, in both instantiations."""
    g = torch.Generator().manual_seed(2000 * G + C)
    part = torch.rand(2, G, C, generator=g) + 0.5
    for form, Cse in S.POOL_FORMS.items():
        assert S.gate_form(2, Cse) == form
        pool = _gate_fwd(part, _mlp(g, C, Cse), 1.0 / 49)[2].cpu()
        want = torch.stack([S.pool_reduce_restated(part[b], S.NSL[form]) for b in range(2)])
        _same(pool, want, 'pool, restated order G%d C%d %s' % (G, C, form))
        _check(pool, part.double().sum(1), TOL[F32], 'pool, random rows G%d C%d %s' % (G, C, form))


# ------------------------------------------------------------------------------------------ (b) the gate MLP on many partial rows
@pytest.mark.parametrize('spike', [False, True])
@pytest.mark.parametrize('case', S.GATE_CASES, ids=lambda c: 'G%d-C%d-Cse%d-B%d' % c)
def test_gate_forward_on_many_partial_rows(case, spike):
    """se_gate_fwd on positive partial rows [B][G][C] vs float64: pool, mid and gate at 1e-4, in the form tests/se_fwd_cases.gate_form
    names for (B, Cse).  spike: the last group row x 1024 -- the pooled sum is then decided by the group the slice walk reaches last;
    checked on pool only (the spike saturates the gate)."""
    G, C, Cse, B = case
    g = torch.Generator().manual_seed(77 + G * 7 + C + Cse * 13 + B)
    part = torch.rand(B, G, C, generator=g) + 0.5
    if spike:
        part[:, G - 1] *= SPIKE
    mlp = _mlp(g, C, Cse)
    gate, mid, pool = _gate_fwd(part, mlp, S.GATE_INV_HW)
    what = 'se_gate_fwd %s G%d C%d Cse%d B%d%s' % (S.gate_form(B, Cse), G, C, Cse, B, ' spiked' if spike else '')
    pool64 = part.double().sum(1)
    _check(pool, pool64, TOL[F32], what + ' pool')
    assert bool(torch.isfinite(gate).all()) and bool(torch.isfinite(mid).all())
    if not spike:
        mid64, gate64 = _gate_ref(pool64, mlp, S.GATE_INV_HW)
        _check(mid, mid64, TOL[F32], what + ' mid')
        _check(gate, gate64, TOL[F32], what + ' gate')


# ------------------------------------------------------------------------------------------ (c) se_dgate across slab counts
def _pixels(t, dtype):
    """[B][HW][C] on the CPU -> a Map of one pixel row per image (the kernels see H * W only)."""
    from efficientdet.pytorch_amd.ops import Map
    return Map.of(t.view(t.shape[0], 1, t.shape[1], t.shape[2]).contiguous().to(DEV, dtype))


@pytest.mark.parametrize('dtype,C', S.DGATE_CH, ids=lambda v: _name(v) if isinstance(v, torch.dtype) else 'C%d' % v)
@pytest.mark.parametrize('HW', S.DGATE_HW)
def test_se_dgate_across_slab_counts(HW, dtype, C):
    """se_dgate at 1, 2, 63 and the capped 64 slabs with equal and unequal pixel ranges, over the row-group forms of DGATE_CH.  Integer
    inputs, ACT_NONE: as many slab rows as effdet_se_dgate_slabs says, every slab row exactly the float64 sum over ITS pixel range, their
    sum exactly sum_p dy x, two launches bitwise equal.  Random inputs, ACT_SWISH: vs float64 sum dy swish(x) at 1e-4 (bf16: 5 x 2e-2), plain
    and with 1024 planted in dy and x at the last pixel of the last image, last channel."""
    from efficientdet.pytorch_amd import _lib as L, ops
    B = S.DGATE_B
    slabs, ranges, _, _, _ = S.dgate_partition(HW, C, dtype)
    assert slabs == int(L.lib().effdet_se_dgate_slabs(HW))
    g = torch.Generator().manual_seed(31 * HW + C)
    what = 'se_dgate HW%d C%d %s' % (HW, C, _name(dtype))
    dy, x = _ints(g, B, HW, C), _ints(g, B, HW, C)
    dym, xm = _pixels(dy, dtype), _pixels(x, dtype)
    dgp = ops.se_dgate(dym, xm)
    assert dgp.shape == (B, slabs, C), (dgp.shape, slabs)
    prod = dy.double() * x.double()
    _exact(dgp, torch.stack([prod[:, p0:p1].sum(1) for p0, p1 in ranges], dim=1), what + ' slab rows')
    _exact(dgp.sum(1), prod.sum(1), what + ' sum of the slab rows')
    assert torch.equal(dgp, ops.se_dgate(dym, xm))
    q = _q(dtype)
    dy, x = q(torch.randn(B, HW, C, generator=g)), q(torch.randn(B, HW, C, generator=g))
    for spike in (False, True):
        if spike:
            dy[B - 1, HW - 1, C - 1] = SPIKE; x[B - 1, HW - 1, C - 1] = SPIKE
        got = ops.se_dgate(_pixels(dy, dtype), _pixels(x, dtype), ops.ACT_SWISH)
        assert got.shape == (B, slabs, C)
        ref = (dy.double() * swish64(x.double())).sum(1)
        got = got.sum(1).cpu()
        if spike:
            assert float(ref[B - 1, C - 1]) > 0.9 * SPIKE * SPIKE
            _check(got[B - 1, C - 1].view(1), ref[B - 1, C - 1].view(1), RED[dtype], what + ' swish (spiked element)')
            keep = torch.ones(B, C, dtype=torch.bool); keep[B - 1, C - 1] = False
            _check(got[keep], ref[keep], RED[dtype], what + ' swish (the rest)')
        else:
            _check(got, ref, RED[dtype], what + ' swish')


# ------------------------------------------------------------------------------------------ (d) elementwise kernels, second round
_ELEM = {}


def _elem(case):
    """Operands of one elementwise case, drawn once and shared by its tests (left unchanged): CPU fp32 values already rounded to the
    storage type, and their device copies.  x carries 1024 in the very last 16-byte chunk of the last image."""
    if case not in _ELEM:
        from efficientdet.pytorch_amd.ops import Map
        dt, B, H, W, C = case
        n, cpr, per_image, rounds = S.elemwise_chunks(*case)
        assert rounds == 2 and n > S.ELEMWISE_ROUND
        g = torch.Generator().manual_seed(900 + C)
        q = _q(dt)
        x, aux = q(torch.randn(B, H, W, C, generator=g)), q(torch.randn(B, H, W, C, generator=g))
        x[B - 1, H - 1, W - 1, C - S.ce(dt):] = SPIKE
        t = dict(x=x, aux=aux, gate=torch.rand(B, C, generator=g) * 0.9 + 0.05, dpool=torch.randn(B, C, generator=g) * 0.1,
                 rs=0.5 + torch.rand(B, generator=g))
        assert len(set(t['rs'].tolist())) == B and not torch.equal(t['gate'][0], t['gate'][1]) and not torch.equal(t['dpool'][0], t['dpool'][1])
        d = {k: v.to(DEV, dt if k in ('x', 'aux') else F32) for k, v in t.items()}
        _ELEM[case] = (t, d, Map.of(d['x']), Map.of(d['aux']))
    return _ELEM[case]


def _elem_check(case, got, ref64, exact_want, what):
    """fp32 storage with a single rounding per element: bitwise equal to the same expression in torch float32 (exact_want, on the device).
    Otherwise vs float64 at the storage type's tolerance, the spiked last chunk apart so that it does not loosen the check of the rest."""
    dt, B, H, W, C = case
    what = '%s %s' % (what, _name(dt))
    got = got.tensor() if hasattr(got, 'tensor') else got
    if dt == F32 and exact_want is not None:
        _same(got, exact_want, what)
        return
    g, r = got.float().cpu().view(-1), ref64.view(-1)
    k = S.ce(dt)
    _check(g[:-k], r[:-k], TOL[dt], what)
    _check(g[-k:], r[-k:], TOL[dt], what + ' (spiked last chunk)')


ELEM_IDS = [_name(c[0]) for c in S.ELEMWISE_CASES]


@pytest.mark.parametrize('case', S.ELEMWISE_CASES, ids=ELEM_IDS)
def test_channel_scale_in_its_second_round(case):
    """channel_scale over more chunks than one round of 4096 workgroups covers (b = row / HW, cc = i % cpr beyond the first round), the
    gate differing per image: ACT_NONE (fp32: one rounding, bitwise x * gate) and ACT_SWISH vs float64."""
    from efficientdet.pytorch_amd import ops
    dt, B, H, W, C = case
    t, d, xm, auxm = _elem(case)
    gate64 = t['gate'].double().view(B, 1, 1, C)
    _elem_check(case, ops.channel_scale(xm, d['gate']), t['x'].double() * gate64,
                d['x'] * d['gate'].view(B, 1, 1, C) if dt == F32 else None, 'channel_scale')
    _elem_check(case, ops.channel_scale(xm, d['gate'], ops.ACT_SWISH), swish64(t['x'].double()) * gate64, None, 'channel_scale swish')


@pytest.mark.parametrize('case', S.ELEMWISE_CASES, ids=ELEM_IDS)
def test_se_bwd_apply_in_its_second_round(case):
    """(dy gate + dpool) swish'(z) vs float64, gate and dpool differing per image."""
    from efficientdet.pytorch_amd import ops
    dt, B, H, W, C = case
    t, d, xm, auxm = _elem(case)
    ref = (t['x'].double() * t['gate'].double().view(B, 1, 1, C) + t['dpool'].double().view(B, 1, 1, C)) * swish_grad64(t['aux'].double())
    _elem_check(case, ops.se_bwd_apply(xm, d['gate'], d['dpool'], auxm), ref, None, 'se_bwd_apply')


@pytest.mark.parametrize('case', S.ELEMWISE_CASES, ids=ELEM_IDS)
def test_act_bwd_in_its_second_round(case):
    """act_bwd: RELU (fp32 bitwise), SWISH with the per-image row scale (i / per_image_chunks beyond the first round) vs float64, NONE
    with the row scale (fp32: one rounding, bitwise dy * rs)."""
    from efficientdet.pytorch_amd import ops
    dt, B, H, W, C = case
    t, d, xm, auxm = _elem(case)
    rs64 = t['rs'].double().view(B, 1, 1, 1)
    _elem_check(case, ops.act_bwd(xm, auxm, ops.ACT_RELU), t['x'].double() * (t['aux'] > 0),
                torch.where(d['aux'] > 0, d['x'], torch.zeros_like(d['x'])) if dt == F32 else None, 'act_bwd relu')
    _elem_check(case, ops.act_bwd(xm, auxm, ops.ACT_SWISH, rowscale=d['rs']), t['x'].double() * swish_grad64(t['aux'].double()) * rs64, None,
                'act_bwd swish rowscale')
    _elem_check(case, ops.act_bwd(xm, None, ops.ACT_NONE, rowscale=d['rs']), t['x'].double() * rs64,
                d['x'] * d['rs'].view(B, 1, 1, 1) if dt == F32 else None, 'act_bwd none rowscale')


@pytest.mark.parametrize('case', S.ELEMWISE_CASES, ids=ELEM_IDS)
def test_add_inplace_in_its_second_round(case):
    """y += x (fp32: bitwise the torch sum); the shared operands stay untouched (the sum goes into a copy)."""
    from efficientdet.pytorch_amd import ops
    from efficientdet.pytorch_amd.ops import Map
    dt, B, H, W, C = case
    t, d, xm, auxm = _elem(case)
    y = Map.of(d['x'].clone())
    ops.add_inplace(y, auxm)
    _elem_check(case, y, t['x'].double() + t['aux'].double(), d['x'] + d['aux'] if dt == F32 else None, 'add_inplace')
    assert torch.equal(d['x'].cpu().float(), t['x'])


# ------------------------------------------------------------------------------------------ (e) layout converters beyond one round
@pytest.mark.parametrize('case', S.TO_NHWC_CASES, ids=lambda c: '%s-%s-C%d-%dx%d-cpad%d' % (c[0], _name(c[1]), c[3], c[4], c[5], c[6]))
def test_nchw_to_nhwc_beyond_one_round(case):
    """More items than one round of 2048 workgroups covers, a partial last workgroup: a permutation of already-rounded values, so the
    real channels are torch.equal to the input and the padding channels are 0.0."""
    from efficientdet.pytorch_amd import ops
    path, dt, B, C, H, W, cpad = case
    assert S.to_nhwc_path(dt, C, cpad) == path and S.pack_items(path, B, H, W, cpad)[1] == 2
    g = torch.Generator().manual_seed(5 + cpad + H)
    x = _q(dt)(torch.randn(B, C, H, W, generator=g))
    m = ops.nchw_to_nhwc(x.to(DEV), dt, cpad=cpad)
    out = m.tensor().float().cpu()
    assert out.shape == (B, H, W, cpad)
    _same(out[..., :C], x.permute(0, 2, 3, 1), 'nchw_to_nhwc %s %s C%d cpad%d' % (path, _name(dt), C, cpad))
    if cpad > C:
        assert float(out[..., C:].abs().max()) == 0.0


@pytest.mark.parametrize('case', S.TO_NCHW_CASES, ids=lambda c: _name(c[0]))
def test_nhwc_to_nchw_beyond_one_round(case):
    from efficientdet.pytorch_amd import ops
    from efficientdet.pytorch_amd.ops import Map
    dt, B, H, W, C = case
    assert B * H * W * C > S.PACK_ROUND
    g = torch.Generator().manual_seed(6)
    x = _q(dt)(torch.randn(B, H, W, C, generator=g))
    out = ops.nhwc_to_nchw(Map.of(x.to(DEV, dt))).cpu()
    assert out.dtype == torch.float32
    _same(out, x.permute(0, 3, 1, 2).contiguous(), 'nhwc_to_nchw %s' % _name(dt))


# ------------------------------------------------------------------------------------------ (f) colsum, exact
@pytest.mark.parametrize('dtype', [F32, BF16], ids=_name)
@pytest.mark.parametrize('rows', S.COLSUM_ROWS)
def test_colsum_is_exact_with_a_row_stride_and_a_filled_output(rows, dtype):
    """out[c] += sum_rows x[row][c] on integers: every exit of the two-chain stride-8 row walk and its tail, C below / at / one past a
    64-column workgroup, the rows at stride C and at stride C + 24 (a view of a wider buffer whose other columns hold 1000), out
    pre-filled with integers -- torch.equal to out0 + x.sum(0)."""
    from efficientdet.pytorch_amd import _lib as L, ops
    g = torch.Generator().manual_seed(11 * rows)
    for C in S.COLSUM_C:
        for extra in S.COLSUM_LD_EXTRA:
            ld = C + extra
            buf = torch.full((rows, ld), 1000.0)
            buf[:, :C] = _ints(g, rows, C)
            out0 = _ints(g, C)
            bd, out = buf.to(DEV, dtype), out0.to(DEV)
            view = bd[:, :C]
            assert view.stride() == (ld, 1) and view.data_ptr() == bd.data_ptr()
            if extra == 0:
                ops.colsum(view, out)
            else:
                L.check(L.lib().effdet_colsum(L.ptr(view), L.ptr(out), L.dtype_code(dtype), rows, C, ld, L.stream_ptr()), 'effdet_colsum')
            _exact(out, out0.double() + buf[:, :C].double().sum(0), 'colsum rows%d C%d ld%d %s' % (rows, C, ld, _name(dtype)))


# ------------------------------------------------------------------------------------------ (g) producer -> consumer chain
def _chain_gates(pp, y64, g, C, HW, tol, what):
    """The producer's partial rows [B][G][C] straight into se_gate_fwd, in both forms, vs the float64 gate of mean(y64)."""
    assert pp.dim() == 3 and pp.shape[1] > 4, pp.shape
    pool64 = y64.sum(dim=(2, 3))
    for Cse in S.CHAIN_CSE:
        mlp = _mlp(g, C, Cse)
        gate, mid, pool = _gate_fwd(pp, mlp, 1.0 / HW)
        mid64, gate64 = _gate_ref(pool64, mlp, 1.0 / HW)
        form = S.gate_form(pp.shape[0], Cse)
        _check(pool, pool64, tol if tol == TOL[F32] else RED[BF16], '%s -> pool (%s, G%d)' % (what, form, pp.shape[1]))
        _check(gate, gate64, tol, '%s -> gate (%s, G%d)' % (what, form, pp.shape[1]))


@pytest.mark.parametrize('dtype', [F32, BF16], ids=_name)
def test_dwconv_partial_rows_into_the_gate(dtype):
    """dwconv_fwd(pool=True) at 2 x 64 x 64 x 96, k 3, stride 1 leaves G > 4 partial rows per image (the count the host query reports);
    se_gate_fwd on them == float64 sigmoid(W2 swish(W1 mean(swish(z)) + b1) + b2) from the same inputs: the real G and the real row
    layout meeting the reducer."""
    from efficientdet.pytorch_amd import _lib as L, ops
    from efficientdet.pytorch_amd.ops import Map
    B, H, W = S.CHAIN_GEOMETRY
    C, k = S.CHAIN_C, S.CHAIN_K
    g = torch.Generator().manual_seed(21)
    x = _q(dtype)(torch.randn(B, C, H, W, generator=g))
    w = torch.randn(C, 1, k, k, generator=g) * (2.0 / (k * k)) ** 0.5
    scale = 0.5 + torch.rand(C, generator=g); shift = torch.randn(C, generator=g) * 0.2
    (pt, _, Ho), (pl, _, Wo) = tf_same(H, k, 1), tf_same(W, k, 1)
    y64 = swish64(dwconv64(x.double(), w.double(), k, 1) * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1))
    xm = Map.of(x.permute(0, 2, 3, 1).contiguous().to(DEV, dtype))
    _, _, pp = ops.dwconv_fwd(xm, ops.dw_pack_weight(w.to(DEV)), scale.to(DEV), shift.to(DEV), k, 1, pt, pl, Ho, Wo, pool=True)
    assert pp.shape[1] == int(L.lib().effdet_dwconv_fwd_pool_groups(L.dtype_code(dtype), B, C, 1, Ho, Wo))
    _chain_gates(pp, y64, g, C, Ho * Wo, TOL[dtype], 'dwconv_fwd %s' % _name(dtype))


def test_expand_dw_partial_rows_into_the_gate():
    """The same for the fused expand -> depthwise forward at Cin 16 (Cexp 96), 2 x 64 x 64, fp32, at 1e-4."""
    from efficientdet.pytorch_amd import _lib as L, ops
    from efficientdet.pytorch_amd.ops import Map
    B, H, W = S.CHAIN_GEOMETRY
    Cin, k = S.CHAIN_CIN, S.CHAIN_K
    Cexp = 6 * Cin
    g = torch.Generator().manual_seed(22)
    x = torch.randn(B, Cin, H, W, generator=g)
    we = torch.randn(Cexp, Cin, 1, 1, generator=g) / Cin ** 0.5
    s0 = 0.5 + torch.rand(Cexp, generator=g); t0 = torch.randn(Cexp, generator=g) * 0.5
    wd = torch.randn(Cexp, 1, k, k, generator=g) * (2.0 / (k * k)) ** 0.5
    s1 = 0.5 + torch.rand(Cexp, generator=g); t1 = torch.randn(Cexp, generator=g) * 0.2
    (pt, _, Ho), (pl, _, Wo) = tf_same(H, k, 1), tf_same(W, k, 1)
    e = swish64(torch.einsum('bihw,oi->bohw', x.double(), we.double().view(Cexp, Cin)) * s0.double().view(1, -1, 1, 1) + t0.double().view(1, -1, 1, 1))
    y64 = swish64(dwconv64(e, wd.double(), k, 1) * s1.double().view(1, -1, 1, 1) + t1.double().view(1, -1, 1, 1))
    xm = Map.of(x.permute(0, 2, 3, 1).contiguous().to(DEV))
    _, pp = ops.expand_dw_fwd(xm, we.to(DEV), s0.to(DEV), t0.to(DEV), ops.dw_pack_weight(wd.to(DEV)), s1.to(DEV), t1.to(DEV), k, 1, pt, pl, Ho, Wo)
    assert pp.shape[1] == int(L.lib().effdet_mbconv_expand_dw_pool_groups(B, Cexp, 1, Ho, Wo))
    _chain_gates(pp, y64, g, Cexp, Ho * Wo, TOL[F32], 'expand_dw_fwd')
