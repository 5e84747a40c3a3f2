"""GPU parity, op by op, of the fused squeeze-excite backward of an MBConv block (functional.mbconv_bwd, the SE_FUSED branch) against
float64 (tests/mbconv_tail_ref.py): (a) per-image weight-gradient slabs, (b) the slab sum + unpack with per-image / per-channel
factors, (c) the gate gradient from the slabs, (d) the gate MLP's backward, (e) the data-gradient epilogue on the MFMA kernels,
(f) the whole branch, fused and un-fused.

Every input is a seeded torch.Generator draw.  Tolerances are the project's own per category: fp32 storage vs float64 1e-4 per element
(assert_close), 2e-5 of tensor scale for raw split-K slabs; bf16x3 products 1e-3; bf16 storage 2e-2, 5x that for reductions.
Loop tails and guards additionally get a PLANTED SPIKE: the element only the tail / guard reaches carries ~1e3 x the rest, so leaving it
out moves the result by orders of magnitude more than any tolerance."""
import pytest
import torch

from tests.gpu_util import assert_close, assert_close_scale
from tests.mbconv_tail_ref import make_tail_inputs, mbconv_tail_ref, se_gate_bwd_ref, swish_grad, unpack_ref
from tests.se_fused_cases import ARITHS, BRANCH_CASES, DGRAD_CASES, IMAGE_SPLIT_CASES

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TOL = {'f32': 1e-4, 'bf16x3': 1e-3, 'bf16': 2e-2}          # per element, vs float64
RAW = {'f32': 2e-5, 'bf16x3': 1e-3, 'bf16': 2e-2}          # raw slabs, at tensor scale
SPIKE = 1024.0                                             # (a power of two: exact in bf16 and in the bf16 hi + lo split)


def _dtype(arith):
    return torch.bfloat16 if arith == 'bf16' else torch.float32


def _q(arith):
    return (lambda t: t.bfloat16().float()) if arith == 'bf16' else (lambda t: t)


class _arith:
    """The fp32-storage arithmetic of the launches inside ('bf16': storage decides, the switch stays 'f32')."""

    def __init__(self, arith):
        self.mode = 'bf16x3' if arith == 'bf16x3' else 'f32'

    def __enter__(self):
        from efficientdet.pytorch_amd import ops
        self.old = ops.set_f32_arith(self.mode)

    def __exit__(self, *a):
        from efficientdet.pytorch_amd import ops
        ops.set_f32_arith(self.old)
        return False


def _check(got, ref, tol, what, scale=False):
    """assert_close (per element) or assert_close_scale (tensor scale), printing the measured figure first."""
    g, r = got.detach().double().cpu(), ref.detach().double().cpu()
    assert g.shape == r.shape, (what, g.shape, r.shape)
    print('FIG %-60s max abs err %.3e  ref max %.3e  tol %g%s' % (what, float((g - r).abs().max()), float(r.abs().max()), tol,
                                                                   ' (scale)' if scale else ''))
    (assert_close_scale if scale else assert_close)(g, r, tol, what)


def _nhwc(t, dtype):
    from efficientdet.pytorch_amd.ops import Map
    return Map.of(t.permute(0, 2, 3, 1).contiguous().to(DEV, dtype))


def _rand(g, *shape):
    return torch.randn(*shape, generator=g)


# ------------------------------------------------------------------------------------------ (a) per-image weight-gradient slabs
def _wgrad_case(case, arith, spike):
    from efficientdet.pytorch_amd import ops
    from efficientdet.pytorch_amd.ops import Map
    B, H, W, Co, Ce = case
    g = torch.Generator().manual_seed(101)
    q_ = _q(arith)
    x = q_(_rand(g, B, H, W, Ce)); dz = q_(_rand(g, B, H, W, Co))
    if spike:       # the last pixel of the last image, last input / output channel: last slab, last K-step, last partial tile
        x[B - 1, H - 1, W - 1, Ce - 1] = SPIKE; dz[B - 1, H - 1, W - 1, Co - 1] = SPIKE
    xm, zm = Map.of(x.to(DEV, _dtype(arith))), Map.of(dz.to(DEV, _dtype(arith)))
    with _arith(arith):
        G, dbp = ops.conv2d_wgrad(xm, zm, Cin=Ce, Cout=Co, KH=1, KW=1, image_splits=True)
        G2, dbp2 = ops.conv2d_wgrad(xm, zm, Cin=Ce, Cout=Co, KH=1, KW=1, image_splits=True)
        kid = ops.conv2d_wgrad_kernel_id(xm, zm, Cin=Ce, Cout=Co, KH=1, KW=1)
    assert torch.equal(G, G2) and torch.equal(dbp, dbp2)
    assert G.shape[0] % B == 0 and G.shape[1:] == (Co, 1, Ce) and dbp.shape == (G.shape[0], Co)
    q = G.shape[0] // B
    per = G.double().view(B, q, Co, Ce).sum(1)
    ref = torch.einsum('bhwn,bhwc->bnc', dz.double(), x.double())
    bias = dbp.double().view(B, q, Co).sum(1)
    return q, kid, per, ref, bias, dz.double().sum(dim=(1, 2))


@pytest.mark.parametrize('case,arith', [(c, a) for c, (qs, _) in IMAGE_SPLIT_CASES.items() for a in ARITHS if qs.get(a) is not None])
def test_per_image_wgrad_slabs(case, arith):
    """conv2d_wgrad(image_splits=True): sum of each image's q slabs == dz_b^T x_b, bias rows == sum_p dz_b, two launches bitwise equal;
    the slab count and the kernel are the ones tests/se_fused_cases.py pins (q = 1, 2 and >= 4; tiled, thin, register-transpose)."""
    qs, kid_want = IMAGE_SPLIT_CASES[case]
    q, kid, per, ref, bias, bias_ref = _wgrad_case(case, arith, spike=False)
    assert q == qs[arith], (case, arith, q)
    assert kid == (kid_want if arith != 'bf16' else 0), (case, arith, kid)
    _check(per, ref, RAW[arith], 'per-image slabs %s %s' % (case, arith), scale=True)
    _check(bias, bias_ref, RAW[arith], 'per-image bias rows %s %s' % (case, arith), scale=True)


SPIKED_WGRAD = [(2, 16, 32, 80, 480), (1, 32, 32, 24, 144), (5, 8, 8, 192, 1152), (3, 8, 8, 54, 240), (8, 64, 64, 24, 144)]


@pytest.mark.parametrize('case,arith', [(c, a) for c in SPIKED_WGRAD for a in ARITHS if IMAGE_SPLIT_CASES[c][0].get(a) is not None])
def test_per_image_wgrad_slabs_last_pixel_spike(case, arith):
    """The same with 1024 planted in x and dz at the last pixel of the last image (last channel of each): the entry (B-1, Co-1, Ce-1) is
    ~1e6, its row and column ~1e3 x the rest -- a dropped last slab, K-step or channel tile misses by far more than the tolerance."""
    B, H, W, Co, Ce = case
    q, kid, per, ref, bias, bias_ref = _wgrad_case(case, arith, spike=True)
    assert float(ref[B - 1, Co - 1, Ce - 1]) > 0.9 * SPIKE * SPIKE
    # the other images at their own scale (the spike must not leak into them, nor loosen their check)
    if B > 1:
        _check(per[:B - 1], ref[:B - 1], RAW[arith], 'spiked: other images %s %s' % (case, arith), scale=True)
    last, rl = per[B - 1], ref[B - 1]
    _check(last[Co - 1, Ce - 1].view(1), rl[Co - 1, Ce - 1].view(1), RAW[arith], 'spiked: the corner', scale=True)
    _check(last[:Co - 1, Ce - 1], rl[:Co - 1, Ce - 1], RAW[arith], 'spiked: last input channel', scale=True)
    _check(last[Co - 1, :Ce - 1], rl[Co - 1, :Ce - 1], RAW[arith], 'spiked: last output channel', scale=True)
    _check(last[:Co - 1, :Ce - 1], rl[:Co - 1, :Ce - 1], RAW[arith], 'spiked: the rest of the last image', scale=True)
    _check(bias, bias_ref, RAW[arith], 'spiked: bias rows', scale=True)


def test_per_image_wgrad_refusals():
    """Image splits need whole K-steps per image (32 pixels fp32, 64 bf16) and one level: anything else raises, no slabs come back."""
    from efficientdet.pytorch_amd import ops
    from efficientdet.pytorch_amd.ops import Map
    mk = lambda B, H, W, C, dt: Map.of(torch.zeros(B, H, W, C, device=DEV, dtype=dt))
    f32, bf = torch.float32, torch.bfloat16
    for (H, W, dt) in [(5, 8, f32), (3, 8, f32), (4, 8, bf), (12, 8, bf)]:
        for arith in (('f32', 'bf16x3') if dt == f32 else ('bf16',)):
            with _arith(arith), pytest.raises(RuntimeError):
                ops.conv2d_wgrad(mk(2, H, W, 240, dt), mk(2, H, W, 40, dt), Cin=240, Cout=40, KH=1, KW=1, image_splits=True)
    with pytest.raises(RuntimeError):
        ops.conv2d_wgrad([mk(2, 8, 8, 240, f32), mk(2, 4, 8, 240, f32)], [mk(2, 8, 8, 40, f32), mk(2, 4, 8, 40, f32)], Cin=240, Cout=40,
                         KH=1, KW=1, image_splits=True)


# ------------------------------------------------------------------------------------------ (b) slab sum + unpack with factors
#   (Co, Cin, k, nslabs, B): branch.  Cin_pad = Cin rounded up to 4, G = taps * Cin_pad / 4 the 16-byte groups of a row.  unpack_row takes
#   the SLICED branch for G <= 128 with >= 8 slabs (256 / G thread slices share the slabs), the GENERIC one otherwise: slab 0, then 8-way
#   passes over slabs 1.., then a one-by-one tail.  The branch of every job is pinned here and asserted in the test.
UNPACK_BRANCH = {
    (24, 144, 1, 60, 5): 'sliced',     # 7 slices do not divide 60 slabs; every slice takes the 8-way pass, slices 0..3 a tail slab too
    (24, 144, 1, 52, 4): 'sliced',     # slices 0..2 take the 8-way pass, slices 3..6 only the tail loop
    (16, 54, 1, 40, 5): 'sliced',      # Cin 54 in 56: 18 slices of 14 threads, threads 252..255 idle (slice < SL guard)
    (8, 128, 1, 8, 2): 'sliced',       # at its threshold: 8 slabs, 8 slices of one slab each
    (12, 16, 3, 10, 2): 'sliced',      # 3x3
    (40, 240, 1, 8, 4): 'sliced', (40, 240, 1, 9, 3): 'sliced', (40, 240, 1, 17, 1): 'sliced',      # G = 60: 4 slices, tail loop only
    (40, 238, 1, 9, 3): 'sliced',      # Cin 238 in 240
    (40, 240, 1, 1, 1): 'generic', (40, 240, 1, 2, 2): 'generic',      # too few slabs to slice: slab 0 alone / slab 0 + a tail of one
    # rows of G = 132 groups: too long to slice.  8 slabs: slab 0 + a tail of 7, no 8-way pass; 9: one pass (slabs 1..8), no tail; 10: one
    # pass + a tail of one (slab 9); 17: two passes, no tail; 18: two passes + a tail of one
    (16, 528, 1, 8, 4): 'generic', (16, 528, 1, 9, 3): 'generic', (16, 528, 1, 10, 5): 'generic', (16, 528, 1, 17, 17): 'generic',
    (16, 528, 1, 18, 6): 'generic',
    (16, 526, 1, 9, 3): 'generic',     # Cin 526 in 528: the padding skip behind an 8-way pass
    (36, 62, 3, 6, 3): 'generic',      # 3x3, Cin 62 in 64 (G = 144), tail only
    (36, 62, 3, 9, 3): 'generic', (36, 62, 3, 17, 1): 'generic',       # 3x3 through one / two 8-way passes
    (16, 54, 1, 3, 3): 'generic',      # short row, too few slabs for the sliced branch
    (24, 1152, 1, 5, 5): 'generic',    # rows of two workgroups (the plain form; one workgroup with the BN gradients)
    (8, 1152, 1, 10, 2): 'generic',    # the same through an 8-way pass and its tail
}
UNPACK_JOBS = list(UNPACK_BRANCH)


def _unpack_branch(job):
    """The branch unpack_row takes for a job (every form of these jobs runs one workgroup per row where the sliced branch is possible)."""
    Co, Cin, k, ns, B = job
    return 'sliced' if (k * k * ((Cin + 3) // 4 * 4) // 4 <= 128 and ns >= 8) else 'generic'


FACTORS = [(False, False), (True, False), (False, True), (True, True)]
MID_SLAB = 5


def _unpack_inputs(job, spike, seed=31):
    Co, Cin, k, ns, B = job
    g = torch.Generator().manual_seed(seed)
    cp, taps = (Cin + 3) // 4 * 4, k * k
    slabs = _rand(g, ns, Co, taps, cp); part = _rand(g, ns, Co)
    cs = torch.rand(B, cp, generator=g)
    slabs[..., Cin:] = 1e6; cs[:, Cin:] = 1e6           # padding channels: never to be read into dw / dgamma
    if spike:       # what only the last slab / the last real input channel / the last output channel / the last image reaches
        slabs[ns - 1, Co - 1, taps - 1, Cin - 1] = SPIKE; part[ns - 1, Co - 1] = SPIKE
        if ns > MID_SLAB:       # and a slab in the middle of the first 8-way pass (generic) / of the slices' walk (sliced), another channel
            slabs[MID_SLAB, Co - 2, 0, 0] = SPIKE; part[MID_SLAB, Co - 2] = SPIKE
    t = dict(g=slabs, part=part, w=_rand(g, Co, Cin, k, k), scale=0.5 + torch.rand(Co, generator=g), mean=_rand(g, Co),
             inv=0.5 + torch.rand(Co, generator=g), rs=0.5 + torch.rand(B, generator=g), cs=cs, dw0=_rand(g, Co, Cin, k, k))
    return {k_: v.to(DEV) for k_, v in t.items()}, cp, taps


def _unpack_runs(job, spike):
    """Every (form, factors) launch of one job -> [(label, outputs dict, float64 reference dict)]."""
    from efficientdet.pytorch_amd import ops
    Co, Cin, k, ns, B = job
    t, cp, taps = _unpack_inputs(job, spike)
    runs = []
    for use_rs, use_cs in FACTORS:
        rs, cs = (t['rs'] if use_rs else None), (t['cs'] if use_cs else None)
        ref = unpack_ref(t['g'], Cin, taps, scale=t['scale'], w=t['w'], dsum_part=t['part'], mean=t['mean'], invstd=t['inv'],
                         slab_scale=rs, slab_cscale=cs)
        dw, dg, db = ops.unpack_wgrad_bn(t['g'], t['w'], t['scale'], t['part'], t['mean'], t['inv'], cin_pad=cp, slab_scale=rs, slab_cscale=cs)
        runs.append(('bn rs%d cs%d' % (use_rs, use_cs), {'dw': dw, 'dgamma': dg, 'dbeta': db}, ref))
        if use_cs:
            continue                       # (the per-channel factor exists on the BN form only)
        dw = torch.empty_like(t['w']); wsum = torch.empty(Co, device=DEV)
        db = ops.unpack_wgrad(t['g'], dw, scale=t['scale'], w_oihw=t['w'], wsum=wsum, cin_pad=cp, dbias_part=t['part'], slab_scale=rs)
        runs.append(('wsum rs%d' % use_rs, {'dw': dw, 'wsum': wsum, 'dbeta': db}, ref))
        # no scale, no dot product: rows wider than 1024 floats go to more than one workgroup
        dw = torch.empty_like(t['w'])
        db = ops.unpack_wgrad(t['g'], dw, cin_pad=cp, dbias_part=t['part'], slab_scale=rs)
        runs.append(('plain rs%d' % use_rs, {'dw': dw, 'dbeta': db}, unpack_ref(t['g'], Cin, taps, dsum_part=t['part'], slab_scale=rs)))
        dw = t['dw0'].clone()
        ops.unpack_wgrad(t['g'], dw, scale=t['scale'], accumulate=True, cin_pad=cp, slab_scale=rs)
        runs.append(('accumulate rs%d' % use_rs, {'dw': dw}, {'dw': ref['dw'] + t['dw0'].double().cpu().view(Co, Cin, taps)}))
    return runs


@pytest.mark.parametrize('spike', [False, True])
@pytest.mark.parametrize('job', UNPACK_JOBS)
def test_unpack_with_slab_factors(job, spike):
    """unpack_wgrad_bn / unpack_wgrad vs float64: dw, dbeta, wsum, dgamma (frozen BN, from the UNSCALED sum) and the accumulate form,
    with neither / the per-image / the per-(image, channel) / both slab factors, on both reduction branches and their tails, with
    padding channels holding 1e6 in the slabs and the factor rows.  spike: 1024 at (last slab, last Co, last tap, last real Cin) -- the last
    lane of an 8-way pass for 9 / 17 slabs, the tail behind a whole pass for 10 / 18 -- and at (slab 5, Co - 2, first tap, channel 0), a
    lane in the middle of the first pass whose factor is another image's than its neighbours'."""
    Co, Cin, k, ns, B = job
    assert _unpack_branch(job) == UNPACK_BRANCH[job], job
    for label, out, ref in _unpack_runs(job, spike):
        for name, got in out.items():
            r = ref[name]
            got = got.view(Co, Cin, k * k) if name == 'dw' else got
            if spike:
                # the two spiked output channels apart, so that the spikes do not loosen the check of the other channels
                _check(got[:Co - 2], r[:Co - 2], TOL['f32'], 'unpack %s %s %s' % (job, label, name))
                _check(got[Co - 2:Co - 1], r[Co - 2:Co - 1], TOL['f32'], 'unpack %s %s %s (channel of the mid-pass spike)' % (job, label, name))
                _check(got[Co - 1:], r[Co - 1:], TOL['f32'], 'unpack %s %s %s (channel of the last-slab spike)' % (job, label, name))
            else:
                _check(got, r, TOL['f32'], 'unpack %s %s %s' % (job, label, name))


def test_unpack_jobs_cover_both_branches_and_every_loop_exit():
    """The job table cannot go shallow: the generic branch is there with 1, 2, 8, 9, 17 slabs (no pass, whole passes) and with a tail behind
    a whole pass (10, 18), the sliced one with a slice count that does not divide the slabs; both with padded input channels."""
    gen = {ns for (Co, Cin, k, ns, B), br in UNPACK_BRANCH.items() if br == 'generic'}
    assert {1, 2, 8, 9, 10, 17, 18} <= gen, gen
    assert all(_unpack_branch(j) == br for j, br in UNPACK_BRANCH.items())
    for br in ('sliced', 'generic'):
        assert any(Cin % 4 and ns >= 9 for (Co, Cin, k, ns, B), b in UNPACK_BRANCH.items() if b == br), br
    assert any(ns % (256 // (k * k * ((Cin + 3) // 4 * 4) // 4)) for (Co, Cin, k, ns, B), b in UNPACK_BRANCH.items() if b == 'sliced')


def test_unpack_with_slab_factors_batched_is_bitwise_the_single_launches():
    """The same jobs recorded inside ops.unpack_batch() (one effdet_backward_tail launch per 24 jobs) == launched one by one."""
    from efficientdet.pytorch_amd import ops
    single = [_unpack_runs(job, True) for job in UNPACK_JOBS]
    with ops.unpack_batch():
        batched = [_unpack_runs(job, True) for job in UNPACK_JOBS]
    torch.cuda.synchronize()
    n = 0
    for rs, rb in zip(single, batched):
        for (label, a, _), (_, b, _) in zip(rs, rb):
            for name in a:
                assert torch.equal(a[name], b[name]), (label, name)
                n += 1
    assert n > 100


# ------------------------------------------------------------------------------------------ (c) gate gradient from the slabs
def _dgate_ref(slabs, w, s2, rs, B):
    S, Co, _, Ce = slabs.shape
    v = (slabs.double().view(B, S // B, Co, Ce) * (w.double().view(Co, Ce) * s2.double().view(Co, 1)).view(1, 1, Co, Ce)).sum(dim=(1, 2))
    return v * rs.double().view(B, 1) if rs is not None else v


@pytest.mark.parametrize('spike', [False, True])
@pytest.mark.parametrize('q,Co', [(1, 8), (2, 4), (1, 9), (2, 8), (4, 4), (1, 17), (4, 6), (1, 25), (2, 80)])
def test_se_dgate_from_wgrad(q, Co, spike):
    """se_dgate_slabs_kernel vs float64 rs_b sum_i sum_n W[n,c] s2[n] slab[b q + i, n, c]: q * Co = 8, 9, 16, 17, 24, 25 (every exit of
    the two-chain stride-16 loop and of its tail) and a block-sized 160; Ce with whole and partial 32-channel workgroups; with and
    without the row scale; B 1 and 5; bitwise run to run.  spike: 1024 at (last slab, Co - 1, Ce - 1)."""
    from efficientdet.pytorch_amd import ops
    g = torch.Generator().manual_seed(41)
    for Ce in (32, 100, 144, 1152):
        for B in (1, 5):
            slabs = _rand(g, B * q, Co, 1, Ce); w = _rand(g, Co, Ce, 1, 1) / Ce ** 0.5
            s2 = 0.5 + torch.rand(Co, generator=g); rs = 0.5 + torch.rand(B, generator=g)
            if spike:
                slabs[B * q - 1, Co - 1, 0, Ce - 1] = SPIKE
            sd, wd, s2d, rsd = (t.to(DEV) for t in (slabs, w, s2, rs))
            for use_rs in (False, True):
                out = ops.se_dgate_from_wgrad(sd, wd, s2d, rsd if use_rs else None, B)
                assert torch.equal(out, ops.se_dgate_from_wgrad(sd, wd, s2d, rsd if use_rs else None, B))
                ref = _dgate_ref(slabs, w, s2, rs if use_rs else None, B)
                what = 'se_dgate_from_wgrad q%d Co%d Ce%d B%d rs%d' % (q, Co, Ce, B, use_rs)
                if spike:
                    _check(out[B - 1, Ce - 1].view(1), ref[B - 1, Ce - 1].view(1), TOL['f32'], what + ' (spiked element)')
                    keep = torch.ones(B, Ce, dtype=torch.bool); keep[B - 1, Ce - 1] = False
                    _check(out.cpu()[keep], ref[keep], TOL['f32'], what + ' (the rest)')
                else:
                    _check(out, ref, TOL['f32'], what)


# ------------------------------------------------------------------------------------------ (d) the gate MLP's backward
def _gate_inputs(g, B, C, Cse):
    return dict(gate=torch.rand(B, C, generator=g) * 0.9 + 0.05, mid=_rand(g, B, Cse), pool=_rand(g, B, C) * 8,
                w1=_rand(g, Cse, C) / C ** 0.5, b1=_rand(g, Cse) * 0.1, w2=_rand(g, C, Cse) / Cse ** 0.5)


def _gate_bwd(rows, t, inv_hw, times_gate):
    from efficientdet.pytorch_amd import ops
    d = {k: v.to(DEV) for k, v in t.items()}
    r = rows if isinstance(rows, torch.Tensor) and rows.is_cuda else rows.to(DEV)
    return ops.se_gate_bwd(r, d['gate'], d['mid'], d['pool'], d['w1'], d['b1'], d['w2'], inv_hw, times_gate=times_gate)


GATE_OUT = ('dpool', 'dw1', 'db1', 'dw2', 'db2')


@pytest.mark.parametrize('times_gate', [False, True])
@pytest.mark.parametrize('C,Cse', [(144, 6), (1152, 48), (2688, 112)])
def test_se_gate_bwd_from_partial_rows(C, Cse, times_gate):
    """se_gate_bwd on synthetic partial rows [B, slabs, C] vs float64, du = (sum of the rows) * g (1 - g), or * (1 - g) with
    times_gate: slabs 1..64 (the 4-way slab sum with every tail length), B 1, 4, 9 (the parameter gradients' 4-image passes: none,
    whole, with a tail); the same call deferred inside unpack_batch() is bitwise equal."""
    from efficientdet.pytorch_amd import ops
    g = torch.Generator().manual_seed(51)
    inv_hw = 1.0 / 64
    for B in (1, 4, 9):
        t = _gate_inputs(g, B, C, Cse)
        for slabs in (1, 3, 4, 5, 7, 8, 64):
            rows = _rand(g, B, slabs, C)
            out = _gate_bwd(rows, t, inv_hw, times_gate)
            with ops.unpack_batch():
                deferred = _gate_bwd(rows, t, inv_hw, times_gate)
            torch.cuda.synchronize()
            ref = se_gate_bwd_ref(rows, t['gate'], t['mid'], t['pool'], t['w1'], t['w2'], inv_hw, times_gate)
            for name, a, b in zip(GATE_OUT, out, deferred):
                assert torch.equal(a, b), name
                _check(a, ref[name], TOL['f32'], 'se_gate_bwd C%d B%d slabs%d tg%d %s' % (C, B, slabs, times_gate, name))


@pytest.mark.parametrize('times_gate', [False, True])
@pytest.mark.parametrize('B,slabs', [(1, 5), (4, 7), (9, 9), (5, 6), (9, 64), (4, 4)])
def test_se_gate_bwd_last_slab_and_last_image_spike(B, slabs, times_gate):
    """The last slab row of every image carries 1024 x the others (the scalar tail of the slab sum for slabs % 4 != 0, the last
    unrolled term otherwise), and the last image 1024 x that (the tail of the 4-image passes for B % 4 != 0): every output is then
    decided by terms only those loop ends reach."""
    C, Cse = 144, 6
    g = torch.Generator().manual_seed(53)
    t = _gate_inputs(g, B, C, Cse)
    rows = _rand(g, B, slabs, C)
    rows[:, slabs - 1] *= SPIKE
    rows[B - 1] *= SPIKE
    ref = se_gate_bwd_ref(rows, t['gate'], t['mid'], t['pool'], t['w1'], t['w2'], 1.0 / 64, times_gate)
    out = _gate_bwd(rows, t, 1.0 / 64, times_gate)
    for name, a in zip(GATE_OUT, out):
        if name == 'dpool':          # per image: each at its own scale
            for b in range(B):
                _check(a[b], ref[name][b], TOL['f32'], 'spiked se_gate_bwd B%d slabs%d tg%d dpool[%d]' % (B, slabs, times_gate, b))
        else:
            _check(a, ref[name], TOL['f32'], 'spiked se_gate_bwd B%d slabs%d tg%d %s' % (B, slabs, times_gate, name))


@pytest.mark.parametrize('arith', ['f32', 'bf16'])
@pytest.mark.parametrize('H,W,slabs', [(8, 10, 5), (8, 14, 7), (32, 32, 64)])
def test_se_dgate_rows_into_se_gate_bwd(H, W, slabs, arith):
    """se_dgate at 80 / 112 / 1024 pixels hands over 5 / 7 / 64 partial rows; se_gate_bwd on them == the float64 chain."""
    from efficientdet.pytorch_amd import ops
    from efficientdet.pytorch_amd.ops import Map
    B, C, Cse = 2, 144, 6
    g = torch.Generator().manual_seed(55)
    q_ = _q(arith)
    dxs = q_(_rand(g, B, H, W, C)); xd = q_(_rand(g, B, H, W, C))
    t = _gate_inputs(g, B, C, Cse)
    rows = ops.se_dgate(Map.of(dxs.to(DEV, _dtype(arith))), Map.of(xd.to(DEV, _dtype(arith))))
    assert rows.shape == (B, slabs, C)
    tol = TOL['f32'] if arith == 'f32' else 5 * TOL['bf16']
    dgate = (dxs.double() * xd.double()).sum(dim=(1, 2))
    _check(rows.sum(1), dgate, tol, 'se_dgate %dx%d %s' % (H, W, arith))
    ref = se_gate_bwd_ref(dgate.view(B, 1, C), t['gate'], t['mid'], t['pool'], t['w1'], t['w2'], 1.0 / (H * W), False)
    for name, a in zip(GATE_OUT, _gate_bwd(rows, t, 1.0 / (H * W), False)):
        _check(a, ref[name], tol, 'se_dgate -> se_gate_bwd %dx%d %s %s' % (H, W, arith, name))


# ------------------------------------------------------------------------------------------ (e) the data-gradient epilogue
@pytest.mark.parametrize('use_rs', [False, True])
@pytest.mark.parametrize('arith', ARITHS)
@pytest.mark.parametrize('case', DGRAD_CASES)
def test_project_dgrad_se_epilogue_on_the_mfma_kernels(case, arith, use_rs):
    """conv2d(dy, W' packed for the data gradient, rowscale, bc_scale = gate, bc_shift = dpool, res = zd, RES_SWISH_GRAD) on the
    implicit-GEMM kernels vs float64 (rs_b (dy W') gate + dpool) * swish'(zd), at the wide low-resolution shapes of the backbone;
    the kernel that ran is read from ops.PROFILE: never the skinny VALU kernel, and the bf16x3 operand form where K allows it."""
    from efficientdet.pytorch_amd import ops
    from efficientdet.pytorch_amd.ops import Map
    B, H, W, Co, Ce = case
    g = torch.Generator().manual_seed(61)
    q_, dt = _q(arith), _dtype(arith)
    dy = q_(_rand(g, B, H, W, Co)); zd = q_(_rand(g, B, H, W, Ce))
    wp = _rand(g, Co, Ce, 1, 1) / Ce ** 0.5; s2 = 0.5 + torch.rand(Co, generator=g)
    gate = torch.rand(B, Ce, generator=g); dpool = _rand(g, B, Ce) * 0.1
    rs = 0.5 + torch.rand(B, generator=g)
    out = Map.new(B, H, W, Ce, dt, DEV)
    prof = ops.LaunchProfile()
    with _arith(arith):
        ops.PROFILE = prof
        try:
            ops.conv2d(Map.of(dy.to(DEV, dt)), ops.pack_weight(wp.to(DEV), dt, mode=1, scale=s2.to(DEV)), out, Cin=Co, Cout=Ce, KH=1, KW=1,
                       rowscale=rs.to(DEV) if use_rs else None, bc_scale=gate.to(DEV), bc_shift=dpool.to(DEV), res=Map.of(zd.to(DEV, dt)),
                       res_mode=ops.RES_SWISH_GRAD)
        finally:
            ops.PROFILE = None
    name = prof.records[-1][0]
    assert name.startswith('conv_igemm') and name != 'conv_pw_f32_kernel', name
    assert ('bf16x3' in name) == (arith == 'bf16x3' and Co % 32 == 0 and Co >= 256), (name, case, arith)
    v = dy.double().view(B, -1, Co) @ q_(wp.view(Co, Ce) * s2.view(Co, 1)).double()      # W' as the pack stores it (bf16: rounded)
    if use_rs:
        v = v * rs.double().view(B, 1, 1)
    v = (v * gate.double().view(B, 1, Ce) + dpool.double().view(B, 1, Ce)) * swish_grad(zd.double().view(B, -1, Ce))
    _check(out.tensor().view(B, -1, Ce), v, TOL[arith], 'dgrad + SE epilogue %s %s rs%d [%s]' % (case, arith, use_rs, name))


def test_project_dgrad_se_epilogue_covers_the_bf16x3_kernel():
    """DGRAD_CASES holds a shape whose data gradient really runs on the bf16x3 operand form (the others fall back to exact fp32)."""
    assert any(Co % 32 == 0 and Co >= 256 for (_, _, _, Co, _) in DGRAD_CASES)


# ------------------------------------------------------------------------------------------ (f) the whole branch, op by op
_REF = {}


def _branch_ref(case, arith):
    """The float64 reference of one (shape, storage rounding), computed once and shared."""
    key = (case, arith == 'bf16')
    if key not in _REF:
        B, H, W, Co, Ce = case
        inp = make_tail_inputs(B, H, W, Co, Ce, Ce // 24, seed=71, rs=torch.tensor([1.25, 0.0, 1.5]))      # drop_connect rows: a dropped image, two kept at 1 / keep_prob > 1
        qb = _q(arith) if arith == 'bf16' else None        # bf16 storage: the activations and the packed weight operand are rounded
        _REF[key] = (inp, mbconv_tail_ref(**inp, q=qb, qw=qb))
    return _REF[key]


def _branch_state(case, arith):
    from efficientdet.pytorch_amd import ops
    inp, r = _branch_ref(case, arith)
    B, H, W, Co, Ce = case
    dt = _dtype(arith)
    f = lambda t: t.float().to(DEV)
    S = dict(B=B, Co=Co, Ce=Ce, inv_hw=1.0 / (H * W), dt=dt, rs=f(r['rs']), wp=f(inp['W']).view(Co, Ce, 1, 1).contiguous(),
             w1=f(inp['w1']), b1=f(inp['b1']), w2=f(inp['w2']), mean=f(inp['mean']),
             gate=f(r['gate']), mid=f(r['mid']), pool=f(r['pool']),
             xd=_nhwc(r['xd'], dt), xs=_nhwc(r['xs'], dt), zd=_nhwc(r['zd'], dt), dy=_nhwc(r['dy'], dt))
    S['s2'], _, S['i2'] = ops.bn_fold(f(inp['gamma']), f(inp['beta']), f(inp['mean']), f(inp['var']), 1e-3)
    return S, r


def _fused(S, giw):
    """functional.mbconv_bwd, the SE_FUSED branch, launch for launch."""
    from efficientdet.pytorch_amd import functional as Fn, ops
    from efficientdet.pytorch_amd.ops import Map
    B, Co, Ce, dy, rs, wp = S['B'], S['Co'], S['Ce'], S['dy'], S['rs'], S['wp']
    G2, dsum2 = ops.conv2d_wgrad(S['xd'] if giw else S['xs'], dy, Cin=Ce, Cout=Co, KH=1, KW=1, image_splits=True)
    dW, dg, db = ops.unpack_wgrad_bn(G2, wp, S['s2'], dsum2, S['mean'], S['i2'], slab_scale=rs, slab_cscale=S['gate'] if giw else None)
    dgg = ops.se_dgate_from_wgrad(G2, wp, S['s2'], rs, B)
    dpool, dw1, db1, dw2, db2 = ops.se_gate_bwd(dgg, S['gate'], S['mid'], S['pool'], S['w1'], S['b1'], S['w2'], S['inv_hw'], times_gate=not giw)
    dzd = ops.pw_dgrad_se(dy, wp, S['s2'], rs, S['gate'], dpool, S['zd']) if Fn.PW_DGRAD_SE and S['dt'] == torch.float32 else None
    if dzd is None:
        dzd = Map.new(B, dy.H, dy.W, Ce, S['dt'], DEV)
        ops.conv2d(dy, ops.pack_weight(wp, S['dt'], mode=1, scale=S['s2']), dzd, Cin=Co, Cout=Ce, KH=1, KW=1, rowscale=rs,
                   bc_scale=S['gate'], bc_shift=dpool, res=S['zd'], res_mode=ops.RES_SWISH_GRAD)
    return dict(dW=dW, dgamma2=dg, dbeta2=db, dw1=dw1, db1=db1, dw2=dw2, db2=db2, dzd=dzd, dgg=dgg, dpool=dpool, q=G2.shape[0] // B)


def _unfused(S):
    """functional.mbconv_bwd, the else branch (act_bwd, se_dgate, se_bwd_apply), launch for launch."""
    from efficientdet.pytorch_amd import ops
    from efficientdet.pytorch_amd.ops import Map
    B, Co, Ce, dy, rs, wp = S['B'], S['Co'], S['Ce'], S['dy'], S['rs'], S['wp']
    dz2 = ops.act_bwd(dy, None, ops.ACT_NONE, rowscale=rs)
    G2, dsum2 = ops.conv2d_wgrad(S['xs'], dz2, Cin=Ce, Cout=Co, KH=1, KW=1)
    dW, dg, db = ops.unpack_wgrad_bn(G2, wp, S['s2'], dsum2, S['mean'], S['i2'])
    dxs = Map.new(B, dy.H, dy.W, Ce, S['dt'], DEV)
    ops.conv2d(dz2, ops.pack_weight(wp, S['dt'], mode=1, scale=S['s2']), dxs, Cin=Co, Cout=Ce, KH=1, KW=1)
    dgate = ops.se_dgate(dxs, S['xd'])
    dpool, dw1, db1, dw2, db2 = ops.se_gate_bwd(dgate, S['gate'], S['mid'], S['pool'], S['w1'], S['b1'], S['w2'], S['inv_hw'])
    dzd = ops.se_bwd_apply(dxs, S['gate'], dpool, S['zd'])
    return dict(dW=dW, dgamma2=dg, dbeta2=db, dw1=dw1, db1=db1, dw2=dw2, db2=db2, dzd=dzd, dgg=dgate.sum(1), dpool=dpool)


SE_CHAIN = ('dgg', 'dpool', 'dw1', 'db1', 'dw2', 'db2')
NAMES = {'dzd': 'dz_d', 'dW': 'project.weight', 'dgamma2': 'bn2.weight', 'dbeta2': 'bn2.bias', 'dgg': 'gate gradient', 'dpool': 'dpool',
         'dw1': 'se dw1', 'db1': 'se db1', 'dw2': 'se dw2', 'db2': 'se db2'}
_UNF = {}


def _pairs(out, r, case, times_gate):
    """{quantity: (kernel output, float64 reference)} of one run of the branch."""
    B, H, W, Co, Ce = case
    p = {'dzd': (out['dzd'].tensor().permute(0, 3, 1, 2), r['dzd']), 'dW': (out['dW'].view(Co, Ce), r['dW']),
         'dgg': (out['dgg'], r['dgate_gate'] if times_gate else r['dgate'])}
    for k in ('dgamma2', 'dbeta2', 'dpool', 'dw1', 'db1', 'dw2', 'db2'):
        p[k] = (out[k], r[k])
    return p


def _scale_err(got, ref):
    g, r = got.detach().double().cpu(), ref.detach().double().cpu()
    assert g.shape == r.shape and bool(torch.isfinite(g).all())
    return float((g - r).abs().max()) / (float(r.abs().max()) + 1e-300)


def _unfused_out(case, arith):
    """One run of the un-fused chain per (shape, arithmetic), shared by its own test and by the bf16 bounds of the fused one."""
    if (case, arith) not in _UNF:
        S, r = _branch_state(case, arith)
        with _arith(arith):
            out = _unfused(S)
        torch.cuda.synchronize()
        _UNF[case, arith] = _pairs(out, r, case, False)
    return _UNF[case, arith]


def _check_branch(pairs, case, arith, what, cancelling=(), twice=None):
    """Every output on its own, per element at its category's figure (fp32 1e-4, bf16x3 1e-3; bf16 2e-2 for the map dz_d, 5 x that for
    the reductions over pixels).  cancelling (bf16 storage only): quantities that are sums with cancellation over operands carrying one
    more 2^-9 rounding than the reference's -- exact arithmetic on the rounded operands already leaves elements next to assert_close's
    floor outside the per-element bound -- compared at tensor scale: against 2 x the error of the un-fused chain on the same inputs
    (twice = its pairs; both sum the same products in another order), or, for the un-fused chain itself (twice None), against the bf16
    figure 2e-2 ~ 10 x 2^-9 of the tensor's maximum: a sum of N terms perturbed by <= 3 roundings each errs by ~ 2^-9 ... 3 x 2^-9 of its
    largest element, and the gate MLP's backward stacks up to three such sums."""
    t = TOL[arith]
    red = 5 * t if arith == 'bf16' else t
    for k, (got, ref) in pairs.items():
        name = '%s %s' % (what, NAMES[k])
        if k not in cancelling:
            _check(got, ref, t if k == 'dzd' else red, name)
        elif twice is None:
            _check(got, ref, TOL['bf16'], name, scale=True)
        else:
            e, eu = _scale_err(got, ref), _scale_err(*twice[k])
            print('FIG %-60s err / ref max %.3e  un-fused chain %.3e  (bound 2 x)' % (name, e, eu))
            assert e <= 2 * eu, '%s: error %.3e of the tensor maximum > 2 x that of the un-fused chain, %.3e' % (name, e, eu)


@pytest.mark.parametrize('giw', [False, True])
@pytest.mark.parametrize('arith', ARITHS)
@pytest.mark.parametrize('case', list(BRANCH_CASES))
def test_fused_branch_matches_float64(case, arith, giw):
    """The fused branch of functional.mbconv_bwd, launch for launch, vs the float64 MBConv tail: every output on its own, per element.
    giw: the slabs are taken on the un-gated activation and the gate re-enters in the unpack (forward with the gate in per-image weights).
    bf16 storage: the gate gradient and what is linear in it (dpool, the four SE gradients), and with giw dW / dgamma (gate * (dy^T
    round(xd)) against the reference's dy^T round(xd * gate)), are sums with cancellation over operands rounded once more than the
    reference's: held at tensor scale to 2 x the error the un-fused chain makes on the same inputs against the same reference.
    Measured (MI355X), error / tensor maximum, fused | un-fused: 8x8, Ce 672: gate gradient 2.7e-3 | 2.3e-3, dpool 2.2e-3 | 2.1e-3, dw1 1.9e-3 | 1.8e-3, db1 1.9e-3 | 1.5e-3, dw2 2.4e-3 | 2.6e-3,
    db2 2.4e-3 | 2.6e-3; giw: dW 1.8e-3 | 2.4e-3, dgamma 7.7e-4 | 1.3e-3.  32x32, Ce 144: gate gradient 1.6e-3 | 1.6e-3, dpool 7.7e-3 | 4.2e-3,
    dw1 7.1e-3 | 5.8e-3, db1 9.3e-3 | 6.6e-3, dw2 1.9e-3 | 2.2e-3, db2 1.9e-3 | 2.2e-3; giw: dW 1.8e-3 | 2.0e-3, dgamma 1.0e-3 | 1.3e-3."""
    S, r = _branch_state(case, arith)
    with _arith(arith):
        out = _fused(S, giw)
    torch.cuda.synchronize()
    assert out['q'] == BRANCH_CASES[case][arith]
    canc = (SE_CHAIN + (('dW', 'dgamma2') if giw else ())) if arith == 'bf16' else ()
    _check_branch(_pairs(out, r, case, not giw), case, arith, 'fused %s %s giw%d' % (case, arith, giw), canc,
                  _unfused_out(case, arith) if canc else None)


@pytest.mark.parametrize('arith', ARITHS)
@pytest.mark.parametrize('case', list(BRANCH_CASES))
def test_unfused_branch_matches_the_same_float64(case, arith):
    """The older chain on the same inputs meets the same reference: per element in fp32 storage.  bf16 storage: it stores dy * rs and the
    data gradient dxs rounded to bf16 (the fused form scales in the fp32 epilogue and never stores dxs), so dz_d, dW and the gate
    gradient chain carry a 2^-9 error per term of a sum with cancellation whatever the element's own size (exact arithmetic on the
    rounded operands: 1.5 % of dz_d outside the per-element bound, 4.4e-3 ... 5.7e-3 of the maximum) -- those at tensor scale, 2e-2;
    bn2.weight and bn2.bias per element."""
    canc = (('dzd', 'dW') + SE_CHAIN) if arith == 'bf16' else ()
    _check_branch(_unfused_out(case, arith), case, arith, 'un-fused %s %s' % (case, arith), canc)
