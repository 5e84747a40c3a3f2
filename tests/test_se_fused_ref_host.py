"""CPU tier: the float64 MBConv-tail reference (tests/mbconv_tail_ref.py) against the identities the fused squeeze-excite backward
rests on (functional.mbconv_bwd, the SE_FUSED branch), and the shape table of the GPU tests against the host-only planning query.
A wrong reference fails here, before a GPU is involved."""
import pytest
import torch

from tests.mbconv_tail_ref import make_tail_inputs, mbconv_tail_ref, se_gate_bwd_ref, swish_grad, unpack_ref
from tests.se_fused_cases import ARITHS, BRANCH_CASES, IMAGE_SPLIT_CASES

REL = 1e-12


def _same(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err, scale = float((a - b).abs().max()), float(b.abs().max())
    assert scale > 0 and err <= REL * scale, '%s: max abs err %g vs scale %g' % (what, err, scale)


def _case(B, H, W, Co, Ce, Cse, rs, seed=7, q=None):
    inp = make_tail_inputs(B, H, W, Co, Ce, Cse, seed, rs=rs)
    return inp, mbconv_tail_ref(**inp, q=q)


@pytest.mark.parametrize('rs', [None, (1.25, 0.0, 0.5)])
@pytest.mark.parametrize('shape', [(3, 4, 8, 12, 40, 4), (3, 5, 3, 7, 24, 2)])
def test_reference_satisfies_the_identities_of_the_fused_backward(shape, rs):
    B, H, W, Co, Ce, Cse = shape
    inp, r = _case(B, H, W, Co, Ce, Cse, torch.tensor(rs) if rs is not None else None)
    d = torch.float64
    Wd, s2, rsd, gate = inp['W'].to(d), r['bn_scale'], r['rs'], r['gate']
    Wp = Wd * s2.view(Co, 1)                                           # W' = W * bn_scale
    # (d loss / d gate) * gate from the per-image weight gradients on the conv's input, d loss / d gate from those on the un-gated map
    _same(rsd.view(B, 1) * (Wp.view(1, Co, Ce) * r['M']).sum(1), r['dgate_gate'], 'dgate * gate from M_b')
    _same(rsd.view(B, 1) * (Wp.view(1, Co, Ce) * r['Mp']).sum(1), r['dgate'], "dgate from M'_b")
    # the project weight gradient from either set of slabs
    _same(s2.view(Co, 1) * (rsd.view(B, 1, 1) * r['M']).sum(0), r['dW'], 'dW from M_b')
    _same(s2.view(Co, 1) * (rsd.view(B, 1, 1) * gate.view(B, 1, Ce) * r['Mp']).sum(0), r['dW'], "dW from gate * M'_b")
    # the data gradient with the SE backward + Swish' epilogue
    dxs = torch.einsum('bnhw,nc->bchw', r['dy'], Wp) * rsd.view(B, 1, 1, 1)
    _same((dxs * gate.view(B, Ce, 1, 1) + r['dpool'].view(B, Ce, 1, 1)) * swish_grad(r['zd']), r['dzd'], 'dzd')
    # frozen-BN parameter gradients from the UNSCALED weight-gradient sum
    G = (rsd.view(B, 1, 1) * r['M']).sum(0)
    dsum = (rsd.view(B, 1) * r['dsum']).sum(0)
    _same(dsum, r['dbeta2'], 'dbeta2')
    _same(r['invstd'] * ((Wd * G).sum(1) - r['mean'] * dsum), r['dgamma2'], 'dgamma2')
    # the gate MLP's backward written out (tests/mbconv_tail_ref.se_gate_bwd_ref) == autograd, from either form of the incoming rows
    for times_gate, rows in ((False, r['dgate']), (True, r['dgate_gate'])):
        m = se_gate_bwd_ref(rows.view(B, 1, Ce), gate, r['mid'], r['pool'], inp['w1'], inp['w2'], 1.0 / (H * W), times_gate)
        for k in ('dpool', 'dw1', 'db1', 'dw2', 'db2'):
            _same(m[k], r[k], 'se_gate_bwd_ref %s (times_gate %d)' % (k, times_gate))
    # the slab sum + unpack written out (unpack_ref) on the per-image slabs, both forms
    u = unpack_ref(r['M'].view(B, Co, 1, Ce), Ce, 1, scale=s2, w=Wd, dsum_part=r['dsum'], mean=r['mean'], invstd=r['invstd'], slab_scale=rsd)
    _same(u['dw'].view(Co, Ce), r['dW'], 'unpack_ref dw'); _same(u['dgamma'], r['dgamma2'], 'unpack_ref dgamma'); _same(u['dbeta'], r['dbeta2'], 'unpack_ref dbeta')
    u = unpack_ref(r['Mp'].view(B, Co, 1, Ce), Ce, 1, scale=s2, w=Wd, dsum_part=r['dsum'], mean=r['mean'], invstd=r['invstd'], slab_scale=rsd,
                   slab_cscale=gate)
    _same(u['dw'].view(Co, Ce), r['dW'], 'unpack_ref dw (gate factor)'); _same(u['dgamma'], r['dgamma2'], 'unpack_ref dgamma (gate factor)')


def test_reference_with_rounded_activations():
    """The straight-through rounding hook: the stored tensors are bf16 values, and the identities that do not mix xs with xd * gate
    (those change by the rounding of xs) still hold exactly."""
    q = lambda t: t.bfloat16().float()
    B, H, W, Co, Ce, Cse = 2, 4, 8, 12, 40, 4
    rs = torch.tensor([1.5, 0.75])
    inp, r = _case(B, H, W, Co, Ce, Cse, rs, q=q)
    for k in ('zd', 'dy', 'xd', 'xs'):
        assert torch.equal(r[k], q(r[k]).double()), k
    exact = mbconv_tail_ref(**inp)
    assert not torch.equal(exact['xs'], r['xs'])
    d = torch.float64
    Wp = inp['W'].to(d) * r['bn_scale'].view(Co, 1)
    _same(r['rs'].view(B, 1) * (Wp.view(1, Co, Ce) * r['Mp']).sum(1), r['dgate'], "dgate from M'_b")
    _same(r['bn_scale'].view(Co, 1) * (r['rs'].view(B, 1, 1) * r['M']).sum(0), r['dW'], 'dW from M_b')
    dxs = torch.einsum('bnhw,nc->bchw', r['dy'], Wp) * r['rs'].view(B, 1, 1, 1)
    _same((dxs * r['gate'].view(B, Ce, 1, 1) + r['dpool'].view(B, Ce, 1, 1)) * swish_grad(r['zd']), r['dzd'], 'dzd')


def test_image_split_shape_table_matches_the_plan():
    """The shapes of the GPU tests get the split plans the table says (host planning query, no device work), and the table covers what
    the tests are for: q = 1, q = 2 and q >= 4 slabs per image in every arithmetic, both the tiled and the thin kernel, the refusals."""
    import ctypes as C
    from efficientdet.pytorch_amd import _lib as L
    from tests.host_util import wgrad_desc
    lib = L.lib()
    code = {'f32': L.F32, 'bf16x3': L.F32_BF16X3, 'bf16': L.BF16}
    splits = lambda dt, B, H, W, Co, Ce, sizes=None: int(lib.effdet_conv2d_wgrad_splits(C.byref(
        wgrad_desc(dt, B, Ce, Co, sizes or [(H, W)], image_splits=1))))
    seen = {a: set() for a in ARITHS}
    kids = set()
    for (B, H, W, Co, Ce), (qs, kid) in list(IMAGE_SPLIT_CASES.items()) + [(k, (v, 0)) for k, v in BRANCH_CASES.items()]:
        for a, q in qs.items():
            s = splits(code[a], B, H, W, Co, Ce)
            if q is None:
                assert s < 1, (B, H, W, Co, Ce, a, s)
                continue
            assert s == B * q, (B, H, W, Co, Ce, a, s)
            seen[a].add(q)
        assert int(lib.effdet_conv2d_wgrad_kernel(C.byref(wgrad_desc(L.F32, B, Ce, Co, [(H, W)])))) == kid
        kids.add(kid)
    for a in ARITHS:
        assert 1 in seen[a] and 2 in seen[a] and max(seen[a]) >= 4, (a, seen[a])
    assert kids == {0, 1}
    # refusals: pixels per image not whole K-steps (32 fp32 / 64 bf16), two levels
    assert splits(L.F32, 2, 5, 8, 40, 240) < 1 and splits(L.F32_BF16X3, 2, 5, 8, 40, 240) < 1
    assert splits(L.BF16, 2, 4, 8, 40, 240) < 1 and splits(L.BF16, 2, 12, 8, 40, 240) < 1
    assert splits(L.F32, 2, 0, 0, 40, 240, sizes=[(8, 8), (4, 8)]) < 1
