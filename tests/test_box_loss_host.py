"""CPU tier of the IoU-family box losses (include/effdet_box_loss.h): the float64 restatement (tests/box_loss_restated.py) against
hand-derived values and central differences, what the seeded cases (tests/box_loss_cases.py) reach, the conditions on their inputs that
tests/test_gpu_box_loss.py relies on, the ctypes table against the header, and the option's validation."""
import math

import numpy as np
import pytest
import torch

from tests import box_loss_cases as BC
from tests import box_loss_restated as R
from tests import loss_cases as LC


def _row(res, b, a):
    """Index of positive (b, a) in a run's per-anchor vectors."""
    pb, pa, _ = res['pos']
    hit = torch.nonzero((pb == b) & (pa == a)).reshape(-1)
    assert len(hit) == 1, (b, a)
    return int(hit[0])


# --------------------------------------------------------------------------- subgradients and hand-derived values
def test_autograd_subgradients_are_the_ones_the_header_states():
    x = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64, requires_grad=True)
    torch.minimum(x, torch.tensor([2.0, 2.0, 2.0], dtype=torch.float64)).sum().backward()
    assert x.grad.tolist() == [1.0, 0.5, 0.0]                       # a tie splits 0.5 / 0.5
    x.grad = None
    torch.maximum(x, torch.tensor([2.0, 2.0, 2.0], dtype=torch.float64)).sum().backward()
    assert x.grad.tolist() == [0.0, 0.5, 1.0]
    y = torch.tensor([-1.0, 0.0, 1.0], dtype=torch.float64, requires_grad=True)
    torch.clamp(y, min=0).sum().backward()
    assert y.grad.tolist() == [0.0, 1.0, 1.0]                       # the clamp at 0 passes at exactly 0
    z = torch.tensor([1.0, R.DW_MAX, 5.0], dtype=torch.float64, requires_grad=True)
    torch.clamp(z, max=R.DW_MAX).sum().backward()
    assert z.grad.tolist() == [1.0, 1.0, 0.0]                       # the cap passes at equality, 0 beyond


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
@pytest.mark.parametrize('kind', R.KINDS)
def test_tie_cases_by_hand(kind, dtype):
    c = BC.get('ties')
    res = R.run(c, kind, dtype=dtype)
    B = 3
    npos = res['num_pos'].tolist()
    # image 0: prediction == annotation.  I = U = C = 1024, rho = 0, v = 0: every kind's loss is 1 - 1024 / (1024 + 1e-7) (0 in fp32)
    # and every term's gradient cancels under the 0.5 / 0.5 split (iou: giw/2 - (-giw/2) halves meet gAp * ph with opposite sign)
    i = _row(res, 0, BC.TIE_T)
    assert abs(float(res['per_anchor'][i]) - (1.0 - 1024.0 / (1024.0 + R.EPS) if dtype == torch.float64 else 0.0)) < 1e-15
    g = res['grad'][0, BC.TIE_T]
    assert float(g[0]) == 0.0 and float(g[1]) == 0.0                # exactly symmetric in dx / dy
    assert float(g[2:].abs().max()) < 1e-9
    # image 1: the prediction (-25.6, 52, 6.4, 84) ends where the annotation (6.4, 52, 38.5, 84) starts: I = 0, iou = 0
    i = _row(res, 1, BC.TIE_SHIFTED)
    pw, gw = 32.0, 38.5 - BC.TIE_GX1
    U = 1024.0 + gw * 32.0
    cw = 38.5 + (-BC.TIE_GX1 + 32.0)                                # hull: from px1 = gx1 - 32 to gx2
    rho2 = (0.5 * (BC.TIE_GX1 - 32.0 + BC.TIE_GX1) - 0.5 * (BC.TIE_GX1 + 38.5)) ** 2
    hand = {'iou': 1.0, 'giou': 1.0 + (cw * 32.0 - U) / (cw * 32.0 + R.EPS), 'diou': 1.0 + rho2 / (cw * cw + 1024.0 + R.EPS)}
    v = R.C_4_PI2 * (math.atan(gw / 32.0) - math.atan(1.0)) ** 2
    hand['ciou'] = hand['diou'] + v / (1.0 + v + R.EPS) * v
    assert abs(float(res['per_anchor'][i]) - hand[kind]) < (1e-12 if dtype == torch.float64 else 1e-6)
    if kind == 'iou':
        # the clamp passes at iw == 0: d iou / d iw = ih / (U + eps), px2 is the selected operand of min(px2, gx2) (6.4 < 38.5), px1
        # is not the one of max(px1, gx1): dL/dpx2 = -32 / (U + eps) = dL/dpcx, dL/dpw = half of it
        dpx2 = -32.0 / (U + R.EPS)
        s = 1.0 / (B * npos[1])
        g = res['grad'][1, BC.TIE_SHIFTED].double()
        tol = 1e-14 if dtype == torch.float64 else 1e-9
        assert abs(float(g[0]) - s * dpx2 * R.STD_XY * 32.0) < tol and abs(float(g[2]) - s * 0.5 * dpx2 * pw * R.STD_WH) < tol
        assert float(g[1]) == 0.0 and float(g[3]) == 0.0            # py1 == gy1, py2 == gy2 tie: the halves cancel; iw = 0 kills d/dph
    # image 2: dw at the cap passes the gradient, dh beyond it gets none
    g = res['grad'][2, BC.TIE_T]
    assert float(g[2]) != 0.0 and float(g[3]) == 0.0
    assert np.float32(0.2) * np.float32(BC.CAP_R_AT) == np.float32(R.DW_MAX)                   # fp32: exactly the cap
    assert R.STD_WH * float(BC.CAP_R_AT) <= R.DW_MAX < R.STD_WH * float(BC.CAP_R_ABOVE)       # exact products: below / above it
    assert np.float32(0.2) * np.float32(BC.CAP_R_ABOVE) > np.float32(R.DW_MAX)
    assert float(np.float32(math.log(1000.0 / 16.0))) == R.DW_MAX


def test_touching_case_is_exact_in_both_precisions():
    """Image 1 of 'ties': the decode of the shifted anchor involves no rounding in fp32, so iw is exactly 0 in fp32 and float64."""
    c = BC.get('ties')
    for dt in (torch.float32, torch.float64):
        anc, r = c['anc'][0, BC.TIE_SHIFTED][None].to(dt), c['reg'][1, BC.TIE_SHIFTED][None].to(dt)
        pcx, pcy, pw, ph = R.decode(anc, r)
        assert float(pcx + 0.5 * pw) == BC.TIE_GX1 and float(pw) == 32.0 and float(pcx) == BC.TIE_GX1 - 16.0
        d = R.selects(anc, c['ann'][1, 0, :4][None].to(dt), r)
        assert float(d[0, 4]) == 0.0 and float(d[0, 5]) == 32.0
    # image 0: all four corner pairs tie
    d = R.selects(c['anc'][0, BC.TIE_T][None].double(), c['ann'][0, 1, :4][None].double(), c['reg'][0, BC.TIE_T][None].double())
    assert d[0, :4].abs().max() == 0.0


# --------------------------------------------------------------------------- autograd against central differences
@pytest.mark.parametrize('kind', R.KINDS)
def test_gradient_against_central_differences(kind):
    c = BC.get('s128_r05')
    b, a, row = R.positives(c)
    pick = torch.arange(0, len(b), 7)
    anc, gt = c['anc'][0].double()[a[pick]], c['ann'].double()[b[pick], row[pick], :4]
    r0 = c['reg'].double()[b[pick], a[pick]]

    if kind == 'ciou':      # alpha is a constant of the gradient: differentiate diou + alpha0 * v with alpha0 from the base point
        def v_of(r):
            _, _, pw, ph = R.decode(anc, r)
            return R.C_4_PI2 * (torch.atan((gt[:, 2] - gt[:, 0]) / (gt[:, 3] - gt[:, 1])) - torch.atan(pw / ph)) ** 2
        iou0, v0 = 1 - R.anchor_loss('iou', anc, gt, r0), v_of(r0)
        alpha0 = v0 / (1 - iou0 + v0 + R.EPS)
        assert float(alpha0.max()) > 1e-3
        f = lambda r: R.anchor_loss('diou', anc, gt, r) + alpha0 * v_of(r)      # noqa: E731
    else:
        f = lambda r: R.anchor_loss(kind, anc, gt, r)      # noqa: E731
    r = r0.clone().requires_grad_(True)
    R.anchor_loss(kind, anc, gt, r).sum().backward()
    h = 1e-6                                                # the selects are >= 1e-2 px from a kink: no step crosses one
    for q in range(4):
        e = torch.zeros_like(r0); e[:, q] = h
        fd = (f(r0 + e) - f(r0 - e)) / (2 * h)
        assert float((fd - r.grad[:, q]).abs().max()) < 1e-8, (kind, q)
    assert float(r.grad.abs().max()) > 1e-2


# --------------------------------------------------------------------------- orderings between the kinds
def test_orderings_between_the_kinds():
    c = BC.get('s128_r20')
    b, a, row = R.positives(c)
    anc, gt, r = c['anc'][0].double()[a], c['ann'].double()[b, row, :4], c['reg'].double()[b, a]
    L = {k: R.anchor_loss(k, anc, gt, r) for k in R.KINDS}
    assert bool((L['giou'] >= L['iou'] - 1e-12).all()) and bool((L['diou'] >= L['iou']).all()) and bool((L['ciou'] >= L['diou']).all())
    assert float((L['giou'] - L['iou']).max()) > 0.1 and float((L['ciou'] - L['diou']).max()) > 1e-3
    # identical centres: diou == iou.  Annotations centred on their anchors (any size), r0 = r1 = 0
    w = gt[:, 2:] - gt[:, :2]
    ctr = 0.5 * (anc[:, :2] + anc[:, 2:])
    gt_c = torch.cat([ctr - 0.5 * w, ctr + 0.5 * w], 1)
    r_c = r.clone(); r_c[:, :2] = 0.0
    assert float((R.anchor_loss('diou', anc, gt_c, r_c) - R.anchor_loss('iou', anc, gt_c, r_c)).abs().max()) < 1e-12
    # equal aspect: ciou == diou.  r2 == r3 keeps the anchor's aspect; the annotation gets the same one
    r_a = r.clone(); r_a[:, 3] = r_a[:, 2]
    aw, ah = anc[:, 2] - anc[:, 0], anc[:, 3] - anc[:, 1]
    gt_a = gt.clone(); gt_a[:, 3] = gt_a[:, 1] + (gt_a[:, 2] - gt_a[:, 0]) * ah / aw
    assert float((R.anchor_loss('ciou', anc, gt_a, r_a) - R.anchor_loss('diou', anc, gt_a, r_a)).abs().max()) < 1e-12


# --------------------------------------------------------------------------- what the cases reach, and the conditions on the inputs
def test_cases_reach_what_they_are_tagged_with():
    c = BC.get('straddle')
    assert c['reg'].shape == (3, 261, 4) and c['ann'].shape[1] == 65 and 261 % 9 == 0 and 261 > 256
    b, a, row = R.positives(c)
    assert bool(((b == 0) & (a >= 256)).any())                                          # a positive in the 5-anchor tail workgroup
    assert bool(((a == BC.STRADDLE_TAIL_ANCHOR) & (row == 64)).any())                   # ... assigned the row of the second chunk
    assert bool((row < 64).any()) and int((c['ann'][0, :, 4] != -1).sum()) == 20
    assert bool((c['ann'][1, :, 4] == -1).all())                                        # image 1: no valid row
    assert bool((c['ann'][2, :, 4] != -1).any()) and not bool((b == 2).any())           # image 2: valid rows, no positive
    codes = LC.oracle_states(c, torch.float64)
    assert bool((codes[1] == LC.CODE_IGN).all()) and bool((codes[2] == LC.CODE_NEG).all())
    for name, scale in (('s128_r05', 0.5), ('s128_r20', 2.0)):
        c = BC.get(name)
        b, a, row = R.positives(c)
        assert c['reg'].shape == (1, 3069, 4) and len(b) > 400
        d = R.selects(c['anc'][0].double()[a], c['ann'].double()[b, row, :4], c['reg'].double()[b, a])
        zero = float(((d[:, 4] < 0) | (d[:, 5] < 0)).double().mean())                   # share of predictions off their annotation
        assert (zero == 0.0) if scale == 0.5 else (0.0 < zero < 0.1), (name, zero)
    c = BC.get('ties')
    assert float(c['reg'][2, BC.TIE_T, 2]) == float(BC.CAP_R_AT) and c['tie']
    c = BC.get('aspect')
    b, a, row = R.positives(c)
    got = {int(n): float((c['ann'][0, n, 2] - c['ann'][0, n, 0]) / (c['ann'][0, n, 3] - c['ann'][0, n, 1])) for n in set(row.tolist())}
    assert sorted(got.values()) == [0.125, 1.0, 8.0]
    res = R.run(c, 'ciou')
    assert float((res['per_anchor'] - R.run(c, 'diou')['per_anchor']).max()) > 1e-3     # v and alpha matter


@pytest.mark.parametrize('name', sorted(BC.CASES))
def test_inputs_are_away_from_every_branch_a_rounding_could_flip(name):
    c = BC.get(name)
    # the assignment: float32 and float64 agree, with room
    assert BC.assignment_margin(c) >= 1e-4
    assert torch.equal(LC.oracle_states(c, torch.float32), LC.oracle_states(c, torch.float64))
    if not c['tie']:
        assert BC.select_margin(c) >= BC.MARGIN
    assert bool(torch.isfinite(c['reg']).all())
    for kind in R.KINDS:
        assert math.isfinite(R.run(c, kind)['loss'])


# --------------------------------------------------------------------------- binding and options
def test_box_loss_signatures_match_the_companion_header():
    """_lib.BOX_LOSS_SIGNATURES against the prototypes of include/effdet_box_loss.h, parsed as tests/test_abi.py parses effdet_hip.h's;
    the built library exports them and lib() binds them with the table's types; none is in effdet_hip.h's table."""
    import os
    import re
    import shutil
    import subprocess
    import tempfile
    from efficientdet.pytorch_amd import build, _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    h = re.sub(r'/\*.*?\*/', '', open(os.path.join(root, 'include', 'effdet_box_loss.h')).read(), flags=re.S)
    scalar = {'int': 'i', 'long long': 'q', 'float': 'f', 'effdet_stream_t': 'p'}
    protos = {}
    for r, name, params in re.findall(r'^([a-z][a-z ]*?\*?)\s*\b(effdet_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', h, flags=re.M):
        kinds = ['p' if '*' in p else scalar[' '.join(p.split()).rsplit(' ', 1)[0]] for p in params.split(',')]
        assert name not in protos, name
        protos[name] = ({'int': 'i'}[' '.join(r.split())], kinds)
    assert sorted(protos) == sorted(set(re.findall(r'\b(effdet_[a-z0-9_]+)\s*\(', h))) == \
        ['effdet_box_loss_bwd_reg', 'effdet_box_loss_fwd', 'effdet_box_loss_fwd_grad']
    assert sorted(_lib.BOX_LOSS_SIGNATURES) == sorted(protos) and not set(protos) & set(_lib.SIGNATURES)
    build.build(verbose=False)
    L = _lib.require(*protos)
    for name, (r, kinds) in protos.items():
        sig = _lib.BOX_LOSS_SIGNATURES[name]
        assert sig[1] == ':' and sig[0] == r, (name, sig, r)
        assert list(sig[2:].replace('s', 'p')) == kinds, (name, sig, ''.join(kinds))
        f = getattr(L, name)
        assert f.restype is _lib._CTYPE[sig[0]] and list(f.argtypes) == [_lib._CTYPE[c] for c in sig[2:]], name
        # the twin's parameters with (kind, weight) in front of the stream
        twin = _lib.SIGNATURES[name.replace('effdet_box_loss', 'effdet_focal_loss')]
        assert sig == twin[:-1] + 'ifs', (name, sig, twin)
    from efficientdet.pytorch_amd import ops
    assert ops.BOX_LOSS_KINDS == {'smooth_l1': 0, 'iou': 1, 'giou': 2, 'diou': 3, 'ciou': 4}
    if shutil.which('gcc') is not None:       # the companion header compiles as C on top of effdet_hip.h, with the values the binding uses
        with tempfile.TemporaryDirectory() as d:
            src = os.path.join(d, 'h.c')
            open(src, 'w').write('#include "effdet_box_loss.h"\nint main(void){return EFFDET_BOX_LOSS_IOU == 1 && EFFDET_BOX_LOSS_GIOU == 2 && '
                                 'EFFDET_BOX_LOSS_DIOU == 3 && EFFDET_BOX_LOSS_CIOU == 4 && EFFDET_BOX_LOSS_DW_MAX == %sf ? 0 : 1;}\n'
                                 % repr(R.DW_MAX))
            subprocess.run(['gcc', '-Wall', '-Werror', '-I', os.path.join(root, 'include'), src, '-o', os.path.join(d, 'h')], check=True)
            subprocess.run([os.path.join(d, 'h')], check=True)


def test_box_loss_options_validate_their_arguments():
    from efficientdet.pytorch_amd import BoxLossOptions, ops
    from efficientdet.pytorch_amd.efficientdet import FocalLoss
    o = BoxLossOptions('ciou', weight=2)
    assert (o.kind, o.weight) == ('ciou', 2.0) and not o.is_default()
    assert o == BoxLossOptions('ciou', 2.0) and o != BoxLossOptions('ciou') and o != BoxLossOptions('giou', 2.0) and o != None     # noqa: E711
    assert BoxLossOptions().key() == ('smooth_l1', 1.0) and BoxLossOptions().is_default()
    assert repr(o) == "BoxLossOptions(kind='ciou', weight=2.0)" and hash(o) == hash(BoxLossOptions('ciou', 2.0))
    for bad in (dict(kind='siou'), dict(kind='iou', weight=-1.0), dict(kind='iou', weight=float('nan')),
                dict(kind='iou', weight=float('inf')), dict(kind='smooth_l1', weight=2.0)):
        with pytest.raises(ValueError):
            BoxLossOptions(**bad)
    assert ops._box_loss_args(None) is None and ops._box_loss_args(BoxLossOptions()) is None
    assert ops._box_loss_args(BoxLossOptions('iou', 0.0)) == (1, 0.0) and ops._box_loss_args(o) == (4, 2.0)
    with pytest.raises(TypeError):
        ops._box_loss_args('ciou')
    with pytest.raises(TypeError):
        FocalLoss(box_loss='ciou')
    assert FocalLoss().box_loss is None and FocalLoss(box_loss=o).box_loss is o


def test_set_box_loss_takes_options_or_none():
    from efficientdet.pytorch_amd import BoxLossOptions, EfficientDet
    m = EfficientDet(num_classes=4)
    assert m.box_loss is None and m.criterion.box_loss is None
    o = BoxLossOptions('giou', 2.0)
    assert m.set_box_loss(o) is m and m.box_loss is o and m.criterion.box_loss is o
    with pytest.raises(TypeError):
        m.set_box_loss('giou')
    with pytest.raises(TypeError):
        m.set_box_loss(('giou', 2.0))
    assert m.box_loss is o
    assert m.set_box_loss(None).box_loss is None and m.criterion.box_loss is None
