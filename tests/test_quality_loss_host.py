"""CPU tier of the IoU-aware class losses (include/effdet_quality_loss.h): the float64 restatement (tests/quality_loss_restated.py)
pinned on hand-derived values and against torch.autograd, the case table (tests/quality_loss_cases.py) proven to reach what it is
tagged with and to keep its margins, the binding against the header, and the Python options."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import pytest
import torch

from tests import box_loss_restated as BR
from tests import loss_cases as LC
from tests import loss_options_restated as R
from tests import quality_loss_cases as QC
from tests import quality_loss_restated as QR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LN2 = math.log(2.0)
ENTRY_POINTS = ['effdet_loss_quality_bwd_cls', 'effdet_loss_quality_fwd', 'effdet_loss_quality_fwd_grad', 'effdet_loss_quality_workspace_bytes']


def _t(*v):
    return torch.tensor(v, dtype=torch.float64)


# --------------------------------------------------------------------------- the restatement
def test_hand_values_of_the_class_terms():
    qfl, vfl = QR.options(kind='qfl'), QR.options(kind='vfl')
    # QFL, beta 2: t = 0, p = 0.5 -> 0.5^2 * ln 2;  t = 1, p = 0.5 -> the same;  t = 0.75, p = 0.25 -> 0.25 * BCE
    l, d = QR.elements_grad(_t(0.5, 0.5, 0.25), _t(0.0, 1.0, 0.75), qfl)
    bce = -(0.75 * math.log(0.25) + 0.25 * math.log(0.75))
    assert torch.allclose(l, _t(0.25 * LN2, 0.25 * LN2, 0.25 * bce), rtol=1e-14, atol=0)
    # d/dp at t = 0, p = 0.5: 2 p BCE + p^2 / (1 - p) = ln 2 + 0.5;  at t = 1 the mirror image
    assert torch.allclose(d, _t(LN2 + 0.5, -(LN2 + 0.5), -2 * 0.5 * bce + 0.25 * (0.25 / 0.75 - 0.75 / 0.25)), rtol=1e-14, atol=0)
    # p == t exactly: loss 0 and derivative 0, not 0 / 0
    l, d = QR.elements_grad(_t(0.5), _t(0.5), qfl)
    assert float(l) == 0.0 and float(d) == 0.0
    # VFL: t = 0.5, p = 0.5 -> 0.5 ln 2 (derivative 0.5 * 0);  t = 0, alpha 0.75, gamma 2, p = 0.5 -> 0.1875 ln 2
    l, d = QR.elements_grad(_t(0.5, 0.5), _t(0.5, 0.0), vfl)
    assert torch.allclose(l, _t(0.5 * LN2, 0.1875 * LN2), rtol=1e-14, atol=0)
    assert torch.allclose(d, _t(0.0, 0.75 * (2 * 0.5 * LN2 + 0.25 / 0.5)), rtol=1e-14, atol=1e-16)
    # gamma 0: the power is 1;  beta 1: |t - p| BCE
    l, _ = QR.elements_grad(_t(0.5), _t(0.0), QR.options(kind='vfl', alpha=1.0, gamma=0.0))
    assert abs(float(l) - LN2) < 1e-15
    l, _ = QR.elements_grad(_t(0.25), _t(0.75), QR.options(kind='qfl', beta=1.0))
    assert abs(float(l) - 0.5 * bce) < 1e-15
    # the clamp: the value is the clamped one, the derivative passes on the closed range only
    for qo in (qfl, vfl):
        p = _t(1e-5, R.P_LO, R.P_HI, 1 - 1e-5)
        for t in (_t(0.0, 0.0, 0.0, 0.0), _t(0.6, 0.6, 0.6, 0.6)):
            l, d = QR.elements_grad(p, t, qo)
            assert float(l[0]) == float(l[1]) and float(l[2]) == float(l[3])
            assert float(d[0]) == 0.0 and float(d[3]) == 0.0 and float(d[1]) != 0.0 and float(d[2]) != 0.0
    # a NaN target stays in the loss, in either kind
    for qo in (qfl, vfl):
        assert bool(torch.isnan(QR.elements_grad(_t(0.3), _t(float('nan')), qo)[0]))


@pytest.mark.parametrize('qn', sorted(QC.QUALITY))
def test_analytic_derivative_against_autograd(qn):
    """elements_grad's hand-written derivative == torch.autograd of `elements` in float64, on random (p, t) that include t = 0, p
    outside the clamp and on its ends, and p == t."""
    qo = QC.quality(qn)
    g = torch.Generator().manual_seed(5)
    p = torch.rand(4000, generator=g, dtype=torch.float64)
    t = torch.rand(4000, generator=g, dtype=torch.float64)
    t[::3] = 0.0
    p[:8] = _t(1e-5, 1 - 1e-5, R.P_LO, R.P_HI, 1e-5, 1 - 1e-5, R.P_LO, R.P_HI)
    t[:4] = 0.0
    p[8], t[8] = 0.5, 0.5
    pr = p.clone().requires_grad_(True)
    l = QR.elements(pr, t, qo)
    l.sum().backward()
    l2, d = QR.elements_grad(p, t, qo)
    assert torch.equal(l.detach(), l2) and bool(torch.isfinite(d).all())
    assert torch.allclose(pr.grad, d, rtol=1e-12, atol=1e-14), float((pr.grad - d).abs().max())
    assert float(d[8]) == 0.0 or qo['kind'] == 'vfl'


def test_quality_is_the_box_loss_iou_clamped_and_zero_off_the_positives():
    c = QC.get('s128_r05')
    codes = QC.codes('s128_r05', 'huber')
    q = QR.quality(c, codes)
    b, a, row = BR.positives(c, codes)
    one_minus = BR.anchor_loss('iou', c['anc'][0].double()[a], c['ann'].double()[b, row, :4], c['reg'].double()[b, a])
    assert torch.allclose(q[b, a], 1 - one_minus, rtol=0, atol=1e-15) and float(q[codes < 0].abs().max()) == 0.0
    assert 0.0 < float(q[b, a].min()) and float(q.max()) <= 1.0
    # a non-finite regression value at a positive anchor: NaN there and nowhere else
    reg = c['reg'].clone()
    reg[int(b[0]), int(a[0]), 2] = float('inf')
    reg[int(b[1]), int(a[1]), 0] = float('nan')
    bad = QR.quality(c, codes, reg=reg)
    assert torch.nonzero(torch.isnan(bad)).tolist() == sorted([[int(b[0]), int(a[0])], [int(b[1]), int(a[1])]])


# --------------------------------------------------------------------------- the case table
@pytest.mark.parametrize('run', QC.RUNS, ids=lambda r: '%s-%s-%s' % r[:3])
def test_every_run_keeps_its_margins(run):
    """No comparison excludes anything beyond the `exact` anchors: every other IoU is at least MARGIN from a band (float64 alone), both
    precisions see the same q == 0 set, and a non-zero q is at least Q_MIN (the varifocal loss jumps where q leaves 0)."""
    name, on, qn, box = run
    c = QC.get(name)
    assert QC.margin(name, on) >= QC.MARGIN, (run, QC.margin(name, on))
    codes = QC.codes(name, on)
    if not QC.is_atss(c):
        assert torch.equal(R.assign(c, QC.opts(on), torch.float32)[0], codes)
    q64, q32 = QR.quality(c, codes, torch.float64), QR.quality(c, codes, torch.float32)
    pos = codes >= 0
    assert torch.equal(q64 == 0, q32 == 0)
    assert bool(((q64[pos] == 0) | (q64[pos] >= QC.Q_MIN)).all())
    b, a, row = BR.positives(c, codes)
    sel = BR.selects(c['anc'][0].double()[a], c['ann'].double()[b, row, :4], c['reg'].double()[b, a])
    zero = q64[b, a] == 0
    assert bool((sel[zero, 4:6].min(dim=1)[0] <= -QC.Q_ZERO_PX).all())
    ref, f32 = QC.reference(name, on, qn, box)
    assert bool(torch.isfinite(ref['losses']).all()) and bool(torch.isfinite(ref['dlogit']).all()) and bool(torch.isfinite(f32['dlogit']).all())
    assert float(ref['losses'][0]) > 0.0


def test_cases_reach_what_they_are_tagged_with():
    seen = set()
    for name in QC.CASES:
        seen |= set(QC.get(name)['tags'])
    assert seen >= {'q_zero', 'q_one', 'p_equals_t', 'p_clamp', 'dw_cap', 'empty_image', 'no_positive_image', 'atss', 'low_quality',
                    'tail_workgroup', 'chunk_crossing', 'scalar_path', 's128'}
    # edges, anchor by anchor
    c = QC.get('edges')
    codes = QC.codes('edges', 'default')
    assert [int(codes[0, a]) for a in (QC.T, QC.T_CAP, QC.T_OFF, QC.T_LOW)] == [1, 1, 1, 1] and int(codes[1, QC.T]) == 2
    q64, q32 = QR.quality(c, codes, torch.float64), QR.quality(c, codes, torch.float32)
    assert float(q32[0, QC.T]) == 1.0 and 0.0 < 1.0 - float(q64[0, QC.T]) < 1e-9                       # q rounds to 1
    assert float(q32[0, QC.T_OFF]) == 0.0 and float(q64[0, QC.T_OFF]) == 0.0                           # q exactly 0 at a positive
    assert float(q32[1, QC.T]) == 0.5 == float(c['cls'][1, QC.T, 2]) and abs(float(q64[1, QC.T]) - 0.5) < 1e-10      # p == t in fp32
    iou, _ = LC.oracle_iou(c, 1, torch.float64)
    assert float(iou[QC.T, 0]) == 0.5 and (1, QC.T) in c['exact']                                       # ... on the pos_iou band
    assert float(BR.STD_WH * c['reg'][0, QC.T_CAP, 2]) > BR.DW_MAX                                      # beyond the dw cap
    p = c['cls'][0]
    assert float(p[QC.T, 0]) < R.P_LO and float(p[QC.T, 1]) > R.P_HI and float(p[QC.T, 2]) == R.P_LO and float(p[QC.T, 3]) == R.P_HI
    assert float(p[QC.T_CAP, 1]) == R.P_LO and float(p[QC.T_OFF, 1]) == R.P_HI and float(p[QC.T_LOW, 1]) < R.P_LO       # ... on the label
    assert not bool((c['ann'][2, :, 4] != -1).any()) and bool((codes[2] == LC.CODE_IGN).all())          # no valid row
    assert bool((c['ann'][3, :, 4] != -1).any()) and bool((codes[3] == LC.CODE_NEG).all())              # rows, no positive
    # the varifocal loss takes the negative branch on T_OFF's label, the positive one on T's
    ref, _ = QC.reference('edges', 'huber', 'vfl', ('giou', 2.0))
    t = QR.targets(c, ref['codes'], ref['q'], 0)
    assert float(t[QC.T_OFF, 1]) == 0.0 and float(t[QC.T, 1]) > 0.99 and float(t[QC.T].sum()) == float(t[QC.T, 1])
    neg = QR.elements_grad(c['cls'][0, QC.T_OFF].double(), torch.zeros(4, dtype=torch.float64), QC.quality('vfl'))[1]
    assert torch.equal(ref['dlogit'][0, QC.T_OFF] != 0, neg != 0)
    # p == t: loss and gradient finite (and 0 in fp32) under QFL
    _, f32 = QC.reference('edges', 'default', 'qfl', None)
    assert float(f32['dlogit'][1, QC.T, 2]) == 0.0 and bool(torch.isfinite(f32['dlogit'][1, QC.T]).all())
    # the other tables
    r20 = QC.get('s128_r20')
    cd = QC.codes('s128_r20', 'default')
    q = QR.quality(r20, cd)
    assert int(((q == 0) & (cd >= 0)).sum()) >= 1 and r20['cls'].shape[1:] == (3069, 4)
    s = QC.get('straddle_lq')
    assert s['anc'].shape[1] == 261 and s['ann'].shape[1] == 65 and not bool((s['ann'][1, :, 4] != -1).any())
    cd = QC.codes('straddle_lq', 'lq')
    assert bool((cd[0, 256:] >= 0).any()) and int((cd[2] >= 0).sum()) == 1                              # tail workgroup; the promoted anchor
    assert int((QC.codes('straddle', 'default')[2] >= 0).sum()) == 0
    assert QC.get('tail_nc3')['cls'].shape[2] == 3 and (3069 * 3) % 4 != 0
    for name in ('atss_nested', 'atss_straddle'):
        assert QC.is_atss(QC.get(name)) and int((QC.codes(name, 'default') >= 0).sum()) > 0


# --------------------------------------------------------------------------- binding
def _prototypes():
    h = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'effdet_quality_loss.h')).read(), flags=re.S)
    scalar = {'int': 'i', 'long long': 'q', 'float': 'f', 'effdet_stream_t': 'p'}
    protos = {}
    for r, name, params in re.findall(r'^([a-z][a-z ]*?\*?)\s*\b(effdet_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', h, flags=re.M):
        kinds = ['p' if '*' in p else scalar[' '.join(p.split()).rsplit(' ', 1)[0]] for p in params.split(',')]
        assert name not in protos, name
        protos[name] = ({'int': 'i', 'long long': 'q'}[' '.join(r.split())], kinds)
    assert sorted(protos) == sorted(set(re.findall(r'\b(effdet_[a-z0-9_]+)\s*\(', h)))
    return protos


def test_signatures_match_the_companion_header_and_workspace_bytes():
    from efficientdet.pytorch_amd import build, _lib
    protos = _prototypes()
    assert sorted(protos) == ENTRY_POINTS == sorted(_lib.QUALITY_LOSS_SIGNATURES)
    assert not set(protos) & (set(_lib.SIGNATURES) | set(_lib.LOSS_OPTS_SIGNATURES) | set(_lib.ATSS_SIGNATURES))
    build.build(verbose=False)
    L = _lib.require(*protos)
    for name, (r, kinds) in protos.items():
        sig = _lib.QUALITY_LOSS_SIGNATURES[name]
        assert sig[1] == ':' and sig[0] == r, (name, sig, r)
        assert list(sig[2:].replace('s', 'p')) == kinds, (name, sig, ''.join(kinds))
        f = getattr(L, name)
        assert f.restype is _lib._CTYPE[sig[0]] and list(f.argtypes) == [_lib._CTYPE[c] for c in sig[2:]], name
    O, Q = _lib.LOSS_OPTS_SIGNATURES, _lib.QUALITY_LOSS_SIGNATURES
    assert Q['effdet_loss_quality_fwd'] == O['effdet_loss_opts_fwd'][:-1] + 'pps'
    assert Q['effdet_loss_quality_fwd_grad'] == O['effdet_loss_opts_fwd_grad'][:-1] + 'pps'
    assert Q['effdet_loss_quality_bwd_cls'] == O['effdet_loss_opts_bwd_cls'][:-1] + 'ps'
    assert Q['effdet_loss_quality_workspace_bytes'] == _lib.ATSS_SIGNATURES['effdet_loss_atss_workspace_bytes']
    # host-only: q [B][A] is the last buffer, past the longer of the two matchers' layouts, whichever matcher is named
    B, A, nc = 3, 261, 4
    atss = _lib.Atss(9, 2)
    for i, v in enumerate([0, 252, 261]):
        atss.level_start[i] = v
    al = lambda n: (n + 255) // 256 * 256      # noqa: E731
    for N in (1, 65, 200):
        a = int(L.effdet_loss_opts_workspace_bytes(B, A, nc, N))
        b = int(L.effdet_loss_atss_workspace_bytes(B, A, nc, N, ctypes.byref(atss)))
        want = max(a, b) + al(4 * B * A)
        assert int(L.effdet_loss_quality_workspace_bytes(B, A, nc, N, None)) == want
        assert int(L.effdet_loss_quality_workspace_bytes(B, A, nc, N, ctypes.byref(atss))) == want
    atss.level_start[2] = 260
    assert int(L.effdet_loss_quality_workspace_bytes(B, A, nc, 65, ctypes.byref(atss))) == -1
    # an invalid struct is refused before anything else (null device pointers: EINVAL either way)
    d = _lib.LossOpts(0.25, 2.0, 0.0, 1.0 / 9.0, 1.0, 0.5, 0.4, 0, 0, 1.0)
    for q in (None, _lib.QualityLoss(0, 2.0, 0.75, 2.0), _lib.QualityLoss(3, 2.0, 0.75, 2.0), _lib.QualityLoss(1, 0.5, 0.75, 2.0)):
        assert L.effdet_loss_quality_fwd(None, None, None, None, None, None, 0, 1, 261, 4, 1, ctypes.byref(d), None,
                                         None if q is None else ctypes.byref(q), None) == -1


def test_struct_matches_the_header_as_gcc_sees_it(tmp_path):
    from efficientdet.pytorch_amd import _lib
    fields = [n for n, _ in _lib.QualityLoss._fields_]
    assert fields == ['kind', 'beta', 'alpha', 'gamma'] and ctypes.sizeof(_lib.QualityLoss) == 16
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    src = tmp_path / 'sz.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "effdet_quality_loss.h"\nint main(void){printf("%zu\\n", sizeof(effdet_quality_loss_t));'
                   + ''.join('printf("%%zu\\n", offsetof(effdet_quality_loss_t, %s));' % f for f in fields)
                   + 'printf("%d\\n%d\\n", EFFDET_QUALITY_QFL, EFFDET_QUALITY_VFL);return 0;}\n')
    exe = tmp_path / 'sz'
    subprocess.run(['gcc', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == ctypes.sizeof(_lib.QualityLoss) and out[-2:] == [_lib.QUALITY_QFL, _lib.QUALITY_VFL]
    for f, off in zip(fields, out[1:]):
        assert getattr(_lib.QualityLoss, f).offset == off, f


# --------------------------------------------------------------------------- the Python options
def test_quality_options_validate_their_arguments():
    from efficientdet.pytorch_amd import QualityLossOptions, ops
    o = QualityLossOptions()
    assert o.key() == ('qfl', 2.0, 0.75, 2.0) and o == QualityLossOptions('qfl', 2.0) and o != QualityLossOptions('vfl') and o != None      # noqa: E711
    assert hash(o) == hash(QualityLossOptions(kind='qfl')) and repr(QualityLossOptions('vfl', alpha=0.5)) == \
        "QualityLossOptions(kind='vfl', beta=2.0, alpha=0.5, gamma=2.0)"
    assert QualityLossOptions(beta=0.1 + 1.0).beta == ctypes.c_float(1.1).value                       # kept as the fp32 the kernels receive
    nan = float('nan')
    for kw in (dict(kind='gfl'), dict(beta=0.5), dict(beta=8.5), dict(beta=nan), dict(alpha=0.0), dict(alpha=1.5), dict(alpha=nan),
               dict(gamma=-0.5), dict(gamma=9.0), dict(gamma=nan)):
        with pytest.raises(ValueError):
            QualityLossOptions(**kw)
    assert QualityLossOptions(beta=1.0, alpha=1.0, gamma=0.0).key() == ('qfl', 1.0, 1.0, 0.0)
    s = ops._quality_struct(QualityLossOptions('vfl', 3.0, 0.5, 1.5))
    assert (s.kind, s.beta, s.alpha, s.gamma) == (2, 3.0, 0.5, 1.5)


def test_focal_parameters_with_a_quality_loss_raise_where_the_second_is_set():
    from efficientdet.pytorch_amd import ATSSOptions, BoxLossOptions, EfficientDet, LossOptions, QualityLossOptions, ops
    from efficientdet.pytorch_amd.efficientdet import FocalLoss
    q = QualityLossOptions('vfl')
    fine = LossOptions(beta=0.1, reg_weight=50.0, pos_iou=0.6, neg_iou=0.3, low_quality=True)
    for bad in (LossOptions(alpha=0.5), LossOptions(gamma=1.5), LossOptions(label_smoothing=0.1)):
        with pytest.raises(ValueError):
            FocalLoss(loss=bad, quality=q)
        with pytest.raises(ValueError):
            ops.check_quality(q, bad)
        m = EfficientDet(4)
        m.set_quality_loss(q)
        with pytest.raises(ValueError):
            m.set_loss(bad)
        assert m.loss_options is None
        m = EfficientDet(4)
        m.set_loss(bad)
        with pytest.raises(ValueError):
            m.set_quality_loss(q)
        assert m.quality_loss is None and m.criterion.quality is None
    with pytest.raises(TypeError):
        FocalLoss(quality='qfl')
    with pytest.raises(TypeError):
        EfficientDet(4).set_quality_loss(LossOptions())
    m = EfficientDet(4)
    assert m.set_quality_loss(q) is m and m.quality_loss is q and m.criterion.quality is q
    m.set_loss(fine).set_box_loss(BoxLossOptions('giou')).set_loss(LossOptions(beta=0.1)).set_matcher(ATSSOptions())
    assert m.set_quality_loss(None).quality_loss is None and m.criterion.quality is None
    assert FocalLoss(loss=fine, quality=q).quality is q


def test_without_a_quality_loss_the_entry_points_are_todays():
    """The recorded call names: None is the same calls as ever for every combination of the other options; with a quality loss the
    forward and the class backward are its own calls and d(reg) the options set's."""
    from efficientdet.pytorch_amd import build, ops
    build.build(verbose=False)
    q = ops.QualityLossOptions()
    box, loss, atss = ops.BoxLossOptions('giou'), ops.LossOptions(beta=0.1), ops.ATSSOptions()
    name = lambda *a, **k: ops._loss_entry(*a, **k)[1]      # noqa: E731
    t = ops._atss_struct(atss, [252, 9], 261)
    for stem in ('fwd', 'fwd_grad', 'bwd_reg'):
        assert name(stem) == name(stem, quality=None) == 'effdet_focal_loss_' + stem
        assert name(stem, None, box, quality=None) == 'effdet_box_loss_' + stem
        assert name(stem, loss, box, quality=None) == 'effdet_loss_opts_' + stem
    assert name('fwd', None, None, atss, t, quality=None) == 'effdet_loss_atss_fwd' and name('bwd_cls', loss) == 'effdet_loss_opts_bwd_cls'
    for kw in (dict(), dict(loss=loss), dict(box=box), dict(loss=loss, box=box, matcher=atss, atss=t)):
        for stem in ('fwd', 'fwd_grad'):
            fn, nm, extra, o, _ = ops._loss_entry(stem, quality=q, **kw)
            assert nm == 'effdet_loss_quality_' + stem and len(extra) == 3 and o and (extra[1] is None) == ('atss' not in kw)
    kw = dict(loss=loss, matcher=atss)
    assert name('bwd_cls', quality=q) == name('bwd_cls', quality=q, **kw) == 'effdet_loss_quality_bwd_cls'
    assert len(ops._loss_entry('bwd_cls', quality=q)[2]) == 2
    assert name('bwd_reg', quality=q) == name('bwd_reg', box=box, quality=q) == name('bwd_reg', quality=q, **kw) == 'effdet_loss_opts_bwd_reg'


def test_quality_targets_view_checks_its_workspace():
    from efficientdet.pytorch_amd import ops
    B, A = 2, 261
    nq = (4 * B * A + 255) // 256 * 256
    ws = torch.arange(4096 + nq, dtype=torch.int64).to(torch.uint8)
    q = ops.loss_quality_targets(ws, B, A, 65)
    assert q.shape == (B, A) and q.dtype == torch.float32 and q.data_ptr() == ws.data_ptr() + 4096
    with pytest.raises(ValueError):
        ops.loss_quality_targets(ws[:nq], B, A, 65)
    with pytest.raises(TypeError):
        ops.loss_quality_targets(ws, B, A, 65, matcher='atss')
