"""CPU tier of the loss options (include/effdet_loss_opts.h): the restatement (tests/loss_options_restated.py) against the oracle at
the defaults, against hand-derived values and central differences; what the cases (tests/loss_options_cases.py) reach and the margin
that tests/test_gpu_loss_options.py relies on; the ctypes table and struct against the header; the options' validation."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from oracle import effdet_oracle as O
from tests import box_loss_cases as BC
from tests import loss_cases as LC
from tests import loss_options_cases as OC
from tests import loss_options_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ['effdet_loss_opts_bwd_cls', 'effdet_loss_opts_bwd_reg', 'effdet_loss_opts_fwd', 'effdet_loss_opts_fwd_grad',
                'effdet_loss_opts_workspace_bytes']


# --------------------------------------------------------------------------- the defaults are the oracle
@pytest.mark.parametrize('name', ['chunks', 'thresholds', 'thresholds_nested', 'tiny_box', 'chunk_ties_N65', 'tails_nc3', 'many_images',
                                  'bc_straddle', 'bc_s128_r05'])
def test_defaults_are_the_oracle(name):
    c = BC.get(name[3:]) if name.startswith('bc_') else LC.CASES[name]()
    o = R.options()
    codes, promoted = R.assign(c, o, torch.float64)
    assert torch.equal(codes, LC.oracle_states(c, torch.float64)) and not bool(promoted.any())
    cl, rl = O.focal_loss(c['cls'].double(), c['reg'].double(), c['anc'].double(), c['ann'].double())
    res = R.run(c, o, codes=codes)
    assert abs(float(res['losses'][0]) - float(cl)) <= 1e-12 * max(1.0, abs(float(cl)))
    # the knee: the oracle's is 1 / 9 in float64, the header's that rounded to fp32 (7.5e-9 larger) -- equal with the oracle's knee,
    # and within that rounding with the header's
    exact = R.run(c, R.options(beta=1.0 / 9.0), codes=codes, fp32_knee=False)
    assert abs(float(exact['losses'][1]) - float(rl)) <= 1e-12 * max(1.0, abs(float(rl)))
    assert abs(float(res['losses'][1]) - float(rl)) <= 2e-8 * max(1.0, abs(float(rl)))
    assert R.DEFAULTS['beta'] == float(np.float32(1.0) / np.float32(9.0)) == float(np.float32(1.0 / 9.0))


# --------------------------------------------------------------------------- hand-derived values
@pytest.mark.parametrize('gamma', [0.0, 1.5, 2.0])
@pytest.mark.parametrize('eps', [0.0, 0.1])
def test_class_term_by_hand(eps, gamma):
    alpha = 0.25
    o = R.options(alpha=alpha, gamma=gamma, label_smoothing=eps)
    p = torch.tensor([[0.3, 0.8], [0.6, 0.05], [0.5, 0.5]], dtype=torch.float64)
    h = torch.tensor([[1.0, 0.0], [0.0, 0.0], [1.0, 0.0]], dtype=torch.float64)
    got = R.focal_elements(p, h, torch.tensor([False, False, True]), o)
    e = float(np.float32(eps))

    def hand(pv, one):
        t = (1.0 - e) + e / 2 if one else e / 2
        u = 1.0 - pv if one else pv
        w = (alpha if one else 1.0 - alpha) * (u ** gamma)
        return -w * (t * math.log(pv) + (1.0 - t) * math.log(1.0 - pv))
    want = [[hand(0.3, True), hand(0.8, False)], [hand(0.6, False), hand(0.05, False)], [0.0, 0.0]]      # (the ignored anchor: nothing)
    assert float((got - torch.tensor(want, dtype=torch.float64)).abs().max()) < 1e-14
    if gamma == 0.0:
        assert abs(float(got[0, 0]) + alpha * ((1 - e / 2) * math.log(0.3) + e / 2 * math.log(0.7))) < 1e-15      # no modulation at all
    if eps == 0.0 and gamma == 2.0:      # the reference's value
        assert abs(float(got[0, 0]) + 0.25 * 0.49 * math.log(0.3)) < 1e-15 and abs(float(got[0, 1]) + 0.75 * 0.64 * math.log(0.2)) < 1e-15
    # the clamp: outside [1e-4f, 1 - 1e-4f] the value is the bound's and the gradient 0, ON the bound the gradient passes
    q = torch.tensor([[1e-6, R.P_LO, R.P_HI, 1.0 - 1e-7]], dtype=torch.float64, requires_grad=True)
    R.focal_elements(q, torch.zeros(1, 4, dtype=torch.float64), torch.tensor([False]), o).sum().backward()
    assert q.grad[0, 0] == 0 and q.grad[0, 3] == 0 and (gamma == 0.0 and eps == 0.0 or q.grad[0, 1] != 0) and q.grad[0, 2] != 0


def test_smooth_l1_with_the_huber_knee_by_hand():
    beta = float(np.float32(0.1))
    anc = torch.tensor([[10.0, 20.0, 30.0, 60.0]], dtype=torch.float64).repeat(2, 1)
    gt = anc.clone()                                                  # annotation == anchor: every target is 0
    r = torch.tensor([[0.05, -0.1, 0.2, -0.3], [beta, -beta, np.nextafter(beta, 1.0), 0.0]], dtype=torch.float64)
    got = R.smooth_l1_elements(anc, gt, r, beta)
    want = [[0.5 * 0.05 ** 2 / beta, 0.5 * 0.1 ** 2 / beta, 0.2 - 0.5 * beta, 0.3 - 0.5 * beta],
            [0.5 * beta, 0.5 * beta, float(np.nextafter(beta, 1.0)) - 0.5 * beta, 0.0]]      # d == beta is on the quadratic side (<=)
    assert float((got - torch.tensor(want, dtype=torch.float64)).abs().max()) < 1e-16
    assert 0.1 <= beta                                                # 0.1 (float64) lies below the fp32 knee: quadratic, as computed above
    # a real target: anchor 20 x 40 at (20, 40), box 30 x 20 at (25, 45): dx = 5 / 20 / 0.1f, dy = 5 / 40 / 0.1f, dw = log(30 / 20) / 0.2f
    gt2 = torch.tensor([[10.0, 35.0, 40.0, 55.0]], dtype=torch.float64)
    t = [5.0 / 20.0 / BC.R.STD_XY, 5.0 / 40.0 / BC.R.STD_XY, math.log(1.5) / BC.R.STD_WH, math.log(0.5) / BC.R.STD_WH]
    got = R.smooth_l1_elements(anc[:1], gt2, torch.tensor([t], dtype=torch.float64) + torch.tensor([[0.01, -0.02, 1.0, -2.0]], dtype=torch.float64), beta)
    want = [0.5 * 1e-4 / beta, 0.5 * 4e-4 / beta, 1.0 - 0.5 * beta, 2.0 - 0.5 * beta]
    assert float((got - torch.tensor([want], dtype=torch.float64)).abs().max()) < 1e-12


def test_reg_weight_and_normalisation_by_hand():
    """losses[1] = reg_weight * mean_b sum / (4 num_pos); losses[0] = mean_b sum / max(num_pos, 1), images without a valid row count in B."""
    c = OC.get('straddle_lq')
    o = OC.opts('paper')
    res = R.run(c, o)
    one = R.run(c, R.options(**dict(OC.OPTS['paper'], reg_weight=1.0)))
    assert abs(float(res['losses'][1]) - 50.0 * float(one['losses'][1])) < 1e-12 * float(res['losses'][1])
    assert float(res['losses'][0]) == float(one['losses'][0]) and res['num_pos'].tolist() == [175, 0, 1]
    # by hand from the per-image pieces: B = 3, image 1 has no valid row
    codes = res['codes']
    tot_c, tot_r = 0.0, 0.0
    for b in (0, 2):
        pos = codes[b] >= 0
        rows = codes[b][pos]
        h = torch.zeros(c['cls'].shape[1], OC.NC, dtype=torch.float64)
        h[pos, c['ann'][b, rows, 4].long()] = 1
        tot_c += float(R.focal_elements(c['cls'][b].double(), h, codes[b] == LC.CODE_IGN, o).sum()) / int(pos.sum())
        tot_r += float(R.smooth_l1_elements(c['anc'][0].double()[pos], c['ann'][b].double()[rows, :4], c['reg'][b].double()[pos],
                                            float(np.float32(0.1))).sum()) / (4 * int(pos.sum()))
    assert abs(float(res['losses'][0]) - tot_c / 3) < 1e-13 and abs(float(res['losses'][1]) - 50.0 * tot_r / 3) < 1e-11


# --------------------------------------------------------------------------- the matcher by hand
@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_low_quality_promotions_by_hand(dtype):
    # a box under 0.5 everywhere, the model's table with one small anchor
    c = OC.get('tiny_lq')
    codes, promoted = R.assign(c, R.options(), dtype)
    assert int((codes >= 0).sum()) == 0 and not bool(promoted.any())                     # no positive: the boxes are never trained
    assert int((codes == LC.CODE_NEG).sum()) == codes.numel()
    codes, promoted = R.assign(c, OC.opts('lq'), dtype)
    assert torch.nonzero(codes >= 0).tolist() == [[0, OC.TINY_SMALL]] and torch.nonzero(promoted).tolist() == [[0, OC.TINY_SMALL]]
    assert int(codes[0, OC.TINY_SMALL]) == 0                                             # its own arg-max row (0.16), not row 2 (0.111)
    iou, rows = LC.oracle_iou(c, 0, torch.float64)
    assert rows.tolist() == [0, 2] and abs(float(iou[OC.TINY_SMALL, 0]) - 0.36 / 2.25) < 1e-6 and abs(float(iou[OC.TINY_SMALL, 1]) - 0.25 / 2.25) < 1e-6
    assert float(iou.max()) < 0.4
    # the existing tiny_box case: low_quality promotes only what is positive anyway (100 and 3000 hold the rows' maxima)
    c = OC.get('tiny_box')
    base, _ = R.assign(c, R.options(), dtype)
    codes, promoted = R.assign(c, OC.opts('lq'), dtype)
    assert torch.equal(base, codes) and torch.nonzero(promoted).tolist() == [[0, 100], [0, 3000]]
    # straddle: image 2's 4 x 4 box, promoted from the tail workgroup; image 0 gains nothing; image 1 has no row
    c = OC.get('straddle_lq')
    base, _ = R.assign(c, R.options(), dtype)
    codes, promoted = R.assign(c, OC.opts('lq'), dtype)
    assert not bool((base[2] >= 0).any()) and torch.nonzero(codes[2] >= 0).tolist() == [[OC.STRADDLE_SMALL]] and int(codes[2, OC.STRADDLE_SMALL]) == 5
    assert torch.equal(base[0], codes[0]) and int(promoted[0].sum()) == 20 and bool((codes[1] == LC.CODE_IGN).all())
    assert OC.STRADDLE_SMALL >= 256 and c['ann'].shape[1] == 65 and c['anc'].shape[1] == 261
    assert abs(float(LC.oracle_iou(c, 2, torch.float64)[0][OC.STRADDLE_SMALL, 0]) - 16.0 / 49.0) < 1e-6


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_exact_ties_and_zero_overlap_by_hand(dtype):
    c = OC.get('lq_ties')
    o = OC.opts('high_bands_lq')
    iou, rows = LC.oracle_iou(c, 0, dtype)
    assert rows.tolist() == [1]
    a, b = iou[OC.TIE_A, 0], iou[OC.TIE_B, 0]
    assert float(a) == float(b) == float(torch.tensor(896.0, dtype=dtype) / torch.tensor(1152.0, dtype=dtype))     # the same operands
    rest = iou[:, 0].clone(); rest[OC.TIE_A] = 0; rest[OC.TIE_B] = 0
    assert float(rest.max()) < 0.64
    codes, promoted = R.assign(c, o, dtype)
    assert torch.nonzero(codes >= 0).tolist() == [[0, OC.TIE_A], [0, OC.TIE_B]] and int(codes[0, OC.TIE_A]) == 1 == int(codes[0, OC.TIE_B])
    assert bool((codes[1] == LC.CODE_NEG).all()) and not bool(promoted[1].any())        # zero overlap: gtmax 0 promotes nothing
    assert float(LC.oracle_iou(c, 1, dtype)[0].max()) == 0.0
    without, _ = R.assign(c, R.options(pos_iou=0.875, neg_iou=0.8125), dtype)
    assert int((without >= 0).sum()) == 0 and int((without == LC.CODE_NEG).sum()) == without.numel()
    # every product of the tie is an exact integer in fp32: 32 * 32, 28 * 32, 1024 + 1024 - 896
    for v in (1024.0, 896.0, 1152.0):
        assert float(np.float32(v)) == v


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_other_bands_on_the_exact_integer_construction(dtype):
    c = OC.get('bands')
    codes, _ = R.assign(c, OC.opts('bands'), dtype)
    for b, a, state, row in c['expect']:
        assert int(codes[b, a]) == LC.state_code(state, row), (b, a, state)
    assert int(codes[1, OC.TIE_B]) == 1                                                  # 864 / 1152 with the next integer anchor
    t = LC.int_anchor(8, 8)
    for b, (num, den) in ((0, (864.0, 1152.0)), (3, (320.0, 1280.0))):
        assert float(LC.oracle_iou(c, b, dtype)[0][t, 0]) == num / den
    # and at the default bands the same inputs are assigned differently
    default, _ = R.assign(c, R.options(), dtype)
    assert int(default[2, t]) == 1 and int(codes[2, t]) == LC.CODE_IGN and int(default[3, t]) == LC.CODE_NEG


# --------------------------------------------------------------------------- autograd against central differences
@pytest.mark.parametrize('run', [('straddle_lq', 'paper', None), ('straddle', 'gamma0', None), ('tiny_lq', 'lq', None),
                                 ('straddle_lq', 'lq', ('giou', 2.0))])
def test_gradients_against_central_differences(run):
    name, on, box = run
    c, o = OC.get(name), OC.opts(on)
    gs = (0.7, 1.3)
    res = R.run(c, o, box=box, gscale=gs)
    codes = res['codes']
    cls0, reg0 = c['cls'].double(), c['reg'].double()
    logit0 = torch.log(cls0) - torch.log1p(-cls0)

    def value(logit, reg):
        r = R.run(c, o, box=box, gscale=gs, codes=codes, inputs=(torch.sigmoid(logit), reg))
        return gs[0] * float(r['losses'][0]) + gs[1] * float(r['losses'][1])
    pb, pa = torch.nonzero(codes >= 0, as_tuple=True)
    nb, na = torch.nonzero(codes == LC.CODE_NEG, as_tuple=True)
    h = 1e-5                                                          # (the sums are O(100): a smaller step drowns in their rounding)
    picks = list(range(0, len(pb), max(1, len(pb) // 4)))[:4]
    worst = 0.0
    for i in picks:                                                   # d(reg) on positives, all four deltas
        for q in range(4):
            e = torch.zeros_like(reg0); e[pb[i], pa[i], q] = h
            fd = (value(logit0, reg0 + e) - value(logit0, reg0 - e)) / (2 * h)
            g = float(res['dreg'][pb[i], pa[i], q])
            assert abs(fd - g) < 1e-7 * max(1.0, abs(g)), (name, on, 'dreg', i, q, fd, g)
            worst = max(worst, abs(g))
    assert worst > 0.0
    elems = [(int(pb[i]), int(pa[i]), k) for i in picks for k in range(c['cls'].shape[2])] + \
            [(int(nb[i]), int(na[i]), 0) for i in range(0, len(nb), max(1, len(nb) // 3))][:3]
    worst = 0.0
    for (b, a, k) in elems:                                           # d(logit): a positive's label and other classes, negatives
        e = torch.zeros_like(logit0); e[b, a, k] = h
        fd = (value(logit0 + e, reg0) - value(logit0 - e, reg0)) / (2 * h)
        g = float(res['dlogit'][b, a, k])
        assert abs(fd - g) < 1e-7 * max(1.0, abs(g)), (name, on, 'dlogit', b, a, k, fd, g)
        worst = max(worst, abs(g))
    assert worst > 0.0
    # nothing reaches an ignored anchor or a non-positive's regression row
    ign = codes == LC.CODE_IGN
    assert float(res['dlogit'][ign].abs().max() if bool(ign.any()) else 0.0) == 0.0 and float(res['dreg'][codes < 0].abs().max()) == 0.0


# --------------------------------------------------------------------------- the margin the device tests rely on
@pytest.mark.parametrize('run', OC.RUNS + [(n, 'lq') for n in ('straddle_lq', 'tiny_lq', 'tiny_box')], ids=lambda r: '%s-%s' % r)
def test_every_run_keeps_its_margin(run):
    name, on = run
    c, o = OC.get(name), OC.opts(on)
    assert OC.MARGIN == 1e-6                                          # tests/loss_cases.skip_mask's default
    assert OC.margin(c, o) >= OC.MARGIN, (name, on, OC.margin(c, o))
    c64, p64 = R.assign(c, o, torch.float64)
    c32, p32 = R.assign(c, o, torch.float32)
    assert torch.equal(c64, c32) and torch.equal(p64, p32)
    for (b, a) in c['exact']:                                         # the exact anchors: integer coordinates, so integer products
        assert bool((c['anc'][0, a] == c['anc'][0, a].round()).all())
        assert bool((c['ann'][b][c['ann'][b, :, 4] != -1][:, :4] == c['ann'][b][c['ann'][b, :, 4] != -1][:, :4].round()).all())
    assert bool(torch.isfinite(R.run(c, o)['losses']).all())
    assert float(c['cls'].min()) > 2e-3 and float(c['cls'].max()) < 1 - 2e-3        # inside the clamp: every live gradient is non-zero


def test_cases_reach_what_they_are_for():
    c = OC.get('nc80')
    assert c['cls'].shape == (2, 3069, 80) and LC.dld_for(80) == 768
    c = OC.get('tail_nc%d' % OC.TAIL_NC)
    assert OC.TAIL_NC in LC.TAIL_NC and (c['cls'].shape[1] * c['cls'].shape[2]) % 4 != 0
    for name, on in OC.RUNS:
        assert name in OC.CASES and on in OC.OPTS
    used = {on for _, on in OC.RUNS}
    assert {'paper', 'lq', 'smooth', 'gamma0', 'bands', 'high_bands_lq'} <= used
    assert OC.OPTS['paper'] == dict(alpha=0.25, gamma=1.5, beta=0.1, reg_weight=50.0, low_quality=True)
    # the paper's options change both terms on a case with positives on both sides of the knee
    c = OC.get('straddle_lq')
    a, b = R.run(c, R.options())['losses'], R.run(c, OC.opts('paper'))['losses']
    assert float(a[0]) != float(b[0]) and float(b[1]) > 10.0 * float(a[1])


# --------------------------------------------------------------------------- binding and options
def _prototypes():
    h = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'effdet_loss_opts.h')).read(), flags=re.S)
    scalar = {'int': 'i', 'long long': 'q', 'float': 'f', 'effdet_stream_t': 'p'}
    protos = {}
    for r, name, params in re.findall(r'^([a-z][a-z ]*?\*?)\s*\b(effdet_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', h, flags=re.M):
        kinds = ['p' if '*' in p else scalar[' '.join(p.split()).rsplit(' ', 1)[0]] for p in params.split(',')]
        assert name not in protos, name
        protos[name] = ({'int': 'i', 'long long': 'q'}[' '.join(r.split())], kinds)
    assert sorted(protos) == sorted(set(re.findall(r'\b(effdet_[a-z0-9_]+)\s*\(', h)))
    return protos


def test_loss_opts_signatures_match_the_companion_header():
    from efficientdet.pytorch_amd import build, _lib
    protos = _prototypes()
    assert sorted(protos) == ENTRY_POINTS == sorted(_lib.LOSS_OPTS_SIGNATURES)
    assert not set(protos) & (set(_lib.SIGNATURES) | set(_lib.BOX_LOSS_SIGNATURES) | set(_lib.ADDED_SIGNATURES))
    build.build(verbose=False)
    L = _lib.require(*protos)                                           # the library exports the symbols
    for name, (r, kinds) in protos.items():
        sig = _lib.LOSS_OPTS_SIGNATURES[name]
        assert sig[1] == ':' and sig[0] == r, (name, sig, r)
        assert list(sig[2:].replace('s', 'p')) == kinds, (name, sig, ''.join(kinds))
        f = getattr(L, name)
        assert f.restype is _lib._CTYPE[sig[0]] and list(f.argtypes) == [_lib._CTYPE[c] for c in sig[2:]], name
    # the twins' parameters with the options in front of the stream
    S = _lib.SIGNATURES
    assert _lib.LOSS_OPTS_SIGNATURES['effdet_loss_opts_fwd'] == S['effdet_focal_loss_fwd'][:-1] + 'ps'
    assert _lib.LOSS_OPTS_SIGNATURES['effdet_loss_opts_fwd_grad'] == S['effdet_focal_loss_fwd_grad'][:-1] + 'ps'
    assert _lib.LOSS_OPTS_SIGNATURES['effdet_loss_opts_bwd_reg'] == S['effdet_focal_loss_bwd_reg'][:-1] + 'ps'
    assert _lib.LOSS_OPTS_SIGNATURES['effdet_loss_opts_workspace_bytes'] == S['effdet_loss_workspace_bytes'] + 'i'
    # host-only calls: the workspace starts with the existing layout and grows by gtmax [B][N], best and barg [B][A]
    B, A, nc, N = 3, 261, 4, 65
    head = int(L.effdet_loss_workspace_bytes(B, A, nc))
    al = lambda n: (n + 255) // 256 * 256      # noqa: E731
    assert int(L.effdet_loss_opts_workspace_bytes(B, A, nc, N)) == head + al(4 * B * N) + 2 * al(4 * B * A)


def test_struct_matches_the_header_as_gcc_sees_it(tmp_path):
    from efficientdet.pytorch_amd import _lib
    fields = [n for n, _ in _lib.LossOpts._fields_]
    assert fields == ['alpha', 'gamma', 'label_smoothing', 'beta', 'reg_weight', 'pos_iou', 'neg_iou', 'low_quality', 'box_kind', 'box_weight']
    assert ctypes.sizeof(_lib.LossOpts) == 40
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    src = tmp_path / 'sz.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "effdet_loss_opts.h"\nint main(void){printf("%zu\\n", sizeof(effdet_loss_opts_t));'
                   + ''.join('printf("%%zu\\n", offsetof(effdet_loss_opts_t, %s));' % f for f in fields) + 'return 0;}\n')
    exe = tmp_path / 'sz'
    subprocess.run(['gcc', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == ctypes.sizeof(_lib.LossOpts)
    for f, off in zip(fields, out[1:]):
        assert getattr(_lib.LossOpts, f).offset == off, f


def test_invalid_options_are_refused_by_the_library_before_anything_else():
    """Host-only: the options are validated first, so a call with null device pointers still tells a bad option (EINVAL either way) --
    what this pins is that no range of the header's table is accepted by Python and refused by C or the reverse."""
    from efficientdet.pytorch_amd import build, _lib
    build.build(verbose=False)
    L = _lib.require(*ENTRY_POINTS)
    ok = dict(alpha=0.25, gamma=2.0, label_smoothing=0.0, beta=1.0 / 9.0, reg_weight=1.0, pos_iou=0.5, neg_iou=0.4, low_quality=0,
              box_kind=0, box_weight=1.0)
    nan, inf = float('nan'), float('inf')
    bad = [dict(alpha=0.0), dict(alpha=1.0), dict(alpha=nan), dict(gamma=-0.5), dict(gamma=8.5), dict(gamma=nan), dict(label_smoothing=1.0),
           dict(label_smoothing=-0.1), dict(label_smoothing=nan), dict(beta=0.0), dict(beta=inf), dict(beta=nan), dict(beta=-1.0),
           dict(reg_weight=-1.0), dict(reg_weight=inf), dict(reg_weight=nan), dict(pos_iou=0.3), dict(pos_iou=1.5), dict(neg_iou=-0.1),
           dict(neg_iou=nan), dict(pos_iou=nan), dict(low_quality=2), dict(low_quality=-1), dict(box_kind=5), dict(box_kind=-1),
           dict(box_weight=-1.0), dict(box_weight=nan), dict(box_weight=inf)]
    # every call below has null device pointers, so it returns EINVAL whatever the options; the python class must agree on the ranges
    from efficientdet.pytorch_amd import ops
    for kw in bad:
        o = _lib.LossOpts(**dict(ok, **kw))
        assert L.effdet_loss_opts_fwd(None, None, None, None, None, None, 0, 1, 9, 4, 1, ctypes.byref(o), None) == -1
        py = {k: v for k, v in kw.items() if k in ops.LossOptions._FIELDS}
        if py:
            with pytest.raises(ValueError):
                ops.LossOptions(**py)
    assert L.effdet_loss_opts_fwd(None, None, None, None, None, None, 0, 1, 9, 4, 1, None, None) == -1


def test_loss_options_validate_their_arguments():
    from efficientdet.pytorch_amd import BoxLossOptions, LossOptions, ops
    from efficientdet.pytorch_amd.efficientdet import FocalLoss
    d = LossOptions()
    assert d.is_default() and d == LossOptions(0.25, 2.0, 0.0, float(np.float32(1.0 / 9.0)), 1.0, 0.5, 0.4, False)
    assert LossOptions(beta=1.0 / 9.0).is_default()                    # the decimal rounds to the fp32 knee
    assert d.key() == (0.25, 2.0, 0.0, float(np.float32(1.0 / 9.0)), 1.0, 0.5, float(np.float32(0.4)), False)
    o = LossOptions(gamma=1.5, beta=0.1, reg_weight=50, low_quality=True)
    assert not o.is_default() and o.gamma == 1.5 and o.beta == float(np.float32(0.1)) and o.reg_weight == 50.0 and o.low_quality is True
    assert o == LossOptions(gamma=1.5, beta=0.1, reg_weight=50.0, low_quality=1) and o != d and o != None and hash(o) == hash(LossOptions(gamma=1.5, beta=0.1, reg_weight=50, low_quality=True))      # noqa: E711
    assert repr(d).startswith('LossOptions(alpha=0.25, gamma=2.0, label_smoothing=0.0, beta=')
    for f in LossOptions._FIELDS[:-1]:
        assert not LossOptions(**{f: {'alpha': 0.3, 'gamma': 1.0, 'label_smoothing': 0.1, 'beta': 0.2, 'reg_weight': 2.0, 'pos_iou': 0.6,
                                      'neg_iou': 0.3}[f]}).is_default(), f
    assert not LossOptions(low_quality=True).is_default()
    for bad in (dict(alpha=0.0), dict(alpha=1.0), dict(alpha=float('nan')), dict(gamma=-1.0), dict(gamma=9.0), dict(label_smoothing=1.0),
                dict(label_smoothing=-0.1), dict(beta=0.0), dict(beta=float('inf')), dict(beta=float('nan')), dict(reg_weight=-1.0),
                dict(reg_weight=float('inf')), dict(pos_iou=0.3), dict(neg_iou=0.6), dict(pos_iou=1.1), dict(neg_iou=-0.1),
                dict(pos_iou=float('nan')), dict(low_quality=2), dict(low_quality='yes')):
        with pytest.raises(ValueError):
            LossOptions(**bad)
    assert LossOptions(pos_iou=0.5, neg_iou=0.5).neg_iou == 0.5 and LossOptions(gamma=0.0).gamma == 0.0 and LossOptions(gamma=8.0).gamma == 8.0
    # what reaches the library
    assert ops._loss_opts_struct(None) is None and ops._loss_opts_struct(d) is None and ops._loss_opts_struct(d, BoxLossOptions('ciou')) is None
    s = ops._loss_opts_struct(o, BoxLossOptions('giou', 2.0))
    assert (s.alpha, s.gamma, s.label_smoothing, s.reg_weight, s.pos_iou, s.low_quality, s.box_kind, s.box_weight) == (0.25, 1.5, 0.0, 50.0, 0.5, 1, 2, 2.0)
    assert s.beta == float(np.float32(0.1)) and s.neg_iou == float(np.float32(0.4))
    s = ops._loss_opts_struct(o, BoxLossOptions('smooth_l1'))
    assert (s.box_kind, s.box_weight) == (0, 1.0) and (ops._loss_opts_struct(o).box_kind, ops._loss_opts_struct(o).box_weight) == (0, 1.0)
    with pytest.raises(TypeError):
        ops._loss_opts_struct(dict(gamma=1.5))
    with pytest.raises(TypeError):
        ops._loss_opts_struct(o, 'giou')
    with pytest.raises(TypeError):
        FocalLoss(loss='paper')
    assert FocalLoss().loss is None and FocalLoss(loss=o).loss is o and FocalLoss(BoxLossOptions('iou'), o).box_loss.kind == 'iou'


def test_set_loss_takes_options_or_none():
    import pickle
    from efficientdet.pytorch_amd import EfficientDet, LossOptions
    m = EfficientDet(num_classes=4)
    assert m.loss_options is None and m.criterion.loss is None
    o = LossOptions(gamma=1.5, low_quality=True)
    assert m.set_loss(o) is m and m.loss_options is o and m.criterion.loss is o
    with pytest.raises(TypeError):
        m.set_loss(dict(gamma=1.5))
    with pytest.raises(TypeError):
        m.set_loss('paper')
    assert m.loss_options is o
    m2 = pickle.loads(pickle.dumps(m))
    assert m2.loss_options == o and m2.criterion.loss == o
    assert m.set_loss(None).loss_options is None and m.criterion.loss is None
