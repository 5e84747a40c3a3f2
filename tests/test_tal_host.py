"""CPU tier of the task-aligned matcher (include/effdet_tal.h): the float64 restatement (tests/tal_restated.py) and its integer-only
twin against the hand-derived case, the decision gaps and tags of the cases (tests/tal_cases.py), the binding against the header,
the host-only entry points and the Python options."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import loss_cases as LC
from tests import tal_cases as TC
from tests import tal_restated as TR
from tests.test_atss_host import ROOT

ENTRY_POINTS = ['effdet_loss_tal_fwd', 'effdet_loss_tal_fwd_grad', 'effdet_loss_tal_metrics', 'effdet_loss_tal_workspace_bytes']


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# --------------------------------------------------------------------------- the restatements against the hand-derived case
def test_hand_case_pairs_winners_codes_and_targets():
    c, r = TC.get('hand'), TC.reference('hand')
    assert TR.valid_rows(c, 0) == [0, 2, 3]
    assert [int(TR.inside(c, 0, n).sum()) for n in (0, 2, 3)] == [36, 9, 45] and c['tal']['topk'] == 12      # row 2: inside set < topk
    m32, u32 = TR.metrics(c, c['tal'], np.float32)
    for (n, a), (m, u) in TC.HAND_METRIC.items():
        assert float(m32[0, n, a]) == m and float(u32[0, n, a]) == u, (n, a)                # exact in fp32
        assert abs(float(r['m'][0, n, a]) - m) < 1e-8 and abs(float(r['u'][0, n, a]) - u) < 1e-8
    assert int((m32 > 0).sum()) == len(TC.HAND_METRIC)                                       # s == 0 elsewhere: m == 0, no candidate
    assert {n: w for (_, n), w in r['winners'].items()} == TC.HAND_WINNERS
    codes = r['codes'][0]
    assert {int(a): int(codes[a]) for a in torch.nonzero(codes >= 0).reshape(-1)} == TC.HAND_CODES
    assert int((codes == LC.CODE_NEG).sum()) == 180 - 7 and r['num_pos'].tolist() == [7]
    assert {a // 144 for a in TC.HAND_CODES} == {0, 1}                                       # positives on both levels
    # the integer-only form on the float32 planes: the same winners and codes, and the targets as literals
    keys, icodes = TR.assign_bits(_bits(m32[0]), _bits(u32[0]), [0, 2, 3], 12)
    assert {n: [k & 0xFFFFFFFF for k in ks] for n, ks in keys.items()} == TC.HAND_WINNERS
    assert np.array_equal(icodes, codes.numpy())
    assert keys[0][0] >> 32 == (~int(_bits(np.float32(1 / 32)).reshape(-1)[0]) & 0xFFFFFFFF)
    q, mm = TR.target(_bits(m32[0]), _bits(u32[0]), icodes, keys)
    assert {int(a): float(q[a]) for a in np.nonzero(q)[0]} == TC.HAND_Q and {n: (float(a), float(b)) for n, (a, b) in mm.items()} == TC.HAND_MM


def test_selection_rules_on_small_vectors():
    m = np.array([0.0, 0.5, np.nan, 0.5, 0.25, -0.0, np.inf, 1e-45], dtype=np.float32)
    assert TR.select(m.astype(np.float64), 3) == [6, 1, 3] and TR.select(m.astype(np.float64), 16) == [6, 1, 3, 4, 7]
    u = np.full_like(m, 0.5)
    keys, codes = TR.assign_bits(_bits(m)[None], _bits(u)[None], [0], 3)
    assert [k & 0xFFFFFFFF for k in keys[0]] == [6, 1, 3] and codes.tolist() == [-1, 0, -1, 0, -1, -1, 0, -1]
    assert all(k != TR.NO_KEY for k in keys[0])
    # two rows on one anchor: the larger u, and the FIRST row on equal bits
    m2 = np.array([[0.5, 0.5, 0.0], [0.25, 0.75, 0.5]], dtype=np.float32)
    u2 = np.array([[0.5, 0.25, 0.0], [0.5, 0.5, 0.125]], dtype=np.float32)
    _, codes = TR.assign_bits(_bits(m2), _bits(u2), [0, 1], 2)
    assert codes.tolist() == [0, 1, 1]
    _, codes = TR.assign_bits(_bits(m2), _bits(u2), [0, 1], 1)                               # row 0 selects anchor 0, row 1 anchor 1
    assert codes.tolist() == [0, 1, -1]
    assert TR._pow(np.array([0.0, 0.25], np.float32), 0.0, np.float32).tolist() == [0.0, 1.0]      # a base of 0 gives 0


@pytest.mark.parametrize('name', sorted(TC.CASES))
def test_every_decision_is_a_tie_of_equal_operands_or_clear(name):
    """The condition that makes the float64 codes the only admissible device answer: every non-zero gap is at least TR.GAP relative
    (the device's metric carries ~1e-6), and no winner's metric is small enough to underflow in fp32."""
    worst, least = TC.gaps(name)
    print('\n%s: smallest non-zero gap %.3g, smallest winner metric %.3g' % (name, worst, least))
    assert worst >= TR.GAP and least >= TR.TINY, (name, worst, least)


@pytest.mark.parametrize('name', sorted(TC.CASES))
def test_integer_form_on_float32_planes_equals_the_float64_form(name):
    """... and under that condition the integer-only form, fed the float32 evaluation's bit patterns, reproduces the float64 codes."""
    c, r = TC.get(name), TC.reference(name)
    m32, u32 = TR.metrics(c, c['tal'], np.float32)
    for b in range(m32.shape[0]):
        rows = TR.valid_rows(c, b)
        if not rows:
            assert bool((r['codes'][b] == LC.CODE_IGN).all())
            continue
        keys, codes = TR.assign_bits(_bits(m32[b]), _bits(u32[b]), rows, c['tal']['topk'])
        assert np.array_equal(codes, r['codes'][b].numpy()), name
        for n in rows:
            assert [k & 0xFFFFFFFF for k in keys[n]] == r['winners'][(b, n)], (name, b, n)


def test_cases_reach_what_they_are_tagged_with():
    tags = {name: set(TC.get(name)['tags']) for name in TC.CASES}
    assert set().union(*tags.values()) >= {'hand', 'two_levels', 'inside_below_topk', 'conflict', 'zero_base', 'pads_between', 'levels_crossed',
                                           'all_inside', 'no_inside', 'empty_image', 'metric_tie', 'conflict_tie', 'label_outside',
                                           'second_chunk', 'seeded'}
    levels = np.array([0, 2304, 2880, 3024, 3060, 3069])
    c, r = TC.get('straddle'), TC.reference('straddle')
    lev = lambda idx: set((np.searchsorted(levels, idx, side='right') - 1).tolist())      # noqa: E731
    assert len(lev(np.nonzero(TR.inside(c, 0, 0))[0])) >= 4                                  # the scan crosses the level boundaries
    assert len(lev(r['winners'][(0, 0)] + r['winners'][(0, 1)])) >= 2                         # ... and the image's winners lie on several levels
    c = TC.get('whole')
    assert bool(TR.inside(c, 0, 0).all()) and c['cls'].shape[1] == 3069 and 3069 % 256 != 0
    c, r = TC.get('narrow'), TC.reference('narrow')
    assert not bool(TR.inside(c, 0, 0).any()) and bool((r['codes'][0] == LC.CODE_NEG).all()) and bool((r['codes'][1] == LC.CODE_IGN).all())
    c, r = TC.get('few'), TC.reference('few')
    assert int(TR.inside(c, 0, 0).sum()) == 9 and len(r['winners'][(0, 0)]) == 9 and len(r['winners'][(0, 1)]) == 13
    r = TC.reference('nested')
    for b in range(2):
        both = set(r['winners'][(b, 0)]) & set(r['winners'][(b, 1)])
        assert both and {int(r['codes'][b, a]) for a in both} <= {0, 1}
    assert {int(r['codes'][b, a]) for b in range(2) for a in set(r['winners'][(b, 0)]) & set(r['winners'][(b, 1)])} == {0, 1}
    c, r = TC.get('dup'), TC.reference('dup')
    for b in range(2):
        ins = np.nonzero(TR.inside(c, b, 0) & (r['u'][b, 0] > 0))[0]
        assert r['winners'][(b, 0)] == ins[:13].tolist() == r['winners'][(b, 2)]              # equal metrics: the lowest indices
        assert len(set(r['m'][b, 0][ins].tolist())) == 1
        assert bool((r['codes'][b, ins[:13]] == 0).all()) and int((r['codes'][b] == 2).sum()) == 0      # equal u: the FIRST row
    c, r = TC.get('bad_label'), TC.reference('bad_label')
    assert r['winners'][(0, 0)] == [] and len(r['winners'][(0, 1)]) == 13 and bool((r['codes'][1] == LC.CODE_NEG).all())
    c, r = TC.get('n70'), TC.reference('n70')
    rows = TR.valid_rows(c, 0)
    assert c['ann'].shape[1] == 70 and len(rows) == 66 and rows[-1] == 68 and bool((r['codes'][0] >= 64).any())
    claims = {}
    for (b, n), w in r['winners'].items():
        for a in w:
            claims.setdefault((b, a), []).append(n)
    assert sum(len(v) > 1 for v in claims.values()) > 50                                     # many conflicts
    assert [TC.get(n)['tal']['topk'] for n in ('topk1', 's128_nc4', 'topk16')] == [1, 13, 16]
    assert TC.get('alpha0')['tal']['alpha'] == 0.0 and TC.get('beta0')['tal']['beta'] == 0.0
    assert {TC.get(n)['cls'].shape[2] for n in ('s128_nc4', 's128_nc80', 'topk16')} == {4, 80}


# --------------------------------------------------------------------------- binding
def _prototypes():
    h = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'effdet_tal.h')).read(), flags=re.S)
    scalar = {'int': 'i', 'long long': 'q', 'float': 'f', 'effdet_stream_t': 'p'}
    protos = {}
    for r, name, params in re.findall(r'^([a-z][a-z ]*?\*?)\s*\b(effdet_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', h, flags=re.M):
        kinds = ['p' if '*' in p else scalar[' '.join(p.split()).rsplit(' ', 1)[0]] for p in params.split(',')]
        assert name not in protos, name
        protos[name] = ({'int': 'i', 'long long': 'q'}[' '.join(r.split())], kinds)
    assert sorted(protos) == sorted(set(re.findall(r'\b(effdet_[a-z0-9_]+)\s*\(', h)))
    return protos


def test_the_header_parser_is_the_atss_tests():
    """tests/test_atss_host._prototypes reads include/effdet_atss.h by name; _prototypes above is that function on effdet_tal.h."""
    import inspect
    from tests import test_atss_host as TA
    mine, theirs = inspect.getsource(_prototypes), inspect.getsource(TA._prototypes)
    assert mine.replace('effdet_tal.h', 'effdet_atss.h') == theirs


def _tal(topk=13, alpha=1.0, beta=6.0, aligned=1):
    from efficientdet.pytorch_amd import _lib
    return _lib.Tal(topk, alpha, beta, aligned)


def test_tal_signatures_match_the_companion_header_and_workspace_bytes():
    from efficientdet.pytorch_amd import build, _lib
    protos = _prototypes()
    assert sorted(protos) == ENTRY_POINTS == sorted(_lib.TAL_SIGNATURES)
    assert not set(protos) & (set(_lib.SIGNATURES) | set(_lib.ATSS_SIGNATURES) | set(_lib.QUALITY_LOSS_SIGNATURES) | set(_lib.LOSS_OPTS_SIGNATURES))
    build.build(verbose=False)
    L = _lib.require(*protos)                                                                # the built library exports the four symbols
    for name, (r, kinds) in protos.items():
        sig = _lib.TAL_SIGNATURES[name]
        assert sig[1] == ':' and sig[0] == r, (name, sig, r)
        assert list(sig[2:].replace('s', 'p')) == kinds, (name, sig, ''.join(kinds))
        f = getattr(L, name)
        assert f.restype is _lib._CTYPE[sig[0]] and list(f.argtypes) == [_lib._CTYPE[c] for c in sig[2:]], name
    Q = _lib.QUALITY_LOSS_SIGNATURES
    for stem in ('workspace_bytes', 'fwd', 'fwd_grad'):                                      # the quality loss's twins, tal in the place of atss
        assert _lib.TAL_SIGNATURES['effdet_loss_tal_' + stem] == Q['effdet_loss_quality_' + stem]
    # host-only: the quality layout first (q where the class backward looks for it), then keys, (mmax, umax), claims
    B, A, nc = 3, 261, 4
    al = lambda n: (n + 255) // 256 * 256      # noqa: E731
    good = _tal()
    sizes = [int(L.effdet_loss_tal_workspace_bytes(B, A, nc, N, ctypes.byref(good))) for N in (1, 2, 65, 66, 200)]
    head = int(L.effdet_loss_quality_workspace_bytes(B, A, nc, 65, None))
    assert sizes[2] == head + al(8 * 16 * B * 65) + al(8 * B * 65) + al(8 * B * A)
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0]
    nan = float('nan')
    for bad in (_tal(0), _tal(17), _tal(-1), _tal(alpha=-0.5), _tal(alpha=4.5), _tal(alpha=nan), _tal(beta=-1.0), _tal(beta=16.5),
                _tal(beta=nan), _tal(aligned=2), _tal(aligned=-1)):
        assert int(L.effdet_loss_tal_workspace_bytes(B, A, nc, 65, ctypes.byref(bad))) == -1
        assert L.effdet_loss_tal_metrics(None, None, None, None, None, B, A, nc, 65, ctypes.byref(bad), None) == -1
    assert int(L.effdet_loss_tal_workspace_bytes(B, A, nc, 65, None)) == -1
    for ok in (_tal(1, 0.0, 0.0, 0), _tal(16, 4.0, 16.0, 1)):
        assert int(L.effdet_loss_tal_workspace_bytes(B, A, nc, 65, ctypes.byref(ok))) == sizes[2]
    # null device pointers: EINVAL before anything is launched
    d = _lib.LossOpts(0.25, 2.0, 0.0, 1.0 / 9.0, 1.0, 0.5, 0.4, 0, 0, 1.0)
    assert L.effdet_loss_tal_fwd(None, None, None, None, None, None, 0, 1, 261, 4, 1, ctypes.byref(d), ctypes.byref(good), None, None) == -1
    assert L.effdet_loss_tal_metrics(None, None, None, None, None, 1, 261, 4, 1, ctypes.byref(good), None) == -1


def test_struct_matches_the_header_as_gcc_sees_it(tmp_path):
    from efficientdet.pytorch_amd import _lib
    fields = [n for n, _ in _lib.Tal._fields_]
    assert fields == ['topk', 'alpha', 'beta', 'aligned_target'] and ctypes.sizeof(_lib.Tal) == 16 and _lib.TAL_MAX_TOPK == 16
    gcc = shutil.which('gcc')
    if gcc is None:
        pytest.skip('no gcc')
    src = tmp_path / 'sz.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "effdet_tal.h"\nint main(void){printf("%zu\\n", sizeof(effdet_tal_t));'
                   + ''.join('printf("%%zu\\n", offsetof(effdet_tal_t, %s));' % f for f in fields)
                   + 'printf("%d\\n", EFFDET_TAL_MAX_TOPK);return 0;}\n')
    exe = tmp_path / 'sz'
    subprocess.run([gcc, '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == ctypes.sizeof(_lib.Tal) and out[-1] == _lib.TAL_MAX_TOPK
    for f, off in zip(fields, out[1:]):
        assert getattr(_lib.Tal, f).offset == off, f


# --------------------------------------------------------------------------- the Python options
def test_task_aligned_options_validate_their_arguments():
    from efficientdet.pytorch_amd import ATSSOptions, TaskAlignedOptions, ops
    o = TaskAlignedOptions()
    assert o.key() == (13, 1.0, 6.0, True) and o == TaskAlignedOptions(13, 1.0, 6.0, True) and hash(o) == hash(TaskAlignedOptions(topk=13))
    assert o != TaskAlignedOptions(12) and o != TaskAlignedOptions(beta=4.0) and o != TaskAlignedOptions(aligned_target=False)
    assert o != None and o != ATSSOptions(13)      # noqa: E711
    assert repr(TaskAlignedOptions(9, 0.5, 2.0, False)) == 'TaskAlignedOptions(topk=9, alpha=0.5, beta=2.0, aligned_target=False)'
    assert TaskAlignedOptions(1).topk == 1 and TaskAlignedOptions(16).topk == 16
    assert TaskAlignedOptions(alpha=0, beta=0).key()[1:3] == (0.0, 0.0) and TaskAlignedOptions(alpha=4, beta=16).key()[1:3] == (4.0, 16.0)
    assert TaskAlignedOptions(alpha=0.1).alpha == float(np.float32(0.1))                     # kept as the fp32 the kernels receive
    nan = float('nan')
    for kw in (dict(topk=0), dict(topk=17), dict(topk=-1), dict(topk=13.0), dict(topk='13'), dict(topk=None), dict(topk=True),
               dict(alpha=-0.1), dict(alpha=4.1), dict(alpha=nan), dict(beta=-1), dict(beta=16.5), dict(beta=nan),
               dict(aligned_target=2), dict(aligned_target='yes'), dict(aligned_target=None)):
        with pytest.raises(ValueError):
            TaskAlignedOptions(**kw)
    t = ops._tal_struct(TaskAlignedOptions(9, 0.5, 2.0, False))
    assert (t.topk, t.alpha, t.beta, t.aligned_target) == (9, 0.5, 2.0, 0)
    assert ops._matcher_struct(None, None, 9) is None and ops._matcher_struct(o, None, 9).topk == 13      # no levels needed
    with pytest.raises(ValueError):
        ops._matcher_struct(ATSSOptions(), None, 9)                                          # ATSS still needs them
    with pytest.raises(TypeError):
        ops.loss_tal_metrics(None, None, None, None, ATSSOptions())
    ws = torch.zeros(16, dtype=torch.uint8)
    with pytest.raises(ValueError):
        ops.loss_tal_candidates(ws, 1, 9, 1)
    with pytest.raises(TypeError):
        ops.loss_quality_targets(ws, 1, 9, 1, matcher='tal')


def test_matcher_combinations_and_type_errors():
    from efficientdet.pytorch_amd import EfficientDet, LossOptions, QualityLossOptions, TaskAlignedOptions, ATSSOptions, ops
    from efficientdet.pytorch_amd.efficientdet import FocalLoss
    o = TaskAlignedOptions()
    for bad in ('tal', 13, 1.0, object()):
        with pytest.raises(TypeError):
            ops.check_matcher(bad, None)
        with pytest.raises(TypeError):
            FocalLoss(matcher=bad)
        with pytest.raises(TypeError):
            EfficientDet(num_classes=4).set_matcher(bad)
    ops.check_matcher(o, None)
    ops.check_matcher(o, LossOptions(gamma=1.5, beta=0.1, reg_weight=50.0))                  # what a matcher does not replace
    for kw in (dict(low_quality=True), dict(pos_iou=0.6), dict(neg_iou=0.3)):
        bad = LossOptions(**kw)
        with pytest.raises(ValueError) as e:
            ops.check_matcher(o, bad)
        assert 'TaskAlignedOptions' in str(e.value) and 'LossOptions' in str(e.value)
        m = EfficientDet(num_classes=4).set_loss(bad)
        with pytest.raises(ValueError):
            m.set_matcher(o)
        assert m.matcher is None and m.criterion.matcher is None
        m = EfficientDet(num_classes=4).set_matcher(o)
        with pytest.raises(ValueError):
            m.set_loss(bad)
        assert m.loss_options is None and m.matcher is o
        with pytest.raises(ValueError):
            FocalLoss(loss=bad, matcher=o)
    m = EfficientDet(num_classes=4)
    assert m.set_matcher(o) is m and m.matcher is o and m.criterion.matcher is o
    assert m.set_quality_loss(QualityLossOptions('qfl')).quality_loss is not None            # the loss half of the recipe composes
    assert m.set_matcher(ATSSOptions()).matcher == ATSSOptions() and m.set_matcher(o).matcher is o      # ATSS first, then TAL
    assert m.set_matcher(None).matcher is None and m.criterion.matcher is None
    assert FocalLoss(matcher=o, quality=QualityLossOptions('vfl')).matcher is o


def test_entry_points_chosen_for_a_task_aligned_matcher():
    from efficientdet.pytorch_amd import ATSSOptions, BoxLossOptions, QualityLossOptions, TaskAlignedOptions, build, ops
    build.build(verbose=False)
    o, q, box = TaskAlignedOptions(), QualityLossOptions('qfl'), BoxLossOptions('giou', 2.0)
    t = ops._matcher_struct(o, None, 261)
    for stem in ('fwd', 'fwd_grad'):
        for quality, n_null in ((None, 1), (q, 0)):
            fn, name, extra, opts, _ = ops._loss_entry(stem, None, box, o, t, quality)
            assert name == 'effdet_loss_tal_' + stem and len(extra) == 3 and opts is True and sum(e is None for e in extra) == n_null
    assert ops._loss_entry('bwd_cls', None, None, o)[1] == 'effdet_loss_opts_bwd_cls'       # no backward entry points of its own
    assert ops._loss_entry('bwd_cls', None, None, o, quality=q)[1] == 'effdet_loss_quality_bwd_cls'
    assert ops._loss_entry('bwd_reg', None, box, o, quality=q)[1] == 'effdet_loss_opts_bwd_reg'
    # without one, and with ATSS, the calls are the ones made before
    assert ops._loss_entry('fwd')[1] == 'effdet_focal_loss_fwd'
    a = ATSSOptions()
    assert ops._loss_entry('fwd', None, None, a, ops._matcher_struct(a, [252, 9], 261))[1] == 'effdet_loss_atss_fwd'
    assert ops._loss_entry('fwd', None, None, a, ops._matcher_struct(a, [252, 9], 261), q)[1] == 'effdet_loss_quality_fwd'
