"""CPU tier: the NumPy restatement of the rescoring NMS (tests/soft_nms_restated.py) on hand-derived cases and against the greedy
restatement the existing NMS tests use, and the validator: it accepts the float64 run and rejects wrong ones."""
import numpy as np
import pytest
import torch

from oracle import effdet_oracle as O
from tests import soft_nms_restated as R
from tests.soft_nms_cases import CASES

TOL = 2e-4
BY_NAME = {c['name']: c for c in CASES}

# three boxes with IoU(A,B) = 80/100 = 0.8, IoU(A,C) = 50/100 = 0.5, IoU(B,C) = 30/(80+50-30) = 0.3 -- all exact in fp32's division
# up to one rounding of 0.8 and 0.3
ABC = np.array([[0, 0, 10, 10], [0, 0, 10, 8], [0, 5, 10, 10]], dtype=np.float32)
ABC_S = np.array([0.9, 0.8, 0.7], dtype=np.float32)


def _opts(case, method, **kw):
    d = dict(threshold=case['threshold'], iou_threshold=case['iou_threshold'], method=method, sigma=0.5, class_aware=False,
             pre_nms_top_n=case['pre_nms_top_n'], max_det=case['max_det'])
    d.update(kw)
    return R.Opts(**d)


@pytest.mark.parametrize('run', [R.run_f32, R.run_f64])
def test_three_boxes_by_hand(run):
    lab = np.zeros(3, dtype=np.int32)
    # hard, IoU threshold 0.4: A suppresses B (0.8) and C (0.5)
    idx, s, n = run(ABC, ABC_S, lab, R.Opts(0.05, 0.4, 'hard'))
    assert n == 1 and idx.tolist() == [0] and s[0] == np.float32(0.9)
    # hard, IoU threshold 0.6: A suppresses B only; C keeps its score
    idx, s, n = run(ABC, ABC_S, lab, R.Opts(0.05, 0.6, 'hard'))
    assert n == 2 and idx.tolist() == [0, 2] and s[1] == np.float32(0.7)
    # hard, IoU threshold exactly 0.5: the test is >, C (IoU 0.5) survives
    idx, s, n = run(ABC, ABC_S, lab, R.Opts(0.05, 0.5, 'hard'))
    assert idx.tolist() == [0, 2]
    # linear, 0.4: after A: B = 0.8 * (1 - 0.8) = 0.16, C = 0.7 * (1 - 0.5) = 0.35; C is next, IoU(C,B) = 0.3 <= 0.4 leaves B alone
    idx, s, n = run(ABC, ABC_S, lab, R.Opts(0.05, 0.4, 'linear'))
    assert n == 3 and idx.tolist() == [0, 2, 1]
    np.testing.assert_allclose(s, [0.9, 0.35, 0.16], rtol=1e-6)
    # gaussian, sigma 0.5: after A: B = 0.8 exp(-0.64 / 0.5) = 0.2224300, C = 0.7 exp(-0.25 / 0.5) = 0.4245715;
    # C is next and B = 0.2224300 exp(-0.09 / 0.5) = 0.1857891
    idx, s, n = run(ABC, ABC_S, lab, R.Opts(0.05, 0.4, 'gaussian', 0.5))
    assert n == 3 and idx.tolist() == [0, 2, 1]
    np.testing.assert_allclose(s, [0.9, 0.4245715, 0.1857891], rtol=2e-6)
    # the same with threshold 0.2: B ends below it after the second rescoring and is dead, not emitted
    idx, s, n = run(ABC, ABC_S, lab, R.Opts(0.2, 0.4, 'gaussian', 0.5))
    assert n == 2 and idx.tolist() == [0, 2]
    # max_det cuts the run
    idx, s, n = run(ABC, ABC_S, lab, R.Opts(0.05, 0.4, 'gaussian', 0.5, False, 1000, 2))
    assert n == 2 and idx.tolist() == [0, 2]
    # the top-N cap drops C before the loop starts
    idx, s, n = run(ABC, ABC_S, lab, R.Opts(0.05, 0.4, 'linear', 0.5, False, 2, 2))
    assert idx.tolist() == [0, 1]
    # classes: B is of another class than A and C -- A rescores C only, and B is picked second with its own score
    idx, s, n = run(ABC, ABC_S, np.array([0, 1, 0]), R.Opts(0.05, 0.4, 'hard', 0.5, True))
    assert idx.tolist() == [0, 1] and s[1] == np.float32(0.8)


def test_two_classes_on_identical_boxes():
    c = BY_NAME['two_classes_identical_boxes']
    for method in ('hard', 'linear', 'gaussian'):
        aware = R.run_f32(c['boxes'][0], c['score'][0], c['label'][0], _opts(c, method, class_aware=True))
        assert aware[2] == 12 and np.array_equal(aware[1], c['score'][0])           # nothing of the same class overlaps: scores untouched
    agnostic = R.run_f32(c['boxes'][0], c['score'][0], c['label'][0], _opts(c, 'hard'))
    assert agnostic[2] == 6 and agnostic[0].tolist() == [0, 2, 4, 6, 8, 10]


def test_candidate_order_and_degenerate_boxes():
    c = BY_NAME['degenerate_and_nan']
    order = R.sorted_candidates(c['score'][0], c['threshold'], 4096)
    assert 23 not in order and 27 not in order and len(order) == 198               # the NaN and the -inf score are no candidates
    sc = c['score'][0][order]
    assert np.all(sc[:-1] >= sc[1:])
    t = BY_NAME['score_ties']
    order = R.sorted_candidates(t['score'][0], t['threshold'], 4096)
    sc = t['score'][0][order]
    assert np.all((sc[:-1] > sc[1:]) | ((sc[:-1] == sc[1:]) & (order[:-1] < order[1:])))
    # gaussian rescoring leaves the degenerate boxes' scores alone, and picking one changes nobody's score
    idx, s, n = R.run_f32(c['boxes'][0], c['score'][0], c['label'][0], _opts(c, 'gaussian', max_det=198))
    got = dict(zip(idx.tolist(), s.tolist()))
    for a in (3, 5, 7, 11, 13, 15, 17, 19, 21):
        assert got[a] == c['score'][0][a], a
    assert idx[:4].tolist() == [3, 11, 15, 19] and got[int(idx[4])] == c['score'][0][int(idx[4])]
    assert np.all(np.isfinite(s)) and np.all(s[:-1] >= s[1:])


@pytest.mark.parametrize('case', [c for c in CASES if c['n'] <= c['pre_nms_top_n']], ids=lambda c: c['name'])
def test_hard_class_agnostic_is_the_greedy_restatement(case):
    for b in range(case['boxes'].shape[0]):
        boxes, score = case['boxes'][b], case['score'][b]
        with np.errstate(invalid='ignore'):
            cand = np.nonzero(score > np.float32(case['threshold']))[0]
        ref = cand[O.nms_greedy(torch.from_numpy(boxes[cand]), torch.from_numpy(score[cand]), case['iou_threshold']).numpy()]
        idx, s, n = R.run_f32(boxes, score, None, _opts(case, 'hard', max_det=max(case['n'], 1)))
        assert n == len(ref) and np.array_equal(idx, ref)
        assert np.array_equal(s, score[ref])


@pytest.mark.parametrize('method', ['hard', 'linear', 'gaussian'])
@pytest.mark.parametrize('name', ['n65', 'n1025', 'n1001_top1000', 'identical_clusters', 'score_ties', 'degenerate_and_nan', 'batch3_500_0_37'])
def test_validator_accepts_the_float64_run(name, method):
    c = BY_NAME[name]
    for aware in (False, True):
        o = _opts(c, method, class_aware=aware)
        for b in range(c['boxes'].shape[0]):
            idx, s, n = R.run_f64(c['boxes'][b], c['score'][b], c['label'][b], o)
            assert R.check_run(c['boxes'][b], c['score'][b], c['label'][b], o, idx, s, n, TOL) == 0.0
            assert np.all(s[:-1] >= s[1:])                                          # emitted scores never increase


def test_validator_rejects_wrong_runs():
    c = BY_NAME['n1023']
    boxes, score, label = c['boxes'][0], c['score'][0], c['label'][0]
    gauss = _opts(c, 'gaussian')
    # a hard-NMS result presented as gaussian
    idx, s, n = R.run_f64(boxes, score, label, _opts(c, 'hard'))
    with pytest.raises(AssertionError):
        R.check_run(boxes, score, label, gauss, idx, s, n, TOL)
    # gaussian with sigma off by 10 %
    idx, s, n = R.run_f64(boxes, score, label, _opts(c, 'gaussian', sigma=0.55))
    with pytest.raises(AssertionError):
        R.check_run(boxes, score, label, gauss, idx, s, n, TOL)
    # two neighbouring picks swapped across a gap larger than tol
    idx, s, n = R.run_f64(boxes, score, label, gauss)
    R.check_run(boxes, score, label, gauss, idx, s, n, TOL)
    k = int(np.argmax(s[:-1] / s[1:]))
    assert s[k] > s[k + 1] * (1 + 2 * TOL)
    idx2, s2 = idx.copy(), s.copy()
    idx2[[k, k + 1]] = idx[[k + 1, k]]; s2[[k, k + 1]] = s[[k + 1, k]]
    with pytest.raises(AssertionError, match='live maximum'):
        R.check_run(boxes, score, label, gauss, idx2, s2, n, TOL)
    # a run that stops early, one that picks an anchor twice, and a score off by 1e-3
    with pytest.raises(AssertionError, match='stopped'):
        R.check_run(boxes, score, label, gauss, idx, s, n - 1, TOL) if n < gauss.max_det else R.check_run(
            boxes, score, label, gauss._replace(max_det=n + 50), idx, s, n - 1, TOL)
    idx3 = idx.copy(); idx3[7] = idx[2]
    with pytest.raises(AssertionError, match='not live'):
        R.check_run(boxes, score, label, gauss, idx3, s, n, TOL)
    s3 = s.copy(); s3[9] *= 1.001
    with pytest.raises(AssertionError, match='device score'):
        R.check_run(boxes, score, label, gauss, idx, s3, n, TOL)


def test_nms_options_validate_their_arguments():
    from efficientdet.pytorch_amd import NMSOptions
    o = NMSOptions('gaussian', sigma=0.3, class_aware=True)
    assert (o.method, o.sigma, o.class_aware, o.pre_nms_top_n, o.max_det) == ('gaussian', 0.3, True, 1000, 100)
    assert o == NMSOptions('gaussian', 0.3, True) and o != NMSOptions('gaussian', 0.5, True) and o != None     # noqa: E711
    for bad in (dict(method='matrix'), dict(sigma=0.0), dict(pre_nms_top_n=4097), dict(pre_nms_top_n=0), dict(max_det=0),
                dict(pre_nms_top_n=50, max_det=51)):
        with pytest.raises(ValueError):
            NMSOptions(**bad)


def test_added_signatures_match_the_companion_header():
    """_lib.ADDED_SIGNATURES against the prototypes of include/effdet_soft_nms.h, parsed as tests/test_abi.py parses effdet_hip.h's:
    the same names, return kind, parameter count and kinds in order; the built library exports both and lib() binds them with the
    table's types; the two names are in neither effdet_hip.h's prototypes nor its table."""
    import ctypes as C
    import os
    import re
    from efficientdet.pytorch_amd import build, _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    h = re.sub(r'/\*.*?\*/', '', open(os.path.join(root, 'include', 'effdet_soft_nms.h')).read(), flags=re.S)
    scalar = {'int': 'i', 'long long': 'q', 'float': 'f', 'effdet_stream_t': 'p'}
    protos = {}
    for r, name, params in re.findall(r'^([a-z][a-z ]*?\*?)\s*\b(effdet_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', h, flags=re.M):
        kinds = ['p' if '*' in p else scalar[' '.join(p.split()).rsplit(' ', 1)[0]] for p in params.split(',')]
        assert name not in protos, name
        protos[name] = ({'int': 'i', 'long long': 'q'}[' '.join(r.split())], kinds)
    assert sorted(protos) == sorted(set(re.findall(r'\b(effdet_[a-z0-9_]+)\s*\(', h))) == ['effdet_soft_nms', 'effdet_soft_nms_workspace_bytes']
    assert sorted(_lib.ADDED_SIGNATURES) == sorted(protos) and not set(protos) & set(_lib.SIGNATURES)
    build.build(verbose=False)
    L = _lib.require(*protos)
    for name, (r, kinds) in protos.items():
        sig = _lib.ADDED_SIGNATURES[name]
        assert sig[1] == ':' and sig[0] == r, (name, sig, r)
        assert list(sig[2:].replace('s', 'p')) == kinds, (name, sig, ''.join(kinds))
        f = getattr(L, name)
        assert f.restype is _lib._CTYPE[sig[0]] and list(f.argtypes) == [_lib._CTYPE[c] for c in sig[2:]], name
    assert [_lib._CTYPE[c] for c in 'iqfp'] == [C.c_int, C.c_longlong, C.c_float, C.c_void_p]
    # the companion header compiles as C on top of effdet_hip.h
    import shutil
    import subprocess
    import tempfile
    if shutil.which('gcc') is not None:
        with tempfile.TemporaryDirectory() as d:
            src = os.path.join(d, 'h.c')
            open(src, 'w').write('#include "effdet_soft_nms.h"\nint main(void){return EFFDET_NMS_GAUSSIAN == 2 && EFFDET_SOFT_NMS_MAX_TOP_N == 4096 ? 0 : 1;}\n')
            subprocess.run(['gcc', '-Wall', '-Werror', '-I', os.path.join(root, 'include'), src, '-o', os.path.join(d, 'h')], check=True)
            subprocess.run([os.path.join(d, 'h')], check=True)
