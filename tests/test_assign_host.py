"""CPU tier of the optimal assignment (include/effdet_assign.h, csrc/assign.h, csrc/assign.hip, ops.linear_assignment,
TrackOptions(assignment=...)): the integer restatement (tests/assign_restated.py) against brute force and against scipy, what the cases
of tests/assign_cases.py reach, the binding's table against the header, the refusals the entry points decide on the host and the
options' rules."""
import os
import re

import numpy as np
import pytest

from tests import assign_restated as A
from tests import assign_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the restatement
def test_the_quantiser():
    f = np.float32
    g = f(0.2)
    sim = np.array([[0.2, np.nextafter(g, f(1)), 0.7, np.nan], [np.inf, -np.inf, 1.5, 0.1]], dtype=np.float32)
    W = A.weights(sim, g)
    assert W[0, 0] == 0 and W[0, 1] == 1 and W[0, 3] == 0 and W[1, 1] == 0 and W[1, 3] == 0
    assert W[1, 0] == 1 << 20 and W[1, 2] == 1 << 20                               # +inf and sim - gate > 1 saturate
    assert W[0, 2] == int(np.rint(np.float64(f(0.7) - g) * 2 ** 20))               # (the fp32 difference times 2^20 is exact)
    # ties go to even: 2.5 and 3.5 grid steps above a gate of 0
    assert list(A.weights(np.array([[2.5 / 2 ** 20, 3.5 / 2 ** 20]], dtype=np.float32), 0.0)[0]) == [2, 4]
    assert A.SCALE_BITS == 20 and A.MAX_COLS * 2 ** A.SCALE_BITS < 2 ** 31


def test_the_restatement_equals_brute_force():
    rng = np.random.RandomState(0)
    n = 0
    for trial in range(400):
        R, Cn = rng.randint(1, 7), rng.randint(1, 7)
        hi = [2, 9, 1 << 20][trial % 3]                                            # small ranges make ties
        W = rng.randint(1, hi + 1, (R, Cn)) * (rng.uniform(size=(R, Cn)) < rng.uniform(0.2, 1.0))
        total, match = A.solve(W)
        assert total == A.brute(W), W
        r2c, c2r = np.full(R, -1), np.full(Cn, -1)
        for r, c in match.items():
            r2c[r], c2r[c] = c, r
        assert A.check_matching(W, r2c, c2r) == total
        sb = A.second_best(W)
        assert (sb is None) == (total == 0) and (sb is None or sb <= total)
        n += 1
    assert n == 400


def test_second_best_on_a_known_problem():
    W = np.array([[10, 9], [8, 1]])                                                # optimum (0,1),(1,0) = 17; then (0,0),(1,1) = 11
    assert A.solve(W) == (17, {0: 1, 1: 0}) and A.second_best(W) == 11
    assert A.second_best(np.array([[5, 5], [5, 5]])) == 10                         # a tie: the second best equals the optimum


def test_the_restatement_equals_scipy_up_to_the_caps():
    opt = pytest.importorskip('scipy.optimize')
    rng = np.random.RandomState(1)
    for R, Cn, dens in ((3, 3, 1.0), (17, 30, 0.5), (65, 24, 0.3), (200, 128, 0.1), (A.MAX_ROWS, A.MAX_COLS, 1.0), (A.MAX_ROWS, A.MAX_COLS, 0.05)):
        W = rng.randint(1, (1 << 20) + 1, (R, Cn)) * (rng.uniform(size=(R, Cn)) < dens)
        pad = np.zeros((R + Cn, R + Cn), dtype=np.int64)                           # square, zeros: anything may stay unmatched
        pad[:R, :Cn] = W
        r, c = opt.linear_sum_assignment(pad, maximize=True)
        assert A.solve(W)[0] == int(pad[r, c].sum()), (R, Cn, dens)


# ------------------------------------------------------------------------------------------------ what the cases reach
def test_the_case_list():
    assert C.NAMES == ('one_by_one', 'one_row', 'one_col', 'tall', 'wide', 'three', 'example', 'waves65', 'waves200', 'cap_dense', 'nothing',
                       'ties', 'gate_edge', 'nonfinite', 'clamp', 'counts', 'batch', 'chain')
    shapes = {n: C.case(n)['sim'].shape for n in C.NAMES}
    assert shapes['one_by_one'] == (1, 1, 1) and shapes['one_row'][1] == 1 and shapes['one_col'][2] == 1 and shapes['three'][1:] == (3, 3)
    assert shapes['tall'][1] > shapes['tall'][2] and shapes['wide'][1] < shapes['wide'][2]
    assert shapes['waves65'][1] == 65 and shapes['waves200'][1] == 200 and shapes['cap_dense'] == (1, A.MAX_ROWS, A.MAX_COLS)
    assert all(s[1] <= A.MAX_ROWS and s[2] <= A.MAX_COLS for s in shapes.values())


@pytest.mark.parametrize('name', C.NAMES)
def test_every_case_reaches_its_tags(name):
    c, probs = C.case(name), C.problems(name)
    tags = c['tags']
    assert set(tags) <= {'unique', 'greedy_differs', 'waves', 'cap', 'nothing', 'ties', 'gate_edge', 'nonfinite', 'clamp', 'counts', 'batch', 'chain'}
    if 'unique' in tags:
        for W, total, _ in probs:
            sb = A.second_best(W)
            assert sb is None or total - sb >= 1, (name, total, sb)
    if 'ties' in tags:
        assert all(A.second_best(W) == total and total > 0 for W, total, _ in probs)
    if 'greedy_differs' in tags:
        W, total, match = probs[0]
        assert match == {0: 1, 1: 0} and W[0, 0] == W.max() and W[1, 1] == 0 and total > W[0, 0]      # greedy: (0, 0), then nothing for row 1
    if 'waves' in tags:
        assert any(max(m) >= 64 for _, _, m in probs if m)                         # a matched row beyond the first wave
    if 'cap' in tags:
        W, total, match = probs[0]
        assert W.shape == (A.MAX_ROWS, A.MAX_COLS) and (W > 0).all() and len(match) == A.MAX_COLS
    if 'nothing' in tags:
        assert all(not W.any() and total == 0 and not m for W, total, m in probs)
    if 'gate_edge' in tags:
        W = probs[0][0]
        assert np.array_equal(W, np.eye(4, dtype=np.int64)) and (c['sim'][0] == np.float32(c['gate'])).sum() == 12
    if 'nonfinite' in tags:
        s, W = c['sim'][0], probs[0][0]
        assert np.isnan(s).sum() == 2 and np.isposinf(s).sum() == 2 and np.isneginf(s).sum() == 2
        assert not W[~np.isfinite(s) & ~np.isposinf(s)].any() and (W[np.isposinf(s)] == 1 << 20).all()
        assert sum(1 for r, col in probs[0][2].items() if np.isposinf(s[r, col])) == 2
    if 'clamp' in tags:
        assert (probs[0][0] == 1 << 20).sum() >= 4 and (probs[0][0] < 1 << 20).any()
    if 'counts' in tags:
        got = [C.shape(c, b) for b in range(c['sim'].shape[0])]
        assert got == [(3, 4), (0, 2), (5, 0), (8, 6), (0, 3), (8, 6)] and [len(m) for _, _, m in probs] == [3, 0, 0, 6, 0, 6]
    if 'batch' in tags:
        assert probs[1][1] == 0 and probs[0][1] > 0 and A.second_best(probs[2][0]) == probs[2][1] and not probs[3][0][5].any()
        assert C.shape(c, 4) == (1, 20) and len(probs[4][2]) == 1
    if 'chain' in tags:
        W, total, match = probs[0]
        n = C.CHAIN
        assert n >= 100 and match == {2 * j: j for j in range(n)}
        _, before = A.solve(W[:, :n - 1])                                           # without the last column: everyone one row further
        assert before == {2 * (j + 1): j for j in range(n - 1)}
        assert all(r != 2 * j for r, j in before.items())                           # every other column changes its partner
        assert len({r // 64 for r in match}) == 4                                   # the rewired path crosses all four waves


# ------------------------------------------------------------------------------------------------ the binding
def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'effdet_assign.h')).read(), flags=re.S)


def _prototypes():
    scalar = {'int': 'i', 'long long': 'q', 'float': 'f', 'double': 'd', 'effdet_stream_t': 'p'}
    protos = {}
    for r, name, params in re.findall(r'^([a-z][a-z ]*?\*?)\s*\b(effdet_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', _header(), flags=re.M):
        kinds = ['p' if '*' in p else scalar[' '.join(p.split()).rsplit(' ', 1)[0]] for p in params.split(',')]
        assert name not in protos, name
        protos[name] = ({'int': 'i', 'long long': 'q'}[' '.join(r.split())], kinds)
    return protos


def test_signatures_match_the_header():
    from efficientdet.pytorch_amd import build, _lib, ops
    protos = _prototypes()
    assert sorted(protos) == ['effdet_assign', 'effdet_track_step_assign']
    others = [getattr(_lib, n) for n in dir(_lib) if n.endswith('SIGNATURES') and n != 'ASSIGN_SIGNATURES']
    assert sorted(_lib.ASSIGN_SIGNATURES) == sorted(protos) and len(others) >= 17 and not any(set(protos) & set(t) for t in others)
    build.build(verbose=False)
    L = _lib.require(*protos)
    for name, (r, kinds) in protos.items():
        sig = _lib.ASSIGN_SIGNATURES[name]
        assert sig[1] == ':' and sig[0] == r and list(sig[2:].replace('s', 'p')) == kinds, (name, sig, r, kinds)
        f = getattr(L, name)
        assert f.restype is _lib._CTYPE[sig[0]] and list(f.argtypes) == [_lib._CTYPE[c] for c in sig[2:]], name
    # the new tracker entry is the old one plus `assignment` in front of the stream
    old, new = _lib.TRACK_SIGNATURES['effdet_track_step'], _lib.ASSIGN_SIGNATURES['effdet_track_step_assign']
    assert new == old[:-1] + 'i' + old[-1]
    for macro, value in (('MAX_ROWS', 256), ('MAX_COLS', 128), ('SCALE_BITS', 20)):
        assert getattr(_lib, 'ASSIGN_' + macro) == value == getattr(A, macro)
        assert int(re.search(r'#define\s+EFFDET_ASSIGN_%s\s+(\d+)' % macro, _header()).group(1)) == value
    assert (ops.ASSIGN_MAX_ROWS, ops.ASSIGN_MAX_COLS) == (256, 128)
    for i, word in enumerate(_lib.ASSIGNMENTS):
        assert int(re.search(r'#define\s+EFFDET_ASSIGN_%s\s+(\d+)' % word.upper(), _header()).group(1)) == i
    assert '-ffp-contract=off' in build.PER_FILE['assign.hip'] and _lib.ABI_VERSION == 11
    for h in ('effdet_hip.h', 'effdet_track.h'):
        text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', h)).read(), flags=re.S)
        assert not any(n in text for n in protos)                                  # additive: the older headers do not declare them
    csrc = os.path.join(ROOT, 'efficientdet', 'pytorch_amd', 'csrc')
    solver, op, track = (open(os.path.join(csrc, n)).read() for n in ('assign.h', 'assign.hip', 'track.hip'))
    assert 'assign_solve(' in solver and 'assign_solve(' in op and 'assign_solve(' in track      # one solver, two weight sources
    assert 'track_similarity(' in track[track.index('struct TrackWeight'):track.index('int track_optimal(')]       # recomputed, not stored
    assert callable(ops.linear_assignment)


def test_refusals_are_decided_on_the_host_and_launch_nothing():
    from efficientdet.pytorch_amd import build, _lib
    build.build(verbose=False)
    L = _lib.require(*_lib.ASSIGN_SIGNATURES)
    buf = np.zeros(1 << 16, dtype=np.uint8)
    p = buf.ctypes.data

    def assign(**kw):
        a = dict(sim=p, B=2, R=8, C=4, nr=None, nc=None, gate=0.2, r2c=p, c2r=p, total=p)
        a.update(kw)
        return L.effdet_assign(a['sim'], a['B'], a['R'], a['C'], a['nr'], a['nc'], a['gate'], a['r2c'], a['c2r'], a['total'], None)
    nan, inf = float('nan'), float('inf')
    for kw in (dict(R=257), dict(C=129)):
        assert assign(**kw) == -3, kw
    for kw in (dict(sim=None), dict(r2c=None), dict(c2r=None), dict(total=None), dict(B=0), dict(R=0), dict(C=0), dict(gate=nan),
               dict(gate=inf), dict(gate=-inf), dict(sim=None, R=257)):
        assert assign(**kw) == -1, kw

    def step(**kw):
        a = dict(d=p, n=p, B=2, D=8, s=p, T=8, tt=0.5, lt=0.1, nt=0.6, ms=0.2, ss=0.5, us=0.3, buf=30, fuse=1, ca=0, o1=p, o2=p, o3=p, how=1)
        a.update(kw)
        return L.effdet_track_step_assign(a['d'], a['n'], a['B'], a['D'], a['s'], a['T'], a['tt'], a['lt'], a['nt'], a['ms'], a['ss'], a['us'],
                                          a['buf'], a['fuse'], a['ca'], a['o1'], a['o2'], a['o3'], a['how'], None)
    for how in (0, 1):
        for kw in (dict(T=257), dict(D=129)):
            assert step(how=how, **kw) == -3, kw
        for kw in (dict(d=None), dict(n=None), dict(s=None), dict(o1=None), dict(o2=None), dict(o3=None), dict(B=0), dict(D=0), dict(T=0),
                   dict(tt=nan), dict(lt=-inf), dict(nt=inf), dict(ms=-0.1), dict(ms=1.5), dict(ss=nan), dict(us=2.0), dict(lt=0.6), dict(buf=-1)):
            assert step(how=how, **kw) == -1, kw
    for how in (-1, 2, 7):
        assert step(how=how) == -1 and step(how=how, T=257) == -1
    assert not buf.any()


def test_the_assignment_option():
    from efficientdet.pytorch_amd import ops
    o, g, x = ops.TrackOptions(), ops.TrackOptions(assignment='greedy'), ops.TrackOptions(assignment='optimal')
    ten = (0.5, 0.1, float(np.float32(np.float32(0.5) + np.float32(0.1))), 0.2, 0.5, 0.3, 30, True, False, 128)
    assert o.assignment == 'greedy' and o.key() == g.key() == ten and o == g and hash(o) == hash(g)
    assert x.assignment == 'optimal' and x.key() == ten + ('optimal',) and x != o
    assert 'assignment' not in repr(o) and 'track_thr=0.5' in repr(o) and repr(x) == repr(o)[:-1] + ", assignment='optimal')"
    for bad in ('lapjv', 'Greedy', None, 0, 1, True, ''):
        with pytest.raises(ValueError):
            ops.TrackOptions(assignment=bad)
    with pytest.raises(ValueError):
        ops.TrackOptions(assignment='optimal', match_sim=1.5)                      # the other rules still hold
    from efficientdet.pytorch_amd.evaluate import TrackedDetector

    class _Model:
        num_classes = 3
        def forward_raw(self, x): raise AssertionError
        def eval(self): pass
        def train(self, mode=True): pass
        def parameters(self): return iter(())
    assert TrackedDetector(_Model(), options=x).options.assignment == 'optimal' and TrackedDetector(_Model()).options.assignment == 'greedy'
