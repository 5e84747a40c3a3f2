"""Seeded similarity matrices for the optimal assignment (include/effdet_assign.h).  A case is a dict: name, sim [B, R, C] float32, gate,
n_rows / n_cols (int32 [B] or None), tags (what tests/test_assign_host.py proves the case reaches; 'unique' = every problem of the case
has exactly one optimal matching, so the device must return that very matching)."""
import numpy as np

from tests import assign_restated as A


def _case(name, sim, gate, tags, n_rows=None, n_cols=None):
    sim = np.asarray(sim, dtype=np.float32)
    sim = sim[None] if sim.ndim == 2 else sim
    i32 = lambda v: None if v is None else np.asarray(v, dtype=np.int32)
    return dict(name=name, sim=np.ascontiguousarray(sim), gate=float(gate), n_rows=i32(n_rows), n_cols=i32(n_cols), tags=tuple(tags))


def _uniform(seed, R, C, B=None):
    shape = (R, C) if B is None else (B, R, C)
    return np.random.RandomState(seed).uniform(0.0, 1.0, shape).astype(np.float32)


def one_by_one():
    return _case('one_by_one', [[0.7]], 0.2, ('unique',))


def one_row():
    return _case('one_row', _uniform(1, 1, 9), 0.3, ('unique',))


def one_col():
    return _case('one_col', _uniform(2, 11, 1), 0.3, ('unique',))


def tall():
    return _case('tall', _uniform(3, 13, 5), 0.25, ('unique',))


def wide():
    return _case('wide', _uniform(4, 5, 13), 0.25, ('unique',))


def three():
    return _case('three', _uniform(5, 3, 3), 0.1, ('unique',))


def example():
    """The header's two-by-two: greedy takes (0, 0) and strands row 1; the optimum is (0, 1), (1, 0)."""
    return _case('example', [[0.90, 0.80], [0.85, 0.10]], 0.2, ('unique', 'greedy_differs'))


def waves65():
    """65 rows: the second wave holds one row, and it is the best partner of column 3"""
    sim = _uniform(6, 65, 24)
    sim[64, 3] = 0.9995
    return _case('waves65', sim, 0.3, ('unique', 'waves'))


def waves200():
    return _case('waves200', _uniform(7, 200, 40), 0.5, ('unique', 'waves'))


def cap_dense():
    """The caps, every pair admissible"""
    return _case('cap_dense', _uniform(8, A.MAX_ROWS, A.MAX_COLS), 0.0, ('cap',))


def nothing():
    return _case('nothing', 0.5 * _uniform(9, 7, 6), 0.5, ('nothing',))


def ties():
    return _case('ties', np.full((5, 3), 0.75), 0.25, ('ties',))


def gate_edge():
    """Every sim equal to the gate (refused) except the diagonal, one ulp above it (weight 1)"""
    g = np.float32(0.5)
    sim = np.full((4, 4), g, dtype=np.float32)
    sim[np.arange(4), np.arange(4)] = np.nextafter(g, np.float32(1))
    return _case('gate_edge', sim, g, ('unique', 'gate_edge'))


def nonfinite():
    nan, inf = float('nan'), float('inf')
    sim = _uniform(10, 6, 6)
    sim[0, 1], sim[2, 2], sim[3, 0], sim[4, 4], sim[5, 3], sim[1, 5] = nan, inf, -inf, nan, inf, -inf
    return _case('nonfinite', sim, 0.2, ('unique', 'nonfinite'))


def clamp():
    """sim - gate above 1: the weight saturates at 2^20"""
    return _case('clamp', _uniform(11, 6, 4), -0.5, ('clamp',))


def counts():
    """Counts below R and C, zero included, a negative one and one above the size (both clamped)"""
    return _case('counts', _uniform(12, 8, 6, B=6), 0.2, ('unique', 'counts'), n_rows=[3, 0, 5, 8, -2, 99], n_cols=[4, 2, 0, 6, 3, 99])


def batch():
    """One launch mixing problem kinds: dense, nothing admissible, all ties, a NaN row, short counts"""
    sim = _uniform(13, 70, 20, B=5)
    sim[1] *= 0.1
    sim[2] = 0.6
    sim[3, 5] = float('nan')
    return _case('batch', sim, 0.3, ('batch', 'waves'), n_rows=[70, 70, 12, 66, 1], n_cols=[20, 20, 7, 20, 20])


CHAIN = 104


def chain():
    """A path r0 - c0 - r1 - c1 - ... - r103 - c103 over rows spread across all four waves (row j sits at index 2 j).  Column j < 103
    prefers row j + 1 (0.9) to row j (0.895); the last column can only take row 103 (0.99).  Without it every column has its preferred
    row; with it every column moves down by one -- inserted last, it rewires all 104 pairs in ONE augmentation."""
    sim = np.zeros((2 * CHAIN, CHAIN), dtype=np.float32)
    for j in range(CHAIN):
        sim[2 * j, j] = 0.895
        if j + 1 < CHAIN:
            sim[2 * (j + 1), j] = 0.9
    sim[2 * (CHAIN - 1), CHAIN - 1] = 0.99
    return _case('chain', sim, 0.0, ('unique', 'chain', 'waves'))


BUILDERS = (one_by_one, one_row, one_col, tall, wide, three, example, waves65, waves200, cap_dense, nothing, ties, gate_edge, nonfinite,
            clamp, counts, batch, chain)
NAMES = tuple(b.__name__ for b in BUILDERS)
_CACHE, _SOLVED = {}, {}


def case(name):
    if name not in _CACHE:
        _CACHE[name] = {b.__name__: b for b in BUILDERS}[name]()
    return _CACHE[name]


def shape(c, b):
    """-> (nr, nc): the rows and columns of problem b that take part"""
    _, R, C = c['sim'].shape
    nr = R if c['n_rows'] is None else min(max(int(c['n_rows'][b]), 0), R)
    nc = C if c['n_cols'] is None else min(max(int(c['n_cols'][b]), 0), C)
    return nr, nc


def problems(name):
    """-> per problem of the case: (W [nr, nc] int64, total, {row: col}) from the restatement, computed once"""
    if name not in _SOLVED:
        c, out = case(name), []
        for b in range(c['sim'].shape[0]):
            nr, nc = shape(c, b)
            W = A.weights(c['sim'][b, :nr, :nc], c['gate'])
            out.append((W,) + A.solve(W))
        _SOLVED[name] = out
    return _SOLVED[name]
