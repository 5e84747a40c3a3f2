"""GPU tier of the optimal assignment op (csrc/assign.hip, ops.linear_assignment) against the integer restatement
tests/assign_restated.py on the cases of tests/assign_cases.py.  Weights are integers, so everything here is an equality: the total is
the restated optimum, the returned matching is valid and sums to that total, and where the optimum is unique (proved on the CPU tier) it
is the restatement's matching."""
import numpy as np
import pytest
import torch

from tests import assign_restated as A
from tests import assign_cases as C

pytestmark = pytest.mark.gpu

GUARD, FILL = 256, 0xA5
_GOT = {}


def _guarded(nbytes):
    whole = torch.full((nbytes + 2 * GUARD,), FILL, dtype=torch.uint8, device='cuda')
    return whole, whole[GUARD:GUARD + nbytes]


def _run(name):
    """One launch of the case into sentinel-filled outputs between guards -> dict(r2c, c2r, total numpy, guards bool)"""
    from efficientdet.pytorch_amd import ops
    c = C.case(name)
    B, R, Cn = c['sim'].shape
    sim = torch.from_numpy(c['sim']).cuda()
    nr = None if c['n_rows'] is None else torch.from_numpy(c['n_rows']).cuda()
    nc = None if c['n_cols'] is None else torch.from_numpy(c['n_cols']).cuda()
    bufs = [_guarded(n) for n in (B * R * 4, B * Cn * 4, B * 8)]
    out = (bufs[0][1].view(torch.int32).view(B, R), bufs[1][1].view(torch.int32).view(B, Cn), bufs[2][1].view(torch.int64))
    r2c, c2r, total = ops.linear_assignment(sim, c['gate'], nr, nc, out=out)
    assert r2c.data_ptr() == out[0].data_ptr() and total.data_ptr() == out[2].data_ptr()
    guards = all(bool((w[:GUARD] == FILL).all()) and bool((w[-GUARD:] == FILL).all()) for w, _ in bufs)
    return dict(r2c=r2c.cpu().numpy(), c2r=c2r.cpu().numpy(), total=total.cpu().numpy(), guards=guards)


def _got(name, run=0):
    if (name, run) not in _GOT:
        _GOT[(name, run)] = _run(name)
    return _GOT[(name, run)]


@pytest.mark.parametrize('name', C.NAMES)
def test_the_total_is_the_optimum_and_the_matching_is_valid(name):
    c, got = C.case(name), _got(name)
    assert got['guards']
    for b, (W, total, match) in enumerate(C.problems(name)):
        nr, nc = C.shape(c, b)
        r2c, c2r = got['r2c'][b], got['c2r'][b]
        assert np.all(r2c[nr:] == -1) and np.all(c2r[nc:] == -1), (name, b)          # -1 over the sentinel outside the counts
        assert np.all(r2c[:nr] < nc) and np.all(c2r[:nc] < nr), (name, b)
        summed = A.check_matching(W, r2c[:nr], c2r[:nc])                             # inverse maps, admissible pairs only
        print('%s[%d]: device total %d, matching sums to %d, restated optimum %d' % (name, b, int(got['total'][b]), summed, total))
        assert int(got['total'][b]) == total == summed, (name, b)
        if 'unique' in c['tags']:
            assert {r: int(r2c[r]) for r in range(nr) if r2c[r] >= 0} == match, (name, b)


@pytest.mark.parametrize('name', C.NAMES)
def test_two_runs_are_bit_equal(name):
    a, b = _got(name), _got(name, 1)
    assert all(np.array_equal(a[k], b[k]) for k in ('r2c', 'c2r', 'total'))


def test_a_two_dimensional_sim_is_a_batch_of_one():
    from efficientdet.pytorch_amd import ops
    c = C.case('tall')
    r2c, c2r, total = ops.linear_assignment(torch.from_numpy(c['sim'][0]).cuda(), c['gate'])
    assert r2c.shape == (13,) and c2r.shape == (5,) and total.shape == () and total.dtype == torch.int64 and r2c.dtype == torch.int32
    got = _got('tall')
    assert np.array_equal(r2c.cpu().numpy(), got['r2c'][0]) and np.array_equal(c2r.cpu().numpy(), got['c2r'][0]) and int(total) == int(got['total'][0])


def test_a_captured_call_replays_the_eager_one():
    from efficientdet.pytorch_amd import ops
    names = ('waves65', 'chain')
    for name in names:
        c = C.case(name)
        sim = torch.from_numpy(c['sim']).cuda()
        static = torch.zeros_like(sim)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            out = ops.linear_assignment(static, c['gate'])
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            ops.linear_assignment(static, c['gate'], out=out)
        static.copy_(sim)
        for t in out:
            t.fill_(-7)
        graph.replay()
        eager = _got(name)
        assert all(np.array_equal(t.cpu().numpy(), eager[k]) for t, k in zip(out, ('r2c', 'c2r', 'total'))), name


def test_the_python_layer_refuses_before_a_launch():
    from efficientdet.pytorch_amd import ops
    sim = torch.zeros((2, 4, 3), device='cuda')
    for bad in (torch.zeros((2, 257, 3), device='cuda'), torch.zeros((2, 4, 129), device='cuda'), torch.zeros(4, device='cuda'),
                torch.zeros((1, 2, 4, 3), device='cuda'), torch.zeros((2, 0, 3), device='cuda')):
        with pytest.raises(ValueError):
            ops.linear_assignment(bad)
    for gate in (float('nan'), float('inf')):
        with pytest.raises(ValueError):
            ops.linear_assignment(sim, gate)
    with pytest.raises(AssertionError):
        ops.linear_assignment(sim.double())
    with pytest.raises(AssertionError):
        ops.linear_assignment(sim, n_rows=torch.zeros(3, dtype=torch.int32, device='cuda'))
