"""CPU tier of the tracker with assignment='optimal': what the scenes of tests/track_lap_cases.py reach in the restatement
(tests/track_lap_restated.py), where they part from the greedy restatement (tests/track_restated.py), and that every association of
every frame has ONE optimum by a margin the device's arithmetic cannot bridge -- so that the GPU tier may ask for the float64
matching exactly."""
import numpy as np
import pytest

from tests import track_restated as R
from tests import track_lap_restated as LR
from tests import track_lap_cases as C

_RUNS = {}


def _run(name, dtype=np.float64, stream=LR.Stream):
    """(frames, streams, trace) of a scene, computed once and shared"""
    k = (name, np.dtype(dtype).name, stream.__module__)
    if k not in _RUNS:
        tr = LR.LapTrace()
        frames, streams = LR.run(C.case(name), dtype, R.Full, tr, stream)
        _RUNS[k] = (frames, streams, tr)
    return _RUNS[k]


def _differs(name):
    """frames on which the optimal and the greedy restatement show different ids (or different numbers of them)"""
    return [f for f, (a, b) in enumerate(zip(_run(name)[0], _run(name, stream=R.Stream)[0]))
            if any(not np.array_equal(x, y) for x, y in zip(a[1], b[1]))]


def test_the_case_list_and_its_sizes():
    assert C.NAMES == ('crossing', 'three_cross', 'crowd6', 'crowd', 'classes_on', 'classes_off', 'fuse_on', 'fuse_off', 'refound', 'cap', 'agree')
    for n in C.NAMES:
        c = C.case(n)
        F, B, D, _ = c['dets'].shape
        if n == 'cap':
            assert (c['options'].max_tracks, D, F) == (R.MAX_TRACKS, R.MAX_DET, 3) and np.all(c['counts'] == D)
        else:
            assert B == 1 and 8 <= c['options'].max_tracks <= 16 and D <= 12 and 6 <= F <= 12, n
        assert all(R.valid_row(r) for f in range(F) for r in c['dets'][f, 0, :c['counts'][f, 0]])
        assert c['dets'][..., :4].min() >= 0 and c['dets'][..., :4].max() <= 512, n


def test_at_least_five_scenes_part_from_the_greedy_rule():
    parted = [n for n in C.NAMES if _differs(n)]
    print('scenes whose ids differ from the greedy restatement:', {n: _differs(n)[:3] for n in parted})
    assert parted == [n for n in C.NAMES if 'differs' in C.case(n)['tags']] and len(parted) >= 5
    assert not _differs('agree') and 'agrees' in C.case('agree')['tags']


def test_the_scenes_reach_what_they_are_tagged_with():
    # the pair on the frame of its move: the four similarities of the docstring, the crossed matching, both ids kept
    tr = _run('crossing')[2]
    assert all(any(abs(s - v) < 1e-3 for s in tr.sims) for v in (0.778, 0.667, 0.311))
    assert [list(f[1][0]) for f in _run('crossing')[0]] == [[1, 2]] * 10
    g = [list(f[1][0]) for f in _run('crossing', stream=R.Stream)[0]]
    assert g[4] == [1, 2] and g[5] == [1] and 3 in g[-1] and 2 not in g[-1]          # greedy: track 2 lost, a duplicate id started
    assert [list(f[1][0]) for f in _run('three_cross')[0]] == [[1, 2, 3]] * 10 and _run('three_cross')[2].picks[1] == 3
    assert [list(f[1][0]) for f in _run('crowd6')[0]][-1] == [1, 2, 3, 4, 5, 6] and _run('crowd6')[2].picks[1] == 6
    # crowd: the second and the third association each decide a crossed pair on frame 7
    tr = _run('crowd')[2]
    assert {w for w, n, _ in tr.gaps if n == 2} == {1, 2, 3} and tr.picks[2] == 2 and tr.picks[3] == 2
    ids = [list(f[1][0]) for f in _run('crowd')[0]]
    assert ids[5] == [1, 2] and ids[6] == [1, 2, 3, 4] and ids[-1] == [1, 2, 3, 4]
    gt = _run('crowd', stream=R.Stream)[2]
    assert gt.picks[2] == 1 and gt.picks[3] == 1                                      # greedy strands one row in each
    # class awareness and score fusion, on and off
    assert _run('classes_on')[2].hits['class_gate_fail'] > 0 and _run('classes_on')[2].hits['class_gate_pass'] > 0
    assert 'class_gate_fail' not in _run('classes_off')[2].hits
    on, off = _run('classes_on')[0], _run('classes_off')[0]
    assert np.array_equal(C.case('classes_on')['dets'], C.case('classes_off')['dets'])
    assert [list(f[1][0]) for f in on] == [list(f[1][0]) for f in off] == [[1, 2]] * 10
    assert list(on[5][0][0][:, 5]) == [1, 2] and list(off[5][0][0][:, 5]) == [1, 2]   # either way track 1 takes the detection labelled 1
    fon, foff = _run('fuse_on')[0], _run('fuse_off')[0]
    assert np.array_equal(C.case('fuse_on')['dets'], C.case('fuse_off')['dets'])
    assert list(fon[5][1][0]) == [1] and list(foff[5][1][0]) == [1, 2]               # fused, (0, 0) alone is the optimum
    # the lost track is re-found only by the optimum
    assert _run('refound')[2].hits.get('refound', 0) == 1 and 'refound' not in _run('refound', stream=R.Stream)[2].hits
    ids = [list(f[1][0]) for f in _run('refound')[0]]
    assert ids[3] == [1, 2] and ids[5] == [1] and ids[7] == [1, 2] and _run('refound')[0][7][0][0][1, 6] == 0      # tracklet_len restarts
    # the caps: 128 rows, 64 components of two on the frame of the move
    tr = _run('cap')[2]
    assert tr.picks[1] == 128 and len(_run('cap')[0][2][1][0]) == 128 and max(n for _, n, _ in tr.gaps) == 128
    assert len(_run('cap', stream=R.Stream)[0][2][1][0]) == 64


@pytest.mark.parametrize('name', C.NAMES)
def test_every_association_has_one_optimum_by_more_than_the_device_can_bridge(name):
    """optimum - second best > 2 * 2n * (delta + 2^-20) in similarity units: a matching has at most n pairs, the device's weight of a
    pair differs from the float64 sim - gate by at most delta (the fp32 similarity) + 2^-21 (the grid) + 2^-24 (the fp32 subtraction),
    so two matchings' totals move against each other by less than 2n * (delta + 2^-20): twice that is asked for."""
    f64, f32 = _run(name), _run(name, np.float32)
    assert all(np.array_equal(a, b) for x, y in zip(f64[0], f32[0]) for a, b in zip(x[1], y[1])), name       # the same decisions
    a, b = np.array(f64[2].sims), np.array(f32[2].sims)
    assert a.shape == b.shape and len(a) > 0
    delta = float(np.abs(a - b).max())
    assert f64[2].gaps
    worst = min(g / (2 * 2 * n * (delta + 2.0 ** -20)) for _, n, g in f64[2].gaps)
    print('%s: delta %.3g, smallest optimum - second best %.4g, smallest ratio to its bound %.4g'
          % (name, delta, min(g for _, _, g in f64[2].gaps), worst))
    assert all(g > 2 * 2 * n * (delta + 2.0 ** -20) for _, n, g in f64[2].gaps)


@pytest.mark.parametrize('name', C.NAMES)
def test_every_float64_decision_clears_its_alternative(name):
    kinds = {}
    for k, v in _run(name)[2].margins:
        kinds[k] = min(kinds.get(k, np.inf), v)
    print(name, {k: '%.4g' % v for k, v in kinds.items()})
    assert {'track_thr', 'low_thr', 'new_thr', 'sim_gate'} <= set(kinds) and 'pick' not in kinds
    assert all(v >= 16 * C.EPS_SIM for v in kinds.values()), kinds


def test_eps_sim_is_the_recorded_float32_error():
    worst = 0.0
    for n in C.NAMES:
        a, b = np.array(_run(n)[2].values), np.array(_run(n, np.float32)[2].values)
        assert a.shape == b.shape and len(a) > 0, n
        worst = max(worst, float(np.abs(a - b).max()))
    print('eps_sim measured %.4g, recorded %.4g' % (worst, C.EPS_SIM))
    assert C.EPS_SIM / 2 <= worst <= C.EPS_SIM
