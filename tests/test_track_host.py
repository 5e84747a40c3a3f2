"""CPU tier of the tracker (include/effdet_track.h, csrc/track.hip, ops.track_step, evaluate.TrackedDetector): what the cases of
tests/track_cases.py reach in the NumPy restatement (tests/track_restated.py), the float32 error of the rule (EPS_SIM) and the distance
of every float64 decision from its alternative, the block-form Kalman filter against the full 8 x 8 one, the binding's table against
the header, the options' validator and the refusals the entry points decide on the host."""
import os
import re

import numpy as np
import pytest

from tests import track_restated as R
from tests import track_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_RUNS = {}


def _run(name, dtype=np.float64, filt=R.Full):
    """(frames, streams, trace) of a case, computed once and shared"""
    k = (name, np.dtype(dtype).name, filt.__name__)
    if k not in _RUNS:
        tr = R.Trace()
        frames, streams = R.run(C.case(name), dtype, filt, tr)
        _RUNS[k] = (frames, streams, tr)
    return _RUNS[k]


def _ids(name, b=0):
    return [list(f[1][b]) for f in _run(name)[0]]


def _lens(name, b=0):
    return [[int(v) for v in f[0][b][:, 6]] for f in _run(name)[0]]


# ------------------------------------------------------------------------------------------------ what the cases reach
def test_the_case_list_and_its_sizes():
    assert C.NAMES == ('crossing', 'gap_short', 'gap_long', 'dip', 'false_positive', 'overflow', 'classes_on', 'classes_off', 'fuse_on',
                       'fuse_off', 'duplicate_tracked_older', 'duplicate_tracked_younger', 'duplicate_equal_age', 'tie', 'resets',
                       'skipped', 'cap')
    for n in C.NAMES:
        c = C.case(n)
        F, B, D, _ = c['dets'].shape
        if n == 'cap':
            assert (c['options'].max_tracks, D, F) == (R.MAX_TRACKS, R.MAX_DET, 2) and np.all(c['counts'] == D)
            assert all(R.valid_row(r) for r in c['dets'].reshape(-1, 6))
        else:
            assert B <= 3 and 8 <= c['options'].max_tracks <= 16 and D <= 12 and 6 <= F <= 40, n
        ok = c['dets'][..., :4][np.isfinite(c['dets'][..., :4])]
        assert ok.min() >= 0 and ok.max() <= 512, n


def test_every_step_every_gate_and_two_picks_per_association_are_reached():
    hits, picks = {}, {1: 0, 2: 0, 3: 0}
    for n in C.NAMES:
        tr = _run(n)[2]
        for k, v in tr.hits.items():
            hits[k] = hits.get(k, 0) + v
        for k in picks:
            picks[k] = max(picks[k], tr.picks[k])
    assert all(hits.get('step%d' % i, 0) > 0 for i in range(1, 11)), hits
    assert all(p >= 2 for p in picks.values()), picks
    for a in (1, 2, 3):
        assert hits['assoc%d_allowed' % a] > 0 and hits['assoc%d_refused' % a] > 0
    for k in ('class_gate_pass', 'class_gate_fail', 'det_high', 'det_low', 'det_ignored', 'row_skipped', 'predict_1', 'predict_2', 'predict_3',
              'lost_vh_zero', 'refound', 'tracked_updated', 'second_updated', 'tracked_to_lost', 'unconfirmed_activated',
              'unconfirmed_removed', 'new_activated', 'new_unconfirmed', 'new_dropped', 'new_refused', 'lost_removed', 'lost_kept', 'dup_lost_removed',
              'dup_tracked_removed', 'dup_equal_age', 'dup_refused'):
        assert hits.get(k, 0) > 0, k


def test_crossing_ids_survive_and_a_stream_without_detections_stays_empty():
    c = C.case('crossing')
    assert _ids('crossing') == [[1, 2]] * 30 and all(i == [] for i in _ids('crossing', 1)) and not c['counts'][:, 1].any()
    f = 15                                                                         # the paths do cross: the two boxes overlap there
    assert R.iou(c['dets'][f, 0, 0, :4], c['dets'][f, 0, 1, :4], np.float64) > 0.3
    assert c['dets'][0, 0, 0, 0] < c['dets'][0, 0, 1, 0] and c['dets'][29, 0, 0, 0] > c['dets'][29, 0, 1, 0]
    assert _lens('crossing')[0] == [0, 0] and _lens('crossing')[29] == [29, 29]    # frame 1: both activated at once


def test_a_short_gap_comes_back_with_its_id_and_a_lone_low_detection_starts_nothing():
    ids, lens = _ids('gap_short'), _lens('gap_short')
    assert ids[5] == [1, 2] and all(ids[f] == [2] for f in range(6, 11)) and ids[11] == [1, 2]
    assert lens[5][0] == 5 and lens[11][0] == 0 and lens[12][0] == 1
    assert all(i == [] for i in _ids('gap_short', 1)) and _run('gap_short')[2].hits['det_low'] == 16
    assert all(s.next_id == n for s, n in zip(_run('gap_short')[1], (3, 1)))


def test_a_long_gap_ends_the_track_and_a_new_id_is_issued():
    ids = _ids('gap_long')
    assert ids[4] == [1, 2] and all(ids[f] == [2] for f in range(5, 14)) and ids[14] == [2, 3] and ids[19] == [2, 3]
    assert ids[13] == [2]                                                           # the returning object is unconfirmed for a frame
    assert _run('gap_long')[2].hits['lost_removed'] == 1


def test_a_dipping_score_keeps_its_id_through_the_second_association():
    ids, lens = _ids('dip'), _lens('dip')
    assert all(ids[f] == [1, 2] for f in range(5, 8)) and ids[4] == ids[8] == [1, 2, 3]
    assert lens[7] == [7, 7] and lens[8] == [8, 8, 0]
    tr = _run('dip')[2]
    assert tr.hits['second_updated'] == 6 and tr.picks[2] == 2 and tr.hits['det_ignored'] == 3


def test_a_one_frame_false_positive_is_never_output():
    ids = _ids('false_positive')
    assert ids[:6] == [[1]] * 6 and ids[6] == [1, 3, 4] and _run('false_positive')[2].hits['unconfirmed_removed'] == 1
    assert not any(2 in i for i in ids) and _run('false_positive')[2].picks[3] == 2


def test_overflow_drops_in_row_order_and_a_freed_slot_is_reused():
    frames = _run('overflow')[0]
    assert list(frames[0][1][0]) == list(range(1, 9)) and frames[0][2] == [4]
    c = C.case('overflow')
    assert np.array_equal(frames[0][0][0][:, 4], c['dets'][0, 0, :8, 4])           # the first eight rows got the slots
    over = [f[2][0] for f in frames]
    assert over == [4, 8, 12, 16, 20, 23, 26, 29, 32]                              # the slot freed on frame 5 takes one of the four after it
    assert 9 in frames[6][1][0] and 9 not in frames[5][1][0] and 3 not in frames[5][1][0] and len(frames[8][1][0]) == 8


def test_class_awareness_and_score_fusion_change_the_outcome():
    on, off = _run('classes_on')[0], _run('classes_off')[0]
    assert np.array_equal(C.case('classes_on')['dets'], C.case('classes_off')['dets'])
    assert on[4][0][0][0, 5] == 1 and off[4][0][0][0, 5] == 2 and list(on[4][1][0]) == list(off[4][1][0]) == [1]
    fon, foff = _run('fuse_on')[0], _run('fuse_off')[0]
    assert np.array_equal(C.case('fuse_on')['dets'], C.case('fuse_off')['dets'])
    assert fon[3][0][0][0, 4] == np.float32(0.95) and foff[3][0][0][0, 4] == np.float32(0.55)
    # fuse_on's leftover row (high, unmatched, 0.55 < new_thr) starts nothing: the new_thr gate's other outcome
    assert _run('fuse_on')[2].hits['new_refused'] == 3 and list(fon[5][1][0]) == [1] and _run('fuse_on')[1][0].next_id == 2


def test_duplicates_on_each_side_of_the_age_comparison():
    assert C.case('duplicate_tracked_older')['tags'] == ('dup_lost_removed',) and _run('duplicate_tracked_older')[2].hits['dup_lost_removed'] == 1
    assert 'dup_tracked_removed' not in _run('duplicate_tracked_older')[2].hits and 'dup_equal_age' not in _run('duplicate_tracked_older')[2].hits
    assert _run('duplicate_tracked_younger')[2].hits['dup_tracked_removed'] == 1 and 'dup_lost_removed' not in _run('duplicate_tracked_younger')[2].hits
    assert _run('duplicate_equal_age')[2].hits['dup_equal_age'] == 1 and 'dup_lost_removed' not in _run('duplicate_equal_age')[2].hits
    assert _ids('duplicate_tracked_older')[12] == [1] and _ids('duplicate_tracked_younger')[15] == [] and _ids('duplicate_equal_age')[12] == []


def test_the_exact_tie_goes_to_the_lower_row_and_the_lower_slot():
    c = C.case('tie')
    assert c['tie'] and np.array_equal(c['dets'][1, 0, 0], c['dets'][1, 0, 1]) and list(c['counts'][:, 0]) == [2, 2, 2, 0, 2, 2, 0, 2]
    tr = _run('tie')[2]
    assert sum(1 for k, v in tr.margins if k == 'pick' and v == 0.0) >= 5
    ids = _ids('tie')
    assert ids[2] == [1, 2] and ids[3] == [] and ids[4] == [1, 2]
    s = _run('tie')[1][0]
    assert [k.id for k in s.slots[:2]] == [1, 2] and np.array_equal(s.slots[0].mean, s.slots[1].mean)


def test_resets_and_skipped_rows():
    ids = [[list(f[1][b]) for b in range(3)] for f in _run('resets')[0]]
    assert ids[4] == [[1, 2]] * 3 and ids[5] == [[1, 2]] * 3 and _lens('resets', 0)[5] == [0, 0] and _lens('resets', 1)[5] == [5, 5]
    assert _lens('resets', 2)[9] == [0, 0] and _lens('resets', 1)[9] == [9, 9] and C.case('resets')['resets'] == {5: (0,), 9: (2,)}
    assert _run('skipped')[2].hits['row_skipped'] == 5 * 6 and _ids('skipped') == [[1, 2]] * 6


# ------------------------------------------------------------------------------------------------ precision
def test_eps_sim_is_the_recorded_float32_error():
    worst = 0.0
    for n in C.NAMES:
        f64, f32 = _run(n), _run(n, np.float32)
        assert all(np.array_equal(a, b) for x, y in zip(f64[0], f32[0]) for a, b in zip(x[1], y[1])), n        # the same decisions
        a, b = np.array(f64[2].values), np.array(f32[2].values)
        assert a.shape == b.shape and len(a) > 0, n
        worst = max(worst, float(np.abs(a - b).max()))
    print('eps_sim measured %.4g, recorded %.4g' % (worst, C.EPS_SIM))
    assert C.EPS_SIM / 2 <= worst <= C.EPS_SIM


def test_eps_cov_is_the_recorded_float32_error_of_the_stored_covariances():
    worst = 0.0
    for n in C.NAMES:
        for s64, s32 in zip(_run(n)[1], _run(n, np.float32)[1]):
            for a, b in zip(s64.slots, s32.slots):
                assert a.state == b.state
                if a.state == R.FREE:
                    continue
                x, y = R.Full.numbers(a.cov), R.Full.numbers(b.cov).astype(np.float64)
                zero = x == 0
                assert not y[zero].any() and (x[~zero] > 0).all()
                worst = max(worst, float((np.abs(x - y)[~zero] / x[~zero]).max(initial=0.0)))
    print('eps_cov measured %.4g, recorded %.4g' % (worst, C.EPS_COV))
    assert C.EPS_COV / 2 <= worst <= C.EPS_COV


@pytest.mark.parametrize('name', C.NAMES)
def test_every_float64_decision_clears_its_alternative(name):
    tr = _run(name)[2]
    kinds = {}
    for k, v in tr.margins:
        if C.case(name)['tie'] and k == 'pick' and v == 0.0:
            continue                                                               # the deliberate exact ties
        kinds[k] = min(kinds.get(k, np.inf), v)
    print(name, {k: '%.4g' % v for k, v in kinds.items()})
    assert {'track_thr', 'low_thr', 'new_thr', 'sim_gate'} <= set(kinds)
    assert all(v >= 16 * C.EPS_SIM for v in kinds.values()), kinds
    if not C.case(name)['tie']:
        assert all(v > 0 for k, v in tr.margins if k == 'pick')


def test_the_margins_cover_every_kind_of_decision():
    seen = {k for n in C.NAMES for k, _ in _run(n)[2].margins}
    assert seen == {'sim_gate', 'track_thr', 'low_thr', 'new_thr', 'dup_gate', 'pick'}


@pytest.mark.parametrize('name', C.NAMES)
def test_the_block_form_equals_the_full_filter(name):
    full, block = _run(name), _run(name, np.float64, R.Block)
    for x, y in zip(full[0], block[0]):
        for a, b in zip(x[1], y[1]):
            assert np.array_equal(a, b)
        for a, b in zip(x[0], y[0]):
            assert np.allclose(a, b, rtol=1e-9, atol=0)
    for sf, sb in zip(full[1], block[1]):
        for kf, kb in zip(sf.slots, sb.slots):
            assert kf.state == kb.state
            if kf.state != R.FREE:
                assert np.allclose(kf.mean, kb.mean, rtol=1e-9, atol=1e-12)
                assert np.allclose(R.Full.numbers(kf.cov), R.Block.numbers(kb.cov), rtol=1e-9, atol=0)
                off = kf.cov.copy()                                                # and the 8 x 8 never grew another term
                for i in range(4):
                    off[i, i] = off[4 + i, 4 + i] = off[i, 4 + i] = off[4 + i, i] = 0
                assert np.abs(off).max() <= 1e-9 * np.abs(kf.cov).max()


# ------------------------------------------------------------------------------------------------ the binding
def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'effdet_track.h')).read(), flags=re.S)


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
    assert sorted(protos) == ['effdet_track_overflow', 'effdet_track_reset', 'effdet_track_state_bytes', 'effdet_track_step']
    others = [getattr(_lib, n) for n in dir(_lib) if n.endswith('SIGNATURES') and n != 'TRACK_SIGNATURES']
    assert sorted(_lib.TRACK_SIGNATURES) == sorted(protos) and len(others) >= 16 and not any(set(protos) & set(t) for t in others)
    build.build(verbose=False)
    L = _lib.require(*protos)
    for name, (r, kinds) in protos.items():
        sig = _lib.TRACK_SIGNATURES[name]
        assert sig[1] == ':' and sig[0] == r and list(sig[2:].replace('s', 'p')) == kinds, (name, sig, r, kinds)
        f = getattr(L, name)
        assert f.restype is _lib._CTYPE[sig[0]] and list(f.argtypes) == [_lib._CTYPE[c] for c in sig[2:]], name
    for macro, value in (('MAX_TRACKS', 256), ('MAX_DET', 128), ('ROW_WORDS', 28)):
        assert getattr(_lib, 'TRACK_' + macro) == getattr(ops, 'TRACK_' + macro) == value
        assert int(re.search(r'#define\s+EFFDET_TRACK_%s\s+(\d+)' % macro, _header()).group(1)) == value
    assert (R.MAX_TRACKS, R.MAX_DET, R.ROW_WORDS) == (256, 128, 28)
    assert '-ffp-contract=off' in build.PER_FILE['track.hip'] and _lib.ABI_VERSION == 11
    main = open(os.path.join(ROOT, 'include', 'effdet_hip.h')).read()
    assert not any(n in main for n in protos)                                      # additive: the main header does not know them
    src = open(os.path.join(ROOT, 'efficientdet', 'pytorch_amd', 'csrc', 'track.hip')).read()
    assert 'track_similarity(' in src and 'track_greedy(' in src                   # the two stages are separate device functions
    assert src.count('atomic') == 1 and 'No atomics of any kind' in src            # winners by integer max on packed keys, nothing else
    assert all(callable(getattr(ops, n)) for n in ('track_state', 'track_reset', 'track_step', 'track_overflow', 'TrackOptions'))


def test_the_options_validator():
    from efficientdet.pytorch_amd import ops
    o = ops.TrackOptions()
    assert o.key() == (0.5, 0.1, float(np.float32(np.float32(0.5) + np.float32(0.1))), 0.2, 0.5, 0.3, 30, True, False, 128)
    r = R.Options()
    assert (float(r.new_thr), r.track_buffer, r.max_tracks) == (o.new_thr, o.track_buffer, o.max_tracks)
    assert ops.TrackOptions(new_thr=0.7).new_thr == 0.7 and ops.TrackOptions() == ops.TrackOptions() and 'track_thr=0.5' in repr(o)
    nan, inf = float('nan'), float('inf')
    for kw in (dict(track_thr=nan), dict(low_thr=inf), dict(new_thr=nan), dict(low_thr=0.6), dict(match_sim=-0.1), dict(match_sim=1.5),
               dict(second_sim=nan), dict(unconfirmed_sim=2), dict(track_buffer=-1), dict(track_buffer=1.5), dict(max_tracks=0),
               dict(max_tracks=257), dict(max_tracks=8.5), dict(track_buffer=inf), dict(track_buffer=nan), dict(max_tracks=inf),
               dict(max_tracks=nan), dict(track_buffer=2 ** 31)):
        with pytest.raises(ValueError):
            ops.TrackOptions(**kw)
    from efficientdet.pytorch_amd.evaluate import TrackedDetector
    with pytest.raises(TypeError):
        TrackedDetector(object())
    class _Model:
        num_classes = 3
        def forward_raw(self, x): raise AssertionError
        def eval(self): self.evaled = True
        def train(self, mode=True): self.mode = mode
        def parameters(self): return iter(())
    m = _Model()
    with pytest.raises(TypeError):
        TrackedDetector(m, options=dict())
    for bad in (0, 129):
        with pytest.raises(ValueError):
            TrackedDetector(m, max_detections=bad)
    with pytest.raises(ValueError):
        TrackedDetector(m, score_threshold=nan)
    t = TrackedDetector(m)
    assert t.score_threshold == t.options.low_thr == 0.1 and t.max_detections == 100 and t.num_classes == 3 and t.state is None
    assert t.eval() is t and m.evaled and t.train(False) is t and m.mode is False and list(t.parameters()) == []
    t.reset()                                                                      # nothing to reset yet: no launch, no error
    assert TrackedDetector(m, score_threshold=0.3).score_threshold == 0.3


def test_refusals_are_decided_on_the_host_and_launch_nothing():
    from efficientdet.pytorch_amd import build, _lib
    build.build(verbose=False)
    L = _lib.require(*_lib.TRACK_SIGNATURES)
    sb = L.effdet_track_state_bytes
    assert sb(2, 8) == 2 * 16 + 2 * 8 * 28 * 4 and sb(1, 256) == 16 + 256 * 112 and sb(0, 8) == 0 and sb(2, 0) == 0 and sb(2, 257) == 0
    buf = np.zeros(1 << 16, dtype=np.uint8)
    p = buf.ctypes.data
    assert L.effdet_track_reset(None, 2, 8, None, None) == -1 and L.effdet_track_reset(p, 0, 8, None, None) == -1
    assert L.effdet_track_reset(p, 2, 0, None, None) == -1 and L.effdet_track_reset(p, 2, 257, None, None) == -3
    assert L.effdet_track_overflow(None, 2, 8, p, None) == -1 and L.effdet_track_overflow(p, 2, 8, None, None) == -1
    assert L.effdet_track_overflow(p, 0, 8, p, None) == -1 and L.effdet_track_overflow(p, 2, 257, p, None) == -3

    def step(**kw):
        a = dict(d=p, n=p, B=2, D=8, s=p, T=8, tt=0.5, lt=0.1, nt=0.6, ms=0.2, ss=0.5, us=0.3, buf=30, fuse=1, ca=0, o1=p, o2=p, o3=p)
        a.update(kw)
        return L.effdet_track_step(a['d'], a['n'], a['B'], a['D'], a['s'], a['T'], a['tt'], a['lt'], a['nt'], a['ms'], a['ss'], a['us'],
                                   a['buf'], a['fuse'], a['ca'], a['o1'], a['o2'], a['o3'], None)
    nan, inf = float('nan'), float('inf')
    for kw in (dict(T=257), dict(D=129)):
        assert step(**kw) == -3, kw
    for kw in (dict(d=None), dict(n=None), dict(s=None), dict(o1=None), dict(o2=None), dict(o3=None), dict(B=0), dict(D=0), dict(T=0),
               dict(tt=nan), dict(lt=-inf), dict(nt=inf), dict(ms=-0.1), dict(ms=1.5), dict(ss=nan), dict(us=2.0), dict(lt=0.6), dict(buf=-1)):
        assert step(**kw) == -1, kw
    assert not buf.any()
