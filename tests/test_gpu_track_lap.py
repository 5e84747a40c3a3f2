"""GPU tier of the tracker with assignment='optimal' (csrc/track.hip's second kernel instance over csrc/assign.h; ops.track_step) against
the restatement tests/track_lap_restated.py on the scenes of tests/track_lap_cases.py, frame by frame: ids, counts, labels, tracklet
lengths, ages, overflow and the integer state exactly -- the CPU tier shows every association's optimum to be the only one the device's
arithmetic can reach -- boxes and scores within 8 * EPS_SIM of the float64 restatement, as tests/test_gpu_track.py holds the greedy
tracker.  And assignment='greedy' against the tracker without the option, bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

from tests import track_restated as R
from tests import track_cases as GC
from tests import track_lap_restated as LR
from tests import track_lap_cases as C

pytestmark = pytest.mark.gpu

GUARD, FILL = 256, 0xA5
_WANT, _GOT = {}, {}


def _options(o, **kw):
    from efficientdet.pytorch_amd import ops
    return ops.TrackOptions(track_thr=float(o.track_thr), low_thr=float(o.low_thr), new_thr=float(o.new_thr), match_sim=float(o.match_sim),
                            second_sim=float(o.second_sim), unconfirmed_sim=float(o.unconfirmed_sim), track_buffer=o.track_buffer,
                            fuse_score=o.fuse_score, class_aware=o.class_aware, max_tracks=o.max_tracks, **kw)


def _want(name):
    if name not in _WANT:
        _WANT[name] = LR.run(C.case(name), np.float64, R.Full)
    return _WANT[name]


def _guarded(nbytes):
    whole = torch.full((nbytes + 2 * GUARD,), FILL, dtype=torch.uint8, device='cuda')
    return whole, whole[GUARD:GUARD + nbytes]


def _sequence(case, o):
    """The case on the device, one launch per frame -> dict(frames=[(rows, ids, count, overflow) numpy], state=bytes, guards=bool)"""
    from efficientdet.pytorch_amd import ops
    F, B, D, _ = case['dets'].shape
    T = o.max_tracks
    sw, sbuf = _guarded(B * 16 + B * T * 4 * ops.TRACK_ROW_WORDS)
    state = ops.track_state(B, T, 'cuda', buf=sbuf)
    rw, rbuf = _guarded(B * T * 8 * 4)
    iw, ibuf = _guarded(B * T * 4)
    cw, cbuf = _guarded(B * 4)
    out = (rbuf.view(torch.float32).view(B, T, 8), ibuf.view(torch.int32).view(B, T), cbuf.view(torch.int32))
    dets, counts = torch.from_numpy(case['dets']).cuda(), torch.from_numpy(case['counts']).cuda()
    frames = []
    for f in range(F):
        if f in case['resets']:
            ops.track_reset(state, [1 if b in case['resets'][f] else 0 for b in range(B)])
        for t in (rbuf, ibuf, cbuf):
            t.fill_(FILL)
        rows, ids, count = ops.track_step(dets[f], counts[f], state, o, out=out)
        frames.append((rows.cpu().numpy(), ids.cpu().numpy(), count.cpu().numpy(), ops.track_overflow(state).cpu().numpy()))
    guards = all(bool((w[:GUARD] == FILL).all()) and bool((w[-GUARD:] == FILL).all()) for w in (sw, rw, iw, cw))
    return dict(frames=frames, state=sbuf.cpu().numpy().copy(), guards=guards)


def _got(name, run=0):
    if (name, run) not in _GOT:
        c = C.case(name)
        _GOT[(name, run)] = _sequence(c, _options(c['options'], assignment='optimal'))
    return _GOT[(name, run)]


def _same(a, b):
    return np.array_equal(a['state'], b['state']) and all(np.array_equal(x.view(np.uint8), y.view(np.uint8))
                                                            for fa, fb in zip(a['frames'], b['frames']) for x, y in zip(fa, fb))


@pytest.mark.parametrize('name', C.NAMES)
def test_every_frame_equals_the_restatement(name):
    want, got = _want(name)[0], _got(name)
    T = C.case(name)['options'].max_tracks
    worst = 0.0
    for f, ((wrows, wids, wover), (rows, ids, count, over)) in enumerate(zip(want, got['frames'])):
        for b in range(len(wids)):
            K = len(wids[b])
            assert count[b] == K and np.array_equal(ids[b, :K], wids[b]), (name, f, b, ids[b], wids[b])
            assert np.array_equal(rows[b, :K, 5:], wrows[b][:, 5:].astype(np.float32)), (name, f, b)       # label, tracklet_len, age
            assert over[b] == wover[b], (name, f, b)
            if K:
                worst = max(worst, float(np.abs(rows[b, :K, :5].astype(np.float64) - wrows[b][:, :5]).max()))
            assert not rows[b, K:].any() and np.all(ids[b, K:] == -1) and rows.shape[1] == T, (name, f, b)
    print('%s: boxes and scores within %.3g of the float64 restatement (bound %.3g)' % (name, worst, 8 * C.EPS_SIM))
    assert worst <= 8 * C.EPS_SIM
    assert got['guards']


@pytest.mark.parametrize('name', C.NAMES)
def test_the_final_integer_state_is_the_restatements_and_two_runs_are_bit_equal(name):
    from efficientdet.pytorch_amd import ops
    a = _got(name)
    assert _same(a, _got(name, 1))
    streams = _want(name)[1]
    B, T = len(streams), streams[0].T
    hdr = a['state'][:B * 16].view(np.int32).reshape(B, 4)
    words = a['state'][B * 16:].view(np.uint32).reshape(B, T, ops.TRACK_ROW_WORDS)
    for i, s in enumerate(streams):
        assert list(hdr[i]) == [s.frame_id, s.next_id, s.overflow, 0]
        want = s.state_words()
        assert np.array_equal(words[i, :, 22:], want[:, 22:])                        # state, id, tracklet_len, start_frame, last_frame
        free = want[:, 22] == R.FREE
        assert not words[i, free].any()
        means = words[i, ~free, :8].view(np.float32).astype(np.float64)
        ref = np.array([k.mean for k in s.slots if k.state != R.FREE]).reshape(-1, 8)
        assert np.abs(means - ref).max(initial=0.0) <= 8 * C.EPS_SIM
        assert np.array_equal(words[i, :, 20:22], want[:, 20:22])                    # score and label: the detection's bits


@pytest.mark.parametrize('name', ('crossing', 'cap'))
def test_the_optimal_tracker_parts_from_the_greedy_one_on_the_device_too(name):
    c = C.case(name)
    greedy = _sequence(c, _options(c['options']))
    assert not _same(greedy, _got(name))
    f = {'crossing': 5, 'cap': 2}[name]
    assert greedy['frames'][f][2][0] == {'crossing': 1, 'cap': 64}[name] and _got(name)['frames'][f][2][0] == {'crossing': 2, 'cap': 128}[name]


@pytest.mark.parametrize('name', ('crossing', 'dip', 'false_positive', 'tie', 'cap'))
def test_assignment_greedy_is_the_tracker_without_the_option(name):
    """Scenes of both case files through TrackOptions() and TrackOptions(assignment='greedy'): one entry point, equal bits -- and the new
    entry point with assignment = 0 gives those bits too."""
    from efficientdet.pytorch_amd import ops, _lib as L
    c = C.case(name) if name == 'crossing' else GC.case(name)
    plain, named = _sequence(c, _options(c['options'])), _sequence(c, _options(c['options'], assignment='greedy'))
    assert _same(plain, named) and plain['guards'] and named['guards']
    o = _options(c['options'])
    F, B, D, _ = c['dets'].shape
    T = o.max_tracks
    state = ops.track_state(B, T, 'cuda')
    out = (torch.empty((B, T, 8), device='cuda'), torch.empty((B, T), dtype=torch.int32, device='cuda'), torch.empty(B, dtype=torch.int32, device='cuda'))
    dets, counts = torch.from_numpy(c['dets']).cuda(), torch.from_numpy(c['counts']).cuda()
    fn = L.require('effdet_track_step_assign').effdet_track_step_assign
    for f in range(F):
        assert f not in c['resets']
        assert fn(L.ptr(dets[f]), L.ptr(counts[f]), B, D, L.ptr(state.buf), T, o.track_thr, o.low_thr, o.new_thr, o.match_sim, o.second_sim,
                  o.unconfirmed_sim, o.track_buffer, int(o.fuse_score), int(o.class_aware), L.ptr(out[0]), L.ptr(out[1]), L.ptr(out[2]), 0,
                  L.stream_ptr()) == 0
        for got, want in zip(out, plain['frames'][f][:3]):
            assert np.array_equal(got.cpu().numpy().view(np.uint8), want.view(np.uint8)), (name, f)
    assert np.array_equal(state.buf.cpu().numpy(), plain['state'])


def test_a_captured_optimal_step_replays_the_eager_sequence_bit_for_bit():
    from efficientdet.pytorch_amd import ops
    name = 'crowd'
    case, eager = C.case(name), _got(name)
    o = _options(case['options'], assignment='optimal')
    F, B, D, _ = case['dets'].shape
    dets, counts = torch.from_numpy(case['dets']).cuda(), torch.from_numpy(case['counts']).cuda()
    sd, sc = torch.zeros_like(dets[0]), torch.zeros_like(counts[0])
    state = ops.track_state(B, o.max_tracks, 'cuda')
    out = (torch.empty((B, o.max_tracks, 8), device='cuda'), torch.empty((B, o.max_tracks), dtype=torch.int32, device='cuda'),
           torch.empty(B, dtype=torch.int32, device='cuda'))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.track_step(sd, sc, state, o, out=out)                                  # warm-up outside the capture; reset afterwards
    torch.cuda.current_stream().wait_stream(side)
    ops.track_reset(state)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.track_step(sd, sc, state, o, out=out)
    for f in range(F):
        sd.copy_(dets[f]); sc.copy_(counts[f])
        graph.replay()
        rows, ids, count = (t.cpu().numpy() for t in out)
        assert np.array_equal(rows.view(np.uint8), eager['frames'][f][0].view(np.uint8)), f
        assert np.array_equal(ids, eager['frames'][f][1]) and np.array_equal(count, eager['frames'][f][2]), f
    assert np.array_equal(state.buf.cpu().numpy(), eager['state'])


def test_the_error_codes_return_with_nothing_enqueued():
    from efficientdet.pytorch_amd import ops, _lib as L
    state = ops.track_state(2, 8, 'cuda')
    before = state.buf.clone()
    dets, counts = torch.zeros((2, 4, 6), device='cuda'), torch.zeros(2, dtype=torch.int32, device='cuda')
    out = (torch.full((2, 8, 8), 7.0, device='cuda'), torch.full((2, 8), 7, dtype=torch.int32, device='cuda'), torch.full((2,), 7, dtype=torch.int32, device='cuda'))
    fn = L.require('effdet_track_step_assign').effdet_track_step_assign

    def call(how, T=8, D=4, ms=0.2):
        return fn(L.ptr(dets), L.ptr(counts), 2, D, L.ptr(state.buf), T, 0.5, 0.1, 0.6, ms, 0.5, 0.3, 30, 1, 0, L.ptr(out[0]), L.ptr(out[1]),
                  L.ptr(out[2]), how, L.stream_ptr())
    assert [call(h) for h in (2, -1, 100)] == [-1, -1, -1] and call(1, T=257) == -3 and call(1, D=129) == -3 and call(1, ms=float('nan')) == -1
    opt = ops.TrackOptions(max_tracks=16, assignment='optimal')
    with pytest.raises(ValueError):
        ops.track_step(dets, counts, state, opt, out=None)                         # the state has 8 slots
    torch.cuda.synchronize()
    assert torch.equal(state.buf, before) and all(bool((t == 7).all()) for t in out)
