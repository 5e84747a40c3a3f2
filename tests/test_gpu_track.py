"""GPU tier of the tracker (csrc/track.hip; ops.track_state / track_reset / track_step / track_overflow) against the NumPy restatement
tests/track_restated.py on the cases of tests/track_cases.py, frame by frame: ids, counts, labels, tracklet lengths, ages and overflow
counts exactly, boxes and scores within 8 * EPS_SIM of the float64 restatement (EPS_SIM is the float32 error of the rule measured on
the CPU tier, where every float64 decision is also shown to clear its alternative by 16 * EPS_SIM)."""
import numpy as np
import pytest
import torch

from tests import track_restated as R
from tests import track_cases as C

pytestmark = pytest.mark.gpu

GUARD, FILL = 256, 0xA5
_WANT, _GOT = {}, {}


def _options(o):
    from efficientdet.pytorch_amd import ops
    return ops.TrackOptions(track_thr=float(o.track_thr), low_thr=float(o.low_thr), new_thr=float(o.new_thr), match_sim=float(o.match_sim),
                            second_sim=float(o.second_sim), unconfirmed_sim=float(o.unconfirmed_sim), track_buffer=o.track_buffer,
                            fuse_score=o.fuse_score, class_aware=o.class_aware, max_tracks=o.max_tracks)


def _want(name):
    if name not in _WANT:
        _WANT[name] = R.run(C.case(name), np.float64, R.Full)
    return _WANT[name]


def _guarded(nbytes):
    """-> (whole uint8 buffer filled with FILL, the nbytes in its middle)"""
    whole = torch.full((nbytes + 2 * GUARD,), FILL, dtype=torch.uint8, device='cuda')
    return whole, whole[GUARD:GUARD + nbytes]


def _guards_intact(whole):
    return bool((whole[:GUARD] == FILL).all()) and bool((whole[-GUARD:] == FILL).all())


def _sequence(name):
    """The case on the device, one launch per frame -> dict(frames=[(rows, ids, count, overflow) numpy], state=bytes, guards=bool)"""
    from efficientdet.pytorch_amd import ops
    case = C.case(name)
    o = _options(case['options'])
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
            t.fill_(FILL)                                                          # a sentinel under every output element
        rows, ids, count = ops.track_step(dets[f], counts[f], state, o, out=out)
        frames.append((rows.cpu().numpy(), ids.cpu().numpy(), count.cpu().numpy(), ops.track_overflow(state).cpu().numpy()))
    return dict(frames=frames, state=sbuf.cpu().numpy().copy(), guards=all(_guards_intact(w) for w in (sw, rw, iw, cw)))


def _got(name, run=0):
    if (name, run) not in _GOT:
        _GOT[(name, run)] = _sequence(name)
    return _GOT[(name, run)]


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
            # rows past the count: zero with id -1, over the sentinel
            assert not rows[b, K:].any() and np.all(ids[b, K:] == -1) and rows.shape[1] == T, (name, f, b)
    print('%s: boxes and scores within %.3g of the float64 restatement (bound %.3g)' % (name, worst, 8 * C.EPS_SIM))
    assert worst <= 8 * C.EPS_SIM
    assert got['guards']


@pytest.mark.parametrize('name', C.NAMES)
def test_the_final_state_is_the_restatements_and_two_runs_are_bit_equal(name):
    from efficientdet.pytorch_amd import ops
    a, b = _got(name), _got(name, 1)
    assert np.array_equal(a['state'], b['state'])
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for fa, fb in zip(a['frames'], b['frames']) for x, y in zip(fa, fb))
    streams = _want(name)[1]
    B, T = len(streams), streams[0].T
    hdr = a['state'][:B * 16].view(np.int32).reshape(B, 4)
    words = a['state'][B * 16:].view(np.uint32).reshape(B, T, ops.TRACK_ROW_WORDS)
    for i, s in enumerate(streams):
        assert list(hdr[i]) == [s.frame_id, s.next_id, s.overflow, 0]
        want = s.state_words()
        assert np.array_equal(words[i, :, 22:], want[:, 22:])                        # state, id, tracklet_len, start_frame, last_frame
        free = want[:, 22] == R.FREE
        assert not words[i, free].any()                                            # a free slot is all zero
        means = words[i, ~free, :8].view(np.float32).astype(np.float64)
        ref = np.array([k.mean for k in s.slots if k.state != R.FREE]).reshape(-1, 8)
        assert np.abs(means - ref).max(initial=0.0) <= 8 * C.EPS_SIM
        # the stored covariance numbers within 8 * EPS_COV relative (an exact 0 stays 0); score and label are the detection's bits
        cov = words[i, ~free, 8:20].view(np.float32).astype(np.float64)
        want_cov = np.array([R.Full.numbers(k.cov) for k in s.slots if k.state != R.FREE]).reshape(-1, 12)
        assert np.all(np.abs(cov - want_cov) <= 8 * C.EPS_COV * np.abs(want_cov)), (name, i, np.abs(cov - want_cov).max(initial=0.0))
        if cov.size:
            print('%s stream %d: stored covariances within %.3g relative (bound %.3g)'
                  % (name, i, float((np.abs(cov - want_cov) / np.where(want_cov == 0, 1, np.abs(want_cov))).max()), 8 * C.EPS_COV))
        assert np.array_equal(words[i, :, 20:22], want[:, 20:22])


def test_a_static_object_is_exact():
    """The same rows for five frames: the innovation is exactly zero, so the boxes repeat bit for bit and every velocity stays 0."""
    from efficientdet.pytorch_amd import ops
    rows = np.array([[[37.25, 41.5, 101.75, 160.125, 0.9, 3.0], [300.1, 200.7, 377.3, 251.9, 0.8, 1.0], [0, 0, 0, 0, 0, -1]]], dtype=np.float32)
    dets, counts = torch.from_numpy(rows).cuda(), torch.tensor([2], dtype=torch.int32, device='cuda')
    o = ops.TrackOptions(max_tracks=8)
    state = ops.track_state(1, 8, 'cuda')
    outs = [tuple(t.clone() for t in ops.track_step(dets, counts, state, o)) for _ in range(5)]
    for f, (r, i, c) in enumerate(outs):
        assert int(c[0]) == 2 and i[0, :2].tolist() == [1, 2]
        assert torch.equal(r[0, :, :6], outs[0][0][0, :, :6]) and r[0, :2, 6].tolist() == [f, f] and r[0, :2, 7].tolist() == [f, f]
    assert torch.allclose(outs[0][0][0, :2, :4], dets[0, :2, :4], atol=1e-4, rtol=0)
    words = state.buf[16:].view(torch.int32).view(8, ops.TRACK_ROW_WORDS)
    assert not words[:2, 4:8].any() and words[:2, 22].tolist() == [R.TRACKED, R.TRACKED] and not words[2:].any()


def test_a_captured_step_replays_the_eager_sequence_bit_for_bit():
    """ops.track_step captured once in a torch.cuda.graph over static dets / counts buffers and replayed over a case's frames."""
    from efficientdet.pytorch_amd import ops
    name = 'gap_short'
    case, eager = C.case(name), _got(name)
    o = _options(case['options'])
    F, B, D, _ = case['dets'].shape
    dets, counts = torch.from_numpy(case['dets']).cuda(), torch.from_numpy(case['counts']).cuda()
    sd, sc = torch.zeros_like(dets[0]), torch.zeros_like(counts[0])
    state = ops.track_state(B, o.max_tracks, 'cuda')
    out = (torch.empty((B, o.max_tracks, 8), device='cuda'), torch.empty((B, o.max_tracks), dtype=torch.int32, device='cuda'),
           torch.empty(B, dtype=torch.int32, device='cuda'))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.track_step(sd, sc, state, o, out=out)                                  # warm-up outside the capture (it advances frame_id:
    torch.cuda.current_stream().wait_stream(side)
    ops.track_reset(state)                                                         #  reset afterwards)
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
    assert np.array_equal(ops.track_overflow(state).cpu().numpy(), eager['frames'][-1][3])


def test_the_python_layer_refuses_before_a_launch():
    from efficientdet.pytorch_amd import ops
    state = ops.track_state(2, 8, 'cuda')
    before = state.buf.clone()
    dets, counts = torch.zeros((2, 4, 6), device='cuda'), torch.zeros(2, dtype=torch.int32, device='cuda')
    with pytest.raises(ValueError):
        ops.track_step(dets, counts, state, ops.TrackOptions(max_tracks=16))
    with pytest.raises(ValueError):
        ops.track_step(dets[:1], counts[:1], state, ops.TrackOptions(max_tracks=8))
    with pytest.raises(ValueError):
        ops.track_step(torch.zeros((2, 129, 6), device='cuda'), counts, state, ops.TrackOptions(max_tracks=8))
    with pytest.raises(TypeError):
        ops.track_step(dets, counts, state.buf, ops.TrackOptions(max_tracks=8))
    with pytest.raises(ValueError):
        ops.track_reset(state, [1])
    with pytest.raises(ValueError):
        ops.track_state(2, 257, 'cuda')
    assert torch.equal(state.buf, before)
    hdr = state.buf[:32].view(torch.int32).view(2, 4)
    assert hdr.tolist() == [[0, 1, 0, 0]] * 2 and not state.buf[32:].any() and ops.track_overflow(state).tolist() == [0, 0]
