"""The tracker's restatement (tests/track_restated.py) with the OPTIMAL assignment of include/effdet_assign.h in its three associations:
Stream overrides _greedy, the assignment stage, and nothing else.  The similarities are the restatement's own (float64, or float32 to
measure the format's error); the matching maximises the sum of (sim - gate) over the allowed pairs, solved by tests/assign_restated.py
on a 2^-40 grid -- far below the device's 2^-20 one, so for a case whose optimum clears its second best by the margin
tests/test_track_lap_host.py asks for, this matching is the only answer the device may give.

LapTrace also collects every similarity (sims) and, per association with a match, (which, n = min(rows, cols), optimum - second best in
similarity units) in gaps."""
import numpy as np

from tests import assign_restated as A
from tests import track_restated as R

SCALE = 1 << 40


class LapTrace(R.Trace):
    def __init__(self):
        super().__init__()
        self.sims, self.gaps = [], []


class Stream(R.Stream):
    def _greedy(self, which, pool, cols, sim_of, gate, opt, tr):
        dt = self.dt
        W = np.zeros((len(pool), len(cols)), dtype=np.int64)
        for i, t in enumerate(pool):
            for j, d in enumerate(cols):
                if opt.class_aware and not self.slots[t].label == self._dl[d]:
                    tr.hit('class_gate_fail')
                    continue
                if opt.class_aware:
                    tr.hit('class_gate_pass')
                s = sim_of(t, d)
                tr.value(s)
                tr.margin('sim_gate', abs(float(s) - float(gate)))
                tr.hit('assoc%d_%s' % (which, 'allowed' if s > dt(gate) else 'refused'))
                if hasattr(tr, 'sims'):
                    tr.sims.append(float(s))
                if s > dt(gate):
                    W[i, j] = max(1, int(round((float(s) - float(gate)) * SCALE)))
        total, match = A.solve(W)
        if match and hasattr(tr, 'gaps'):
            tr.gaps.append((which, min(len(pool), len(cols)), (total - A.second_best(W)) / SCALE))
        tr.picks[which] = max(tr.picks[which], len(match))
        tr.hit('step%d' % {1: 3, 2: 4, 3: 5}[which])
        return {pool[i]: cols[j] for i, j in match.items()}


def run(case, dtype=np.float64, filt=R.Full, trace=None, stream=Stream):
    """tests/track_restated.run with the optimal Stream (stream=R.Stream gives the greedy one on the same case)"""
    opt = case['options']
    B = case['dets'].shape[1]
    streams = [stream(opt.max_tracks, dtype, filt) for _ in range(B)]
    frames = []
    for f in range(case['dets'].shape[0]):
        for b in case['resets'].get(f, ()):
            streams[b].reset()
        out = [streams[b].step(case['dets'][f, b], case['counts'][f, b], opt, trace) for b in range(B)]
        frames.append(([o[0] for o in out], [o[1] for o in out], [s.overflow for s in streams]))
    return frames, streams
