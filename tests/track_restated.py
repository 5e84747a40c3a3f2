"""NumPy restatement of include/effdet_track.h (ByteTrack over finalize_dets' rows), written from the header.  One Stream per camera
stream; step() is the ten-step per-frame rule.  The Kalman filter here is the FULL 8 x 8 one (Full); Block is the header's block form
(three covariance numbers per coordinate), kept beside it so that the host tier can hold the two against each other.  dtype switches
the arithmetic between float64 (the reference the kernel is held to) and float32 (what measures the format's own error).

A Trace collects what the host tier asserts on: which branches ran, every decision's distance from its alternative, and the values
(similarities, Kalman means) whose float32 / float64 difference is eps_sim."""
import numpy as np

FREE, UNCONFIRMED, TRACKED, LOST = 0, 1, 2, 3
MAX_TRACKS, MAX_DET, ROW_WORDS = 256, 128, 28
DUP_IOU = 0.85


class Options:
    def __init__(self, track_thr=0.5, low_thr=0.1, new_thr=None, match_sim=0.2, second_sim=0.5, unconfirmed_sim=0.3, track_buffer=30,
                 fuse_score=True, class_aware=False, max_tracks=128):
        f = np.float32                                                             # the thresholds are fp32 scalars of the C call
        self.track_thr, self.low_thr = f(track_thr), f(low_thr)
        self.new_thr = f(f(track_thr) + f(0.1)) if new_thr is None else f(new_thr)
        self.match_sim, self.second_sim, self.unconfirmed_sim = f(match_sim), f(second_sim), f(unconfirmed_sim)
        self.track_buffer, self.fuse_score, self.class_aware, self.max_tracks = int(track_buffer), bool(fuse_score), bool(class_aware), int(max_tracks)


class Trace:
    def __init__(self):
        self.hits, self.margins, self.values, self.picks = {}, [], [], {1: 0, 2: 0, 3: 0}

    def hit(self, tag, n=1):
        self.hits[tag] = self.hits.get(tag, 0) + n

    def margin(self, kind, value):
        self.margins.append((kind, float(value)))

    def value(self, v):
        self.values.extend(np.asarray(v, dtype=np.float64).reshape(-1).tolist())


class _NoTrace:
    picks = {1: 0, 2: 0, 3: 0}

    def hit(self, tag, n=1): pass
    def margin(self, kind, value): pass
    def value(self, v): pass


# ------------------------------------------------------------------------------------------------ the filter, two ways
class Full:
    """ByteTrack's KalmanFilter: 8 x 8 covariance, F = I + the velocity shift, H = the first four rows."""

    def __init__(self, dtype):
        self.dt = dtype
        self.F = np.eye(8, dtype=dtype)
        for i in range(4):
            self.F[i, 4 + i] = 1
        self.H = np.eye(4, 8, dtype=dtype)

    def start(self, z):
        dt = self.dt
        h = z[3]
        sp, su = dt(2) * (h / dt(20)), dt(10) * (h / dt(160))
        std = np.array([sp, sp, dt(np.float32(1e-2)), sp, su, su, dt(np.float32(1e-5)), su], dtype=dt)
        var = std * std
        var[2], var[6] = dt(np.float32(1e-4)), dt(np.float32(1e-10))
        return np.concatenate([z, np.zeros(4, dtype=dt)]).astype(dt), np.diag(var).astype(dt)

    def predict(self, mean, P):
        dt = self.dt
        h = mean[3]
        sp, su = h / dt(20), h / dt(160)
        std = np.array([sp, sp, dt(np.float32(1e-2)), sp, su, su, dt(np.float32(1e-5)), su], dtype=dt)
        return self.F @ mean, self.F @ P @ self.F.T + np.diag(std * std)

    def update(self, mean, P, z):
        dt = self.dt
        sp = mean[3] / dt(20)
        r = np.array([sp * sp, sp * sp, dt(np.float32(1e-2)), sp * sp], dtype=dt)
        S = self.H @ P @ self.H.T + np.diag(r)
        K = P @ self.H.T @ np.linalg.inv(S)
        return mean + K @ (z - self.H @ mean), P - K @ S @ K.T

    @staticmethod
    def numbers(P):
        """-> the 12 numbers the block form keeps: (p, c, v) per coordinate"""
        return np.array([[P[i, i], P[i, 4 + i], P[4 + i, 4 + i]] for i in range(4)]).reshape(-1)


class Block:
    """The header's block form: cov is [4][3] = (p, c, v) per coordinate."""

    def __init__(self, dtype):
        self.dt = dtype

    def start(self, z):
        dt = self.dt
        sp, su = dt(2) * (z[3] / dt(20)), dt(10) * (z[3] / dt(160))
        cov = np.zeros((4, 3), dtype=dt)
        cov[:, 0], cov[:, 2] = sp * sp, su * su
        cov[2, 0], cov[2, 2] = dt(np.float32(1e-4)), dt(np.float32(1e-10))
        return np.concatenate([z, np.zeros(4, dtype=dt)]).astype(dt), cov

    def predict(self, mean, cov):
        dt = self.dt
        mean, cov = mean.copy(), cov.copy()
        h = mean[3]
        for i in range(4):
            sp = dt(np.float32(1e-2)) if i == 2 else h / dt(20)
            su = dt(np.float32(1e-5)) if i == 2 else h / dt(160)
            p, c, v = cov[i]
            mean[i] = mean[i] + mean[4 + i]
            cov[i] = ((p + c) + (c + v)) + sp * sp, c + v, v + su * su
        return mean, cov

    def update(self, mean, cov, z):
        dt = self.dt
        mean, cov = mean.copy(), cov.copy()
        h = mean[3]
        for i in range(4):
            sp = h / dt(20)
            r = dt(np.float32(1e-2)) if i == 2 else sp * sp
            p, c, v = cov[i]
            S, y = p + r, z[i] - mean[i]
            mean[i] = mean[i] + (p / S) * y
            mean[4 + i] = mean[4 + i] + (c / S) * y
            cov[i] = p - (p * p) / S, c - (p * c) / S, v - (c * c) / S
        return mean, cov

    @staticmethod
    def numbers(cov):
        return np.asarray(cov).reshape(-1)


# ------------------------------------------------------------------------------------------------ boxes
def det_z(box, dt):
    x1, y1, x2, y2 = (dt(v) for v in box)
    w, h = x2 - x1, y2 - y1
    return np.array([x1 + dt(0.5) * w, y1 + dt(0.5) * h, w / h, h], dtype=dt)


def mean_box(mean, dt):
    w = mean[2] * mean[3]
    x1, y1 = mean[0] - dt(0.5) * w, mean[1] - dt(0.5) * mean[3]
    return np.array([x1, y1, x1 + w, y1 + mean[3]], dtype=dt)


def iou(a, b, dt):
    iw = min(a[2], b[2]) - max(a[0], b[0])
    ih = min(a[3], b[3]) - max(a[1], b[1])
    if not iw > 0 or not ih > 0:
        return dt(0)
    inter = iw * ih
    return dt(inter / (((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1])) - inter))


def valid_row(r):
    return bool(np.all(np.isfinite(r[:5])) and r[2] > r[0] and r[3] > r[1])


class Track:
    __slots__ = ('state', 'id', 'len', 'start', 'last', 'score', 'label', 'mean', 'cov')

    def __init__(self):
        self.state = FREE


class Stream:
    def __init__(self, max_tracks, dtype=np.float64, filt=Full):
        self.dt, self.kf, self.T = dtype, filt(dtype), int(max_tracks)
        self.reset()

    def reset(self):
        self.slots = [Track() for _ in range(self.T)]
        self.frame_id, self.next_id, self.overflow = 0, 1, 0

    # -- greedy assignment over precomputed similarities; sims[(slot, row)] holds only the pairs the labels allow
    def _greedy(self, which, pool, cols, sim_of, gate, opt, tr):
        dt = self.dt
        sims = {}
        for t in pool:
            for d in cols:
                if opt.class_aware and not self.slots[t].label == self._dl[d]:
                    tr.hit('class_gate_fail')
                    continue
                if opt.class_aware:
                    tr.hit('class_gate_pass')
                s = sim_of(t, d)
                sims[(t, d)] = s
                tr.value(s)
                tr.margin('sim_gate', abs(float(s) - float(gate)))
                tr.hit('assoc%d_%s' % (which, 'allowed' if s > dt(gate) else 'refused'))
        live = {k: s for k, s in sims.items() if s > dt(gate)}
        out, picks = {}, 0
        while live:
            (t, d), s = min(live.items(), key=lambda kv: (-kv[1], kv[0][1], kv[0][0]))       # largest sim, lower row, lower slot
            rivals = [v for (tt, dd), v in live.items() if (tt == t) != (dd == d)]
            if rivals:
                tr.margin('pick', float(s) - float(max(rivals)))
            out[t] = d
            picks += 1
            live = {k: v for k, v in live.items() if k[0] != t and k[1] != d}
        tr.picks[which] = max(tr.picks[which], picks)
        tr.hit('step%d' % {1: 3, 2: 4, 3: 5}[which])
        return out

    def _match(self, t, d, frame):
        k = self.slots[t]
        k.mean, k.cov = self.kf.update(k.mean, k.cov, det_z(self._db[d], self.dt))
        k.score, k.label, k.last = self._ds[d], self._dl[d], frame

    def step(self, dets, count, opt, tr=None):
        """dets [max_det, 6] float32, count -> (rows [K, 8] of dtype, ids [K] int64)"""
        tr = _NoTrace() if tr is None else tr
        dt, sl = self.dt, self.slots
        dets = np.asarray(dets, dtype=np.float32)
        self.frame_id += 1                                                                 # step 0
        frame = self.frame_id
        # 1. predict
        for k in sl:
            if k.state == FREE:
                continue
            if k.state == LOST:
                k.mean = k.mean.copy()
                k.mean[7] = dt(0)
                tr.hit('lost_vh_zero')
            tr.hit('predict_%d' % k.state)
            k.mean, k.cov = self.kf.predict(k.mean, k.cov)
        tr.hit('step1')
        pbox = {t: mean_box(k.mean, dt) for t, k in enumerate(sl) if k.state != FREE}
        # 2. split
        n = min(max(int(count), 0), dets.shape[0])
        self._db, self._ds, self._dl = {}, {}, {}
        high, low = [], []
        for d in range(n):
            r = dets[d]
            if not valid_row(r):
                tr.hit('row_skipped')
                continue
            s = r[4]
            for name, thr in (('track_thr', opt.track_thr), ('low_thr', opt.low_thr), ('new_thr', opt.new_thr)):
                tr.margin(name, abs(float(s) - float(thr)))
            self._db[d], self._ds[d], self._dl[d] = r[:4], s, r[5]
            if s >= opt.track_thr:
                high.append(d); tr.hit('det_high')
            elif s > opt.low_thr:
                low.append(d); tr.hit('det_low')
            else:
                tr.hit('det_ignored')
        tr.hit('step2')

        def fused(t, d):
            v = iou(pbox[t], self._db[d].astype(dt), dt)
            return v * dt(self._ds[d]) if opt.fuse_score else v

        def plain(t, d):
            return iou(pbox[t], self._db[d].astype(dt), dt)
        state0 = [k.state for k in sl]
        # 3. first association
        pool = [t for t in range(self.T) if state0[t] in (TRACKED, LOST)]
        m1 = self._greedy(1, pool, high, fused, opt.match_sim, opt, tr)
        for t, d in m1.items():
            self._match(t, d, frame)
            if state0[t] == LOST:
                sl[t].state, sl[t].len = TRACKED, 0
                tr.hit('refound')
            else:
                sl[t].len += 1
                tr.hit('tracked_updated')
        # 4. second association
        pool = [t for t in range(self.T) if state0[t] == TRACKED and t not in m1]
        m2 = self._greedy(2, pool, low, plain, opt.second_sim, opt, tr)
        for t, d in m2.items():
            self._match(t, d, frame)
            sl[t].len += 1
            tr.hit('second_updated')
        for t in pool:
            if t not in m2:
                sl[t].state = LOST
                tr.hit('tracked_to_lost')
        # 5. third association
        left = [d for d in high if d not in m1.values()]
        pool = [t for t in range(self.T) if state0[t] == UNCONFIRMED]
        m3 = self._greedy(3, pool, left, fused, opt.unconfirmed_sim, opt, tr)
        for t in pool:
            if t in m3:
                self._match(t, m3[t], frame)
                sl[t].len += 1
                sl[t].state = TRACKED
                tr.hit('unconfirmed_activated')
            else:
                sl[t] = Track()
                tr.hit('unconfirmed_removed')
        tr.hit('step6', len(m1) + len(m2) + len(m3))
        # 7. new tracks
        born = [d for d in left if d not in m3.values() and self._ds[d] >= opt.new_thr]
        tr.hit('new_refused', sum(1 for d in left if d not in m3.values() and not self._ds[d] >= opt.new_thr))
        free = [t for t in range(self.T) if sl[t].state == FREE]
        for k_, (t, d) in enumerate(zip(free, born)):
            k = sl[t]
            k.mean, k.cov = self.kf.start(det_z(self._db[d], dt))
            k.score, k.label, k.id, k.len, k.start, k.last = self._ds[d], self._dl[d], self.next_id + k_, 0, frame, frame
            k.state = TRACKED if frame == 1 else UNCONFIRMED
            tr.hit('new_activated' if frame == 1 else 'new_unconfirmed')
        self.next_id += min(len(born), len(free))
        self.overflow += max(len(born) - len(free), 0)
        tr.hit('new_dropped', max(len(born) - len(free), 0))
        tr.hit('step7')
        # 8. removal
        for t, k in enumerate(sl):
            if k.state == LOST:
                if frame - k.last > opt.track_buffer:
                    sl[t] = Track()
                    tr.hit('lost_removed')
                else:
                    tr.hit('lost_kept')
        tr.hit('step8')
        # 9. duplicates
        boxes = {t: mean_box(k.mean, dt) for t, k in enumerate(sl) if k.state != FREE}
        marked = set()
        for t, k in enumerate(sl):
            if k.state != TRACKED:
                continue
            for l, q in enumerate(sl):
                if q.state != LOST:
                    continue
                v = iou(boxes[t], boxes[l], dt)
                tr.value(v)
                tr.margin('dup_gate', abs(float(v) - DUP_IOU))
                if v > dt(np.float32(DUP_IOU)):
                    at, al = frame - k.start, frame - q.start
                    marked.add(l if at > al else t)
                    tr.hit('dup_lost_removed' if at > al else ('dup_equal_age' if at == al else 'dup_tracked_removed'))
                else:
                    tr.hit('dup_refused')
        for t in marked:
            sl[t] = Track()
        tr.hit('step9')
        # 10. output
        shown = sorted((k.id, t) for t, k in enumerate(sl) if k.state == TRACKED)
        rows = np.zeros((len(shown), 8), dtype=dt)
        for i, (_, t) in enumerate(shown):
            k = sl[t]
            rows[i] = list(boxes[t]) + [dt(k.score), dt(k.label), k.len, frame - k.start]
        for t, k in enumerate(sl):
            if k.state != FREE:
                tr.value(k.mean)
        tr.hit('step10')
        return rows, np.array([i for i, _ in shown], dtype=np.int64)

    def state_words(self):
        """The stream's slots as the header lays them out: [T][ROW_WORDS] uint32 (block-form filter and float32 only)."""
        out = np.zeros((self.T, ROW_WORDS), dtype=np.uint32)
        for t, k in enumerate(self.slots):
            if k.state == FREE:
                continue
            f = np.concatenate([k.mean, self.kf.numbers(k.cov), [k.score, k.label]]).astype(np.float32)
            out[t, :22] = f.view(np.uint32)
            out[t, 22:27] = [k.state, k.id, k.len, k.start, k.last]
        return out


def run(case, dtype=np.float64, filt=Full, trace=None):
    """A case of tests/track_cases.py through B streams -> per frame: (rows list, ids list, overflow list); also the streams."""
    opt = case['options']
    B = case['dets'].shape[1]
    streams = [Stream(opt.max_tracks, dtype, filt) for _ in range(B)]
    frames = []
    for f in range(case['dets'].shape[0]):
        for b in case['resets'].get(f, ()):
            streams[b].reset()
        out = [streams[b].step(case['dets'][f, b], case['counts'][f, b], opt, trace) for b in range(B)]
        frames.append(([o[0] for o in out], [o[1] for o in out], [s.overflow for s in streams]))
    return frames, streams
