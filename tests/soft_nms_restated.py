"""NumPy restatement of the rescoring NMS (include/effdet_hip.h: effdet_soft_nms) for ONE image, in two forms, and a validator.

``run_f32`` does every operation in np.float32 in the kernel's order: bit-reproducible for 'hard' and 'linear' (IEEE add, multiply,
divide); for 'gaussian' only expf differs by an ulp or so, which is what ``check_run`` is for.  ``run_f64`` is the float64 form.

``check_run`` replays the DEVICE's own pick order in float64, so it needs no score-gap condition on the inputs: every pick must have
been live, (nearly) the best live candidate, and carry (nearly) the float64 score.
"""
import collections

import numpy as np

Opts = collections.namedtuple('Opts', 'threshold iou_threshold method sigma class_aware pre_nms_top_n max_det')
Opts.__new__.__defaults__ = (0.5, False, 1000, 100)          # sigma, class_aware, pre_nms_top_n, max_det


def sorted_candidates(score, threshold, top_n):
    """Anchor indices with score > threshold (NaN excluded) by descending score, ties by index -- by the kernel's own 32-bit key
    (ascending ~orderable(score), stable) -- cut to the first top_n."""
    s = np.ascontiguousarray(score, dtype=np.float32)
    cand = np.nonzero(s > np.float32(threshold))[0]
    u = s[cand].view(np.uint32)
    u = u ^ np.where(u >> np.uint32(31), np.uint32(0xffffffff), np.uint32(0x80000000))
    order = cand[np.argsort(~u, kind='stable')]
    return order[:int(top_n)]


class _State:
    """Candidates of one image in sorted order with running scores of type T; pick(p) applies one pick's rescoring."""

    def __init__(self, boxes, score, label, o, T, dead_slack=0.0):
        self.o, self.T = o, T
        self.order = sorted_candidates(score, o.threshold, o.pre_nms_top_n)
        b32 = np.ascontiguousarray(boxes, dtype=np.float32)[self.order]
        with np.errstate(all='ignore'):
            a32 = (b32[:, 2] - b32[:, 0]) * (b32[:, 3] - b32[:, 1])
            self.ok = (a32 > 0) & (a32 < np.inf)                       # the stored fp32 area decides, in both forms
            self.b = b32.astype(T)
            self.area = (self.b[:, 2] - self.b[:, 0]) * (self.b[:, 3] - self.b[:, 1])
        self.s = np.asarray(score, dtype=np.float32)[self.order].astype(T)
        self.lab = np.asarray(label)[self.order] if o.class_aware else np.zeros(len(self.order), dtype=np.int64)
        self.live = np.ones(len(self.order), dtype=bool)
        self.thr = T(np.float32(o.threshold))
        self.dead_below = self.thr - T(dead_slack) * abs(self.thr)     # (validator: a candidate dies a little below the threshold)
        self.iou_thr, self.sigma = T(np.float32(o.iou_threshold)), T(np.float32(o.sigma))

    def best(self):
        """Position of the live candidate with the largest running score (ties: smallest position), or -1."""
        if not self.live.any():
            return -1
        return int(np.argmax(np.where(self.live, self.s, -np.inf)))

    def pick(self, p):
        T, b = self.T, self.b
        self.live[p] = False
        m = self.live & self.ok & bool(self.ok[p]) & (self.lab == self.lab[p])
        if not m.any():
            return
        with np.errstate(all='ignore'):
            iw = np.fmin(b[p, 2], b[:, 2]) - np.fmax(b[p, 0], b[:, 0])
            ih = np.fmin(b[p, 3], b[:, 3]) - np.fmax(b[p, 1], b[:, 1])
            inter = iw * ih
            iou = np.where((iw <= 0) | (ih <= 0), T(0), inter / (self.area[p] + self.area - inter))
            if self.o.method == 'hard':
                self.live &= ~(m & (iou > self.iou_thr))
            elif self.o.method == 'linear':
                u = m & (iou > self.iou_thr)
                self.s[u] = self.s[u] * (T(1) - iou[u])
            else:
                assert self.o.method == 'gaussian', self.o.method
                self.s[m] = self.s[m] * np.exp(-(iou[m] * iou[m]) / self.sigma)
            self.live &= ~(m & ~(self.s > self.dead_below))


def _run(boxes, score, label, o, T):
    st = _State(boxes, score, label, o, T)
    idx, out = [], []
    for _ in range(int(o.max_det)):
        p = st.best()
        if p < 0:
            break
        idx.append(int(st.order[p])); out.append(st.s[p])
        st.pick(p)
    return np.asarray(idx, dtype=np.int32), np.asarray(out, dtype=T), len(idx)


def run_f32(boxes, score, label, o):
    """-> (idx [count] int32 anchor indices in pick order, scores [count] float32, count) of one image, all arithmetic in float32."""
    return _run(boxes, score, label, o, np.float32)


def run_f64(boxes, score, label, o):
    return _run(boxes, score, label, o, np.float64)


def check_run(boxes, score, label, o, dev_idx, dev_score, dev_count, tol):
    """Assert that (dev_idx, dev_score, dev_count) is a valid run of the pick loop on one image within relative tolerance tol, by
    replaying ITS pick order in float64.  -> the largest relative deviation |dev_score - s64| / s64 seen."""
    st = _State(boxes, score, label, o, np.float64, dead_slack=tol)
    count = int(dev_count)
    assert 0 <= count <= int(o.max_det), (count, o.max_det)
    pos = {int(a): p for p, a in enumerate(st.order)}
    worst = 0.0
    for k in range(count):
        a = int(dev_idx[k])
        assert a in pos, 'pick %d: anchor %d is not among the top-N candidates' % (k, a)
        p = pos[a]
        assert st.live[p], 'pick %d: anchor %d was not live (picked before, or suppressed)' % (k, a)
        s64 = float(st.s[p])
        top = float(st.s[st.live].max())
        assert s64 >= (1.0 - tol) * top, 'pick %d: anchor %d has float64 score %.9g, the live maximum is %.9g' % (k, a, s64, top)
        dev = abs(float(dev_score[k]) - s64)
        assert dev <= tol * abs(s64), 'pick %d: device score %.9g, float64 %.9g (rel %.3g > %.3g)' % (k, float(dev_score[k]), s64, dev / abs(s64), tol)
        worst = max(worst, dev / abs(s64) if s64 else 0.0)
        st.pick(p)
    if count < int(o.max_det):
        left = st.live & (st.s > st.thr + tol * abs(st.thr))
        assert not left.any(), 'stopped after %d picks with %d live candidates above the threshold (best %.9g)' % (
            count, int(left.sum()), float(st.s[left].max()))
    return worst
