"""NumPy restatement of the weighted boxes fusion (include/effdet_wbf.h: effdet_wbf) for ONE image, in two forms.

``run_f32`` does every operation in np.float32 in the kernel's order (IEEE add, subtract, multiply, divide, min / max, nothing
contracted): the device must equal it bit for bit.  ``run_f64`` is the float64 twin: the same inputs (fp32 values), the same
participation and candidate order (both decided by the fp32 values, as on the device), every later operation in float64.

A view of one image is (score [A], label [A], boxes [A, 4], count); ``run_*`` return a ``Run``:
  clusters  per cluster, in founding order: the (view, row) members in joining order
  boxes, avg, max, label   per cluster, in founding order: fused box, the two scores, label
  margin    the smallest distance over all decisions of the best IoU from iou_thr and, where the candidate joined, from the runner-up
``emit(run, conf_type)`` orders the clusters as the device emits them -> (score [n], label [n] int64, boxes [n, 4]).
"""
import collections

import numpy as np

Opts = collections.namedtuple('Opts', 'iou_thr skip_thr top_n')
Opts.__new__.__defaults__ = (0.55, 0.0, 1000)
Run = collections.namedtuple('Run', 'clusters boxes avg max label margin T')


def _transform(b, flip, mul, T):
    b = b.astype(T)
    if flip is not None:
        w = T(np.float32(flip))
        b = np.stack([w - b[:, 2], b[:, 1], w - b[:, 0], b[:, 3]], 1)
    return b * T(np.float32(mul))


def candidates(views, weights, flips, muls, o, T):
    """The image's candidates in the kernel's order -> (boxes [M,4] T, conf [M] T, label [M], view [M], row [M])."""
    f32 = np.float32
    bs, cs, ls, vs, rs, c32 = [], [], [], [], [], []
    with np.errstate(all='ignore'):
        for v, (s, l, b, n) in enumerate(views):
            s = np.ascontiguousarray(s, dtype=f32); b = np.ascontiguousarray(b, dtype=f32).reshape(-1, 4); l = np.asarray(l)
            n = max(0, min(int(n), int(o.top_n), len(s)))
            s, l, b = s[:n], l[:n], b[:n]
            b32 = _transform(b, flips[v], muls[v], f32)
            conf32 = s * f32(weights[v])
            area32 = (b32[:, 2] - b32[:, 0]) * (b32[:, 3] - b32[:, 1])
            ok = (s >= f32(o.skip_thr)) & (conf32 > 0) & (conf32 < np.inf) & (area32 > 0) & (area32 < np.inf)
            r = np.nonzero(ok)[0]
            bs.append(_transform(b, flips[v], muls[v], T)[r]); cs.append(s[r].astype(T) * T(f32(weights[v])))
            ls.append(l[r].astype(np.int64)); vs.append(np.full(len(r), v)); rs.append(r); c32.append(conf32[r])
    b, c, l, v, r, c32 = (np.concatenate(x) for x in (bs, cs, ls, vs, rs, c32))
    order = np.lexsort((r, v, ~np.ascontiguousarray(c32, dtype=f32).view(np.uint32)))      # conf descending, view, row
    return b[order], c[order], l[order], v[order], r[order]


def _run(views, weights, flips, muls, o, T):
    V = len(views)
    flips = [None] * V if flips is None else flips
    muls = [1.0] * V if muls is None else muls
    weights = [1.0] * V if weights is None else weights
    cb, cc, cl, cv, cr = candidates(views, weights, flips, muls, o, T)
    M = len(cc)
    thr = T(np.float32(o.iou_thr))
    fb = np.zeros((M, 4), T); S = np.zeros((M, 4), T); sc = np.zeros(M, T); cmax = np.zeros(M, T)
    cnt = np.zeros(M, np.int64); lab = np.zeros(M, np.int64)
    members, ncl, margin = [], 0, np.inf
    with np.errstate(all='ignore'):
        for i in range(M):
            b, c = cb[i], cc[i]
            best, b1 = -1, T(-np.inf)
            if ncl:
                F = fb[:ncl]
                iw = np.fmin(F[:, 2], b[2]) - np.fmax(F[:, 0], b[0])
                ih = np.fmin(F[:, 3], b[3]) - np.fmax(F[:, 1], b[1])
                inter = iw * ih
                fa = (F[:, 2] - F[:, 0]) * (F[:, 3] - F[:, 1])
                ca = (b[2] - b[0]) * (b[3] - b[1])
                iou = np.where((iw <= 0) | (ih <= 0), T(0), inter / (fa + ca - inter))
                iou = np.where((lab[:ncl] == cl[i]) & (iou == iou), iou, T(-np.inf))
                best = int(np.argmax(iou)); b1 = iou[best]                     # (the first of equal maxima: the lowest cluster index)
                if b1 > -np.inf:
                    margin = min(margin, abs(float(b1) - float(thr)))
                    if b1 > thr and ncl > 1:
                        iou[best] = -np.inf
                        margin = min(margin, float(b1) - float(iou.max()))
            if b1 > thr:
                S[best] = S[best] + c * b
                sc[best] = sc[best] + c; cmax[best] = max(cmax[best], c); cnt[best] += 1
                fb[best] = S[best] / sc[best]
                members[best].append((int(cv[i]), int(cr[i])))
            else:
                S[ncl] = c * b; sc[ncl] = c; cmax[ncl] = c; cnt[ncl] = 1; lab[ncl] = cl[i]; fb[ncl] = b
                members.append([(int(cv[i]), int(cr[i]))]); ncl += 1
        w = [T(np.float32(x)) for x in weights]
        wsum = T(0)
        for x in w:
            wsum = wsum + x
        n = cnt[:ncl]
        avg = ((sc[:ncl] / n.astype(T)) * np.minimum(n, V).astype(T)) / wsum
        mx = cmax[:ncl] / max(w)
    return Run(members, fb[:ncl].copy(), avg, mx, lab[:ncl].copy(), margin, T)


def run_f32(views, weights=None, flips=None, muls=None, o=Opts()):
    return _run(views, weights, flips, muls, o, np.float32)


def run_f64(views, weights=None, flips=None, muls=None, o=Opts()):
    return _run(views, weights, flips, muls, o, np.float64)


def emit(run, conf_type='avg'):
    """The clusters by score descending, then cluster index -> (score [n], label [n] int64, boxes [n, 4])."""
    s = run.avg if conf_type == 'avg' else run.max
    if run.T is np.float32:                              # the kernel's own key: ascending ~bits (scores are >= 0), then index
        order = np.lexsort((np.arange(len(s)), ~np.ascontiguousarray(s).view(np.uint32)))
    else:
        order = np.lexsort((np.arange(len(s)), -s))
    return s[order], run.label[order], run.boxes[order]
