"""NumPy restatement of include/effdet_op_point.h, written from the header's text (not from csrc/op_point.hip): the records of
effdet_voc_match, the confidence curves of effdet_op_curves and the confusion matrix of effdet_confusion_match.  Counts are integers;
every fp64 value is produced by single NumPy scalar operations in the header's order, and the sums of the means are Python loops."""
import numpy as np

EPS = np.finfo(np.float64).eps
MAX_THRESHOLDS = 4096
MAX_GT = 2048


def score_key(s):
    """csrc/radix_sort.h's descending-score key of fp32 scores -> uint32 (ascending keys = descending scores, +0 before -0)."""
    u = np.asarray(s, dtype=np.float32).reshape(-1).view(np.uint32).astype(np.uint64)
    u = np.where(u >> np.uint64(31), u ^ np.uint64(0xffffffff), u ^ np.uint64(0x80000000))
    return ((~u) & np.uint64(0xffffffff)).astype(np.uint32)


def iou_row(box, gts):
    """effdet_voc_match's fp64 IoU of one box against gts [g, 4], in its operation order."""
    a = np.asarray(box, dtype=np.float64)
    g = np.asarray(gts, dtype=np.float64).reshape(-1, 4)
    area = (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1])
    iw = np.minimum(a[2], g[:, 2]) - np.maximum(a[0], g[:, 0])
    ih = np.minimum(a[3], g[:, 3]) - np.maximum(a[1], g[:, 1])
    iw = np.maximum(iw, 0.0)
    ih = np.maximum(ih, 0.0)
    ua = (a[2] - a[0]) * (a[3] - a[1]) + area - iw * ih
    ua = np.maximum(ua, EPS)
    return iw * ih / ua


def _int_label(v, C):
    """label value -> class in [0, C) when it is an integer there, else -1"""
    return int(v) if 0 <= v < C and v == np.floor(v) else -1


def _rows(dets, counts, b):
    d = np.asarray(dets, dtype=np.float32)
    n = min(max(int(counts[b]), 0), d.shape[1])
    return d[b, :n]


def _objects(gt, C):
    g = np.asarray(gt, dtype=np.float64).reshape(-1, 5)
    lab = np.array([_int_label(v, C) for v in g[:, 4]], dtype=np.int64)
    return g[:, :4], lab


def voc_records(dets, counts, gts, C, iou_threshold=0.5):
    """effdet_voc_match: dets [B, max_det, 6] fp32, counts [B], gts: B arrays [g, 5] -> (key uint64 [B * max_det], tp uint8, gt_count
    int32 [C])."""
    dets = np.asarray(dets, dtype=np.float32)
    B, S = dets.shape[:2]
    key = np.full(B * S, (C << 32) | 0xffffffff, dtype=np.uint64)
    tp = np.zeros(B * S, dtype=np.uint8)
    gt_count = np.zeros(C, dtype=np.int32)
    for b in range(B):
        gb, gl = _objects(gts[b], C)
        for c in gl[gl >= 0]:
            gt_count[c] += 1
        taken = set()
        for k, r in enumerate(_rows(dets, counts, b)):
            c = _int_label(r[5], C)
            if c < 0:
                continue
            key[b * S + k] = (np.uint64(c) << np.uint64(32)) | np.uint64(score_key(r[4])[0])
            own = np.nonzero(gl == c)[0]
            if len(own) == 0:
                continue
            ov = iou_row(r[:4], gb[own])
            a = int(np.argmax(ov))                                 # first maximum
            if ov[a] >= iou_threshold and (c, own[a]) not in taken:
                taken.add((c, own[a]))
                tp[b * S + k] = 1
    return key, tp, gt_count


def check_thresholds(thresholds=None):
    """The host-side rule of the binding: default grid, else 1..4096 finite strictly ascending fp32 values, -0.0 -> +0.0."""
    if thresholds is None:
        return (np.arange(1001) / 1000).astype(np.float32)
    t = np.array(thresholds, dtype=np.float32).reshape(-1)
    if not 1 <= t.size <= MAX_THRESHOLDS or not np.all(np.isfinite(t)) or not np.all(t[1:] > t[:-1]):
        raise ValueError('thresholds')
    t[t == 0] = 0.0
    return t


def curves(key, tp_byte, gt_count, C, thresholds):
    """effdet_op_curves over the records -> dict(tp, npred int32 [C, M]; precision, recall, f1 fp64 [C, M]; mean [3, M]; best [C + 1, 4])."""
    key = np.asarray(key, dtype=np.uint64)
    th = np.asarray(thresholds, dtype=np.float32)
    M = len(th)
    order = np.argsort(key, kind='stable')
    skey, stp = key[order], np.asarray(tp_byte, dtype=np.int64)[order]
    cls, low = (skey >> np.uint64(32)).astype(np.int64), (skey & np.uint64(0xffffffff)).astype(np.int64)
    tkey = score_key(th).astype(np.int64)
    tp = np.zeros((C, M), dtype=np.int32); npred = np.zeros((C, M), dtype=np.int32)
    P = np.zeros((C, M)); R = np.zeros((C, M)); F = np.zeros((C, M))
    for c in range(C):
        seg_low, seg_tp = low[cls == c], stp[cls == c]
        cum = np.concatenate([[0], np.cumsum(seg_tp)])           # integers: exact
        n = int(gt_count[c])
        for j in range(M):
            k = int(np.count_nonzero(seg_low < tkey[j]))           # the segment is key-ascending: a prefix
            assert np.all(seg_low[:k] < tkey[j])
            t = int(cum[k])
            npred[c, j], tp[c, j] = k, t
            p = np.float64(1.0) if k == 0 else np.float64(t) / np.float64(k)
            r = np.float64(0.0) if n == 0 else np.float64(t) / np.float64(n)
            s = p + r
            P[c, j], R[c, j], F[c, j] = p, r, (np.float64(0.0) if s == 0 else (np.float64(2.0) * p * r) / s)
    with_gt = [c for c in range(C) if gt_count[c] > 0]
    mean = np.zeros((3, M))
    for q, A in enumerate((P, R, F)):
        for j in range(M):
            acc = np.float64(0.0)
            for c in with_gt:
                acc = acc + A[c, j]
            mean[q, j] = acc / np.float64(len(with_gt)) if with_gt else 0.0
    best = np.zeros((C + 1, 4))
    best[:, 0] = -1
    for c in with_gt:
        j = int(np.argmax(F[c]))                                   # first maximum
        best[c] = j, P[c, j], R[c, j], F[c, j]
    if with_gt:
        j = int(np.argmax(mean[2]))
        best[C] = j, mean[0, j], mean[1, j], mean[2, j]
    return {'tp': tp, 'npred': npred, 'precision': P, 'recall': R, 'f1': F, 'mean': mean, 'best': best}


def confusion(dets, counts, gts, C, conf_threshold=0.25, iou_threshold=0.45):
    """effdet_confusion_match over a batch -> int64 [C + 1, C + 1] (row = predicted class, column = true class, C = background)."""
    dets = np.asarray(dets, dtype=np.float32)
    m = np.zeros((C + 1, C + 1), dtype=np.int64)
    conf = np.float32(conf_threshold)
    for b in range(dets.shape[0]):
        gb, gl = _objects(gts[b], C)
        obj = np.nonzero(gl >= 0)[0]
        kept = {}                                                  # object row -> [(iou, prediction row)]
        preds = []
        for k, r in enumerate(_rows(dets, counts, b)):
            c = _int_label(r[5], C)
            if c < 0 or not r[4] > conf:
                continue
            preds.append((k, c))
            if len(obj) == 0:
                continue
            ov = iou_row(r[:4], gb[obj])
            a = int(np.argmax(ov))                                 # the largest IoU, the first such object in GT row order
            if ov[a] > iou_threshold:
                kept.setdefault(int(obj[a]), []).append((ov[a], k))
        winner = {}                                                # prediction row -> object row
        for o, cand in kept.items():
            top = max(v for v, _ in cand)
            winner[min(k for v, k in cand if v == top)] = o        # the largest IoU, the lowest row among equals
        for k, c in preds:
            m[c, gl[winner[k]] if k in winner else C] += 1
        for o in obj:
            if int(o) not in winner.values():
                m[C, gl[o]] += 1
    return m
