"""NumPy fp32 restatement of sliced inference (include/effdet_slices.h), written from the header: the tile plan of ops.slice_plan, the
tile extractor effdet_slice_images and the cross-tile merge effdet_slice_merge.  Every arithmetic step is one NumPy fp32 operation in
the header's order (NumPy contracts nothing), so the device results must equal these bit for bit.

A table is a list of (y0, x0, h, w, my, mx) records, ops.slice_plan's format."""
import collections
import math

import numpy as np

F = np.float32
MAX_IN, MAX_TILES = 8192, 1024


# ----------------------------------------------------------------------------------------------------------------------------- plan
def positions(L, s, ratio):
    """Tile origins along an axis of length L: k * step while k * step + s < L, then L - s."""
    if L < s:
        raise ValueError('axis %d is smaller than the slice %d' % (L, s))
    step = s - int(math.floor(ratio * s))
    pos = [k * step for k in range(L) if k * step + s < L]
    return pos + [L - s]


def plan(H, W, slice_hw, overlap, full_view=True):
    h, w = slice_hw
    out = [(y, x, h, w, 1.0, 1.0) for y in positions(H, h, overlap[0]) for x in positions(W, w, overlap[1])]
    if full_view and (H, W) != (h, w):
        out.append((0, 0, h, w, float(F(float(H) / float(h))), float(F(float(W) / float(w)))))
    return out


# --------------------------------------------------------------------------------------------------------------------------- slicer
def slice_images(src, table, t0, t1, ce):
    """src [B][H][W][3] of any dtype (channels 0..2 of every source pixel) -> [t1 - t0][h][w][ce]: flat tile t = b * T + j is
    src(b, clamp(y0 + oy), clamp(x0 + ox)) copied as it is, channels 3..ce-1 zero bits.  All tiles of a table share (h, w)."""
    B, H, W, _ = src.shape
    T = len(table)
    h, w = table[0][2], table[0][3]
    out = np.zeros((t1 - t0, h, w, ce), dtype=src.dtype)
    for t in range(t0, t1):
        b, j = divmod(t, T)
        y0, x0 = int(table[j][0]), int(table[j][1])
        ys = np.clip(y0 + np.arange(h, dtype=np.int64), 0, H - 1)
        xs = np.clip(x0 + np.arange(w, dtype=np.int64), 0, W - 1)
        out[t - t0, :, :, :3] = src[b][ys][:, xs]
    return out


# ---------------------------------------------------------------------------------------------------------------------------- merge
def score_key(s):
    """csrc/radix_sort.h's rs_score_key: ascending order of the keys is descending order of the scores (+0 before -0)."""
    u = np.asarray(s, dtype=F).view(np.uint32)
    u = np.where(u >> 31, ~u, u ^ np.uint32(0x80000000))
    return ~u


Run = collections.namedtuple('Run', 'score label boxes keepers absorbed own')
# score / label / boxes: the emitted rows; keepers: [(tile, row)]; absorbed: per keeper [(tile, row)] of what it took; own: the keepers'
# own transformed boxes (boxes differs from it only under 'nmm')


def candidates(score, label, boxes, count, table, W, H, skip_thr):
    """Steps 1 and 2 for one image: score [TPI][R], label [TPI][R] int64, boxes [TPI][R][4], count [TPI] -> (boxes [M][4] transformed
    and clipped, score [M], label [M], tile [M], row [M]) of the survivors in order."""
    score, boxes, label = np.asarray(score, dtype=F), np.asarray(boxes, dtype=F), np.asarray(label, dtype=np.int64)
    TPI, R = score.shape
    assert len(table) == TPI and 1 <= TPI <= MAX_TILES and TPI * R <= MAX_IN
    mx = np.asarray([r[5] for r in table], dtype=F)[:, None]
    my = np.asarray([r[4] for r in table], dtype=F)[:, None]
    fx = np.asarray([r[1] for r in table], dtype=np.int32).astype(F)[:, None]
    fy = np.asarray([r[0] for r in table], dtype=np.int32).astype(F)[:, None]
    Wf, Hf, zero = F(W), F(H), F(0)
    with np.errstate(all='ignore'):
        t = np.empty_like(boxes)
        for k, (m, f, lim) in enumerate(((mx, fx, Wf), (my, fy, Hf), (mx, fx, Wf), (my, fy, Hf))):
            v = boxes[:, :, k] * m                                   # multiply,
            v = v + f                                                # then add: two roundings
            t[:, :, k] = np.fmax(np.fmin(v, lim), zero)              # fminf / fmaxf: a NaN loses
        area = (t[:, :, 2] - t[:, :, 0]) * (t[:, :, 3] - t[:, :, 1])
        rows = np.minimum(np.maximum(np.asarray(count, dtype=np.int64), 0), R)[:, None]
        part = (np.arange(R)[None, :] < rows) & (score >= F(skip_thr)) & np.isfinite(score) & (label >= 0) & (label < 65536) & \
            (area > 0) & np.isfinite(area)
    tile, row = np.nonzero(part)                                     # tile-major
    order = np.argsort(score_key(score[tile, row]), kind='stable')
    tile, row = tile[order], row[order]
    return t[tile, row], score[tile, row], label[tile, row], tile, row


def merge(score, label, boxes, count, table, W, H, method='nmm', metric='ios', thr=0.5, class_aware=True, skip_thr=0.0, max_det=300):
    """effdet_slice_merge for one image -> Run."""
    assert method in ('nms', 'nmm') and metric in ('iou', 'ios')
    tb, ts, tl, tile, row = candidates(score, label, boxes, count, table, W, H, skip_thr)
    M = len(ts)
    area = (tb[:, 2] - tb[:, 0]) * (tb[:, 3] - tb[:, 1])
    alive = np.ones(M, dtype=bool)
    thr = F(thr)
    keepers, absorbed, out_b = [], [], []
    for i in range(M):
        if not alive[i]:
            continue
        if len(keepers) == max_det:
            break
        alive[i] = False
        idx = np.nonzero(alive)[0]                                   # (every alive candidate is later than i)
        a = tb[i]
        with np.errstate(all='ignore'):
            iw = np.fmin(a[2], tb[idx, 2]) - np.fmax(a[0], tb[idx, 0])
            ih = np.fmin(a[3], tb[idx, 3]) - np.fmax(a[1], tb[idx, 1])
            inter = iw * ih
            if metric == 'ios':
                m = inter / np.fmin(area[i], area[idx])
            else:
                m = inter / ((area[i] + area[idx]) - inter)
            hit = (iw > 0) & (ih > 0) & (m > thr)
        if class_aware:
            hit &= tl[idx] == tl[i]
        took = idx[hit]
        alive[took] = False
        hull = a.copy()
        if method == 'nmm' and len(took):
            hull[0] = np.fmin(hull[0], tb[took, 0].min()); hull[1] = np.fmin(hull[1], tb[took, 1].min())
            hull[2] = np.fmax(hull[2], tb[took, 2].max()); hull[3] = np.fmax(hull[3], tb[took, 3].max())
        keepers.append(i); absorbed.append([(int(tile[q]), int(row[q])) for q in took]); out_b.append(hull)
    k = np.asarray(keepers, dtype=np.int64)
    return Run(ts[k], tl[k], np.asarray(out_b, dtype=F).reshape(-1, 4), [(int(tile[q]), int(row[q])) for q in k], absorbed, tb[k].reshape(-1, 4))


def merge_batch(score, label, boxes, count, table, W, H, max_det, **opts):
    """The whole batch in the entry point's output layout: (out_score [B][max_det], out_label, out_boxes [B][max_det][4], out_count [B]),
    zero rows past the count; and the Runs."""
    B = len(score)
    os_, ol, ob = np.zeros((B, max_det), dtype=F), np.zeros((B, max_det), dtype=np.int64), np.zeros((B, max_det, 4), dtype=F)
    oc, runs = np.zeros(B, dtype=np.int32), []
    for b in range(B):
        r = merge(score[b], label[b], boxes[b], count[b], table, W, H, max_det=max_det, **opts)
        n = len(r.score)
        os_[b, :n], ol[b, :n], ob[b, :n], oc[b] = r.score, r.label, r.boxes, n
        runs.append(r)
    return os_, ol, ob, oc, runs
