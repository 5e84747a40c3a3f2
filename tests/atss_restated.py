"""The ATSS matcher of include/effdet_atss.h restated in NumPy, in two forms:

  the float32 MIRROR: the key and the threshold spelled operation by operation in the header's order on np.float32 values (every
      operation rounds to fp32, nothing is fused), so its candidate sets are the device's bit for bit and its codes the device's
      wherever margin() holds;
  the float64 FORM: the same rules on the fp32 inputs taken into float64, which margin() measures distances with.

From the codes on, the loss and its gradients are tests/loss_options_restated.run(case, opts, codes=...): nothing is restated twice.
A case is a tests/loss_cases.py case dict plus level_start (list, level_start[-1] == A), topk and exact ([(image, anchor)])."""
import numpy as np
import torch

from tests import loss_cases as LC

INSIDE = np.float32(0.01)


def d2(anc, box, dtype=np.float32):
    """[A] squared centre distances of the anchors [A, 4] from the box [4]: cx = 0.5 (x1 + x2), dx = cx_a - cx_n, dx dx + dy dy."""
    anc, box = anc.astype(dtype), box.astype(dtype)
    half = dtype(0.5)
    acx = half * (anc[:, 0] + anc[:, 2])
    acy = half * (anc[:, 1] + anc[:, 3])
    gcx = half * (box[0] + box[2])
    gcy = half * (box[1] + box[3])
    dx = acx - gcx
    dy = acy - gcy
    xx = dx * dx
    yy = dy * dy
    return xx + yy


def iou(anc, box, dtype=np.float32):
    """assign_iou of loss.hip: iw ih / max(area_a + area_n - iw ih, 1e-8), iw and ih clamped at 0."""
    anc, box = anc.astype(dtype), box.astype(dtype)
    aarea = (anc[:, 2] - anc[:, 0]) * (anc[:, 3] - anc[:, 1])
    barea = (box[2] - box[0]) * (box[3] - box[1])
    iw = np.minimum(anc[:, 2], box[2]) - np.maximum(anc[:, 0], box[0])
    ih = np.minimum(anc[:, 3], box[3]) - np.maximum(anc[:, 1], box[1])
    iw = np.maximum(iw, dtype(0))
    ih = np.maximum(ih, dtype(0))
    inter = iw * ih
    ua = np.maximum(aarea + barea - inter, dtype(1e-8) if dtype is np.float64 else np.float32(1e-8))
    return inter / ua


def inside(anc, box, dtype=np.float32):
    """min(cx_a - x1, cy_a - y1, x2 - cx_a, y2 - cy_a): the quantity mmdet's centre test compares with 0.01."""
    anc, box = anc.astype(dtype), box.astype(dtype)
    half = dtype(0.5)
    acx = half * (anc[:, 0] + anc[:, 2])
    acy = half * (anc[:, 1] + anc[:, 3])
    return np.minimum(np.minimum(acx - box[0], acy - box[1]), np.minimum(box[2] - acx, box[3] - acy))


def candidates(anc, box, level_start, topk, dtype=np.float32):
    """-> global anchor indices of the row's candidates in level order, then rank order under the key (d2, index)."""
    dist = d2(anc, box, dtype)
    out = []
    for lo, hi in zip(level_start[:-1], level_start[1:]):
        order = np.lexsort((np.arange(hi - lo), dist[lo:hi]))             # by d2, a tie to the lower index
        out.extend((lo + order[:min(topk, hi - lo)]).tolist())
    return out


def threshold(ious, dtype=np.float32):
    """mean + sqrt(unbiased variance) of the candidates' IoUs, summed sequentially in the order given; variance 0 for m < 2."""
    m = len(ious)
    s = dtype(0)
    for v in ious:
        s = dtype(s + v)
    mean = dtype(s / dtype(m))
    q = dtype(0)
    for v in ious:
        d = dtype(v - mean)
        q = dtype(q + dtype(d * d))
    var = dtype(q / dtype(m - 1)) if m >= 2 else dtype(0)
    return dtype(mean + np.sqrt(var, dtype=dtype))


def rows_of(case, b):
    return [int(n) for n in torch.nonzero(case['ann'][b, :, 4] != -1).reshape(-1)]


def row_view(case, b, n, topk=None, dtype=np.float32, cand=None):
    """-> dict of row n of image b: cand (level then rank order), iou [m], thr, inside [m], pos (bool [m])."""
    anc = case['anc'][0].numpy()
    box = case['ann'][b, n, :4].numpy()
    topk = case['topk'] if topk is None else topk
    cand = candidates(anc, box, case['level_start'], topk, dtype) if cand is None else cand
    v = iou(anc[cand], box, dtype)
    thr = threshold(list(v), dtype)
    ins = inside(anc[cand], box, dtype)
    return {'cand': cand, 'iou': v, 'thr': thr, 'inside': ins, 'pos': (v >= thr) & (ins > dtype(INSIDE))}


def assign(case, topk=None):
    """The float32 mirror -> codes int64 [B, A]: LC.CODE_IGN in an image without a valid row, else LC.CODE_NEG or the row with the
    largest IoU among the rows the anchor is positive for (the first on a tie)."""
    B, A = case['cls'].shape[:2]
    code = torch.full((B, A), LC.CODE_IGN, dtype=torch.int64)
    for b in range(B):
        rows = rows_of(case, b)
        if not rows:
            continue
        code[b] = LC.CODE_NEG
        best = np.full(A, -1.0, dtype=np.float32)
        for n in rows:
            r = row_view(case, b, n, topk)
            for a, v, p in zip(r['cand'], r['iou'], r['pos']):
                if p and v > best[a]:                                     # strict: the first row keeps a tie
                    best[a] = v
                    code[b, a] = n
    return code


def margin(case, topk=None):
    """-> the float64 distance a rounding would have to bridge to change a code, over the float32 mirror's candidates with the `exact`
    anchors left out: per candidate the distance of its IoU from the row's threshold and of the centre quantity from 0.01 (a positive
    needs both to hold: the smaller; a candidate that fails: the larger of the failing tests'), and per anchor positive for several
    rows its best IoU from the runner-up row's.  (A single candidate's IoU IS its threshold, exactly: only its centre test counts.)"""
    m = 1.0
    B, A = case['cls'].shape[:2]
    exact = set(map(tuple, case.get('exact', [])))
    for b in range(B):
        claims = {}
        for n in rows_of(case, b):
            r32 = row_view(case, b, n, topk)
            r = row_view(case, b, n, topk, np.float64, cand=r32['cand'])
            for a, v, ins, p in zip(r['cand'], r['iou'], r['inside'], r['pos']):
                if (b, a) in exact:
                    continue
                d_iou, d_in = float(v - r['thr']), float(ins - np.float64(INSIDE))
                if len(r['cand']) == 1:
                    d_iou = 1.0                                           # m = 1: thr = (0 + iou) / 1 + 0 is the IoU itself in any precision
                fails = ([-d_iou] if d_iou < 0 else []) + ([-d_in] if d_in <= 0 else [])      # (>= passes the IoU, > the centre)
                m = min(m, min(d_iou, d_in) if p else max(fails))
                if p:
                    claims.setdefault(a, []).append(float(v))
        for a, vs in claims.items():
            if len(vs) > 1:
                vs = sorted(vs)
                m = min(m, vs[-1] - vs[-2])
    return m
