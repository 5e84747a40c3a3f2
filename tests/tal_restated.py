"""The task-aligned matcher of include/effdet_tal.h restated in NumPy, twice:

  the FLOAT form (`metrics`, `assign`, `target`): pairs, candidates, selection, conflicts and the aligned target on the fp32 inputs taken
      into float64 (the reference) or kept in float32 (the same lines: the yardstick that sizes the metric tolerance).  The centre test
      is tests/atss_restated.inside in float32 in either precision: it involves only fp32 subtract, add and a multiply by 0.5, so it
      is the device's decision bit for bit;
  the INTEGER form (`assign_bits`): selection and conflicts on the BIT PATTERNS of m and u alone -- no floating-point operation at
      all -- which reproduces the device's winners and codes exactly when it is fed the device's own planes.

`gaps` measures the float64 decision gaps of a case: where every gap is exactly 0 (equal operands: the index rule decides) or at
least GAP relative, the float64 codes are the only admissible device answer.
From the codes (and q) on, the loss and its gradients are tests/loss_options_restated.py / tests/quality_loss_restated.py."""
import numpy as np
import torch

from tests import atss_restated as AR
from tests import box_loss_restated as BR
from tests import loss_cases as LC
from tests import loss_options_restated as R
from tests import quality_loss_restated as QR

DEFAULTS = dict(topk=13, alpha=1.0, beta=6.0, aligned_target=True)
MAX_TOPK = 16
NO_KEY = (1 << 64) - 1
GAP = 1e-3
TINY = 1e-30                                         # a winner's float64 metric below this could underflow in fp32


def options(**kw):
    assert set(kw) <= set(DEFAULTS), kw
    o = dict(DEFAULTS)
    o.update(kw)
    return o


def _pow(x, e, dtype):
    """exp2(e * log2(x)), 0 at x == 0."""
    with np.errstate(divide='ignore', invalid='ignore'):
        safe = np.where(x == 0, dtype(1), x)
        return np.where(x == 0, dtype(0), np.exp2(dtype(np.float32(e)) * np.log2(safe))).astype(dtype)


def overlap(anc, box, r, dtype):
    """[A] u: effdet_box_loss.h's decode and overlap between the decoded predictions r [A, 4] of the anchors [A, 4] and the box [4],
    clamped to [0, 1], NaN for a non-finite r."""
    anc, box, r = anc.astype(dtype), box.astype(dtype), r.astype(dtype)
    c = lambda v: dtype(v)      # noqa: E731  (the fp32 constants, taken as they are into either precision)
    aw, ah = anc[:, 2] - anc[:, 0], anc[:, 3] - anc[:, 1]
    acx, acy = anc[:, 0] + c(0.5) * aw, anc[:, 1] + c(0.5) * ah
    pcx, pcy = acx + c(BR.STD_XY) * r[:, 0] * aw, acy + c(BR.STD_XY) * r[:, 1] * ah
    pw = np.exp(np.minimum(c(BR.STD_WH) * r[:, 2], c(BR.DW_MAX))) * aw
    ph = np.exp(np.minimum(c(BR.STD_WH) * r[:, 3], c(BR.DW_MAX))) * ah
    px1, px2, py1, py2 = pcx - c(0.5) * pw, pcx + c(0.5) * pw, pcy - c(0.5) * ph, pcy + c(0.5) * ph
    iw = np.maximum(np.minimum(px2, box[2]) - np.maximum(px1, box[0]), c(0))
    ih = np.maximum(np.minimum(py2, box[3]) - np.maximum(py1, box[1]), c(0))
    inter = iw * ih
    iou = inter / (pw * ph + (box[2] - box[0]) * (box[3] - box[1]) - inter + c(BR.EPS))
    return (np.clip(iou, c(0), c(1)) + (r - r).sum(1)).astype(dtype)


def row_label(case, b, n):
    """The class index of row n of image b, or -1 for a pad row or a label outside [0, nc)."""
    lab = float(case['ann'][b, n, 4])
    return int(lab) if lab != -1.0 and 0.0 <= lab < case['cls'].shape[2] else -1


def inside(case, b, n):
    """[A] bool: the centre test of row n, as the device decides it."""
    return AR.inside(case['anc'][0].numpy(), case['ann'][b, n, :4].numpy()) > AR.INSIDE


def metrics(case, tal, dtype=np.float64):
    """-> (m, u), each [B, N, A] (dtype): the pair quantities where the anchor's centre is inside the row, 0 elsewhere, for a pad row
    and for a label outside the classes."""
    B, A, nc = case['cls'].shape
    N = case['ann'].shape[1]
    m, u = np.zeros((B, N, A), dtype), np.zeros((B, N, A), dtype)
    anc = case['anc'][0].numpy()
    for b in range(B):
        for n in range(N):
            lab = row_label(case, b, n)
            if lab < 0:
                continue
            ins = inside(case, b, n)
            uu = overlap(anc, case['ann'][b, n, :4].numpy(), case['reg'][b].numpy(), dtype)
            s = case['cls'][b, :, lab].numpy().astype(dtype)
            mm = (_pow(s, tal['alpha'], dtype) * _pow(uu, tal['beta'], dtype)).astype(dtype)
            m[b, n], u[b, n] = np.where(ins, mm, dtype(0)), np.where(ins, uu, dtype(0))
    return m, u


def valid_rows(case, b):
    return [n for n in range(case['ann'].shape[1]) if float(case['ann'][b, n, 4]) != -1.0]


def select(m_row, topk):
    """-> the anchors of the min(topk, #candidates) candidates of one row (m_row [A], 0 off the inside set) under the key (largest m,
    then lowest index); a NaN is no candidate."""
    cand = np.nonzero(m_row > 0)[0]
    order = cand[np.argsort(-m_row[cand], kind='stable')]      # (cand ascends: a stable sort keeps the lower index first on a tie)
    return order[:topk].tolist()


def assign(case, tal, m=None, u=None):
    """The float64 form -> dict: codes int64 [B, A], winners {(b, n): [anchors in rank order]}, num_pos [B], m, u."""
    if m is None:
        m, u = metrics(case, tal, np.float64)
    B, N, A = m.shape
    codes = torch.full((B, A), LC.CODE_IGN, dtype=torch.int64)
    winners = {}
    for b in range(B):
        rows = valid_rows(case, b)
        if not rows:
            continue
        best, arg = np.full(A, -1.0), np.full(A, -1, dtype=np.int64)
        for n in rows:
            w = winners[(b, n)] = select(m[b, n], tal['topk'])
            for a in w:
                if u[b, n, a] > best[a]:                       # strict: the first row keeps a tie
                    best[a], arg[a] = u[b, n, a], n
        codes[b] = torch.from_numpy(arg)
    return {'codes': codes, 'winners': winners, 'num_pos': (codes >= 0).sum(1), 'm': m, 'u': u}


def assign_bits(mbits, ubits, rows, topk):
    """The INTEGER form for one image: mbits, ubits uint32 [N, A] (the bit patterns of the metric and IoU planes), rows the valid rows.
    -> (keys {n: [64-bit keys in rank order]}, codes int64 [A] with -1 where no row selected the anchor).  A candidate has
    0 < bits(m) <= bits(+inf): positive and no NaN."""
    A = mbits.shape[1]
    claim = np.zeros(A, dtype=np.uint64)
    keys = {}
    idx = np.arange(A, dtype=np.uint64)
    for n in rows:
        mb = mbits[n].astype(np.uint64)
        cand = (mb > 0) & (mb <= 0x7F800000)
        k = (((~mb) & np.uint64(0xFFFFFFFF)) << np.uint64(32)) | idx
        chosen = np.sort(k[cand])[:topk]
        keys[n] = [int(v) for v in chosen]
        a = (chosen & np.uint64(0xFFFFFFFF)).astype(np.int64)
        c = (ubits[n, a].astype(np.uint64) << np.uint64(32)) | np.uint64(0xFFFFFFFF - n)
        claim[a] = np.maximum(claim[a], c)                     # (a row selects an anchor once: no duplicate indices)
    codes = np.where(claim != 0, 0xFFFFFFFF - (claim & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)
    return keys, codes


def target(mbits, ubits, codes, keys):
    """The aligned target of one image in float32 from bit patterns: mbits, ubits uint32 [N, A], codes [A], keys from assign_bits.
    -> (q float32 [A], mm {n: (mmax, umax)} for the rows with a finally assigned anchor)."""
    A = mbits.shape[1]
    q = np.zeros(A, np.float32)
    mm = {}
    for n, ks in keys.items():
        a = np.array([k & 0xFFFFFFFF for k in ks if codes[k & 0xFFFFFFFF] == n], dtype=np.int64)
        if len(a) == 0:
            continue
        mv, uv = mbits[n, a].view(np.float32), ubits[n, a].view(np.float32)
        mmax, umax = mv.max(), uv.max()
        q[a] = (mv * umax) / (mmax + np.float32(1e-9))
        mm[n] = (mmax, umax)
    return q, mm


def gaps(case, tal):
    """The float64 decision gaps of a case -> (smallest non-zero relative gap, smallest winner metric): between the k-th and the
    (k+1)-th candidate metric of every row and between the best and the second-best u at every anchor that several rows selected."""
    r = assign(case, tal)
    m, u = r['m'], r['u']
    worst, least = np.inf, np.inf
    claims = {}
    for (b, n), w in r['winners'].items():
        if not w:
            continue
        least = min(least, float(m[b, n, w].min()))
        cand = np.sort(m[b, n][m[b, n] > 0])[::-1]
        k = len(w)
        if len(cand) > k and cand[k - 1] != cand[k]:
            worst = min(worst, float((cand[k - 1] - cand[k]) / cand[k - 1]))
        for a in w:
            claims.setdefault((b, a), []).append(float(u[b, n, a]))
    for us in claims.values():
        if len(us) > 1:
            us = sorted(us, reverse=True)
            if us[0] != us[1]:
                worst = min(worst, (us[0] - us[1]) / us[0])
    return worst, least


def downstream(case, codes, q, opts, qo=None, box=None, gscale=(1.0, 1.0), dtype=torch.float64):
    """The loss and its gradients on given codes and (with a quality loss qo) given targets q [B, A]: tests/loss_options_restated.run,
    and tests/quality_loss_restated.run's class term with q in the place of its IoU.  -> its dict."""
    base = R.run(case, opts, box=box, gscale=gscale, dtype=dtype, codes=codes)
    if qo is None:
        return base
    B, A, nc = case['cls'].shape
    q = q.to(dtype)
    cls = case['cls'].to(dtype)
    cl, dlogit = [], torch.zeros(B, A, nc, dtype=dtype)
    for b in range(B):
        p = cls[b]
        if not bool((case['ann'][b, :, 4] != -1).any()):
            cl.append(torch.zeros((), dtype=dtype))
            dlogit[b] = p - p
            continue
        norm = max(int(base['num_pos'][b]), 1)
        l, d = QR.elements_grad(p, QR.targets(case, codes, q, b), qo)
        live = (codes[b] != LC.CODE_IGN)[:, None]
        cl.append(torch.where(live, l, torch.zeros_like(l)).sum() / norm)
        dlogit[b] = torch.where(live, gscale[0] / (B * norm) * d * p * (1 - p), p - p)
    losses = torch.stack([torch.stack(cl).mean().double(), base['losses'][1]])
    return {'losses': losses, 'codes': codes, 'num_pos': base['num_pos'], 'q': q, 'dlogit': dlogit, 'dreg': base['dreg']}
