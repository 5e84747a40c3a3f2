"""The IoU-aware class losses of include/effdet_quality_loss.h restated in torch, in any precision: the assignment and the box term are
tests/loss_options_restated.py's (bands, low-quality matches; the ATSS codes of tests/atss_restated.py are passed in), decode and IoU
are tests/box_loss_restated.py's, and the class term -- the quality target q, the quality focal / varifocal loss per element and its
ANALYTIC derivative wrt the probability -- is written out here.  float64 is the reference of tests/test_gpu_quality_loss.py, float32
(the same code) the yardstick that sizes its tolerances; tests/test_quality_loss_host.py checks the analytic derivative against
torch.autograd of `elements` in float64.

The header fixes every quantity as fp32, so the constants are the fp32 ones taken as they are into either precision, and the powers are
spelled exp2(x * log2(u)) as the header spells them."""
import numpy as np
import torch

from tests import box_loss_restated as BR
from tests import loss_cases as LC
from tests import loss_options_restated as R

KINDS = ('qfl', 'vfl')
DEFAULTS = dict(kind='qfl', beta=2.0, alpha=0.75, gamma=2.0)


def _f32(v):
    return float(np.float32(v))


def options(**kw):
    """-> the full quality-loss dict (DEFAULTS overridden by kw)."""
    assert set(kw) <= set(DEFAULTS) and kw.get('kind', 'qfl') in KINDS, kw
    o = dict(DEFAULTS)
    o.update(kw)
    return o


def iou(anc, gt, r):
    """[P] the `overlap` line of include/effdet_box_loss.h after its `decode`: I / (U + 1e-7f)."""
    pcx, pcy, pw, ph = BR.decode(anc, r)
    px1, px2, py1, py2 = pcx - 0.5 * pw, pcx + 0.5 * pw, pcy - 0.5 * ph, pcy + 0.5 * ph
    gx1, gy1, gx2, gy2 = gt[:, 0], gt[:, 1], gt[:, 2], gt[:, 3]
    iw = torch.clamp(torch.minimum(px2, gx2) - torch.maximum(px1, gx1), min=0)
    ih = torch.clamp(torch.minimum(py2, gy2) - torch.maximum(py1, gy1), min=0)
    inter = iw * ih
    return inter / (pw * ph + (gx2 - gx1) * (gy2 - gy1) - inter + BR.EPS)


def quality(case, codes, dtype=torch.float64, reg=None):
    """-> q [B, A] (dtype): the clamped IoU at the positives of codes (NaN for a non-finite regression row), 0 elsewhere."""
    B, A = case['cls'].shape[:2]
    b, a, row = BR.positives(case, codes)
    r = (case['reg'] if reg is None else reg).to(dtype)[b, a]
    v = iou(case['anc'][0].to(dtype)[a], case['ann'].to(dtype)[b, row, :4], r).clamp(0, 1) + (r - r).sum(1)      # (torch.clamp keeps a NaN)
    q = torch.zeros(B, A, dtype=dtype)
    q[b, a] = v
    return q


def _pow(x, u):
    """exp2(x * log2(u)) for u > 0, 0 at u == 0 (with a zero derivative there)."""
    zero = u == 0
    return torch.where(zero, torch.zeros_like(u), torch.exp2(x * torch.log2(torch.where(zero, torch.ones_like(u), u))))


def elements(p, t, qo):
    """Per-element class loss for probabilities p and soft targets t (same shape): the forward alone, differentiable wrt p."""
    pc = p.clamp(R.P_LO, R.P_HI)
    bce = -(t * torch.log(pc) + (1 - t) * torch.log(1 - pc))
    if qo['kind'] == 'qfl':
        return _pow(_f32(qo['beta']), (t - pc).abs()) * bce
    neg = _f32(qo['alpha']) * _pow(_f32(qo['gamma']), pc) * -torch.log(1 - pc)
    return torch.where(t <= 0, neg, t * bce)


def elements_grad(p, t, qo):
    """-> (l, d l / d p) per element, the derivative by hand: the clamp passes it on the closed range [1e-4f, 1 - 1e-4f]."""
    pc = p.clamp(R.P_LO, R.P_HI)
    inside = (p >= R.P_LO) & (p <= R.P_HI)
    bce = -(t * torch.log(pc) + (1 - t) * torch.log(1 - pc))
    dbce = (1 - t) / (1 - pc) - t / pc
    if qo['kind'] == 'qfl':
        beta = _f32(qo['beta'])
        u = (t - pc).abs()
        pw = _pow(beta, u)
        dpw = torch.where(u == 0, torch.zeros_like(u), beta * pw / torch.where(u == 0, torch.ones_like(u), u))
        l, d = pw * bce, torch.where(pc > t, dpw, -dpw) * bce + pw * dbce
    else:
        alpha, gamma = _f32(qo['alpha']), _f32(qo['gamma'])
        pw, ce0 = _pow(gamma, pc), -torch.log(1 - pc)
        l = torch.where(t <= 0, alpha * pw * ce0, t * bce)
        d = torch.where(t <= 0, alpha * (gamma * pw / pc * ce0 + pw / (1 - pc)), t * dbce)
    return l, torch.where(inside, d, torch.zeros_like(d))


def targets(case, codes, q, b):
    """-> t [A, nc] of image b: q on the assigned row's label of a positive anchor, 0 elsewhere."""
    A, nc = case['cls'].shape[1:]
    t = torch.zeros(A, nc, dtype=q.dtype)
    pos = codes[b] >= 0
    t[pos, case['ann'][b, codes[b][pos], 4].long()] = q[b, pos]
    return t


def run(case, opts, qo, box=None, gscale=(1.0, 1.0), dtype=torch.float64, codes=None):
    """opts: a tests/loss_options_restated.options dict (its alpha / gamma / label_smoothing are not read), qo: options(...) here, box:
    None or (kind, weight), codes: the assignment where it is not the bands' (ATSS).  -> dict: losses [2] (float64), codes, num_pos,
    q [B, A], dlogit [B, A, nc], dreg [B, A, 4] (dtype).  losses[1], codes, num_pos and dreg are R.run's: the quality loss does not
    touch them."""
    base = R.run(case, opts, box=box, gscale=gscale, dtype=dtype, codes=codes)
    codes = base['codes']
    B, A, nc = case['cls'].shape
    q = quality(case, codes, dtype)
    cls = case['cls'].to(dtype)
    cl, dlogit = [], torch.zeros(B, A, nc, dtype=dtype)
    for b in range(B):
        p = cls[b]
        if not bool((case['ann'][b, :, 4] != -1).any()):
            cl.append(torch.zeros((), dtype=dtype))
            dlogit[b] = p - p
            continue
        norm = max(int(base['num_pos'][b]), 1)
        l, d = elements_grad(p, targets(case, codes, q, b), qo)
        live = (codes[b] != LC.CODE_IGN)[:, None]
        cl.append(torch.where(live, l, torch.zeros_like(l)).sum() / norm)
        dlogit[b] = torch.where(live, gscale[0] / (B * norm) * d * p * (1 - p), p - p)
    losses = torch.stack([torch.stack(cl).mean().double(), base['losses'][1]])
    return {'losses': losses, 'codes': codes, 'num_pos': base['num_pos'], 'q': q, 'dlogit': dlogit, 'dreg': base['dreg']}
