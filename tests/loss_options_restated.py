"""The detection loss with the options of include/effdet_loss_opts.h restated in torch: matcher -> focal class term with label
smoothing -> smooth-L1 with the knee beta (or an IoU-family box term, tests/box_loss_restated.py) -> .backward(), in any precision.
float64 is the reference of tests/test_gpu_loss_options.py, float32 (the same code) the yardstick that sizes its gradient tolerance.

The header fixes every quantity as fp32, so the constants of the loss are the fp32 ones (alpha, gamma, eps, beta, reg_weight as the
fp32 the device receives, the clamp 1e-4f / 1 - 1e-4f, the target scales 0.1f / 0.2f) taken as they are into either precision, and
the power is spelled exp2(gamma * log2(u)) as the header spells it, so the float32 run carries the same amplification of the
logarithm's rounding as the device's form.

The matcher compares the IoU (tests/loss_cases.oracle_iou: the oracle's calc_iou, which is loss_assign_kernel's expression) with the
bands in the run's precision, each band rounded from the option's decimal IN that precision -- as tests/loss_cases.oracle_states
does with 0.4 / 0.5, which it reproduces at the defaults: a ratio that equals the decimal in exact arithmetic (768 / 1920 and 0.4)
lands on the band in both precisions.  tests/test_loss_options_host.py proves that both precisions assign the same codes on every
case the device tests use."""
import numpy as np
import torch

from tests import box_loss_restated as BR
from tests import loss_cases as LC


def _f32(v):
    return float(np.float32(v))


DEFAULTS = dict(alpha=0.25, gamma=2.0, label_smoothing=0.0, beta=_f32(1.0 / 9.0), reg_weight=1.0, pos_iou=0.5, neg_iou=0.4,
                low_quality=False)
P_LO = _f32(1e-4)
P_HI = _f32(np.float32(1.0) - np.float32(1e-4))


def options(**kw):
    """-> the full option dict (DEFAULTS overridden by kw)."""
    assert set(kw) <= set(DEFAULTS), kw
    o = dict(DEFAULTS)
    o.update(kw)
    return o


def assign(case, opts, dtype=torch.float64):
    """-> (codes int64 [B, A]: LC.CODE_IGN / LC.CODE_NEG / the assigned annotation row, promoted bool [B, A]: positive by the
    low-quality rule (whether or not also by the band))."""
    B, A = case['cls'].shape[:2]
    code = torch.full((B, A), LC.CODE_IGN, dtype=torch.int64)
    promoted = torch.zeros(B, A, dtype=torch.bool)
    for b in range(B):
        iou, rows = LC.oracle_iou(case, b, dtype)
        if len(rows) == 0:
            continue
        best, arg = iou.max(dim=1)                                      # (the first maximum)
        code[b, best < torch.tensor(opts['neg_iou'], dtype=dtype)] = LC.CODE_NEG
        pos = best >= torch.tensor(opts['pos_iou'], dtype=dtype)
        if opts['low_quality']:
            gtmax = iou.max(dim=0)[0]
            promoted[b] = ((iou == gtmax[None]) & (gtmax[None] > 0)).any(dim=1)
            pos = pos | promoted[b]
        code[b, pos] = rows[arg[pos]]
    return code, promoted


def focal_elements(p, h, ignored, opts):
    """Per-element class loss [A, nc] for probabilities p, hard targets h (0 / 1) and the ignored-anchor mask [A]."""
    alpha, gamma, eps = _f32(opts['alpha']), _f32(opts['gamma']), _f32(opts['label_smoothing'])
    pc = p.clamp(P_LO, P_HI)
    one = h == 1
    t = h * (1 - eps) + eps / 2
    u = torch.where(one, 1 - pc, pc)
    w = torch.where(one, torch.full_like(pc, alpha), torch.full_like(pc, 1 - alpha)) * torch.exp2(gamma * torch.log2(u))
    l = -w * (t * torch.log(pc) + (1 - t) * torch.log(1 - pc))
    return torch.where(ignored[:, None], torch.zeros_like(l), l)


def smooth_l1_elements(anc, gt, r, beta):
    """[P, 4] smooth-L1 of the encoded deltas of positives (anchors anc, assigned boxes gt, regression rows r) with the knee beta."""
    aw, ah = anc[:, 2] - anc[:, 0], anc[:, 3] - anc[:, 1]
    acx, acy = anc[:, 0] + 0.5 * aw, anc[:, 1] + 0.5 * ah
    gw, gh = gt[:, 2] - gt[:, 0], gt[:, 3] - gt[:, 1]
    gcx, gcy = gt[:, 0] + 0.5 * gw, gt[:, 1] + 0.5 * gh
    gw, gh = gw.clamp(min=1), gh.clamp(min=1)
    t = torch.stack(((gcx - acx) / aw / BR.STD_XY, (gcy - acy) / ah / BR.STD_XY, torch.log(gw / aw) / BR.STD_WH,
                     torch.log(gh / ah) / BR.STD_WH), 1)
    d = (t - r).abs()
    return torch.where(d <= beta, 0.5 * d * d / beta, d - 0.5 * beta)


def run(case, opts, box=None, gscale=(1.0, 1.0), dtype=torch.float64, codes=None, inputs=None, fp32_knee=True):
    """box: None (smooth-L1) or (kind, weight) of tests/box_loss_restated.py.  -> dict: losses [2] (float64 tensor), codes [B, A],
    num_pos [B], dlogit [B, A, nc] and dreg [B, A, 4] (dtype) = d(gscale[0] losses[0] + gscale[1] losses[1]) / d(logit | reg).
    inputs: (cls, reg) in the place of the case's (the central differences of tests/test_loss_options_host.py).  fp32_knee=False
    takes beta as the float64 it is given (1 / 9 there is the oracle's knee; the device's is that rounded to fp32, 7.5e-9 larger)."""
    B, A, nc = case['cls'].shape
    codes = assign(case, opts, torch.float64)[0] if codes is None else codes
    cls, reg = (case['cls'], case['reg']) if inputs is None else inputs
    cls = cls.to(dtype).clone().requires_grad_(True)
    reg = reg.to(dtype).clone().requires_grad_(True)
    anc, ann = case['anc'][0].to(dtype), case['ann'].to(dtype)
    beta, reg_weight = _f32(opts['beta']) if fp32_knee else float(opts['beta']), _f32(opts['reg_weight'])
    zero = torch.zeros((), dtype=dtype)
    cl, rl, num_pos = [], [], []
    for b in range(B):
        code = codes[b]
        pos = code >= 0
        npos = int(pos.sum())
        num_pos.append(npos)
        if not bool((case['ann'][b, :, 4] != -1).any()):
            cl.append(zero); rl.append(zero)
            continue
        h = torch.zeros(A, nc, dtype=dtype)
        rows = code[pos]
        h[pos, ann[b, rows, 4].long()] = 1
        cl.append(focal_elements(cls[b], h, code == LC.CODE_IGN, opts).sum() / max(npos, 1))
        if npos == 0:
            rl.append(zero)
        elif box is None:
            rl.append(reg_weight * smooth_l1_elements(anc[pos], ann[b, rows, :4], reg[b, pos], beta).sum() / (4 * npos))
        else:
            rl.append(_f32(box[1]) * BR.anchor_loss(box[0], anc[pos], ann[b, rows, :4], reg[b, pos]).sum() / npos)
    losses = torch.stack([torch.stack(cl).mean(), torch.stack(rl).mean()])
    (gscale[0] * losses[0] + gscale[1] * losses[1]).backward()
    p = cls.detach()
    dlogit = (cls.grad if cls.grad is not None else torch.zeros_like(p)) * p * (1 - p)
    dreg = reg.grad if reg.grad is not None else torch.zeros_like(reg.detach())
    return {'losses': losses.detach().double(), 'codes': codes, 'num_pos': torch.tensor(num_pos), 'dlogit': dlogit, 'dreg': dreg}
