"""NumPy float32 restatement of the SGD rule of csrc/optim.hip (include/effdet_opt_groups.h; torch.optim.SGD's update).  Every operand
is an np.float32 scalar or array, so each NumPy operation rounds once, to nearest: no FMA, no wider intermediate.

    g' = coef * g
    d  = g' + wd * p            (wd != 0; g' otherwise)
    momentum != 0:  buf = d if t == 1 else momentum * buf + (1 - dampening) * d;   u = d + momentum * buf if nesterov else buf
    momentum == 0:  u = d
    p  = p - lr * u

t is the tensor's own step count after this step; 1 - dampening is the double difference rounded to fp32 (torch's alpha)."""
import numpy as np

F = np.float32


def clip_coef(max_norm, norm):
    """min(1, max_norm / (norm + 1e-6)) in fp32 from the fp32 norm the device measured; 1 without clipping."""
    if not max_norm > 0.0:
        return F(1.0)
    return np.minimum(F(1.0), F(max_norm) / (F(norm) + F(1e-6)))


def sgd(p, buf, g, t, lr, momentum=0.0, dampening=0.0, nesterov=False, weight_decay=0.0, coef=1.0):
    """One step of one tensor: float32 arrays p, buf, g (unchanged) and the step count t after this step -> (new p, new buf)."""
    p, buf, g = np.asarray(p), np.asarray(buf), np.asarray(g)
    assert p.dtype == np.float32 and buf.dtype == np.float32 and g.dtype == np.float32
    lr, mom, od, wd, coef = F(lr), F(momentum), F(1.0 - dampening), F(weight_decay), F(coef)
    with np.errstate(invalid='ignore', over='ignore'):
        gp = coef * g
        d = gp
        if wd != 0:
            w = wd * p
            d = gp + w
        u = d
        if mom != 0:
            if t == 1:
                buf = d.copy()
            else:
                a = mom * buf
                b = od * d
                buf = a + b
            if nesterov:
                a = mom * buf
                u = d + a
            else:
                u = buf
        s = lr * u
        out = p - s
    assert out.dtype == np.float32 and buf.dtype == np.float32
    return out, buf
