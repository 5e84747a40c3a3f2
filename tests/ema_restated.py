"""NumPy float32 restatement of the parameter EMA of csrc/optim.hip (include/effdet_ema.h), and the float64 recurrence it is checked
against.  Every operand is an np.float32 scalar or array, so each NumPy operation rounds once, to nearest: no FMA, no wider
intermediate.

    t  = (float)updates
    d  = decay;  if warmup: d = min(d, (1 + t) / (10 + t))
    om = 1 - d
    e  = e + om * (p - e)
    updates += 1                 (once per step)"""
import numpy as np

F = np.float32


def one_minus_decay(decay, warmup, updates):
    """-> om as np.float32: 1 - d, with d the fp32 decay or, during the warm-up, min(decay, (1 + t) / (10 + t))."""
    d = F(decay)
    if warmup:
        t = F(updates)
        d = np.minimum(d, (F(1.0) + t) / (F(10.0) + t))
    return F(F(1.0) - d)


def update(e, p, decay, warmup, updates):
    """One EMA update of the float32 array e from the float32 array p (both unchanged) -> the new e.  NaN and Inf follow IEEE-754."""
    e, p = np.asarray(e), np.asarray(p)
    assert e.dtype == np.float32 and p.dtype == np.float32
    om = one_minus_decay(decay, warmup, updates)
    with np.errstate(invalid='ignore', over='ignore'):
        d = p - e
        q = om * d
        out = e + q
    assert out.dtype == np.float32
    return out


def run(e0, ps, decay, warmup=True, updates=0):
    """e0 and the parameter values after each applied step -> (the final e, the final counter)."""
    e = np.asarray(e0, dtype=np.float32).copy()
    for p in ps:
        e = update(e, p, decay, warmup, updates)
        updates += 1
    return e, updates


def warmup_end(decay):
    """The first t at which (1 + t) / (10 + t) >= decay in fp32, i.e. from which the decay itself is used."""
    t = 0
    while one_minus_decay(decay, True, t) != one_minus_decay(decay, False, t):
        t += 1
    return t


def update_f64(e, p, decay, warmup, updates):
    """The same recurrence in float64 from the float32 decay: the yardstick for the restatement's rounding."""
    d = float(F(decay))
    if warmup:
        d = min(d, (1.0 + updates) / (10.0 + updates))
    e = np.asarray(e, dtype=np.float64)
    return e + (1.0 - d) * (np.asarray(p, dtype=np.float64) - e)
