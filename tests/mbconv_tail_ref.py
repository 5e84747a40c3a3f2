"""Float64 reference of the MBConv tail (models/efficientnet.py:89-104) and its backward: plain torch, autograd, no project code.

    xd = swish(zd);  pool = sum_p xd;  gate = sigmoid(W2 swish(W1 pool / hw + b1) + b2);  xs = xd * gate
    y  = rs_b * BN2(conv1x1(xs, W))                  (frozen BN: gamma, beta, running mean / var, eps 1e-3)

mbconv_tail_ref returns, from y.backward(dy), every gradient the fused squeeze-excite backward of functional.mbconv_bwd produces and
the intermediates its kernels hand to each other.  tests/test_se_fused_ref_host.py checks the identities the kernels rest on against
it on the CPU; tests/test_gpu_se_fused_bwd.py compares the kernels with it.
"""
import torch

BN_EPS = 1e-3


def swish(z):
    return z * torch.sigmoid(z)


def swish_grad(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


def _through(t, q):
    """Straight-through rounding: the value of q(t), the gradient of t."""
    if q is None:
        return t
    d = t.detach()
    return t + (q(d) - d)


def mbconv_tail_ref(zd, w1, b1, w2, b2, W, gamma, beta, mean, var, rs, dy, q=None, qw=None, eps=BN_EPS):
    """zd [B,Ce,H,W] depthwise pre-activation; w1 [Cse,Ce], b1 [Cse], w2 [Ce,Cse], b2 [Ce] the SE weights; W [Co,Ce] the project weight;
    gamma / beta / mean / var [Co] the frozen BN2; rs [B] or None the drop_connect row scale; dy [B,Co,H,W] the upstream gradient.
    q (optional): rounding of the stored activations (bf16 runs): zd, dy, and -- straight through -- xd and xs are seen rounded.
    qw (optional): rounding of the conv's stored weight operand W' = W * bn_scale (a bf16 run packs it folded and rounded; it gets the
    float32 product, as the pack forms it) -- straight through as well, so dW and dgamma2 keep their form.
    -> dict of float64 tensors (no graph attached)."""
    d = torch.float64
    leaf = lambda t: t.detach().to(d).clone().requires_grad_(True)
    rnd = (lambda t: q(t).to(d)) if q is not None else (lambda t: t)
    zd = leaf(rnd(zd.detach().to(d))); dy = rnd(dy.detach().to(d))
    w1, b1, w2, b2, W, gamma, beta = (leaf(t) for t in (w1, b1, w2, b2, W, gamma, beta))
    mean, var = mean.detach().to(d), var.detach().to(d)
    B, Ce, H, Wd = zd.shape
    Co, hw = W.shape[0], H * Wd
    rsd = rs.detach().to(d) if rs is not None else torch.ones(B, dtype=d)
    xd = _through(swish(zd), q)
    pool = xd.sum(dim=(2, 3)); pool.retain_grad()                       # the pooled SUM, as the kernels keep it
    mid = (pool / hw) @ w1.t() + b1
    gate = torch.sigmoid(swish(mid) @ w2.t() + b2); gate.retain_grad()
    xs = _through(xd * gate.view(B, Ce, 1, 1), q)
    invstd = 1.0 / torch.sqrt(var + eps)
    bn_scale = invstd * gamma
    Wf = W * bn_scale.view(Co, 1)                                       # BN2 folded into the weight, as the packed operand holds it
    if qw is not None:
        Wf = Wf + (qw(Wf.detach().float()).to(d) - Wf.detach())
    conv = torch.einsum('nc,bchw->bnhw', Wf, xs)
    y = (conv + (beta - mean * bn_scale).view(1, Co, 1, 1)) * rsd.view(B, 1, 1, 1)
    y.backward(dy)
    o = {'dW': W.grad, 'dgamma2': gamma.grad, 'dbeta2': beta.grad, 'dw1': w1.grad, 'db1': b1.grad, 'dw2': w2.grad, 'db2': b2.grad,
         'dzd': zd.grad, 'dgate': gate.grad, 'dgate_gate': gate.grad * gate.detach(), 'dpool': pool.grad,
         # per-image partial weight gradients of the project conv, on its input (M) and on the un-gated activation (M')
         'M': torch.einsum('bnhw,bchw->bnc', dy, xs.detach()), 'Mp': torch.einsum('bnhw,bchw->bnc', dy, xd.detach()),
         'dsum': dy.sum(dim=(2, 3)),                                    # [B,Co] per-image sums of dy (the bias rows)
         'zd': zd, 'dy': dy, 'xd': xd, 'xs': xs, 'pool': pool, 'mid': mid, 'gate': gate, 'rs': rsd,
         'bn_scale': gamma * invstd, 'invstd': invstd, 'mean': mean}
    return {k: v.detach() for k, v in o.items()}


def make_tail_inputs(B, H, W, Co, Ce, Cse, seed, rs=None):
    """Seeded float32 inputs of mbconv_tail_ref at the magnitudes of a trained block (fan-in scaled weights)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(zd=r(B, Ce, H, W), w1=r(Cse, Ce) / Ce ** 0.5, b1=r(Cse) * 0.1, w2=r(Ce, Cse) / Cse ** 0.5, b2=r(Ce) * 0.1,
                W=r(Co, Ce) / Ce ** 0.5, gamma=0.5 + torch.rand(Co, generator=g), beta=r(Co) * 0.1, mean=r(Co) * 0.3,
                var=0.5 + torch.rand(Co, generator=g), rs=rs, dy=r(B, Co, H, W))


# ---- float64 forms of the single ops (direct sums, no autograd) ----
def unpack_ref(g, Cin, taps, scale=None, w=None, dsum_part=None, mean=None, invstd=None, slab_scale=None, slab_cscale=None):
    """Slab sum + unpack of effdet_unpack_conv_wgrad*: g [nslabs,Co,taps,Cin_pad] ->
    dw[co,ci,tap] = scale[co] * sum_sl f(sl) c(sl,ci) g[sl,co,tap,ci],  dbeta = sum_sl f(sl) dsum_part[sl],
    wsum[co] = sum w * (the sum unscaled by scale),  dgamma = invstd * (wsum - mean * dbeta);
    f(sl) = slab_scale[sl // (nslabs / B)], c(sl, ci) = slab_cscale[sl // (nslabs / B), ci].  -> dict (dw as [Co,Cin,taps])."""
    d = torch.float64
    g = g.detach().cpu().to(d)
    ns, Co = g.shape[0], g.shape[1]
    f = torch.ones(ns, dtype=d)
    if slab_scale is not None:
        f = slab_scale.detach().cpu().to(d).repeat_interleave(ns // slab_scale.numel())
    gs = g[..., :Cin] * f.view(ns, 1, 1, 1)
    if slab_cscale is not None:
        c = slab_cscale.detach().cpu().to(d)[:, :Cin].repeat_interleave(ns // slab_cscale.shape[0], dim=0)
        gs = gs * c.view(ns, 1, 1, Cin)
    G = gs.sum(0).permute(0, 2, 1)                                      # [Co,Cin,taps], unscaled
    out = {'dw': G * (scale.detach().cpu().to(d).view(Co, 1, 1) if scale is not None else 1.0)}
    if dsum_part is not None:
        out['dbeta'] = (dsum_part.detach().cpu().to(d) * f.view(ns, 1)).sum(0)
    if w is not None:
        out['wsum'] = (w.detach().cpu().to(d).reshape(Co, Cin, taps) * G).sum(dim=(1, 2))
        if mean is not None:
            out['dgamma'] = invstd.detach().cpu().to(d) * (out['wsum'] - mean.detach().cpu().to(d) * out['dbeta'])
    return out


def se_gate_bwd_ref(rows, gate, mid, pool, w1, w2, inv_hw, times_gate):
    """Backward of the gate MLP from partial rows [B,slabs,C] of d(loss)/d(gate) (times_gate: of that times the gate)."""
    d = torch.float64
    rows, gate, mid, pool, w1, w2 = (t.detach().cpu().to(d) for t in (rows, gate, mid, pool, w1, w2))
    dg = rows.sum(1)
    du = dg * ((1 - gate) if times_gate else gate * (1 - gate))
    dmid = swish_grad(mid) * (du @ w2)
    return {'dpool': inv_hw * (dmid @ w1), 'dw1': inv_hw * (dmid.t() @ pool), 'db1': dmid.sum(0), 'dw2': du.t() @ swish(mid),
            'db2': du.sum(0)}
