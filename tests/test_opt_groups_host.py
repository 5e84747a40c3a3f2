"""CPU tier of the parameter groups and the SGD rule of the fused optimizer step (include/effdet_opt_groups.h, optim.ClipAdamW with
several groups, optim.ClipSGD, optim.split_param_groups): the binding's signature table against the companion header, the NumPy
float32 restatement of the SGD rule (tests/opt_groups_restated.py) against torch.optim.SGD on CPU tensors, the host table builder,
what the constructors refuse, and that a one-group ClipAdamW is what it was.  Builds and loads the library; no GPU call."""
import os
import re

import numpy as np
import pytest
import torch

from tests import opt_groups_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _prototypes():
    h = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'effdet_opt_groups.h')).read(), flags=re.S)
    scalar = {'int': 'i', 'long long': 'q', 'float': 'f', 'effdet_stream_t': 'p'}
    protos = {}
    for r, name, params in re.findall(r'^([a-z][a-z ]*?\*?)\s*\b(effdet_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', h, flags=re.M):
        kinds = ['p' if '*' in p else scalar[' '.join(p.split()).rsplit(' ', 1)[0]] for p in params.split(',')]
        assert name not in protos, name
        protos[name] = ({'int': 'i', 'long long': 'q'}[' '.join(r.split())], kinds)
    return h, protos


def test_signatures_match_the_companion_header():
    """_lib.OPT_GROUPS_SIGNATURES against the prototypes of include/effdet_opt_groups.h, parsed as tests/test_ema_host.py parses its
    header; the built library exports the entry point and lib() binds it with the table's types; no other table declares it, the ABI
    generation stays 11 and the header's constants are the binding's."""
    from efficientdet.pytorch_amd import build, _lib
    h, protos = _prototypes()
    assert sorted(protos) == sorted(set(re.findall(r'\b(effdet_[a-z0-9_]+)\s*\(', h))) == ['effdet_opt_step_groups']
    assert sorted(_lib.OPT_GROUPS_SIGNATURES) == sorted(protos)
    others = [getattr(_lib, n) for n in dir(_lib) if n.endswith('SIGNATURES') and n != 'OPT_GROUPS_SIGNATURES']
    assert len(others) >= 12 and not any(set(protos) & set(t) for t in others)
    build.build(verbose=False)
    L = _lib.require(*protos)
    assert int(L.effdet_abi_version()) == 11 == _lib.ABI_VERSION
    for name, (r, kinds) in protos.items():
        sig = _lib.OPT_GROUPS_SIGNATURES[name]
        assert sig[1] == ':' and sig[0] == r, (name, sig, r)
        assert list(sig[2:].replace('s', 'p')) == kinds, (name, sig, ''.join(kinds))
        f = getattr(L, name)
        assert f.restype is _lib._CTYPE[sig[0]] and list(f.argtypes) == [_lib._CTYPE[c] for c in sig[2:]], name
    consts = dict(re.findall(r'#define (EFFDET_OPT_[A-Z_]+) (\d+)', h))
    assert {k: int(v) for k, v in consts.items()} == {
        'EFFDET_OPT_ROW': _lib.OPT_ROW, 'EFFDET_OPT_RULE_ADAMW': _lib.OPT_RULE_ADAMW, 'EFFDET_OPT_RULE_SGD': _lib.OPT_RULE_SGD,
        'EFFDET_OPT_GATED': _lib.OPT_GATED, 'EFFDET_OPT_EMA': _lib.OPT_EMA}


def test_entry_point_refuses_bad_rules_flags_and_tables():
    from efficientdet.pytorch_amd import build, _lib
    build.build(verbose=False)
    L = _lib.require('effdet_opt_step_groups')
    P, N = 0x1000, None          # "some non-null pointer": never dereferenced, every call below is refused before a launch
    # rule, flags, params, grads, acc, moment1, moment2, ema, numel, block_tensor, block_first, tensor_group, ntensors, nblocks, ngroups,
    # scratch, steps, hyper_table, max_norm, write_grad, ema_warmup, ctl, ema_ctl, stream
    plain = [0, 0, P, P, N, P, P, N, P, P, P, P, 1, 1, 1, P, P, P, 0.1, 0, 1, N, N, N]
    for i in (2, 3, 5, 6, 8, 9, 10, 11, 15, 16, 17):
        a = list(plain); a[i] = N
        assert L.effdet_opt_step_groups(*a) == -1, i
    for i in (12, 13, 14):
        a = list(plain); a[i] = 0
        assert L.effdet_opt_step_groups(*a) == -1, i
    for rule, flags in ((2, 0), (-1, 0), (0, 4), (0, -1)):
        a = list(plain); a[0], a[1] = rule, flags
        assert L.effdet_opt_step_groups(*a) == -1, (rule, flags)
    a = list(plain); a[0] = _lib.OPT_RULE_SGD                   # SGD has ONE moment arena: a second one is refused ...
    assert L.effdet_opt_step_groups(*a) == -1
    a = list(plain); a[4] = P                                    # ... and so are an accumulation arena without the gate,
    assert L.effdet_opt_step_groups(*a) == -1
    a = list(plain); a[7] = P                                    # an average without its flag,
    assert L.effdet_opt_step_groups(*a) == -1
    a = list(plain); a[1] = _lib.OPT_GATED                       # the gate without arena and control block,
    assert L.effdet_opt_step_groups(*a) == -1
    a = list(plain); a[1] = _lib.OPT_EMA; a[7] = P               # the average without its control block,
    assert L.effdet_opt_step_groups(*a) == -1
    a = list(plain); a[1] = _lib.OPT_GATED; a[4] = P; a[21] = P; a[19] = 1      # and write_grad with the gate
    assert L.effdet_opt_step_groups(*a) == -1


# ------------------------------------------------------------------------------------------------ the SGD rule
CONFIGS = [dict(momentum=0.0), dict(momentum=0.9), dict(momentum=0.9, dampening=0.1), dict(momentum=0.9, nesterov=True),
           dict(momentum=0.9, weight_decay=4e-5), dict(momentum=0.0, weight_decay=1e-2),
           dict(momentum=0.9, dampening=0.1, weight_decay=4e-5), dict(momentum=0.5, nesterov=True, weight_decay=1e-2)]


@pytest.mark.parametrize('cfg', CONFIGS, ids=lambda c: ','.join('%s=%g' % kv for kv in c.items()))
def test_restatement_is_torch_sgd_on_cpu(cfg):
    """4 steps of torch.optim.SGD(foreach=False) on CPU fp32 tensors (sizes 1, 5, 1023, 4097; the third has no gradient in step 2, so
    its buffer stays and its own step count lags) against the restatement.  Bit equality was the expectation and is NOT what torch's
    CPU kernels give: their add-with-alpha (g + wd * p, momentum * buf + (1 - dampening) * d, p - lr * u) is a fused multiply-add, one
    rounding where the rule has two.  So the bound is the fallback one: after n steps at most 2 n ulp of the parameter, the ulp taken
    of the largest magnitude the element's operands have had so far (|p| before and after, |lr * u|) -- a contracted step differs
    from the separately rounded one by at most half an ulp of the product plus the two final roundings, and p's own recurrence has
    gain 1.  Seen (torch 2.x, x86-64), worst over elements and steps: momentum 0: 3.0; 0.9: 2.0; 0.9 with dampening 0.1: 6.0 (of 8);
    nesterov: 3.0; 0.9 with wd 4e-5: 3.0; momentum 0 with wd 1e-2: 2.0; 0.9, dampening 0.1, wd 4e-5: 3.1; nesterov 0.5 with wd 1e-2:
    2.0.  The buffers are held to 1e-5 of their largest magnitude (a sanity check: the parameters are the pin)."""
    g = torch.Generator().manual_seed(7)
    sizes = (1, 5, 1023, 4097)
    ps = [torch.nn.Parameter(torch.randn(n, generator=g)) for n in sizes]
    opt = torch.optim.SGD(ps, lr=0.05, foreach=False, **cfg)
    mine = [p.detach().numpy().copy() for p in ps]
    bufs = [np.zeros(n, F) for n in sizes]
    big = [np.abs(x) for x in mine]
    counts = [0] * len(sizes)
    worst = 0.0
    for step in range(1, 5):
        for i, p in enumerate(ps):
            p.grad = None if (i == 2 and step == 2) else torch.randn(p.shape, generator=g)
        opt.step()
        for i, p in enumerate(ps):
            if p.grad is None:
                continue
            counts[i] += 1
            new, bufs[i] = R.sgd(mine[i], bufs[i], p.grad.numpy(), counts[i], lr=0.05, **cfg)
            big[i] = np.maximum(big[i], np.maximum(np.abs(new), np.abs(new - mine[i])))
            mine[i] = new
        for i, p in enumerate(ps):
            ref = p.detach().numpy()
            ulp = float((np.abs(mine[i].astype(np.float64) - ref) / np.spacing(big[i]).astype(np.float64)).max())
            worst = max(worst, ulp)
            assert ulp <= 2.0 * step, (cfg, step, i, ulp)
            if cfg['momentum'] and counts[i]:
                b = opt.state[p]['momentum_buffer'].numpy()
                assert float(np.abs(bufs[i] - b).max()) <= 1e-5 * float(np.abs(b).max()), (cfg, step, i)
    print('worst difference from torch.optim.SGD on CPU: %.2f ulp of the largest operand so far' % worst)
    assert counts == [4, 4, 3, 4]


def test_restatement_by_hand():
    """p = 1, g = 0.5, lr = 0.1, wd = 0.5: d = 0.5 + 0.5 = 1; first step buf = d = 1, p = 1 - 0.1 = 0.9f.  Second step with g = 0 at
    momentum 0.5, dampening 0.5: d = 0.45f, buf = 0.5 * 1 + 0.5 * 0.45f, nesterov off: p = 0.9f - 0.1f * buf."""
    p, b = R.sgd(np.ones(1, F), np.zeros(1, F), np.full(1, 0.5, F), 1, lr=0.1, momentum=0.5, dampening=0.5, weight_decay=0.5)
    assert b[0] == F(1.0) and p[0] == F(1.0) - F(0.1)
    p2, b2 = R.sgd(p, b, np.zeros(1, F), 2, lr=0.1, momentum=0.5, dampening=0.5, weight_decay=0.5)
    d = F(0.5) * p[0]
    assert b2[0] == F(0.5) * F(1.0) + F(0.5) * d and p2[0] == p[0] - F(0.1) * b2[0]
    # momentum 0 never touches the buffer; coef scales the gradient before the decay term
    p3, b3 = R.sgd(np.ones(2, F), np.full(2, 7.0, F), np.ones(2, F), 5, lr=0.5, coef=0.5)
    assert np.all(b3 == F(7.0)) and np.all(p3 == F(0.75))
    assert R.clip_coef(0.0, 3.0) == F(1.0) and R.clip_coef(0.1, 0.01) == F(1.0)
    assert R.clip_coef(0.1, 2.0) == F(0.1) / (F(2.0) + F(1e-6))


# ------------------------------------------------------------------------------------------------ host tables and refusals
def test_layout_tables_across_group_boundaries():
    from efficientdet.pytorch_amd.optim import layout_tables
    lay = layout_tables([[4096, 5], [1], [], [8193, 3]], 4096)
    assert lay['numel'] == [4096, 5, 1, 8193, 3]
    assert lay['tensor_group'] == [0, 0, 1, 3, 3]                 # the empty group owns no tensor; its row of the table stays unused
    assert lay['offs'].tolist() == [0, 4096, 4160, 4224, 4224 + 8256, 4224 + 8256 + 64]      # each tensor padded to 64 elements
    assert lay['block_tensor'] == [0, 1, 2, 3, 3, 3, 4] and lay['block_first'] == [0, 1, 2, 3, 6] and lay['nblocks'] == 7
    one = layout_tables([[4097]], 4096)
    assert one['block_tensor'] == [0, 0] and one['tensor_group'] == [0] and one['offs'].tolist() == [0, 4160]
    with pytest.raises(ValueError):
        layout_tables([[3, 0]], 4096)


def _ps(n=4):
    return [torch.nn.Parameter(torch.zeros(3)) for _ in range(n)]


def test_groups_that_disagree_on_the_shared_values_are_refused():
    from efficientdet.pytorch_amd.optim import ClipAdamW, ClipSGD
    p = _ps()
    for cls in (ClipAdamW, ClipSGD):
        with pytest.raises(ValueError, match=r'max_norm is optimizer-wide.*group 1'):
            cls([{'params': p[:2]}, {'params': p[2:], 'max_norm': 0.5}], lr=0.1, max_norm=0.1)
        with pytest.raises(ValueError, match=r'ema_decay is optimizer-wide.*groups 1, 2'):
            cls([{'params': p[:1]}, {'params': p[1:2], 'ema_decay': 0.5}, {'params': p[2:], 'ema_decay': 0.25}], lr=0.1, ema_decay=0.9)
        # ... also when the disagreement appears later, where the values are read
        o = cls([{'params': p[:2]}, {'params': p[2:]}], lr=0.1, max_norm=0.1)
        o.param_groups[1]['max_norm'] = 0.2
        with pytest.raises(ValueError, match='max_norm is optimizer-wide'):
            o._hyper_values()
        o.param_groups[1]['max_norm'] = 0.1
        o.param_groups[1]['lr'] = 0.0                             # lr is per group
        assert [r[1] for r in o._hyper_values()] == [0.1, 0.0]


def test_a_parameter_may_not_appear_twice():
    import warnings
    from efficientdet.pytorch_amd.optim import ClipAdamW, ClipSGD
    p = _ps()
    for cls in (ClipAdamW, ClipSGD):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            with pytest.raises(ValueError, match='twice'):
                cls([p[0], p[1], p[0]], lr=0.1)
        with pytest.raises(ValueError):                          # (across groups torch itself refuses)
            cls([{'params': p[:2]}, {'params': p[1:]}], lr=0.1)


def test_nesterov_misuse_is_refused_as_torch_refuses_it():
    from efficientdet.pytorch_amd.optim import ClipSGD
    p = _ps()
    for kw in (dict(momentum=0.0, nesterov=True), dict(momentum=0.9, dampening=0.1, nesterov=True)):
        with pytest.raises(ValueError, match='Nesterov'):
            torch.optim.SGD(p, lr=0.1, **kw)
        with pytest.raises(ValueError, match='Nesterov'):
            ClipSGD(p, lr=0.1, **kw)
    with pytest.raises(ValueError, match='Nesterov'):            # a group's own override
        ClipSGD([{'params': p[:2]}, {'params': p[2:], 'momentum': 0.0}], lr=0.1, momentum=0.9, nesterov=True)
    o = ClipSGD([{'params': p[:2]}, {'params': p[2:], 'nesterov': False, 'dampening': 0.1}], lr=0.1, momentum=0.9, nesterov=True,
                weight_decay=4e-5, max_norm=0.1, ema_decay=0.5)
    rows = o._hyper_values()
    assert rows[0] == (0.1, 0.1, 0.9, 1.0, 1.0, 4e-5, 0.5, 0.0)
    assert rows[1] == (0.1, 0.1, 0.9, float(F(1.0 - 0.1)), 0.0, 4e-5, 0.5, 0.0)
    assert sorted(o.param_groups[0]) == ['dampening', 'ema_decay', 'lr', 'max_norm', 'momentum', 'nesterov', 'params', 'weight_decay']
    assert o.MOMENTS == (('momentum_buf', 'momentum_buffer'),) and len(o.MOMENTS) == 1
    assert not hasattr(o, 'write_clipped_grads') or o.write_clipped_grads is False


def test_one_group_clip_adamw_is_what_it_was():
    from efficientdet.pytorch_amd.optim import ClipAdamW
    p = _ps()
    o = ClipAdamW(p, lr=1e-3, max_norm=0.1)
    assert sorted(o.param_groups[0]) == ['betas', 'eps', 'lr', 'max_norm', 'params', 'weight_decay']
    assert o._hyper_values() == (0.1, 1e-3, 0.9, 0.999, 1e-8, 1e-2) and not o._grouped()
    o = ClipAdamW([{'params': p}], lr=1e-3, max_norm=0.1, ema_decay=0.5)
    assert sorted(o.param_groups[0]) == ['betas', 'ema_decay', 'eps', 'lr', 'max_norm', 'params', 'weight_decay']
    assert o._hyper_values() == (0.1, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 0.5) and not o._grouped()
    # two groups: the table, one row of eight per group, per-group lr / betas / eps / weight_decay
    o = ClipAdamW([{'params': p[:2], 'weight_decay': 0.0}, {'params': p[2:], 'lr': 1e-5, 'betas': (0.8, 0.99), 'eps': 1e-6}], lr=1e-3,
                  max_norm=0.1)
    assert o._grouped() and o._hyper_values() == ((0.1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.0, 0.0), (0.1, 1e-5, 0.8, 0.99, 1e-6, 1e-2, 0.0, 0.0))
    o.add_param_group({'params': _ps(1)})                        # legal until the device tables exist
    assert len(o._hyper_values()) == 3


# ------------------------------------------------------------------------------------------------ split_param_groups
def test_split_param_groups_partitions_the_trainable_parameters_of_d0():
    from efficientdet.pytorch_amd import EfficientDet, EFFICIENTDET
    from efficientdet.pytorch_amd.optim import split_param_groups
    c = EFFICIENTDET['efficientdet-d0']
    torch.manual_seed(0)
    m = EfficientDet(8, network='efficientdet-d0', W_bifpn=c['W_bifpn'], D_bifpn=c['D_bifpn'], D_class=c['D_class'])
    frozen = next(p for n, p in m.named_parameters() if n.startswith('bbox_head'))
    frozen.requires_grad_(False)
    names = {id(p): n for n, p in m.named_parameters()}
    trainable = [p for p in m.parameters() if p.requires_grad]
    fusion = [p for n, p in m.named_parameters() if re.search(r'stack_bifpn_convs\.\d+\.w[12]$', n)]
    assert len(fusion) == 2 * c['D_bifpn'] and all(p.ndim == 2 for p in fusion)

    groups = split_param_groups(m, 4e-5, backbone_lr_scale=0.1)
    assert [g['name'] for g in groups] == ['decay', 'no_decay', 'backbone_decay', 'backbone_no_decay']
    got = [p for g in groups for p in g['params']]
    assert len(got) == len(set(map(id, got))) == len(trainable) and set(map(id, got)) == set(map(id, trainable))
    assert id(frozen) not in set(map(id, got)) and all(g['params'] for g in groups)
    for g in groups:
        back = [names[id(p)].startswith('backbone.') for p in g['params']]
        assert all(back) or not any(back)
        assert g['lr_scale'] == (0.1 if back[0] else 1.0)
        if g['weight_decay'] == 0.0:
            assert all(p.ndim <= 1 or any(p is f for f in fusion) for p in g['params'])
        else:
            assert g['weight_decay'] == 4e-5 and all(p.ndim > 1 and not any(p is f for f in fusion) for p in g['params'])
    no_decay = {id(p) for g in groups if g['weight_decay'] == 0.0 for p in g['params']}
    assert all(id(f) in no_decay for f in fusion) and all(id(p) in no_decay for p in trainable if p.ndim <= 1)

    two = split_param_groups(m, 4e-5)                            # scale 1: the backbone needs no groups of its own
    assert [g['name'] for g in two] == ['decay', 'no_decay'] and all(g['lr_scale'] == 1.0 for g in two)
    assert sum(len(g['params']) for g in two) == len(trainable)
    every = split_param_groups(m, 4e-5, decay_norm_and_bias=True)
    nd = [g for g in every if g['weight_decay'] == 0.0]
    assert len(nd) == 1 and sorted(map(id, nd[0]['params'])) == sorted(map(id, fusion))
    # the groups go straight into the optimizers; lr_scale is the caller's to multiply in
    from efficientdet.pytorch_amd.optim import ClipAdamW, ClipSGD
    fresh = lambda: split_param_groups(m, 4e-5, backbone_lr_scale=0.1)      # (an optimizer keeps, and fills in, the dicts it is given)
    for opt in (ClipAdamW(fresh(), lr=1e-3, max_norm=0.1), ClipSGD(fresh(), lr=0.08, momentum=0.9, weight_decay=4e-5)):
        for g in opt.param_groups:
            g['lr'] *= g['lr_scale']
        lrs = [r[1] for r in opt._hyper_values()]
        assert lrs[2] == pytest.approx(0.1 * lrs[0]) and lrs[3] == lrs[2] and lrs[1] == lrs[0]
        assert [r[5] for r in opt._hyper_values()] == [4e-5, 0.0, 4e-5, 0.0]


def test_documents_name_the_groups_and_the_second_rule():
    for name in ('README.md', 'DESIGN.md', 'INTEGRATION.md'):
        md = open(os.path.join(ROOT, name)).read()
        assert 'ClipSGD' in md and 'split_param_groups' in md, name
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert 'effdet_opt_step_groups' in design and 'tensor_group' in design
