"""CPU tier of the parameter EMA (include/effdet_ema.h, optim.ClipAdamW(ema_decay=...)): the NumPy float32 restatement
(tests/ema_restated.py) on hand-derived cases and against the float64 recurrence, the binding's third signature table against the
companion header, and what the constructor refuses.  Builds and loads the library; no GPU call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import ema_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NEW = ('effdet_clip_adamw_step_ema', 'effdet_clip_adamw_step_gated_ema', 'effdet_ema_swap')


def test_first_update_with_warmup_by_hand():
    """t = 0: d = min(decay, 1 / 10) = 0.1f, om = 1 - 0.1f, and e: 0 -> 0 + om * (1 - 0) = om, which is 0.9 to fp32's last bit."""
    for decay in (0.5, 0.9, 0.9998):
        om = R.one_minus_decay(decay, True, 0)
        assert om == F(1.0) - F(1.0) / F(10.0)
        e = R.update(np.zeros(3, F), np.ones(3, F), decay, True, 0)
        assert e.dtype == np.float32 and np.all(e == om) and abs(float(om) - 0.9) <= float(np.spacing(F(0.9)))
    # without the warm-up the decay itself is used from the first update on: 0 -> 1 - 0.5
    assert np.all(R.update(np.zeros(3, F), np.ones(3, F), 0.5, False, 0) == F(0.5))
    # decay 0: the average is the parameter
    p = np.array([1.5, -2.25, 3e-7], F)
    assert np.array_equal(R.update(np.zeros(3, F), p, 0.0, False, 5), p)


def test_e_equal_p_is_a_fixed_point():
    g = np.random.default_rng(0)
    p = g.standard_normal(1000).astype(F)
    for decay, warm, t in ((0.5, True, 0), (0.9998, True, 3), (0.9998, False, 10 ** 6), (0.0, False, 0)):
        assert np.array_equal(R.update(p.copy(), p, decay, warm, t), p)


def test_the_warmup_ends_where_the_fraction_reaches_the_decay():
    """(1 + t) / (10 + t) >= 0.5 from t = 8 (9 / 18, exact), >= 0.9 from t = 80 (81 / 90, which rounds to fp32's 0.9)."""
    assert R.warmup_end(0.5) == 8 and R.warmup_end(0.9) == 80
    assert R.one_minus_decay(0.5, True, 7) == F(1.0) - F(8.0) / F(17.0) > F(0.5)
    assert R.one_minus_decay(0.5, True, 8) == F(0.5) == R.one_minus_decay(0.5, True, 10 ** 6)
    assert R.one_minus_decay(0.9, True, 79) > R.one_minus_decay(0.9, False, 0) == R.one_minus_decay(0.9, True, 80)
    e, u = R.run(np.zeros(2, F), [np.ones(2, F)] * 3, 0.5)
    assert u == 3 and e.dtype == np.float32


@pytest.mark.parametrize('decay', [0.5, 0.9, 0.9998])
def test_restatement_against_the_float64_recurrence(decay):
    """40 steps on 10 000 seeded normal values while p takes a random walk; after n = 40 steps the float32 restatement is within
    2 n = 80 ulp of max(|e|, |p|) of the float64 recurrence: a step adds at most three roundings of about that size and amplifies none
    (the recurrence is a convex combination).  Measured on this data: 2.7 ulp (decay 0.5) and 31.9 ulp (0.9 and 0.9998, still in the
    warm-up: e trails p, so the ulp of their current maximum can be smaller than that of earlier operands), against the bound of 80.
    On the way every step is held to the bound that can be derived exactly: with M the largest magnitude any operand has had so far
    (|e0| and every |p|), p - e and om * d are at most 2 M, so each rounds by at most 1 ulp(M), and e + q by at most 1/2: 2.5 n ulp(M)
    after n steps (measured: 2.5 at most at any step, 1.0 to 1.6 after 40: the errors mostly cancel).
    torch.lerp is NOT a pin for this recurrence: it switches formula at weight 0.5 (e + w (p - e) below, p - (p - e)(1 - w) from there
    on) and differs from the restatement by up to 12 ulp on the same data, so it is not asserted here."""
    g = np.random.default_rng(1234)
    p = g.standard_normal(10000).astype(F)
    e32 = g.standard_normal(10000).astype(F)
    e64 = e32.astype(np.float64)
    big = np.abs(e32)
    for n in range(1, 41):
        p = (p + F(0.05) * g.standard_normal(10000).astype(F)).astype(F)
        e64 = R.update_f64(e64, p, decay, True, n - 1)
        e32 = R.update(e32, p, decay, True, n - 1)
        big = np.maximum(big, np.abs(p))
        step_err = float((np.abs(e32.astype(np.float64) - e64) / np.spacing(big).astype(np.float64)).max())
        assert step_err <= 2.5 * n, (n, step_err)
    ulp = np.spacing(np.maximum(np.abs(e32), np.abs(p))).astype(np.float64)
    err = float((np.abs(e32.astype(np.float64) - e64) / ulp).max())
    print('decay %g: %.2f ulp of max(|e|, |p|) after 40 steps (bound 80); %.2f ulp of the largest operand so far' % (decay, err, step_err))
    assert err <= 2 * 40, err


def test_non_finite_values_follow_ieee():
    e = np.array([1.0, 1.0, np.inf, 2.0], F)
    p = np.array([np.nan, np.inf, np.inf, 2.0], F)
    out = R.update(e, p, 0.5, False, 0)
    assert np.isnan(out[0]) and out[1] == np.inf and np.isnan(out[2]) and out[3] == F(2.0)


def _prototypes():
    h = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'effdet_ema.h')).read(), flags=re.S)
    scalar = {'int': 'i', 'long long': 'q', 'float': 'f', 'effdet_stream_t': 'p'}
    protos = {}
    for r, name, params in re.findall(r'^([a-z][a-z ]*?\*?)\s*\b(effdet_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', h, flags=re.M):
        kinds = ['p' if '*' in p else scalar[' '.join(p.split()).rsplit(' ', 1)[0]] for p in params.split(',')]
        assert name not in protos, name
        protos[name] = ({'int': 'i', 'long long': 'q'}[' '.join(r.split())], kinds)
    return h, protos


def test_ema_signatures_match_the_companion_header():
    """_lib.EMA_SIGNATURES against the prototypes of include/effdet_ema.h, parsed as tests/test_soft_nms_host.py parses its header: the
    same names, return kind, parameter count and kinds in order; the built library exports all three and lib() binds them with the
    table's types; none of them is in effdet_hip.h's table or in ADDED_SIGNATURES, and the ABI generation stays 11."""
    from efficientdet.pytorch_amd import build, _lib
    h, protos = _prototypes()
    assert sorted(protos) == sorted(set(re.findall(r'\b(effdet_[a-z0-9_]+)\s*\(', h))) == sorted(NEW)
    assert sorted(_lib.EMA_SIGNATURES) == sorted(protos)
    assert not set(protos) & (set(_lib.SIGNATURES) | set(_lib.ADDED_SIGNATURES))
    assert len(_lib.SIGNATURES) == 91 and sorted(_lib.ADDED_SIGNATURES) == ['effdet_soft_nms', 'effdet_soft_nms_workspace_bytes']
    build.build(verbose=False)
    L = _lib.require(*protos)
    assert int(L.effdet_abi_version()) == 11 == _lib.ABI_VERSION
    for name, (r, kinds) in protos.items():
        sig = _lib.EMA_SIGNATURES[name]
        assert sig[1] == ':' and sig[0] == r, (name, sig, r)
        assert list(sig[2:].replace('s', 'p')) == kinds, (name, sig, ''.join(kinds))
        f = getattr(L, name)
        assert f.restype is _lib._CTYPE[sig[0]] and list(f.argtypes) == [_lib._CTYPE[c] for c in sig[2:]], name
    # the EMA entry points extend the plain ones: the same leading tables, the average's table behind the moments
    plain = _lib.SIGNATURES['effdet_clip_adamw_step']
    assert len(_lib.EMA_SIGNATURES['effdet_clip_adamw_step_ema']) == len(plain) + 4
    assert len(_lib.EMA_SIGNATURES['effdet_clip_adamw_step_gated_ema']) == len(_lib.SIGNATURES['effdet_clip_adamw_step_gated']) + 4


def test_the_header_compiles_as_c_and_the_control_block_matches(tmp_path):
    import shutil
    import subprocess
    from efficientdet.pytorch_amd import _lib
    assert [n for n, _ in _lib.EmaCtl._fields_] == ['updates', 'reserved'] and C.sizeof(_lib.EmaCtl) == 16
    if shutil.which('gcc') is None:
        return                                                   # (the layout assertions above hold without a compiler)
    src = tmp_path / 'h.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "effdet_ema.h"\n'
                   'int main(void){printf("%zu %zu %d\\n", sizeof(effdet_ema_ctl_t), offsetof(effdet_ema_ctl_t, updates), EFFDET_ABI_VERSION);return 0;}\n')
    exe = tmp_path / 'h'
    subprocess.run(['gcc', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [16, 0, 11]
    assert _lib.EmaCtl.updates.offset == 0


def test_entry_points_refuse_null_tables_empty_grids_and_bad_decays():
    from efficientdet.pytorch_amd import build, _lib
    build.build(verbose=False)
    L = _lib.require(*NEW)
    P, N = 0x1000, None          # "some non-null pointer": never dereferenced, every call below is refused before a launch
    # params, grads, exp_avg, exp_avg_sq, ema, numel, block_tensor, block_first, ntensors, nblocks, scratch, steps, 6 floats,
    # write_grad, ema_decay, ema_warmup, hyper_dev, ema_ctl, stream
    good = [P, P, P, P, P, P, P, P, 1, 1, P, P, 0.1, 1e-4, 0.9, 0.999, 1e-8, 1e-2, 0, 0.5, 1, N, P, N]
    for i in (0, 1, 2, 3, 4, 5, 6, 7, 10, 11, 22):
        a = list(good); a[i] = N
        assert L.effdet_clip_adamw_step_ema(*a) == -1, i
    for i in (8, 9):
        a = list(good); a[i] = 0
        assert L.effdet_clip_adamw_step_ema(*a) == -1, i
    for bad in (1.0, -0.5, 2.0, float('nan')):                   # by-value decay (no device hyper buffer) outside [0, 1)
        a = list(good); a[19] = bad
        assert L.effdet_clip_adamw_step_ema(*a) == -1, bad
    # params, grads, acc, exp_avg, exp_avg_sq, ema, numel, block_tensor, block_first, ntensors, nblocks, scratch, steps, 6 floats,
    # ema_decay, ema_warmup, hyper_dev, ctl, ema_ctl, stream
    good = [P, P, P, P, P, P, P, P, P, 1, 1, P, P, 0.1, 1e-4, 0.9, 0.999, 1e-8, 1e-2, 0.5, 1, N, P, P, N]
    for i in (0, 1, 2, 3, 4, 5, 6, 7, 8, 11, 12, 22, 23):
        a = list(good); a[i] = N
        assert L.effdet_clip_adamw_step_gated_ema(*a) == -1, i
    a = list(good); a[19] = float('nan')
    assert L.effdet_clip_adamw_step_gated_ema(*a) == -1
    good = [P, P, P, P, P, 1, 1, N]                              # params, ema, numel, block_tensor, block_first, ntensors, nblocks, stream
    for i in (0, 1, 2, 3, 4):
        a = list(good); a[i] = N
        assert L.effdet_ema_swap(*a) == -1, i
    for i in (5, 6):
        a = list(good); a[i] = 0
        assert L.effdet_ema_swap(*a) == -1, i


def test_constructor_refuses_bad_decays_and_plain_optimizers_refuse_the_ema_surface():
    import torch
    from efficientdet.pytorch_amd.optim import ClipAdamW
    p = torch.nn.Parameter(torch.zeros(3))
    for bad in (1.0, 1.5, -1e-3, float('nan'), float('inf'), 1.0 - 2.0 ** -30, 'half'):      # (1 - 2^-30 rounds to 1.0f)
        with pytest.raises(ValueError, match='ema_decay'):
            ClipAdamW([p], ema_decay=bad)
    for ok in (0.0, 0.5, 0.9998):
        o = ClipAdamW([p], ema_decay=ok)
        assert o.ema is True and o.ema_warmup is True and o.param_groups[0]['ema_decay'] == ok
    assert ClipAdamW([p], ema_decay=0.5, ema_warmup=False).ema_warmup is False
    assert ClipAdamW([p], ema_decay=0.5, accumulate=True).accumulate is True
    plain = ClipAdamW([p])
    assert plain.ema is False and 'ema_decay' not in plain.param_groups[0] and 'ema_updates' not in plain.state_dict()
    for call in (plain.ema_params, plain.ema_updates, plain.swap_ema, lambda: plain.ema_weights().__enter__()):
        with pytest.raises(RuntimeError, match='ema_decay'):
            call()
    assert ClipAdamW([p], ema_decay=0.5).ema_updates() == 0      # nothing built yet
    # a decay changed through param_groups is checked where it is read
    o = ClipAdamW([p], ema_decay=0.5)
    o.param_groups[0]['ema_decay'] = 1.0
    with pytest.raises(ValueError, match='ema_decay'):
        o._hyper_values()
    from efficientdet.pytorch_amd import checkpoint
    assert callable(checkpoint.ema_state_dict)


def test_documents_name_the_average():
    for name in ('README.md', 'DESIGN.md', 'INTEGRATION.md'):
        md = open(os.path.join(ROOT, name)).read()
        assert 'ema_decay' in md, name
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert 'ema_swap_kernel' in design and 'freeze_bn' in design
