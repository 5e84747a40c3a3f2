"""CPU tier: the path functions of the MBConv section (functional.mbconv_path, mbconv_gate_settled, mbconv_bwd_path) against the
recording of tests/golden/mbconv_call_sequence.json -- for every run and every block the records they compute, for that block's geometry
under that run's switches, say what the recorded step did (no device work: the planner queries take host tensors, which only lend
their addresses) -- and the rule that nothing else in functional.py reads an MBConv switch."""
import os
import re

import pytest
import torch

from tests.mbconv_path_cases import B, NBLOCKS, RUNS, SWITCHES, block_geometry, load_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def expected():
    return load_fixture()


def _paths(run):
    """[(forward record, backward record or None)] of the 16 blocks of RUNS[run]"""
    from efficientdet.pytorch_amd import build, ops, functional as Fn
    from efficientdet.pytorch_amd.config import conv_out
    from efficientdet.pytorch_amd.ops import ACT_NONE, ACT_SWISH, RES_ADD, RES_NONE, Map
    build.build(verbose=False)
    r = RUNS[run]
    dtype = torch.bfloat16 if r['storage'] == 'bf16' else torch.float32
    fwd_arith, bwd_arith, _ = ops.MODEL_ARITH[r['arith']]
    m = lambda side, C: Map(torch.empty(1, dtype=dtype), B, side, side, C)                  # (addresses only)
    names = sorted((set(r['before']) | set(r['between'])) - {'STEM_LINK'})
    old, old_arith = {k: getattr(Fn, k) for k in names}, (ops.F32_ARITH, ops.F32_ARITH_BWD)
    stem_link = r['before'].get('STEM_LINK', True)
    out = []
    try:
        for i, (blk, side) in enumerate(block_geometry()):
            for k in names:
                setattr(Fn, k, r['before'].get(k, old[k]))
            ops.set_f32_arith(fwd_arith)
            x = m(side, blk.cin)
            so = conv_out(side, blk.k, blk.stride, blk.pad)
            in_act = ACT_SWISH if (i == 0 and r['train'] and stem_link) else ACT_NONE
            path = Fn.mbconv_path(blk, x, dtype, r['train'], in_act)
            if path.gate == Fn.GATE_OPERAND:
                skip = blk.skip
                pkw = dict(Cin=blk.cexp, Cout=blk.cout, KH=1, KW=1, scale=torch.empty(blk.cout), shift=torch.empty(blk.cout), act=ACT_NONE,
                           rowscale=torch.empty(B) if skip else None, res=x if skip else None, res_mode=RES_ADD if skip else RES_NONE)
                path = Fn.mbconv_gate_settled(path, m(so, blk.cexp), torch.empty(blk.cout * blk.cexp), m(so, blk.cout), torch.empty(B, blk.cexp), pkw)
            bp = None
            if r['train']:
                for k in names:
                    setattr(Fn, k, r['between'].get(k, r['before'].get(k, old[k])))
                ops.set_f32_arith(bwd_arith)
                bp = Fn.mbconv_bwd_path(path, dtype, so * so)
            out.append((path, bp))
    finally:
        for k, v in old.items():
            setattr(Fn, k, v)
        ops.F32_ARITH, ops.F32_ARITH_BWD = old_arith
    return out


def _names(entries):
    return [e[0] for e in entries]


@pytest.mark.parametrize('run', list(RUNS))
def test_the_records_say_what_the_recorded_step_did(expected, run):
    from efficientdet.pytorch_amd import functional as Fn
    paths = _paths(run)
    assert len(paths) == len(expected[run]) == NBLOCKS
    for i, ((path, bp), rec) in enumerate(zip(paths, expected[run])):
        fwd, bwd = rec['fwd'], rec['bwd']
        gated = [e for e in fwd if e[0] == 'conv2d' and e[1][-1].get('a_gate') is not None]
        assert ('channel_scale' in _names(fwd)) == (path.gate in (Fn.GATE_XS_FROM_ZD, Fn.GATE_XS_FROM_XD)), (run, i, path)
        assert bool(gated) == (path.gate == Fn.GATE_OPERAND), (run, i, path)
        assert ('scale_pack_weight' in _names(fwd)) == (path.gate == Fn.GATE_WEIGHTS), (run, i, path)
        assert ('expand_dw_fwd' in _names(fwd)) == (path.expand == Fn.EXPAND_IN_DW), (run, i, path)
        if RUNS[run]['train']:
            assert ('se_dgate_from_wgrad' in _names(bwd)) == bp.se_fused, (run, i, bp)
            # what the backward materialises itself, and from which tensor: a channel_scale call there, with or without the Swish
            cs = [e for e in bwd if e[0] == 'channel_scale']
            gated_wgrad = [e for e in bwd if e[0] == 'conv2d_wgrad' and e[1][-1].get('a_gate') is not None]
            assert len(cs) == (0 if bp.xs_from is None or gated_wgrad else 1), (run, i, bp)
            assert bool(gated_wgrad) <= (bp.gate == Fn.GATE_OPERAND), (run, i, bp)
            if cs:
                assert (len(cs[0][1]) == 4) == (bp.xs_from == 'zd'), (run, i, bp, cs)          # (zd, gate, ACT_SWISH, {}) | (xd, gate, {})
        else:
            assert bp is None and not bwd


def test_every_gate_form_and_every_reaction_is_among_the_runs():
    """The runs reach all four forward gate forms, all four expand forms, and the backward's three sources of xs."""
    from efficientdet.pytorch_amd import functional as Fn
    fw, ex, xs = set(), set(), set()
    for run in RUNS:
        for path, bp in _paths(run):
            fw.add(path.gate); ex.add(path.expand)
            if bp is not None:
                xs.add((bp.se_fused, bp.xs_from))
    assert fw == {Fn.GATE_WEIGHTS, Fn.GATE_OPERAND, Fn.GATE_XS_FROM_ZD, Fn.GATE_XS_FROM_XD}
    assert ex == {Fn.EXPAND_NONE, Fn.EXPAND_IN_DW, Fn.EXPAND_Z, Fn.EXPAND_YZ}
    assert {(True, None), (False, None), (False, 'xd'), (True, 'zd')} <= xs, xs


def test_only_the_two_path_functions_read_the_switches():
    """Each of the twelve switch names occurs in functional.py, comments aside, in its definition and inside mbconv_path /
    mbconv_bwd_path, nowhere else."""
    src = open(os.path.join(ROOT, 'efficientdet', 'pytorch_amd', 'functional.py')).read().split('\n')
    code = [ln.split('#', 1)[0] for ln in src]
    inside, owner = [], None
    for ln in code:
        if ln[:1] not in ('', ' ', '\t', ')'):            # a statement at module level ends whatever function was open
            mt = re.match(r'def (\w+)', ln)
            owner = mt.group(1) if mt else None
        inside.append(owner)
    for name in SWITCHES:
        uses = [(i + 1, inside[i]) for i, ln in enumerate(code) if re.search(r'\b%s\b' % name, ln)]
        defs = [u for u in uses if re.match(r'%s = ' % name, code[u[0] - 1])]
        assert len(defs) == 1, (name, defs)
        others = [u for u in uses if u not in defs]
        assert others, name
        assert all(fn in ('mbconv_path', 'mbconv_bwd_path') for _, fn in others), (name, others)
