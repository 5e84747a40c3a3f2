"""CPU tier: include/effdet_gate_operand.h against the binding (_lib.GATE_OPERAND_SIGNATURES) and the built library, and what the two
planners accept and refuse for the operand-gate form (no device work: the tensors only lend their addresses)."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACT_NONE, ACT_RELU, ACT_SWISH = 0, 1, 2


def test_signatures_match_the_header_and_the_library():
    """The table against the header's prototypes, parsed as tests/test_abi.py parses effdet_hip.h's; the built library exports the names
    and lib() binds them with the table's types; the names are not in effdet_hip.h's table, whose ABI generation and descriptor layouts
    are unchanged."""
    from efficientdet.pytorch_amd import build, _lib
    h = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'effdet_gate_operand.h')).read(), flags=re.S)
    scalar = {'int': 'i', 'long long': 'q', 'float': 'f', 'effdet_stream_t': 'p'}
    protos = {}
    for r, name, params in re.findall(r'^([a-z][a-z ]*?\*?)\s*\b(effdet_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', h, flags=re.M):
        kinds = []
        for p in params.split(','):
            p = ' '.join(p.split())
            kinds.append('p' if '*' in p else scalar[p.rsplit(' ', 1)[0]])
        assert ' '.join(r.split()) == 'int'
        protos[name] = kinds
    assert sorted(_lib.GATE_OPERAND_SIGNATURES) == sorted(protos) == ['effdet_conv2d_gated', 'effdet_conv2d_gated_plan_info',
                                                                      'effdet_conv2d_wgrad_gated', 'effdet_conv2d_wgrad_gated_kernel']
    assert not set(protos) & set(_lib.SIGNATURES)
    build.build(verbose=False)
    L = _lib.require(*protos)
    for name, kinds in protos.items():
        sig = _lib.GATE_OPERAND_SIGNATURES[name]
        assert sig[:2] == 'i:' and list(sig[2:].replace('s', 'p')) == kinds, (name, sig, ''.join(kinds))
        f = getattr(L, name)
        assert f.restype is C.c_int and list(f.argtypes) == [_lib._CTYPE[c] for c in sig[2:]], name
    assert int(L.effdet_abi_version()) == _lib.ABI_VERSION


def _maps(B, H, W, Cin, Cout):
    from efficientdet.pytorch_amd.ops import Map
    x = Map(torch.empty(1), B, H, W, Cin); y = Map(torch.empty(1), B, H, W, Cout)       # (addresses only)
    return x, y, torch.empty(Cout * Cin), torch.empty(B, Cin)


def _d0_blocks():
    """(block index, map side, expanded channels, project output channels) of D0's 16 MBConv blocks @512"""
    from efficientdet.pytorch_amd.config import backbone_plan
    side, out = 256, []
    for i, blk in enumerate(backbone_plan('efficientnet-b0')[2]):
        side = (side + blk.stride - 1) // blk.stride
        out.append((i, side, blk.cexp, blk.cout))
    return out


def test_the_benchmarks_maps():
    assert [b[1] for b in _d0_blocks()] == [256, 128, 128, 64, 64, 32, 32, 32, 16, 16, 16, 8, 8, 8, 8, 4]


@pytest.mark.parametrize('i,S,Ce,Co', _d0_blocks())
def test_both_planners_on_every_project_conv_of_the_benchmark(i, S, Ce, Co):
    """D0, B = 32 @512: blocks 0 .. 10 (maps of 256^2 .. 16^2: whole 128-pixel tiles per image) are accepted by both planners, in the
    exact arithmetic (forward) and in both gradient arithmetics, and the gated forward launch is the 128-pixel-tile kernel of the plain
    one -- same tile, stages and grid, plus the gate row in LDS; blocks 11 .. 15 (8 x 8 and 4 x 4) are refused by the forward planner."""
    from efficientdet.pytorch_amd import build, ops
    build.build(verbose=False)
    x, y, wp, gate = _maps(32, S, S, Ce, Co)
    kw = dict(Cin=Ce, Cout=Co, KH=1, KW=1, scale=torch.empty(Co), shift=torch.empty(Co))
    old = (ops.F32_ARITH, ops.F32_ARITH_BWD)
    try:
        ops.set_f32_arith('f32')
        if (S * S) % 128:
            assert i >= 11 and not ops.conv2d_gated_ok(x, wp, y, gate, ACT_SWISH, **kw)
            return
        assert i <= 10
        assert ops.conv2d_gated_ok(x, wp, y, gate, ACT_SWISH, **kw) and ops.conv2d_gated_ok(x, wp, y, gate, ACT_NONE, **kw)
        plain = ops.conv2d_plan_info(x, wp, y, **kw)
        info = ops.conv2d_gated_plan_info(x, wp, y, gate, ACT_SWISH, **kw)
        assert info['gate'] == 2 and info['form'] == 'plain' and not info['persistent']
        for k in ('id', 'tile_m', 'tile_n', 'stages', 'threads', 'mtiles', 'ntiles', 'grid', 'ksteps'):
            assert info[k] == plain[k], (k, info[k], plain[k])
        assert info['lds_bytes'] == plain['lds_bytes'] + info['ksteps'] * 128
        for arith in ('f32', 'bf16x3'):
            ops.set_f32_arith(arith)
            plain_id = ops.conv2d_wgrad_kernel_id(x, y, image_splits=True, Cin=Ce, Cout=Co, KH=1, KW=1)
            assert plain_id == (1 if i <= 3 else 0)                 # the thin pointwise kernel on blocks 0 .. 3 (<= 192 channels in all)
            assert ops.conv2d_wgrad_kernel_id(x, y, image_splits=True, a_gate=gate, a_act=ACT_SWISH, Cin=Ce, Cout=Co, KH=1, KW=1) == plain_id
            assert ops.conv2d_wgrad_gated_ok(x, y, gate, ACT_SWISH, Cin=Ce, Cout=Co)
    finally:
        ops.F32_ARITH, ops.F32_ARITH_BWD = old


def test_refusals():
    """Never a plain launch on ungated data: what the form does not cover is EFFDET_EUNSUPPORTED (False / -3), a bad activation code or a
    null gate EFFDET_EINVAL."""
    from efficientdet.pytorch_amd import build, ops, _lib
    from efficientdet.pytorch_amd.ops import Map
    build.build(verbose=False)
    old = (ops.F32_ARITH, ops.F32_ARITH_BWD)
    try:
        ops.set_f32_arith('f32')
        x, y, wp, gate = _maps(2, 16, 16, 144, 24)
        kw = dict(Cin=144, Cout=24, KH=1, KW=1)
        assert ops.conv2d_gated_ok(x, wp, y, gate, ACT_SWISH, **kw)
        with pytest.raises(RuntimeError, match='EFFDET_EINVAL'):
            ops.conv2d_gated_ok(x, wp, y, gate, ACT_RELU, **kw)
        x6, y6, _, _ = _maps(2, 6, 6, 144, 24)
        assert not ops.conv2d_gated_ok(x6, wp, y6, gate, ACT_SWISH, **kw)                       # images are no whole 128-pixel tiles
        assert not ops.conv2d_gated_ok(x, wp, y, gate, ACT_SWISH, **dict(kw, KH=3, KW=3, pad_t=1, pad_l=1))     # not pointwise
        assert not ops.conv2d_gated_ok(x, wp, y, gate, ACT_SWISH, w_image_stride=144 * 24 * 4, **kw)          # per-image weights
        xb, yb = Map(torch.empty(1, dtype=torch.bfloat16), 2, 16, 16, 144), Map(torch.empty(1, dtype=torch.bfloat16), 2, 16, 16, 24)
        assert not ops.conv2d_gated_ok(xb, wp, yb, gate, ACT_SWISH, **kw)                       # bf16 storage
        x2, y2, wp2, gate2 = _maps(2, 16, 16, 480, 80)
        ops.set_f32_arith('bf16x3')
        assert not ops.conv2d_gated_ok(x2, wp2, y2, gate2, ACT_SWISH, Cin=480, Cout=80, KH=1, KW=1)     # the bf16x3 forward (K >= 256)
        ops.set_f32_arith('f32')
        wk = dict(Cin=144, Cout=24, KH=1, KW=1)
        assert ops.conv2d_wgrad_kernel_id(x, y, image_splits=True, a_gate=gate, a_act=ACT_SWISH, **wk) == 0
        assert ops.conv2d_wgrad_kernel_id(x, y, image_splits=False, a_gate=gate, a_act=ACT_SWISH, **wk) == -3
        assert ops.conv2d_wgrad_kernel_id(x, y, image_splits=True, a_gate=gate, a_act=ACT_RELU, **wk) == -1
        assert ops.conv2d_wgrad_kernel_id(xb, yb, image_splits=True, a_gate=gate, a_act=ACT_SWISH, **wk) == -3
        assert not ops.conv2d_wgrad_gated_ok(x6, y6, gate, ACT_SWISH, Cin=144, Cout=24)         # 36 pixels: no per-image splits at all
        L = _lib.require('effdet_conv2d_gated', 'effdet_conv2d_wgrad_gated')
        d, _, _ = ops._conv_desc(x, wp, y, **kw)
        assert int(L.effdet_conv2d_gated(C.byref(d), None, ACT_SWISH, None)) == -1
        info = _lib.ConvPlanInfo()
        assert int(L.effdet_conv2d_gated_plan_info(C.byref(d), None, ACT_SWISH, C.byref(info))) == -1
        assert int(L.effdet_conv2d_wgrad_gated_kernel(None, gate.data_ptr(), ACT_SWISH)) == -1
    finally:
        ops.F32_ARITH, ops.F32_ARITH_BWD = old
