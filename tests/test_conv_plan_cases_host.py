"""CPU tier of the large dense-conv tests: the case table of tests/conv_plan_cases.py reaches the kernel instances it is tagged with
(asked of the library's planner through effdet_conv2d_plan_info, no device work), the walking cases meet their tile conditions on a
256-CU device, the table covers every class it was written for, and its float64 reference is a convolution."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

from tests import conv_plan_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_query_binding_matches_its_header(tmp_path):
    """_lib.CONV_PLAN_SIGNATURES, CONV_FORMS and the ConvPlanInfo mirror against include/effdet_conv_plan.h, parsed as tests/test_abi.py
    parses effdet_hip.h; a pure addition: the ABI generation stays where it was."""
    from efficientdet.pytorch_amd import _lib as L
    h = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'effdet_conv_plan.h')).read(), flags=re.S)
    protos = re.findall(r'^([a-z][a-z ]*?\*?)\s*\b(effdet_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', h, flags=re.M)
    assert [n for _, n, _ in protos] == list(L.CONV_PLAN_SIGNATURES) == ['effdet_conv2d_plan_info']
    r, name, params = protos[0]
    assert all('*' in p for p in params.split(',')) and L.CONV_PLAN_SIGNATURES[name] == 'i:' + 'p' * len(params.split(',')) and r.strip() == 'int'
    enums = {k: int(v) for k, v in re.findall(r'(EFFDET_CONV_FORM_[A-Z0-9_]+)\s*=\s*(\d+)', h)}
    assert [enums['EFFDET_CONV_FORM_' + n.upper()] for n in L.CONV_FORMS] == list(range(len(L.CONV_FORMS))) and len(enums) == len(L.CONV_FORMS)
    # the struct: the header's int fields in order, and the size gcc gives it
    body = re.search(r'typedef struct effdet_conv_plan_info_t \{(.*?)\}', h, flags=re.S).group(1)
    fields = [f.strip() for line in re.findall(r'int ([^;]*);', body) for f in line.split(',')]
    assert fields == [n for n, _ in L.ConvPlanInfo._fields_[:-1]] + ['reserved[2]']
    assert C.sizeof(L.ConvPlanInfo) == 4 * 16
    if shutil.which('gcc') is not None:
        src = tmp_path / 'sz.c'
        src.write_text('#include <stdio.h>\n#include "effdet_conv_plan.h"\nint main(void){printf("%zu\\n", sizeof(effdet_conv_plan_info_t));return 0;}\n')
        subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(tmp_path / 'sz')], check=True)
        assert int(subprocess.run([str(tmp_path / 'sz')], capture_output=True, text=True, check=True).stdout) == C.sizeof(L.ConvPlanInfo)
    f = L.require('effdet_conv2d_plan_info').effdet_conv2d_plan_info
    assert f.restype is L._CTYPE['i'] and list(f.argtypes) == [L._CTYPE['p'], L._CTYPE['p']]
    assert L.ABI_VERSION == 11


@pytest.mark.parametrize('c', P.CASES, ids=P.case_id)
def test_case_reaches_the_class_it_is_tagged_with(c):
    info = P.plan(c)
    assert P.reached(c, info) == c.expect, info
    assert info['ksteps'] >= c.min_ksteps, info
    assert info['grid'] == info['mtiles'] * info['ntiles'] and info['mtiles'] == sum(-(-c.B * h * w // info['tile_m']) for h, w in c.sizes)
    assert info['ntiles'] == -(-c.Cout // info['tile_n']) and info['threads'] in (256, 512, 1024)
    if c.expect[4]:
        f = P.walk_facts(c, info, P.MI355X_CUS)
        # tiles >= 2 * CUs + 1: some workgroup takes over a tile AND hands one on; a ragged last round; a partial last channel tile; a
        # hand-over into another pyramid level (other W, HoWo, descriptor)
        assert info['grid'] >= 2 * P.MI355X_CUS + 1 and f['rounds'] >= c.min_rounds >= 3, (info, f)
        assert f['remainder'] != 0 and f['partial_n'] and f['level_changes'] >= 1, f
        assert len(c.sizes) == 5
    else:
        # (a) / (b) / (f): past one workgroup per tile slot of the two-stage kernels; (c): the four-stage window above the narrow tile
        tiles = info['grid']
        assert (128 < tiles <= 256) if info['stages'] == 4 else tiles > 256, info
        assert (c.B * c.sizes[0][0] * c.sizes[0][1]) % 128 != 0 or len(c.sizes) > 1         # a partial pixel tile
    if c.flagged:
        assert info['id'] in (8, 9) and not c.bias and c.act == 0


def test_query_agrees_with_the_kernel_id_query_and_with_the_launch_codes():
    """Same id as effdet_conv2d_kernel on every case's descriptor; on refused descriptors the code effdet_conv2d_kernel (and so the launch,
    which returns plan_conv's code before it touches the device) gives, with the info left alone."""
    from efficientdet.pytorch_amd import ops, _lib as L, functional as Fn
    from efficientdet.pytorch_amd.ops import Map
    lib = L.require('effdet_conv2d_plan_info')
    for c in P.CASES:
        _, xm = Fn.pyramid_alloc(c.B, c.sizes, c.Cin, P.storage_dtype(c), 'cpu')
        _, ym = Fn.pyramid_alloc(c.B, c.sizes, c.Cout, P.out_dtype(c), 'cpu')
        wp, sh = torch.empty(c.Cout * 9 * c.Cin + c.Cout, dtype=P.storage_dtype(c)), torch.empty(c.Cout)
        with P.tuned(c):
            d, _, _ = ops._conv_desc(xm, wp, ym, **P.conv_kwargs(c, sh if c.bias else None, ym))
            info = L.ConvPlanInfo()
            rc = int(lib.effdet_conv2d_plan_info(C.byref(d), C.byref(info)))
            assert rc == int(lib.effdet_conv2d_kernel(C.byref(d))) == info.id == P.plan(c)['id'] >= 0, c.name
    ids = {P.plan(c)['id'] for c in P.CASES}
    assert ids == {0, 1, 4, 5, 8, 9, 30, 31, 10 + 442, 10 + 242, 10 + 243, 10 + 423, 10000 + 442}
    # refused descriptors
    x, y, w = Map.new(1, 8, 8, 64, torch.float32, 'cpu'), Map.new(1, 8, 8, 64, torch.float32, 'cpu'), torch.empty(64 * 9 * 64 + 64)
    kw = dict(Cin=64, Cout=64, KH=3, KW=3, pad_t=1, pad_l=1)
    refused = [
        (dict(kw, Cin=62), -3),                                            # Cin % 4: EFFDET_EUNSUPPORTED
        (dict(kw, stride=0), -3),
        (dict(kw, res_mode=ops.RES_ADD), -1),                              # a residual mode without a residual: EFFDET_EINVAL
        (dict(kw, hsplit=True, res=y, res_mode=ops.RES_ADD, out_f32=True), -3),      # the f16x3 form has no residual op
        (dict(kw, split=True, zs=y), -3),                                  # no pre-activation copy from the split layout
        (dict(kw, bc_scale=torch.empty(64)), -1),                          # bc_scale without bc_shift
    ]
    for args, code in refused:
        d, _, _ = ops._conv_desc(x, w, y, **args)
        info = L.ConvPlanInfo(id=-7, grid=-7)
        assert int(lib.effdet_conv2d_plan_info(C.byref(d), C.byref(info))) == int(lib.effdet_conv2d_kernel(C.byref(d))) == code, args
        assert info.id == -7 and info.grid == -7                           # written only on success
        with pytest.raises(RuntimeError):
            ops.conv2d_plan_info(x, w, y, **args)
    d, _, _ = ops._conv_desc(x, w, y, **kw)
    assert int(lib.effdet_conv2d_plan_info(C.byref(d), None)) == -1 and int(lib.effdet_conv2d_plan_info(None, C.byref(L.ConvPlanInfo()))) == -1
    d.nseg = 11
    assert int(lib.effdet_conv2d_plan_info(C.byref(d), C.byref(L.ConvPlanInfo()))) == int(lib.effdet_conv2d_kernel(C.byref(d))) == -1


def test_query_tells_apart_what_the_kernel_id_does_not():
    """The blind spot the query closes: ids 0 and 4 each name three template instances (two-stage, four-stage, the narrow 32-channel
    tile), which the plan reports apart; the skinny pointwise kernel reports no matrix-core tile."""
    from efficientdet.pytorch_amd import ops
    from efficientdet.pytorch_amd.ops import Map
    seen = {}
    for B, hw in ((2, 92), (1, 92), (1, 40)):                              # 266, 134 and 26 tiles of 128 x 128
        x, y = Map.new(B, hw, hw, 64, torch.float32, 'cpu'), Map.new(B, hw, hw, 256, torch.float32, 'cpu')
        i = ops.conv2d_plan_info(x, torch.empty(256 * 9 * 64), y, Cin=64, Cout=256, KH=3, KW=3, pad_t=1, pad_l=1)
        seen[(i['tile_n'], i['stages'])] = i['id']
        assert i['lds_bytes'] == i['stages'] * (128 + i['tile_n']) * 128 and not i['persistent'] and not i['m32']
    assert seen == {(128, 2): 0, (128, 4): 0, (32, 4): 0}
    x, y = Map.new(16, 64, 64, 16, torch.float32, 'cpu'), Map.new(16, 64, 64, 96, torch.float32, 'cpu')
    i = ops.conv2d_plan_info(x, torch.empty(96 * 16), y, Cin=16, Cout=96, KH=1, KW=1)
    assert (i['id'], i['form'], i['tile_n'], i['grid'], i['ksteps'], i['lds_bytes']) == (20, 'skinny', 96, 64, 1, 0)


def test_table_reaches_every_required_class_and_the_existing_tables_do_not():
    """Closure over (a)-(f), read off the planner's answers; and the gap itself: the largest shapes the existing op-level files run stay at
    one tile per workgroup on a 256-CU device, or below 257 / 129 tiles with a long K loop."""
    from efficientdet.pytorch_amd import ops, _lib as L
    from efficientdet.pytorch_amd.ops import Map
    got = {P.reached(c, P.plan(c)) for c in P.CASES}
    assert got >= P.REQUIRED_CLASSES, P.REQUIRED_CLASSES - got
    assert {c.expect for c in P.CASES} == got
    # both output forms of the persistent split-layout kernel, a flagged launch per split-layout tile width, ReLU and no activation
    assert {(c.out, c.mask) for c in P.CASES if c.expect == ('split', 256, 256, 2, True)} == {('f32', False), ('same', True)}
    assert {c.expect[2] for c in P.CASES if c.flagged} == {128, 64}
    assert {c.act for c in P.CASES} == {0, 1} and any(c.Cout == 200 for c in P.CASES if c.expect[:4] == ('f32', 128, 128, 2))
    # tests/test_gpu_split.py's "tile walk" shape under the persistent knob: 7 tiles, one per workgroup
    x, y = Map.new(3, 24, 24, 256, torch.float32, 'cpu'), Map.new(3, 24, 24, 256, torch.float32, 'cpu')
    old = (ops.tuning_set(L.TUNE_SPLIT_PERS, 1), ops.tuning_set(L.TUNE_IGEMM_BIG_MIN_M, 0))
    try:
        i = ops.conv2d_plan_info(x, torch.empty(256 * 9 * 256), y, Cin=256, Cout=256, KH=3, KW=3, pad_t=1, pad_l=1, split=True)
    finally:
        ops.tuning_set(L.TUNE_SPLIT_PERS, old[0]); ops.tuning_set(L.TUNE_IGEMM_BIG_MIN_M, old[1])
    assert i['persistent'] and i['grid'] == 7 < P.MI355X_CUS


@pytest.mark.parametrize('c', [c for c in P.CASES if c.flagged], ids=P.case_id)
def test_flagged_case_deals_dead_and_live_tiles_into_later_groups_and_the_tail(c):
    info = P.plan(c)
    live = P.tile_flags(c, P.live_pixels(c))
    mtiles, ntiles = info['mtiles'], info['ntiles']
    assert live.numel() == mtiles >= 17 and mtiles % 8 != 0
    slots = P.deal(mtiles, ntiles)
    assert sorted((mt, nt) for mt, nt, _ in slots) == [(mt, nt) for mt in range(mtiles) for nt in range(ntiles)]       # a bijection
    later = [int(live[mt]) for mt, _, j in slots if j >= 1]
    tail = [int(live[mt]) for mt, _, j in slots if j < 0]
    assert 0 in later and 1 in later and 0 in tail and 1 in tail
    assert max(j for _, _, j in slots) == mtiles // 8 - 1 >= 20
    # a dead tile really has no non-zero tap: no live pixel inside it or next to it (checked on level 0, where a tile is whole rows)
    px = P.live_pixels(c)[0]
    h, w = c.sizes[0]
    rows_per_tile = 128 // w
    for t in range(0, c.B * h * w // 128, 7):
        b, r0 = divmod(t * rows_per_tile, h)
        near = px[b, max(r0 - 1, 0):min(r0 + rows_per_tile + 1, h)].any()
        assert bool(near) == bool(live[t]), t


# ----------------------------------------------------------------------------- the reference
def _tiny(seed, B, H, W, Cin, Cout):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, H, W, Cin, generator=g, dtype=torch.float64), torch.randn(Cout, Cin, 3, 3, generator=g, dtype=torch.float64),
            torch.randn(Cout, generator=g, dtype=torch.float64))


@pytest.mark.parametrize('pads', [(1, 1, 1, 1), (0, 2, 1, 0), (2, 0, 0, 1)])
def test_unfold_reference_is_a_convolution(pads):
    """conv64_unfold against nested loops at tiny shapes: stride 1, symmetric and asymmetric padding, two levels of different sizes (as
    two calls, the way the GPU test walks a pyramid), a bias, and S = the same sum on absolute values."""
    for lvl, (H, W) in enumerate([(5, 4), (3, 6)]):
        x, w, b = _tiny(3 + lvl, 2, H, W, 3, 4)
        want = P.naive_conv(x, w, b, pads)
        ref, S = P.conv64_unfold(x, w, b, pads)
        assert ref.shape == want.shape == S.shape and float((ref - want).abs().max()) <= 1e-13 * float(want.abs().max())
        assert float((S - P.naive_conv(x.abs(), w.abs(), b.abs(), pads)).abs().max()) <= 1e-13 * float(S.max())
        assert bool((S >= ref.abs() - 1e-13).all())
        assert float((P.conv64_cpu(x, w, b, pads) - want).abs().max()) <= 1e-13 * float(want.abs().max())
        ref0, _ = P.conv64_unfold(x, w, None, pads)
        assert float((ref0 + b - ref).abs().max()) <= 1e-13


def test_unfold_reference_matches_conv2d_on_a_small_pyramid():
    """Three levels at the cases' own geometry (3x3 'same', NHWC) against F.conv2d in float64."""
    for lvl, (H, W) in enumerate([(16, 16), (8, 8), (4, 4)]):
        x, w, b = _tiny(11 + lvl, 3, H, W, 32, 40)
        ref, S = P.conv64_unfold(x, w, b)
        want = P.conv64_cpu(x, w, b)
        assert float((ref - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_layout_decoders_and_bounds():
    """from_split64 / from_hsplit64 on hand-made groups, and value_bound's constants."""
    hi, lo = torch.randn(2, 3, 64).bfloat16(), (torch.randn(2, 3, 64) * 2.0 ** -9).bfloat16()
    t = torch.stack([hi.view(2, 3, 2, 32), lo.view(2, 3, 2, 32)], dim=3).reshape(2, 3, 128).contiguous().view(torch.float32)
    assert t.shape == (2, 3, 64) and torch.equal(P.from_split64(t), hi.double() + lo.double())
    hh, hl = torch.randn(2, 3, 64).half(), torch.randn(2, 3, 64).half()
    t = torch.stack([hh.view(2, 3, 2, 32), hl.view(2, 3, 2, 32)], dim=3).reshape(2, 3, 128).contiguous().view(torch.float32)
    assert torch.equal(P.from_hsplit64(t), hh.double() + hl.double() / 2048.0)
    S, ref = torch.tensor([2.0], dtype=torch.float64), torch.tensor([-0.5], dtype=torch.float64)
    by = {c.name: c for c in P.CASES}
    base = lambda cin: 2.0 * (9 * cin + 3) * 2.0 ** -24 * 2.0
    assert float(P.value_bound(by['a-f32'], S, ref)) == base(64)
    assert float(P.value_bound(by['a-bf16'], S, ref)) == base(128) + 2.0 ** -8 * 0.5
    assert float(P.value_bound(by['a-bf16x3'], S, ref)) == base(64) + 2.0 ** -14 * 2.0
    assert float(P.value_bound(by['d-split-f32out'], S, ref)) == base(256) + 2.0 ** -14 * 2.0
    assert float(P.value_bound(by['d-split-mask'], S, ref)) == base(256) + 2.0 ** -14 * 2.0 + 2.0 ** -16 * 0.5
    assert 3 * 2.0 ** -16 * (1 + 2.0 ** -7) < P.X3_PER_PRODUCT
