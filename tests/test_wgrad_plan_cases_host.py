"""CPU tier of the multi-range weight-gradient tests: the new plan query against its header, the case table of tests/wgrad_plan_cases.py
against the planner (effdet_conv2d_wgrad_plan_info, no device work), the three older queries, a restatement of the paired launch's
block map, the flag patterns of the flagged cases, and the float64 reference against nested loops."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

from tests import wgrad_plan_cases as P
from tests.conv_plan_cases import xcd_remap
from tests.host_util import wgrad_desc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BY_NAME = {c.name: c for c in P.CASES}


def test_plan_query_binding_matches_its_header(tmp_path):
    """_lib.WGRAD_PLAN_SIGNATURES, WGRAD_PATHS and the WgradPlanInfo mirror against include/effdet_wgrad_plan.h, parsed as
    tests/test_abi.py parses effdet_hip.h; a pure addition: effdet_hip.h's table and the ABI generation stay where they were."""
    from efficientdet.pytorch_amd import _lib as L
    h = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'effdet_wgrad_plan.h')).read(), flags=re.S)
    protos = re.findall(r'^([a-z][a-z ]*?\*?)\s*\b(effdet_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', h, flags=re.M)
    assert [n for _, n, _ in protos] == list(L.WGRAD_PLAN_SIGNATURES) == ['effdet_conv2d_wgrad_plan_info']
    r, name, params = protos[0]
    assert all('*' in p for p in params.split(',')) and L.WGRAD_PLAN_SIGNATURES[name] == 'i:' + 'p' * len(params.split(',')) and r.strip() == 'int'
    assert name not in L.SIGNATURES and name not in open(os.path.join(ROOT, 'include', 'effdet_hip.h')).read()
    enums = {k: int(v) for k, v in re.findall(r'(EFFDET_WGRAD_PATH_[A-Z0-9_]+)\s*=\s*(\d+)', h)}
    assert [enums['EFFDET_WGRAD_PATH_' + n.upper()] for n in L.WGRAD_PATHS] == list(range(len(L.WGRAD_PATHS))) and len(enums) == len(L.WGRAD_PATHS)
    # the struct: the header's int fields in order (arrays with their extents), and the size gcc gives it
    body = re.search(r'typedef struct effdet_wgrad_plan_info_t \{(.*?)\}', h, flags=re.S).group(1)
    fields = [f.strip() for line in re.findall(r'int ([^;]*);', body) for f in line.split(',')]
    mirror = [n if t is C.c_int else '%s[%s]' % (n, {L.MAX_SEG: 'EFFDET_MAX_SEG'}.get(t._length_, t._length_)) for n, t in L.WgradPlanInfo._fields_]
    assert fields == mirror, (fields, mirror)
    assert all(t is C.c_int or t._type_ is C.c_int for _, t in L.WgradPlanInfo._fields_)
    assert C.sizeof(L.WgradPlanInfo) == 4 * (11 + 2 * L.MAX_SEG + 3)
    if shutil.which('gcc') is not None:
        src = tmp_path / 'sz.c'
        src.write_text('#include <stdio.h>\n#include "effdet_wgrad_plan.h"\nint main(void){printf("%zu %d\\n", '
                       'sizeof(effdet_wgrad_plan_info_t), EFFDET_MAX_SEG);return 0;}\n')
        subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(tmp_path / 'sz')], check=True)
        out = subprocess.run([str(tmp_path / 'sz')], capture_output=True, text=True, check=True).stdout.split()
        assert [int(v) for v in out] == [C.sizeof(L.WgradPlanInfo), L.MAX_SEG]
    f = L.require('effdet_conv2d_wgrad_plan_info').effdet_conv2d_wgrad_plan_info
    assert f.restype is L._CTYPE['i'] and list(f.argtypes) == [L._CTYPE['p'], L._CTYPE['p']]
    assert L.ABI_VERSION == 11


@pytest.mark.parametrize('c', P.CASES, ids=P.case_id)
def test_case_has_its_class_and_facts(c):
    info = P.plan(c)
    for form in c.forms:
        assert P.reached(c, info, form) == (c.arith, 'split' if c.kind == 'split' else 'tiled', c.launches, form if c.kind == 'split' else c.layout)
    f = P.facts(c, info)
    assert P.holds(c.need, f) == [], (info, f)
    assert info['splits'] == sum(info['count']) == len(P.ranges(c, info)) and info['gate'] == 0 and info['thin_ns'] == 0
    assert info['stage_pixels'] == (64 if c.arith == 'bf16' else 32) and info['mchunk'] % info['stage_pixels'] == 0
    assert info['ntiles'] == -(-c.lddz // 128) if c.kind == 'split' else info['ntiles'] == -(-c.Cout // 128)
    assert info['jtiles'] == -(-c.k * c.k * c.Cin // 128)
    # every case is a multi-range plan: more than one range on some level, and a range that starts past pixel 0
    assert max(info['count']) > 1 and any(m0 > 0 for _, m0, _ in P.ranges(c, info))
    if c.layout == 'image':
        hw = c.sizes[0][0] * c.sizes[0][1]
        q = f['q']
        assert info['count'] == [c.B * q] and info['mchunk'] * q == hw and not f['cross']
        for s, (_, m0, m1) in enumerate(P.ranges(c, info)):                 # slab s = image s // q, pixels (s % q) hw / q ...
            assert (m0, m1) == ((s // q) * hw + (s % q) * hw // q, (s // q) * hw + (s % q + 1) * hw // q)
    if len(c.sizes) > 1:
        assert sum(n > 1 for n in info['count'][1:]) >= 1                   # a later level (split_start > 0) with several ranges


def test_table_reaches_every_required_class():
    """Closure, read off the planner's answers; both template instances of the split-layout body (ALLR) under every form; the second
    flag window, the second round and the register-transpose launch each in some case."""
    got, allr = set(), set()
    for c in P.CASES:
        info = P.plan(c)
        for form in c.forms:
            got.add(P.reached(c, info, form))
            if c.kind == 'split':
                allr.add((info['allr'], form))
    assert got >= P.REQUIRED_CLASSES, P.REQUIRED_CLASSES - got
    assert allr == {(a, f) for a in (False, True) for f in P.SPLIT3}
    flagged = [c for c in P.CASES if 'flagged' in c.forms]
    assert any(P.plan(c)['mchunk'] // 32 > 64 for c in flagged)
    assert any(P.facts(c, P.plan(c))['rounds'] >= 2 for c in P.CASES if c.kind == 'split')
    assert any(P.facts(c, P.plan(c))['rounds'] >= 2 for c in P.CASES if c.kind == 'tiled')
    assert any(P.facts(c, P.plan(c))['midrow'] for c in P.CASES if c.kind == 'split')
    assert {c.arith for c in P.CASES if P.facts(c, P.plan(c))['midrow'] and c.kind == 'tiled'} == {'f32', 'bf16x3', 'bf16'}


def test_query_agrees_with_the_three_existing_queries():
    """splits, path and first / count against effdet_conv2d_wgrad_splits, _kernel and _seg_slabs on every case's descriptor (the one
    ops.conv2d_wgrad would launch), the workspace size the plan implies, the thin kernel and the stem (reported apart), and refusals."""
    from efficientdet.pytorch_amd import ops, _lib as L
    lib = L.require('effdet_conv2d_wgrad_plan_info')
    for c in P.CASES:
        xm, zm = P.alloc(c, 'cpu')
        kw = P.wgrad_kwargs(c)
        with P.tuned(c):
            d = ops._wgrad_desc(xm, zm, None, None, c.Cin, c.Cout, c.k, c.k, 1, kw['pad_t'], kw['pad_l'], True, kw['split'], kw['image_splits'])
            info = L.WgradPlanInfo()
            rc = int(lib.effdet_conv2d_wgrad_plan_info(C.byref(d), C.byref(info)))
            n = len(c.sizes)
            first, count = (C.c_int * n)(), (C.c_int * n)()
            assert rc == info.path == int(lib.effdet_conv2d_wgrad_kernel(C.byref(d))) == (2 if c.kind == 'split' else 0), c.name
            assert info.splits == int(lib.effdet_conv2d_wgrad_splits(C.byref(d))) == int(lib.effdet_conv2d_wgrad_seg_slabs(C.byref(d), first, count))
            assert list(info.first[:n]) == list(first) and list(info.count[:n]) == list(count) and info.nseg == n
            assert int(lib.effdet_conv2d_wgrad_workspace_bytes(C.byref(d))) == 4 * info.splits * (c.Cout * c.k * c.k * c.Cin + c.Cout)
            assert P.plan(c) == ops.conv2d_wgrad_plan_info(xm, zm, **kw)
            assert list(info.reserved) == [0, 0, 0] and list(info.first[n:]) == [0] * (L.MAX_SEG - n)
    # the thin pointwise kernel and the stem: one workgroup per slab; the stem has a path value of its own
    d = wgrad_desc(L.F32, 8, 16, 96, [(64, 64)])
    info = L.WgradPlanInfo()
    assert int(lib.effdet_conv2d_wgrad_plan_info(C.byref(d), C.byref(info))) == 1 == int(lib.effdet_conv2d_wgrad_kernel(C.byref(d)))
    assert (info.ntiles, info.jtiles, info.nfast) == (1, 1, info.splits) and info.stage_pixels in (32, 64, 128) and info.thin_ns in (2, 3)
    d = wgrad_desc(L.F32, 8, 4, 32, [(128, 128)], k=3, stride=2)
    assert int(lib.effdet_conv2d_wgrad_plan_info(C.byref(d), C.byref(info))) == 3 and int(lib.effdet_conv2d_wgrad_kernel(C.byref(d))) == 1
    assert L.WGRAD_PATHS[info.path] == 'stem' and info.stage_pixels == 64 and info.thin_ns == 3 and info.splits == int(lib.effdet_conv2d_wgrad_splits(C.byref(d)))
    # refusals: the launch's own code, the info left alone
    for d, code in ((wgrad_desc(L.F32, 2, 62, 64, [(8, 8)]), -3), (wgrad_desc(L.F32_SPLIT, 2, 48, 64, [(8, 8)], k=3, pad=1), -1),
                    (wgrad_desc(L.F32_SPLIT, 2, 64, 64, [(16, 32), (1, 2)], k=3, pad=1), -3)):
        info = L.WgradPlanInfo(path=-7, splits=-7)
        assert int(lib.effdet_conv2d_wgrad_plan_info(C.byref(d), C.byref(info))) == int(lib.effdet_conv2d_wgrad_kernel(C.byref(d))) == code
        assert info.path == -7 and info.splits == -7
    d = wgrad_desc(L.F32, 2, 64, 64, [(8, 8)])
    assert int(lib.effdet_conv2d_wgrad_plan_info(C.byref(d), None)) == -1 and int(lib.effdet_conv2d_wgrad_plan_info(None, C.byref(info))) == -1
    x = ops.Map.new(2, 8, 8, 62, torch.float32, 'cpu')
    with pytest.raises(RuntimeError):
        ops.conv2d_wgrad_plan_info(x, ops.Map.new(2, 8, 8, 64, torch.float32, 'cpu'), Cin=62, Cout=64, KH=1, KW=1)


# ----------------------------------------------------------------------------- the paired launch's block map
def _pair_grids():
    """(tiles, ntiles, splits a, splits b) of the paired cases, and grids that are no multiple of 8 in either problem or in the sum"""
    out = []
    for c in P.CASES:
        if 'pair-flagged' in c.forms:
            info = P.plan(c)
            out.append((info['ntiles'] * info['jtiles'], info['ntiles'], info['splits'], info['splits']))
    return out + [(3, 1, 5, 5), (5, 5, 3, 7), (1, 1, 1, 1), (1, 1, 2, 9), (36, 2, 7, 3), (7, 1, 13, 11), (2, 2, 1, 6)]


@pytest.mark.parametrize('first', [0, 1])
@pytest.mark.parametrize('liveb', [False, True])
def test_pair_block_map_is_a_bijection(first, liveb):
    """conv_wgrad_pair_kernel's block -> (problem, tile, split) map, restated in wgrad_plan_cases.pair_block: onto both problems' blocks,
    each exactly once; every XCD takes xcd_remap's eighth of problem `first`, then a contiguous run of the other one; the dense problems run
    tile-fastest in the single launch's order, the flagged one split-fastest with its splits descending."""
    grids = _pair_grids()
    assert len(grids) >= 3 + 7 and any((t * (a + b)) % 8 for t, _, a, b in grids) and any((t * a) % 8 == 0 and (t * a) > 8 for t, _, a, _ in grids)
    for tiles, ntiles, sa, sb in grids:
        splits, grid = (sa, sb), tiles * (sa + sb)
        got = [P.pair_block(bid, tiles, ntiles, splits, first, liveb) for bid in range(grid)]
        want = sorted((p, t % ntiles, t // ntiles, s) for p in (0, 1) for s in range(splits[p]) for t in range(tiles))
        assert sorted(got) == want, (tiles, ntiles, sa, sb)
        for xcd in range(8):
            mine = got[xcd::8]
            probs = [p for p, _, _, _ in mine]
            assert probs == sorted(probs, reverse=bool(first)), (xcd, probs)          # problem `first` first, then the other
            for prob in (0, 1):
                logical = [(s, jt * ntiles + nt) for p, nt, jt, s in mine if p == prob]
                n, nfirst = tiles * splits[prob], tiles * splits[first]
                if prob == first:
                    lo, hi = P.eighth(n, xcd), P.eighth(n, xcd + 1)
                else:                                  # what the XCD's share of the whole grid leaves behind its share of problem `first`
                    lo, hi = P.eighth(grid, xcd) - P.eighth(nfirst, xcd), P.eighth(grid, xcd + 1) - P.eighth(nfirst, xcd + 1)
                assert len(logical) == hi - lo and 0 <= lo <= hi <= n
                if liveb and prob == 1:
                    assert logical == [(splits[1] - 1 - l % splits[1], l // splits[1]) for l in range(lo, hi)]
                else:
                    assert logical == [(l // tiles, l % tiles) for l in range(lo, hi)]
                    if prob == first:                  # ... the order the problem's own launch gives that XCD (common.h xcd_remap)
                        assert [s * tiles + t for s, t in logical] == [xcd_remap(b, n) for b in range(xcd, n, 8)]
            assert len(mine) == P.eighth(grid, xcd + 1) - P.eighth(grid, xcd)


# ----------------------------------------------------------------------------- the flagged cases' patterns
@pytest.mark.parametrize('c', [c for c in P.CASES if 'flagged' in c.forms], ids=P.case_id)
def test_flag_patterns_take_every_branch_of_the_flag_walk(c):
    info = P.plan(c)
    steps, masks = P.live_steps(c, info), P.live_pixel_masks(c, info)
    flags = P.step_flags(masks)
    per, o = info['mchunk'] // 32, 0
    by_range, nsteps = {}, {}
    for l, M in enumerate(P.level_pixels(c)):
        n = -(-M // 32)
        assert flags[o:o + n].nonzero().flatten().tolist() == steps[l] and int(masks[l].sum()) == len(steps[l])      # one pixel per live step
        for r in range(info['count'][l]):
            by_range[(l, r)] = [s - r * per for s in steps[l] if r * per <= s < (r + 1) * per]
            nsteps[(l, r)] = min(per, n - r * per)
        o += n
    assert flags.numel() == o
    last0 = (0, info['count'][0] - 1)
    assert by_range[(0, 0)][0] == 0 and by_range[(0, 0)][-1] == per - 1                    # first and last step of a whole range
    assert by_range[(0, 1)] and min(by_range[(0, 1)]) > 0                                   # a walk that starts with a seek
    assert nsteps[last0] < per and by_range[last0] == [nsteps[last0] - 1]                   # the short last range: its last step only
    assert any(len(v) == nsteps[k] for k, v in by_range.items())                            # a range walked like the dense one
    assert any(k[0] > 0 and 0 < len(v) < nsteps[k] for k, v in by_range.items())            # a sparse range of a later level
    if info['count'][0] >= 5:
        assert by_range[(0, 2)] == [] and len(by_range[(0, 3)]) == per                      # no live step: the zero-slab branch
    if c.name == 's-long':
        assert per == 84 and by_range[(0, 0)] == [0, 63, 64, 65, 83]                       # both sides of the 64-step flag window
        assert by_range[(0, 1)] == [70]                                                    # dead in steps 0-63, live only beyond
        assert by_range[(0, 2)] == [] and by_range[(0, 9)] == [11]


# ----------------------------------------------------------------------------- the reference and the bounds
@pytest.mark.parametrize('k', [1, 3])
def test_range_reference_matches_nested_loops(k):
    """range_refs against loops over every pixel, tap and channel at a tiny shape: the whole level, a range that crosses an image
    boundary, one that starts inside a row and ends inside another, one pixel, and ranges that tile the level (their sum = the whole)."""
    g = torch.Generator().manual_seed(5 + k)
    B, H, W, Cin, Cout = 3, 3, 4, 2, 3
    x = torch.randn(B, H, W, Cin, generator=g, dtype=torch.float64)
    dz = torch.randn(B, H, W, Cout, generator=g, dtype=torch.float64)
    M = B * H * W
    rngs = [(0, M), (7, 17), (5, 10), (13, 14), (0, 5), (5, 29), (29, M)]
    assert 7 // (H * W) != 16 // (H * W) and 5 % W != 0 and 10 % W != 0
    G, S, bias, Sb = P.range_refs(x, dz, k, rngs)
    assert G.shape == S.shape == (len(rngs), Cout, k * k, Cin) and bias.shape == Sb.shape == (len(rngs), Cout)
    for i, (m0, m1) in enumerate(rngs):
        wG, wS, wb, wSb = P.naive_range(x, dz, k, m0, m1)
        for got, want in ((G[i], wG), (S[i], wS), (bias[i], wb), (Sb[i], wSb)):
            assert float((got - want).abs().max()) <= 1e-13 * max(float(want.abs().max()), 1.0), (k, m0, m1)
    assert float((G[4] + G[5] + G[6] - G[0]).abs().max()) <= 1e-12 and bool((S >= G.abs() - 1e-13).all()) and bool((Sb >= bias.abs() - 1e-13).all())
    # the whole level is the weight gradient autograd gives
    w = torch.zeros(Cout, Cin, k, k, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(Cout, dtype=torch.float64, requires_grad=True)
    (torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), w, b, padding=(k - 1) // 2) * dz.permute(0, 3, 1, 2)).sum().backward()
    assert float((G[0].view(Cout, k, k, Cin).permute(0, 3, 1, 2) - w.grad).abs().max()) <= 1e-12
    assert float((bias[0] - b.grad).abs().max()) <= 1e-12


def test_bounds_and_stored_values():
    S = torch.tensor([2.0], dtype=torch.float64)
    base = lambda n: 2.0 * (n + 3) * 2.0 ** -24 * 2.0
    assert float(P.sum_bound(BY_NAME['t-long-f32'], 2688, S)) == base(2688)
    assert float(P.sum_bound(BY_NAME['t-long-bf16'], 2688, S)) == base(2688)                  # exact products: nothing added
    assert float(P.sum_bound(BY_NAME['t-long-bf16x3'], 384, S)) == base(384) + 2.0 ** -14 * 2.0
    assert float(P.sum_bound(BY_NAME['s-long'], 384, S)) == base(384) + 2.0 ** -14 * 2.0
    assert float(P.sum_bound(BY_NAME['s-long'], 5, torch.zeros(1, dtype=torch.float64))) == 0.0
    hi, lo = torch.randn(2, 3, 64).bfloat16(), (torch.randn(2, 3, 64) * 2.0 ** -9).bfloat16()
    t = torch.stack([hi.view(2, 3, 2, 32), lo.view(2, 3, 2, 32)], dim=3).reshape(2, 3, 128).contiguous().view(torch.float32)
    assert torch.equal(P.stored64(BY_NAME['s-long'], t), hi.double() + lo.double())
    v = torch.randn(4, 8).bfloat16()
    assert torch.equal(P.stored64(BY_NAME['t-long-bf16'], v), v.double())
