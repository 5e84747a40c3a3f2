"""CPU tier of the multi-tile depthwise tests: the case table of tests/dwconv_cases.py reaches the kernel paths it is tagged with
(asked of the library's planner through effdet_dwconv_plan_info, no device work), covers every class the benchmark geometries take,
and its float64 reference is a depthwise conv."""
import os
import re

import pytest
import torch

from tests import dwconv_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ('fwd', 'dgrad', 'wgrad', 'bwd', 'expand_fwd')


def test_plan_query_binding_matches_its_header():
    """_lib.PLAN_SIGNATURES and the EFFDET_DW_* numbers against include/effdet_dwconv_plan.h, parsed as tests/test_abi.py parses
    effdet_hip.h; a pure addition: the ABI generation stays where it was."""
    from efficientdet.pytorch_amd import _lib as L
    h = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'effdet_dwconv_plan.h')).read(), flags=re.S)
    protos = re.findall(r'^([a-z][a-z ]*?\*?)\s*\b(effdet_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', h, flags=re.M)
    assert [n for _, n, _ in protos] == list(L.PLAN_SIGNATURES) == ['effdet_dwconv_plan_info']
    r, name, params = protos[0]
    kinds = ''.join('p' if '*' in p else {'int': 'i'}[' '.join(p.split()).rsplit(' ', 1)[0]] for p in params.split(','))
    assert L.PLAN_SIGNATURES[name] == 'i:' + kinds and r.strip() == 'int'
    enums = {k: int(v) for k, v in re.findall(r'(EFFDET_DW_[A-Z_]+)\s*=\s*(\d+)', h)}
    assert [enums['EFFDET_DW_PLAN_' + n] for n in ('FWD', 'DGRAD', 'WGRAD', 'BWD', 'EXPAND_FWD')] == \
        [L.DW_PLAN_FWD, L.DW_PLAN_DGRAD, L.DW_PLAN_WGRAD, L.DW_PLAN_BWD, L.DW_PLAN_EXPAND_FWD]
    assert [enums['EFFDET_DW_INFO_' + n.upper()] for n in L.DW_INFO] == list(range(len(L.DW_INFO)))
    assert enums['EFFDET_DW_INFO_COUNT'] == len(L.DW_INFO)
    f = L.require('effdet_dwconv_plan_info').effdet_dwconv_plan_info
    assert f.restype is L._CTYPE['i'] and list(f.argtypes) == [L._CTYPE[c] for c in L.PLAN_SIGNATURES[name][2:]]
    assert L.ABI_VERSION == 11


def test_plan_query_agrees_with_the_other_host_queries_and_refuses_what_the_entry_points_refuse():
    """The query reads the plan the launches read: its groups are effdet_dwconv_fwd_pool_groups / _expand_dw_pool_groups, its groups x
    B the slab rows of the workspace queries; the codes are the entry points' (tests/test_host_logic.py pins those)."""
    import ctypes as C
    from efficientdet.pytorch_amd import _lib as L, ops
    lib = L.lib()
    for c in D.RUN_CASES:
        geo = D.geometry(c)
        H, W, Cc, k, s, pt, pl, Ho, Wo = geo
        assert D.plan('fwd', c)['groups'] == int(lib.effdet_dwconv_fwd_pool_groups(L.dtype_code(c.dtype), c.B, Cc, s, Ho, Wo))
        assert c.B * D.plan('wgrad', c)['groups'] * (k * k + 1) * Cc * 4 == \
            int(lib.effdet_dwconv_wgrad_workspace_bytes(L.dtype_code(c.dtype), c.B, *geo))
    for c in D.BWD_CASES:
        geo = D.geometry(c)
        assert c.B * D.plan('bwd', c)['groups'] * (c.k * c.k + 1) * c.C * 4 == int(lib.effdet_dwconv_bwd_workspace_bytes(L.F32, c.B, *geo))
    for c in D.EXPAND_CASES:
        _, _, Cexp, _, s, _, _, Ho, Wo = D.geometry(c)
        assert D.plan('expand_fwd', c)['groups'] == int(lib.effdet_mbconv_expand_dw_pool_groups(c.B, Cexp, s, Ho, Wo))
    # the D0 pin of test_depthwise_planning_entry_points: 512 tiles per image, 64 groups -> 8 tiles per workgroup
    i = ops.dwconv_plan_info('fwd', torch.float32, 32, 256, 256, 32, 3, 1, 1, 1, 256, 256)
    assert (i['tpi'], i['groups'], i['ppt'], i['nbuf'], i['cq'], i['nslab'], i['direct']) == (512, 64, 8, 2, 8, 1, 0)
    i = ops.dwconv_plan_info('wgrad', torch.float32, 32, 8, 8, 1152, 3, 2, 0, 0, 4, 4)
    assert i['direct'] == 1 and i['cq'] == 0 and i['nbuf'] == 0
    info = (C.c_int * 7)(*([-7] * 7))
    q = lambda kind, dt, *a: int(lib.effdet_dwconv_plan_info(kind, dt, *a, info))
    g = (32, 64, 64, 240, 3, 1, 1, 1, 64, 64)
    assert q(L.DW_PLAN_FWD, L.F32, *g, 0) == 0 and info[2] >= 1
    info[2] = -7
    assert q(5, L.F32, *g, 0) == -1 and q(L.DW_PLAN_FWD, 7, *g, 0) == -1                    # kind, dtype: EFFDET_EINVAL
    assert q(L.DW_PLAN_DGRAD, L.F32, 32, 64, 64, 240, 7, 1, 3, 3, 64, 64, 0) == -3          # k = 7: EFFDET_EUNSUPPORTED
    assert q(L.DW_PLAN_WGRAD, L.BF16, 32, 64, 64, 36, 3, 1, 1, 1, 64, 64, 0) == -3          # C % 8
    assert q(L.DW_PLAN_BWD, L.BF16, *g, 0) == -3                                            # fused backward: fp32 only
    assert q(L.DW_PLAN_EXPAND_FWD, L.F32, 32, 64, 64, 288, 3, 1, 1, 1, 64, 64, 48) == -3    # Cin
    assert int(lib.effdet_dwconv_plan_info(L.DW_PLAN_FWD, L.F32, *g, 0, None)) == -1
    assert info[2] == -7                                                                    # written only on EFFDET_OK
    assert ops.dwconv_plan_info('bwd', torch.bfloat16, *g) is None


@pytest.mark.parametrize('c', D.RUN_CASES, ids=D.case_id)
def test_run_case_reaches_the_class_it_is_tagged_with(c):
    for fam in D.FAMILIES:
        assert D.reached(D.plan(fam, c)) == c.expect[fam], (fam, D.plan(fam, c))
        assert D.plan(fam, c)['groups'] < D.plan(fam, c)['tpi']
        # the bitwise checks compare with one image launched alone: that launch is the single-tile path
        assert D.plan(fam, c, B=1)['ppt'] == 1, fam
    assert D.plan('wgrad', c)['direct'] == 0


@pytest.mark.parametrize('c', D.SINGLE_TILE_CASES, ids=D.case_id)
def test_single_tile_case_reaches_the_class_it_is_tagged_with(c):
    for fam in D.FAMILIES:
        assert D.reached(D.plan(fam, c)) == c.expect[fam] and D.plan(fam, c)['direct'] == 0, (fam, D.plan(fam, c))


@pytest.mark.parametrize('c', D.BWD_CASES, ids=D.case_id)
def test_fused_backward_case_reaches_the_class_it_is_tagged_with(c):
    info = D.plan('bwd', c)
    assert info is not None and D.reached(info) == c.expect, info
    assert info['groups'] < info['tpi']


@pytest.mark.parametrize('c', D.EXPAND_CASES, ids=D.case_id)
def test_fused_expand_case_reaches_the_class_it_is_tagged_with(c):
    info = D.plan('expand_fwd', c)
    assert D.reached(info) == c.expect and info['groups'] < info['tpi'], info
    assert D.plan('expand_fwd', c, B=1)['ppt'] == 1


def test_table_holds_every_instance_and_every_edge_the_runs_have():
    """What the table promises as a whole, read off the planner's answers (not off the tags)."""
    seen = {fam: {} for fam in D.FAMILIES}
    for c in D.RUN_CASES:
        for fam in D.FAMILIES:
            cq, nbuf, ppt, ragged = D.reached(D.plan(fam, c))
            assert ppt >= 2
            seen[fam].setdefault((c.k, c.s, cq, c.dtype), []).append((nbuf, ppt, ragged, c.pre))
    instances = {(k, s, cq, dt) for k in (3, 5) for s in (1, 2) for cq in (4, 8) for dt in (D.F32, D.BF16)}
    for fam in D.FAMILIES:
        assert set(seen[fam]) == instances, (fam, instances ^ set(seen[fam]))
        runs = [r for v in seen[fam].values() for r in v]
        for nbuf in {r[0] for r in runs}:
            assert any(r[2] for r in runs if r[0] == nbuf), (fam, nbuf, 'no ragged last run')
        assert any(r[1] >= 3 for r in runs), fam
    # the forward restages a single buffer where two tiles pass 80 KiB: k5 / stride 2 at 8-chunk slabs, and bf16 k3 / stride 2
    one = {key for key, v in seen['fwd'].items() if any(r[0] == 1 for r in v)}
    assert one == {(5, 2, 8, D.F32), (5, 2, 8, D.BF16), (3, 2, 8, D.BF16)}
    assert {r[0] for v in seen['dgrad'].values() for r in v} == {2} and {r[0] for v in seen['wgrad'].values() for r in v} == {1}
    # in_act = SWISH runs on both forward buffer schemes
    assert {r[0] for v in seen['fwd'].values() for r in v if r[3]} == {1, 2}
    # partial edge tiles in both directions (forward 16 x 8 / 8 x 8 outputs, data gradient 16 x 8 / 16 x 16 inputs), asymmetric pads at stride 2
    for c in D.RUN_CASES:
        _, _, _, k, s, pt, pl, Ho, Wo = D.geometry(c)
        assert Ho % (16 if s == 1 else 8) and Wo % 8 and c.H % 16 and c.W % (8 if s == 1 else 16)
        if s == 2:
            assert (pt, pl) == ((0, 0) if k == 3 else (1, 1)) and D.tf_same(c.H, k, s)[1] == pt + 1
    bwd = {(c.k, c.s, D.plan('bwd', c)['cq']) for c in D.BWD_CASES}
    assert bwd == {(k, s, cq) for k in (3, 5) for s in (1, 2) for cq in (4, 8)}
    assert all(D.plan('bwd', c)['ppt'] >= 2 for c in D.BWD_CASES) and any(D.plan('bwd', c)['ppt'] >= 3 for c in D.BWD_CASES)
    assert {D.plan('bwd', c)['nbuf'] for c in D.BWD_CASES} == {2}
    assert sorted((c.k, c.s) for c in D.EXPAND_CASES) == [(3, 1), (3, 2), (5, 1), (5, 2)]
    assert sorted(c.Cin for c in D.EXPAND_CASES) == [16, 24, 32, 40]
    # operands stay at or below ~110 MB
    for c in D.RUN_CASES:
        assert c.B * c.H * c.W * c.C * (4 if c.dtype == D.F32 else 2) <= 110e6, D.case_id(c)


def _existing_tables():
    """The case tables of tests/test_gpu_backbone_ops.py, read from their parametrize marks."""
    from tests import test_gpu_backbone_ops as T

    def cfgs(fn):
        return [m.args[1] for m in fn.pytestmark if m.name == 'parametrize' and m.args[0] == 'cfg'][0]
    return cfgs(T.test_dwconv_fwd_bwd), cfgs(T.test_dwconv_fused_data_and_weight_gradient), cfgs(T.test_fused_expand_depthwise_forward)


def _plan_cfg(kind, dtype, cfg, expand=False):
    """Plan of a cfg of the existing tables, which pass their low pad for both directions and take Ho, Wo from the padded conv."""
    from efficientdet.pytorch_amd import ops
    from efficientdet.pytorch_amd.config import conv_out
    B, H, W, Cc, k, s, pad = cfg
    return ops.dwconv_plan_info(kind, dtype, B, H, W, 6 * Cc if expand else Cc, k, s, pad[0], pad[0], conv_out(H, k, s, pad), conv_out(W, k, s, pad),
                                Cin=Cc if expand else 0)


def test_existing_op_level_tables_keep_the_single_tile_paths():
    """The split of responsibilities: tests/test_gpu_backbone_ops.py runs every family at one tile per workgroup (small, odd, tiny
    maps; the direct weight-gradient kernel), the table here at runs of tiles.  One fused-backward case plans 2 tiles with an even
    tile count (no ragged run)."""
    plain, bwd, expand = _existing_tables()
    for cfg in plain:
        for dt in (D.F32, D.BF16):
            for fam in D.FAMILIES:
                assert _plan_cfg(fam, dt, cfg)['ppt'] == 1 or _plan_cfg(fam, dt, cfg)['direct'], (fam, cfg)
    multi = {}
    for cfg in bwd:
        info = _plan_cfg('bwd', D.F32, cfg)
        if info is not None and info['ppt'] != 1:
            multi[cfg] = (info['ppt'], info['tpi'] % info['ppt'])
        assert all(_plan_cfg(fam, D.F32, cfg)['ppt'] == 1 for fam in ('dgrad', 'wgrad')), cfg
    assert multi == {(4, 128, 128, 32, 3, 1, (1, 1)): (2, 0)}
    for cfg in expand:
        assert _plan_cfg('expand_fwd', D.F32, cfg, expand=True)['ppt'] == 1, cfg


def test_every_class_a_benchmark_geometry_takes_is_taken_by_a_case():
    """Closure: plan every depthwise geometry of the BASELINE.json configs in every family; each (family, dtype, k, stride, CQ, nbuf,
    ppt > 1, direct) class that comes out must be the class of some op-level case -- a multi-tile class of a case of the table here,
    a single-tile class of a case of either this table or the existing ones."""
    from efficientdet.pytorch_amd import ops
    configs = D.benchmark_configs()
    assert {(b, n, s) for b, n, s, _ in configs} == {('efficientnet-b0', 32, 512), ('efficientnet-b4', 8, 1024)}
    bench = {}
    for (dt, B, H, W, Cexp, k, s, pt, pl, Ho, Wo, Cin) in D.benchmark_geometries():
        for kind in KINDS:
            if kind == 'expand_fwd' and (Cin == 0 or dt != D.F32):
                continue
            info = ops.dwconv_plan_info(kind, dt, B, H, W, Cexp, k, s, pt, pl, Ho, Wo, Cin=Cin)
            if info is not None:                  # (None: the fused backward / fused expand does not serve it, the model takes the plain kernels)
                bench.setdefault(D.plan_class(kind, dt, k, s, info), (B, H, W, Cexp))
    for kind in KINDS:
        assert any(c[0] == kind and c[6] for c in bench), kind            # every family does run multi-tile in the benchmark
    table = set()
    for c in D.RUN_CASES:
        table |= {D.plan_class(fam, c.dtype, c.k, c.s, D.plan(fam, c)) for fam in D.FAMILIES}
    table |= {D.plan_class('bwd', D.F32, c.k, c.s, D.plan('bwd', c)) for c in D.BWD_CASES}
    table |= {D.plan_class('expand_fwd', D.F32, c.k, c.s, D.plan('expand_fwd', c)) for c in D.EXPAND_CASES}
    single = set(table)
    for c in D.SINGLE_TILE_CASES:
        single |= {D.plan_class(fam, c.dtype, c.k, c.s, D.plan(fam, c)) for fam in D.FAMILIES}
    plain, bwd, expand = _existing_tables()
    for cfg in plain:
        single |= {D.plan_class(fam, dt, cfg[4], cfg[5], _plan_cfg(fam, dt, cfg)) for fam in D.FAMILIES for dt in (D.F32, D.BF16)}
    for cfg in bwd:
        if _plan_cfg('bwd', D.F32, cfg) is not None:
            single.add(D.plan_class('bwd', D.F32, cfg[4], cfg[5], _plan_cfg('bwd', D.F32, cfg)))
    for cfg in expand:
        single.add(D.plan_class('expand_fwd', D.F32, cfg[4], cfg[5], _plan_cfg('expand_fwd', D.F32, cfg, expand=True)))
    missing = sorted((c, g) for c, g in bench.items() if c not in (table if c[6] else single))
    assert not missing, missing


@pytest.mark.parametrize('k,s,H,W', [(3, 1, 5, 4), (3, 2, 6, 4), (3, 2, 5, 7), (5, 1, 4, 6), (5, 2, 6, 8), (5, 2, 7, 5)])
def test_float64_reference_is_a_depthwise_conv(k, s, H, W):
    """dwconv64 (F.conv2d on the explicitly padded input) and its transposed form against nested loops, one tiny shape per (k, stride,
    pad): even sizes pad 0 | 1 and 1 | 2 at stride 2, odd ones symmetrically."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(3, 1, k, k, generator=g, dtype=torch.float64)
    ref = D.naive_dwconv(x, w, k, s)
    got = D.dwconv64(x, w, k, s)
    assert got.shape == ref.shape and float((got - ref).abs().max()) <= 1e-14 * float(ref.abs().max())
    # the transposed conv used for the data gradient's bound is the autograd gradient
    dz = torch.randn(ref.shape, generator=g, dtype=torch.float64)
    xg = x.clone().requires_grad_(True)
    D.dwconv64(xg, w, k, s).backward(dz)
    tr = D.dwconv64_transposed(dz, w, k, s, H, W)
    assert tr.shape == x.shape and float((tr - xg.grad).abs().max()) <= 1e-14 * float(xg.grad.abs().max())


def test_reference_pieces_on_a_small_case():
    """D.reference on a small geometry: z, dx, g, dsum against their definitions with the naive conv; the bounds' scales dominate."""
    c = D.Case(2, 6, 8, 8, 3, 2, D.BF16, False, {})
    r = D.reference(c)
    assert float((r.x.bfloat16().float() - r.x).abs().max()) == 0.0 and float((r.dz.bfloat16().float() - r.dz).abs().max()) == 0.0
    conv = D.naive_dwconv(r.x.double(), r.w.double(), c.k, c.s)
    z = conv * r.scale.double().view(1, -1, 1, 1) + r.shift.double().view(1, -1, 1, 1)
    assert float((r.z - z).abs().max()) <= 1e-13
    for t in range(9):                                                      # g[tap][c] = sum dz * x(tap)
        e = torch.zeros(8, 1, 3, 3, dtype=torch.float64)
        e[:, 0, t // 3, t % 3] = 1.0
        assert float((r.g[t] - (D.naive_dwconv(r.x.double(), e, c.k, c.s) * r.dz.double()).sum(dim=(0, 2, 3))).abs().max()) <= 1e-12
    assert float((r.dsum - r.dz.double().sum(dim=(0, 2, 3))).abs().max()) <= 1e-12
    assert bool((r.z_abs >= r.z.abs() - 1e-15).all()) and bool((r.dx_abs >= r.dx.abs() - 1e-15).all())
    assert float((D.value_bound(c, r.z_abs, r.z) - (2 * 12 * 2.0 ** -24 * r.z_abs + 2.0 ** -8 * r.z.abs())).abs().max()) == 0.0
