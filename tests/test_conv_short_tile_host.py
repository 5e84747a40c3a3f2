"""The planner's side of the short pixel tile (csrc/conv_igemm.hip, TUNE_SHORT_TILE), asked through effdet_conv2d_plan_info without a
device: the benchmark's small-map descriptors take 32-pixel tiles with the knob on and the 128-pixel plans with it off, the plans other
host tests pin stay what they are under both settings, and the knob is a tuning index of its own."""
import pytest
import torch

from tests import conv_plan_cases as P

CU_LDS = 160 * 1024
# (name, B, H = W, Cin, Cout, k, the 128-pixel plan: tile_n, stages; the short plan's stages)
SMALL_MAPS = [
    ('bifpn 3x3 64->64 @4', 32, 4, 64, 64, 3, 32, 4, 8),
    ('bifpn 3x3 64->64 @8', 32, 8, 64, 64, 3, 32, 4, 8),
    ('bifpn 3x3 64->64 @16', 32, 16, 64, 64, 3, 32, 4, 8),
    ('project 1x1 672->192 @8', 32, 8, 672, 192, 1, 32, 4, 8),
    ('project 1x1 1152->192 @8', 32, 8, 1152, 192, 1, 32, 4, 8),
]


class short_tile:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from efficientdet.pytorch_amd import ops, _lib as L
        self.old = ops.tuning_set(L.TUNE_SHORT_TILE, self.on)

    def __exit__(self, *a):
        from efficientdet.pytorch_amd import ops, _lib as L
        ops.tuning_set(L.TUNE_SHORT_TILE, self.old)
        return False


def _plan(B, hw, Cin, Cout, k, arith):
    from efficientdet.pytorch_amd import ops
    from efficientdet.pytorch_amd.ops import Map
    x, y = Map.new(B, hw, hw, Cin, torch.float32, 'cpu'), Map.new(B, hw, hw, Cout, torch.float32, 'cpu')
    old = ops.set_f32_arith(arith)
    try:
        return ops.conv2d_plan_info(x, torch.empty(Cout * k * k * Cin), y, Cin=Cin, Cout=Cout, KH=k, KW=k, pad_t=k // 2, pad_l=k // 2)
    finally:
        ops.set_f32_arith(old)


@pytest.mark.parametrize('arith', ['f32', 'bf16x3'])
@pytest.mark.parametrize('case', SMALL_MAPS, ids=[c[0] for c in SMALL_MAPS])
def test_small_map_descriptors_take_the_short_tile(case, arith):
    _, B, hw, Cin, Cout, k, tn, ns, short_ns = case
    M = B * hw * hw
    with short_tile(1):
        i = _plan(B, hw, Cin, Cout, k, arith)
    assert i['form'] == ('plain' if arith == 'f32' else 'bf16x3') and i['id'] == (0 if Cout > 64 else 1) + (4 if arith == 'bf16x3' else 0)
    assert i['tile_m'] == 32 < 128 and i['tile_n'] == 32 and i['stages'] == short_ns and i['threads'] == 256
    assert i['lds_bytes'] == short_ns * (32 + 32) * 128 <= CU_LDS
    assert i['mtiles'] == -(-M // i['tile_m']) and i['ntiles'] == -(-Cout // i['tile_n']) and i['grid'] == i['mtiles'] * i['ntiles']
    assert i['ksteps'] == -(-(k * k * Cin // 4) // 8)
    # two workgroups per CU, and never more than one round of them
    assert 2 * i['lds_bytes'] <= CU_LDS and i['grid'] <= 2 * P.MI355X_CUS
    with short_tile(0):
        o = _plan(B, hw, Cin, Cout, k, arith)
    assert (o['id'], o['form'], o['ksteps'], o['kord']) == (i['id'], i['form'], i['ksteps'], i['kord'])
    assert (o['tile_m'], o['tile_n'], o['stages'], o['threads']) == (128, tn, ns, 256)
    assert o['lds_bytes'] == ns * (128 + tn) * 128 and o['mtiles'] == -(-M // 128) and o['grid'] == o['mtiles'] * o['ntiles']
    # what the rule is keyed on: the narrow plan leaves most of the 256 CUs idle (up to half of them where it is two channel tiles wide)
    assert o['grid'] <= 96 or (Cout <= 64 and o['grid'] <= 128)


@pytest.mark.parametrize('on', [0, 1])
def test_pinned_plans_are_unchanged_under_both_settings(on):
    from efficientdet.pytorch_amd import ops
    from efficientdet.pytorch_amd.ops import Map
    with short_tile(on):
        seen = {}
        for B, hw in ((2, 92), (1, 92), (1, 40)):                          # 266, 134 and 26 tiles of 128 x 128 (26: 104 narrow workgroups)
            x, y = Map.new(B, hw, hw, 64, torch.float32, 'cpu'), Map.new(B, hw, hw, 256, torch.float32, 'cpu')
            i = ops.conv2d_plan_info(x, torch.empty(256 * 9 * 64), y, Cin=64, Cout=256, KH=3, KW=3, pad_t=1, pad_l=1)
            seen[(i['tile_m'], i['tile_n'], i['stages'])] = i['id']
            assert i['lds_bytes'] == i['stages'] * (128 + i['tile_n']) * 128
        assert seen == {(128, 128, 2): 0, (128, 128, 4): 0, (128, 32, 4): 0}
        for c in P.CASES:
            info = P.plan(c)
            assert P.reached(c, info) == c.expect and info['tile_m'] in (128, 256), (c.name, info)
        # outside the rule: bf16 storage, a short K loop, a per-image-weights launch, the operand-gate form
        x, y = Map.new(32, 8, 8, 64, torch.bfloat16, 'cpu'), Map.new(32, 8, 8, 64, torch.bfloat16, 'cpu')
        assert ops.conv2d_plan_info(x, torch.empty(64 * 9 * 64, dtype=torch.bfloat16), y, Cin=64, Cout=64, KH=3, KW=3, pad_t=1, pad_l=1)['tile_m'] == 128
        x, y = Map.new(32, 8, 8, 112, torch.float32, 'cpu'), Map.new(32, 8, 8, 192, torch.float32, 'cpu')
        assert ops.conv2d_plan_info(x, torch.empty(192 * 112), y, Cin=112, Cout=192, KH=1, KW=1)['tile_m'] == 128
        x, y = Map.new(2, 16, 16, 672, torch.float32, 'cpu'), Map.new(2, 16, 16, 192, torch.float32, 'cpu')
        assert ops.conv2d_plan_info(x, torch.empty(2 * 192 * 672), y, Cin=672, Cout=192, KH=1, KW=1, w_image_stride=192 * 672 * 4)['tile_m'] == 128
        g = ops.conv2d_gated_plan_info(x, torch.empty(192 * 672), y, torch.empty(2, 672), Cin=672, Cout=192, KH=1, KW=1)
        assert g is not None and g['gate'] == 1 and g['tile_m'] == 128


def test_knob_returns_the_previous_value():
    from efficientdet.pytorch_amd import ops, _lib as L
    assert L.TUNE_SHORT_TILE == 7 and L.ABI_VERSION == 11
    assert ops.tuning_set(6, 0) == -1                                      # the index in front of it is no key: EFFDET_EINVAL as before
    first = ops.tuning_set(L.TUNE_SHORT_TILE, 0)
    try:
        assert first in (0, 1)
        assert ops.tuning_set(L.TUNE_SHORT_TILE, 1) == 0 and ops.tuning_set(L.TUNE_SHORT_TILE, 0) == 1
    finally:
        ops.tuning_set(L.TUNE_SHORT_TILE, first)
    assert ops.tuning_set(L.TUNE_SHORT_TILE, first) == first
    assert ops.tuning_set(L.TUNE_SHORT_TILE + 1, 0) == -1                  # EFFDET_EINVAL: the last index
