"""The planner's side of the row-slab staging (csrc/conv_igemm.hip, TUNE_ROWSLAB), asked through effdet_conv2d_plan_info without a device:
an eligible launch reserves the larger activation buffers -- the largest slab among its segments, rounded up to whole 8-entry DMA
pieces -- and the present 128-row buffers with the knob off, or where no segment stages a slab."""
import torch


def _lds(sizes, Cout, on, **kw):
    from efficientdet.pytorch_amd import ops, functional as Fn, _lib as L
    B, Cin = 2, 64
    _, xm = Fn.pyramid_alloc(B, sizes, Cin, torch.float32, 'cpu')
    _, ym = Fn.pyramid_alloc(B, sizes, Cout, torch.float32, 'cpu')
    old = ops.tuning_set(L.TUNE_ROWSLAB, on)
    try:
        i = ops.conv2d_plan_info(xm, torch.empty(Cout * 9 * Cin + Cout), ym, Cin=Cin, Cout=Cout, KH=3, KW=3, pad_t=1, pad_l=1, **kw)
    finally:
        ops.tuning_set(L.TUNE_ROWSLAB, old)
    assert i['stages'] == 2 and i['tile_m'] == 128 and i['kord'] == 1 and not i['persistent']
    return i['tile_n'], i['lds_bytes']


def test_plan_reports_the_slab_buffers():
    from efficientdet.pytorch_amd import ops, _lib as L
    h = dict(hsplit=True)
    s = dict(split=True)
    for kw in (h, s):
        # 128-wide tile: weights 2 x 16 KiB; slabs of 132 (136 as DMA pieces) / 136 / 144 / 160 entries of 128 bytes, two buffers
        assert _lds([(4, 64)], 128, 1, **kw) == (128, 2 * (136 + 128) * 128)
        assert _lds([(8, 32)], 128, 1, **kw) == (128, 2 * (136 + 128) * 128)
        assert _lds([(8, 16)], 128, 1, **kw) == (128, 2 * (144 + 128) * 128)
        assert _lds([(8, 8)], 128, 1, **kw) == (128, 2 * (160 + 128) * 128)
        assert _lds([(4, 64), (4, 16), (8, 8), (4, 4)], 128, 1, **kw) == (128, 73728)         # the launch takes its largest segment's
        assert 73728 <= 80 * 1024                                                            # two workgroups per CU
        # ... and the present value with the knob off, for widths without a slab (4; 12 does not divide 128) and under the tap-major walk
        assert _lds([(4, 64), (8, 8)], 128, 0, **kw) == (128, 65536)
        assert _lds([(4, 4)], 128, 1, **kw) == (128, 65536)
        assert _lds([(12, 12)], 128, 1, **kw) == (128, 65536)
        old = ops.tuning_set(L.TUNE_SPLIT_KORD, 0)
        try:
            from efficientdet.pytorch_amd import functional as Fn
            _, xm = Fn.pyramid_alloc(2, [(8, 16)], 64, torch.float32, 'cpu')
            _, ym = Fn.pyramid_alloc(2, [(8, 16)], 128, torch.float32, 'cpu')
            i = ops.conv2d_plan_info(xm, torch.empty(128 * 9 * 64 + 128), ym, Cin=64, Cout=128, KH=3, KW=3, pad_t=1, pad_l=1, **kw)
            assert i['kord'] == 0 and i['lds_bytes'] == 65536
        finally:
            ops.tuning_set(L.TUNE_SPLIT_KORD, old)
        # 64-wide tile: slabs up to 144 entries (52 KiB: three workgroups per CU, as with 48); W = 8 stays per tap
        assert _lds([(8, 16)], 64, 1, **kw) == (64, 2 * (144 + 64) * 128)
        assert _lds([(8, 16), (8, 8)], 64, 1, **kw) == (64, 2 * (144 + 64) * 128)
        assert _lds([(8, 8)], 64, 1, **kw) == (64, 49152)
        assert _lds([(8, 16)], 64, 0, **kw) == (64, 49152)
        assert 3 * 2 * (144 + 64) * 128 <= 160 * 1024


def test_knob_is_a_tuning_index_of_its_own():
    from efficientdet.pytorch_amd import ops, _lib as L
    assert L.TUNE_ROWSLAB == 5
    old = ops.tuning_set(L.TUNE_ROWSLAB, 0)
    assert old in (0, 1, -1) and ops.tuning_set(L.TUNE_ROWSLAB, old) == 0
    assert ops.tuning_set(L.TUNE_ROWSLAB + 1, 0) == -1               # EFFDET_EINVAL: the last index
