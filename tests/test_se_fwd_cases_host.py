"""CPU tier of the squeeze-excite forward / streaming-helper tests: the tables of tests/se_fwd_cases.py reach every branch and loop exit
tests/test_gpu_se_fwd_ops.py is there for, read off the plain-Python restatement of the kernels' partitions (and, where the library has
a host query, off the library).  Trimming a listed G, HW or shape out of the tables fails here, before a GPU is involved."""
import torch

from tests import se_fwd_cases as S


def _pow2(n):
    return n & (n - 1) == 0


def _lengths(G, nsl):
    return [g1 - g0 for g0, g1 in S.pool_slices(G, nsl)]


# ----------------------------------------------------------------------------- pool_reduce
def test_pool_tables_hold_every_listed_size():
    assert set(S.POOL_G) >= {1, 4, 5, 16, 17, 33, 64, 65, 144} and set(S.POOL_C) == {32, 144, 672, 1152}
    assert S.NSL == {'one': 1024 // 64, 'split': 256 // 64}
    # the forms: below Cse = 8 and above 16 images the split entry point forwards to the one-workgroup kernel
    assert S.gate_form(2, S.POOL_FORMS['one']) == 'one' and S.gate_form(S.SPLIT_MAX_B, S.POOL_FORMS['split']) == 'split'
    assert S.gate_form(S.SPLIT_MAX_B + 1, S.POOL_FORMS['split']) == 'one' and S.gate_form(2, 7) == 'one' and S.gate_form(2, 8) == 'split'
    # channel rounds of 64: less than one round, a partial last round (two sizes), whole rounds
    assert min(S.POOL_C) < 64 and sum(1 for c in S.POOL_C if c > 64 and c % 64) >= 2 and any(c % 64 == 0 for c in S.POOL_C)


def test_pool_slices_are_the_ones_the_kernel_text_gives():
    assert S.pool_slices(1, 4) is None and S.pool_slices(4, 16) is None and S.pool_slices(5, 4) is not None
    # four slices (the split form)
    assert _lengths(5, 4) == [2, 2, 1, 0] and _lengths(16, 4) == [4] * 4 and _lengths(17, 4) == [5, 5, 5, 2]
    assert _lengths(28, 4) == [7] * 4 and _lengths(33, 4) == [9, 9, 9, 6] and _lengths(64, 4) == [16] * 4
    assert _lengths(65, 4) == [17, 17, 17, 14] and _lengths(144, 4) == [36] * 4
    # sixteen slices (one workgroup per image)
    assert _lengths(5, 16) == [1] * 5 + [0] * 11 and _lengths(16, 16) == [1] * 16 and _lengths(17, 16) == [2] * 8 + [1] + [0] * 7
    assert _lengths(33, 16) == [3] * 11 + [0] * 5 and _lengths(64, 16) == [4] * 16 and _lengths(65, 16) == [5] * 13 + [0] * 3
    assert _lengths(144, 16) == [9] * 16
    for nsl in S.NSL.values():
        for G in range(5, 300):
            sl = S.pool_slices(G, nsl)
            assert len(sl) == nsl and sl[0][0] == 0 and all(a[1] == b[0] for a, b in zip(sl, sl[1:])) and sl[-1][1] == G, (G, nsl)


def test_pool_table_reaches_both_branches_and_every_exit_of_the_slice_walk():
    assert {G <= 4 for G in S.POOL_G} == {True, False} and 1 in S.POOL_G and 4 in S.POOL_G and 5 in S.POOL_G
    walks = {}
    for form, nsl in S.NSL.items():
        w = set()
        for G in S.POOL_G:
            if G > 4:
                w |= {S.slice_walk(n) for n in _lengths(G, nsl)}
        walks[form] = w
        assert (0, 0) in w, (form, 'no empty slice')
        assert any(p >= 2 for p, _ in w) and any(p >= 1 and t == 0 for p, t in w) and any(p >= 1 and t for p, t in w), (form, w)
        assert any(p == 0 and t for p, t in w), (form, 'no slice that is a tail only')
    both = walks['one'] | walks['split']
    for t in (0, 1, 2, 3):
        assert any(p >= 1 and tt == t for p, tt in both), ('no tail of %d behind a 4-chain pass' % t)
    for t in (1, 2, 3):
        assert (0, t) in both, ('no slice of %d groups' % t)


def test_restated_pool_order_is_a_sum():
    g = torch.Generator().manual_seed(3)
    for G in (1, 3, 4, 5, 17, 28, 65):
        part = torch.randint(-3, 4, (G, 70), generator=g).float()
        for nsl in S.NSL.values():
            assert torch.equal(S.pool_reduce_restated(part, nsl), part.double().sum(0).float())
    # and it is an order: on values that do not add exactly, the two slice counts round differently somewhere
    part = torch.randn(144, 4096, generator=g)
    a, b = S.pool_reduce_restated(part, 4), S.pool_reduce_restated(part, 16)
    assert not torch.equal(a, b) and float((a - b).abs().max()) < 1e-4


def test_gate_cases_cover_both_forms_on_both_branches():
    assert {c[2] for c in S.GATE_CASES} == set(S.GATE_CSE) == {4, 6, 8, 48, 112} and {c[3] for c in S.GATE_CASES} == set(S.GATE_B) == {2, 17}
    assert {(c[2], c[3]) for c in S.GATE_CASES} == {(cse, b) for cse in S.GATE_CSE for b in S.GATE_B}
    assert {c[0] for c in S.GATE_CASES} >= {1, 4, 5, 16, 17, 33, 64, 65, 144} and {c[1] for c in S.GATE_CASES} == set(S.POOL_C)
    assert all(c[0] in S.POOL_G and c[1] in S.POOL_C for c in S.GATE_CASES)
    assert len(set(S.GATE_CASES)) == len(S.GATE_CASES) and 2 * len(S.GATE_CASES) <= 60           # plain + spiked: a few dozen launches
    for form, nsl in S.NSL.items():
        mine = [c for c in S.GATE_CASES if S.gate_form(c[3], c[2]) == form]
        assert any(c[0] <= 4 for c in mine) and any(c[0] == 1 for c in mine), form
        w = set()
        for c in mine:
            if c[0] > 4:
                w |= {S.slice_walk(n) for n in _lengths(c[0], nsl)}
        assert (0, 0) in w and any(p >= 2 for p, _ in w) and any(p >= 1 and t for p, t in w) and any(p >= 1 and t == 0 for p, t in w), (form, w)
        assert any(c[1] % 64 for c in mine if c[0] > 4) and any(c[1] < 64 for c in mine if c[0] > 4), form
    # the squeezed-channel loops: the one-workgroup kernel's rounds of 48 (Cse 48 fills one, 112 wraps into a third), reached at
    # Cse >= 8 only through B = 17; the split kernel's rounds of 32
    one = {c[2] for c in S.GATE_CASES if S.gate_form(c[3], c[2]) == 'one'}
    split = {c[2] for c in S.GATE_CASES if S.gate_form(c[3], c[2]) == 'split'}
    assert one == {4, 6, 8, 48, 112} and split == {8, 48, 112}
    # LDS of both launchers: (C + Cse + 1024) and max(C + 256, Cse) floats stay below the 60 000-byte refusal
    assert all(4 * (c[1] + c[2] + 1024) <= 60000 for c in S.GATE_CASES)


# ----------------------------------------------------------------------------- se_dgate
def test_dgate_cases_reach_every_slab_count_and_row_group_form():
    from efficientdet.pytorch_amd import _lib as L
    lib = L.lib()
    for hw in list(range(1, 1200)) + [1600, 4096, 65536]:
        assert S.dgate_slabs(hw) == int(lib.effdet_se_dgate_slabs(hw)), hw
    assert set(S.DGATE_HW) == {1, 16, 17, 1008, 1009, 1089, 1600} and 1089 == 33 * 33
    assert [S.dgate_slabs(hw) for hw in sorted(S.DGATE_HW)] == [1, 1, 2, 63, 64, 64, 64]
    lens = {hw: [p1 - p0 for p0, p1 in S.dgate_partition(hw, 32, S.F32)[1]] for hw in S.DGATE_HW}
    assert lens[1] == [1] and lens[16] == [16] and lens[17] == [8, 9] and lens[1008] == [16] * 63
    assert set(lens[1009]) == {15, 16} and set(lens[1089]) == {17, 18} and lens[1600] == [25] * 64
    for hw in S.DGATE_HW:
        r = S.dgate_partition(hw, 32, S.F32)[1]
        assert r[0][0] == 0 and r[-1][1] == hw and all(a[1] == b[0] for a, b in zip(r, r[1:]))
    assert set(S.DGATE_CH) == {(S.F32, 32), (S.F32, 144), (S.F32, 1152), (S.F32, 2688), (S.BF16, 240), (S.BF16, 1152)}
    forms = [S.dgate_partition(16, C, dt)[2:] for dt, C in S.DGATE_CH]           # (tcols, rpp, column passes)
    assert [(rpp, passes) for _, rpp, passes in forms] == [(32, 1), (7, 1), (1, 2), (1, 3), (8, 1), (1, 1)]
    assert [256 - tcols * rpp for tcols, rpp, _ in forms] == [0, 4, 0, 0, 16, 112]           # idle threads (r0 < rpp guard)
    # a slab shorter than the row groups (most groups add nothing), and one longer than a pass of every form
    assert any(min(lens[hw]) < rpp for hw in S.DGATE_HW for _, rpp, _ in forms if rpp > 1)
    assert max(max(v) for v in lens.values()) < 32 and any(max(v) > 8 for v in lens.values())
    assert all(rpp * C * 4 <= 60000 for (dt, C), (_, rpp, _) in zip(S.DGATE_CH, forms)) and S.DGATE_B == 2


# ----------------------------------------------------------------------------- elementwise kernels
def test_elementwise_cases_run_a_second_round_with_a_partial_workgroup():
    one_round = 4096 * 256
    assert S.ELEMWISE_ROUND == one_round == 1048576
    assert sorted(str(c[0]) for c in S.ELEMWISE_CASES) == ['torch.bfloat16', 'torch.float32']
    for c in S.ELEMWISE_CASES:
        dt, B, H, W, C = c
        n, cpr, per_image, rounds = S.elemwise_chunks(*c)
        assert C % S.ce(dt) == 0 and n == B * H * W * C // S.ce(dt)
        assert one_round < n < 2 * one_round and rounds == 2, c
        assert n % 256 and not _pow2(cpr) and B >= 2, c
        assert (one_round // per_image) >= 1 and one_round % per_image and one_round % cpr      # the round boundary falls inside an image and inside a pixel row
        assert B * H * W * C * (4 if dt == S.F32 else 2) <= 20e6
    # what the existing op-level helper test runs stays far below one round
    assert S.elemwise_chunks(S.F32, 3, 5, 6, 40)[3] == 1


# ----------------------------------------------------------------------------- layout converters
def test_converter_cases_run_a_second_round():
    assert S.PACK_ROUND == 2048 * 256 == 524288
    # the batch the per-pixel image path was written for fits one round exactly; a third image is the first loop iteration
    assert S.pack_items('image', 2, 512, 512, 4) == (524288, 1) and S.pack_items('image', 3, 512, 512, 4)[1] == 2
    seen = set()
    for path, dt, B, C, H, W, cpad in S.TO_NHWC_CASES:
        assert S.to_nhwc_path(dt, C, cpad) == path and cpad >= C
        n, rounds = S.pack_items(path, B, H, W, cpad)
        assert S.PACK_ROUND < n < 2 * S.PACK_ROUND and rounds == 2 and n % 256, (path, dt, n)
        seen.add((path, dt, C, cpad))
    assert seen >= {('image', S.F32, 3, 4), ('image', S.BF16, 3, 8), ('generic', S.F32, 3, 8), ('generic', S.F32, 40, 40)}
    assert {c[0] for c in S.TO_NCHW_CASES} == {S.F32, S.BF16}
    for dt, B, H, W, C in S.TO_NCHW_CASES:
        assert (B, H, W, C) == (2, 64, 64, 88) and S.PACK_ROUND < B * H * W * C < 2 * S.PACK_ROUND


# ----------------------------------------------------------------------------- colsum
def test_colsum_cases_reach_every_exit_of_the_row_walk():
    assert set(S.COLSUM_ROWS) == {1, 3, 4, 5, 8, 9, 12, 13, 1000} and set(S.COLSUM_C) == {40, 64, 65} and set(S.COLSUM_LD_EXTRA) == {0, 24}
    w = {rows: [S.colsum_walk(rows, sl) for sl in range(4)] for rows in S.COLSUM_ROWS}
    assert w[1] == [(0, True), (0, False), (0, False), (0, False)] and w[3] == [(0, True)] * 3 + [(0, False)]
    assert w[4] == [(0, True)] * 4 and w[5] == [(1, False)] + [(0, True)] * 3 and w[8] == [(1, False)] * 4
    assert w[9] == [(1, True)] + [(1, False)] * 3 and w[12] == [(1, True)] * 4 and w[13] == [(2, False)] + [(1, True)] * 3
    assert w[1000] == [(125, False)] * 4
    # every row is walked exactly once
    for rows in S.COLSUM_ROWS:
        assert sum(2 * p + int(t) for p, t in w[rows]) == rows
    # columns: a partial workgroup, exactly one, and a second workgroup with a single live column
    assert min(S.COLSUM_C) < 64 and 64 in S.COLSUM_C and 65 in S.COLSUM_C


# ----------------------------------------------------------------------------- producer -> consumer chain
def test_chain_geometry_hands_over_more_than_four_partial_rows():
    from efficientdet.pytorch_amd import _lib as L
    lib = L.lib()
    B, H, W = S.CHAIN_GEOMETRY
    for dt in (L.F32, L.BF16):
        assert int(lib.effdet_dwconv_fwd_pool_groups(dt, B, S.CHAIN_C, 1, H, W)) > 4
    assert int(lib.effdet_mbconv_expand_dw_pool_groups(B, 6 * S.CHAIN_CIN, 1, H, W)) > 4
    assert {S.gate_form(B, cse) for cse in S.CHAIN_CSE} == {'one', 'split'}
