"""CPU tier: tools/unit_count.py -- the numpy restatement of csrc/live_tiles.hip's flag geometry and of the compacted unit lists
(include/effdet_unit_lists.h) -- on hand-made maps whose flags can be written down: an empty map, a full map, one pixel at an image
corner, a cluster straddling the boundary of two levels, and the committed table of the benchmark's batch."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import unit_count as U          # noqa: E402

B = 2
SIZES = [(16, 16), (8, 8), (4, 4)]           # M = 512, 128, 32 -> 16 + 4 + 1 steps, 4 + 1 + 1 tiles
PIX = [B * h * w for h, w in SIZES]
STEP0, TILE0 = [0, 16, 20], [0, 4, 5]


def _flags(pmap):
    f32, f128 = U.unit_flags(pmap, B, SIZES, 32), U.unit_flags(pmap, B, SIZES, 128)
    assert f32.shape == (6, 21) and f128.shape == (6, 6) and f32.dtype == np.uint8
    # a tile is flagged iff one of its steps is, and the flags grow with the radius
    for l, (h, w) in enumerate(SIZES):
        ns = (PIX[l] + 31) // 32
        for t in range((PIX[l] + 127) // 128):
            steps = f32[:, STEP0[l] + 4 * t:STEP0[l] + min(4 * t + 4, ns)]
            assert np.array_equal(steps.any(axis=1).astype(np.uint8), f128[:, TILE0[l] + t])
    assert (np.diff(f32.astype(int), axis=0) >= 0).all()
    return f32, f128


def test_empty_map():
    f32, f128 = _flags(np.zeros(sum(PIX), dtype=np.uint8))
    assert not f32.any() and not f128.any()
    units, n = U.unit_lists(f32)
    assert n == [0] * 6 and all(len(u) == 0 for u in units)
    t = U.count_table(np.zeros(sum(PIX), dtype=np.uint8), B, SIZES)
    assert [r['live128'] for r in t['radii']] == [0] * 6 and [r['ratio'] for r in t['radii']] == [None] * 6


def test_full_map():
    f32, f128 = _flags(np.ones(sum(PIX), dtype=np.uint8))
    assert f32.all() and f128.all()
    units, n = U.unit_lists(f32)
    assert n == [21] * 6 and all(np.array_equal(u, np.arange(21)) for u in units) and units[0].dtype == np.int32
    t = U.count_table(np.ones(sum(PIX), dtype=np.uint8), B, SIZES)
    assert t['tiles'] == 6 and t['steps'] == 21
    assert [r['gathered_tiles'] for r in t['radii']] == [6] * 6 and [r['ratio'] for r in t['radii']] == [1.0] * 6


def test_one_pixel_at_an_image_corner():
    """the last pixel of image 0 at level 0 (h = w = 15): radius r reaches rows 15 - r .. 15, i.e. step 7 and, from r = 2 on (two 16-pixel
    rows per step), step 6 -- and never image 1, whose first pixel is the next byte of the map"""
    pmap = np.zeros(sum(PIX), dtype=np.uint8)
    pmap[255] = 1
    f32, f128 = _flags(pmap)
    for r in range(6):
        want = [7] if r < 2 else ([6, 7] if r < 4 else [5, 6, 7])
        assert np.flatnonzero(f32[r]).tolist() == want, r
        assert np.flatnonzero(f128[r]).tolist() == [1], r
    units, n = U.unit_lists(f32)
    assert n == [1, 1, 2, 2, 3, 3] and units[5].tolist() == [5, 6, 7]


def test_a_cluster_straddling_two_levels():
    """the last two pixels of level 0 (image 1, h = 15, w = 14 .. 15) and the first two of level 1 (image 0, h = 0, w = 0 .. 1): neighbours
    in the map, but the distance never crosses a level, and the two levels' units are listed in level-major order"""
    pmap = np.zeros(sum(PIX), dtype=np.uint8)
    pmap[510:514] = 1
    f32, f128 = _flags(pmap)
    assert np.flatnonzero(f32[0]).tolist() == [15, 16] and np.flatnonzero(f128[0]).tolist() == [3, 4]
    # level 1 is 8 wide, a step = 4 rows: radius 4 reaches row 4 = step 17 of the map (the level's second)
    assert np.flatnonzero(f32[3]).tolist() == [14, 15, 16] and np.flatnonzero(f32[4]).tolist() == [13, 14, 15, 16, 17]
    assert not f32[5, 20] and not f128[5, 5]                   # level 2 is never reached
    units, n = U.unit_lists(f32)
    assert units[4].tolist() == [13, 14, 15, 16, 17] and n[4] == 5
    t = U.count_table(pmap, B, SIZES)
    r4 = t['radii'][4]
    assert r4['live128'] == 2 and r4['live32'] == 5 and r4['gathered_tiles'] == 2 and r4['ratio'] == 1.0
    assert [p['live32'] for p in r4['per_level']] == [3, 2, 0]


def test_chebyshev_distance():
    m = np.zeros((1, 9, 9), dtype=bool)
    m[0, 2, 3] = True
    d = U.chebyshev(m)[0]
    yy, xx = np.mgrid[0:9, 0:9]
    assert np.array_equal(d, np.minimum(np.maximum(abs(yy - 2), abs(xx - 3)), 6))


def test_positive_pixel_map_of_a_box_that_is_an_anchor():
    from oracle import effdet_oracle as O
    anc = O.anchors_for_image(128, 128)[0].numpy()
    sizes = U.level_sizes(128)
    ann = np.full((2, 3, 5), -1.0, dtype=np.float32)
    k = 9 * (5 * 16 + 7) + 4                                   # level 0, pixel (5, 7)
    ann[1, 1, :4] = anc[k]; ann[1, 1, 4] = 2.0
    pm = U.positive_pixel_map(anc, ann, sizes)
    assert pm.size == 2 * (256 + 64 + 16 + 4 + 1) and not pm[:256].any()            # image 0 has padding rows only
    assert pm[256 + 5 * 16 + 7] == 1 and pm.sum() >= 1


def test_the_committed_table_is_the_tools_output():
    """profiles/unit_count_b32_512.json: the tile fractions are those of profiles/sparse_reg_fwd_launch_timing.json (measured on the device),
    and the go / no-go ratio at radius 3 is what the summary quotes"""
    t = json.load(open(os.path.join(ROOT, 'profiles', 'unit_count_b32_512.json')))
    dev = json.load(open(os.path.join(ROOT, 'profiles', 'sparse_reg_fwd_launch_timing.json')))
    assert [r['live128_fraction'] for r in t['radii']] == dev['needed128_fraction']
    assert t['tiles'] == 1364 and t['steps'] == 5456 and t['go'] is True
    assert all(r['gathered_tiles'] == (r['live32'] + 3) // 4 for r in t['radii'])
    assert t['radii'][3]['ratio'] == 0.7412
