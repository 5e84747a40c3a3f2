"""CPU checks of tests/detect_out_cases.py: every case reaches the path of postprocess.hip / pipeline.hip it is tagged with, by the
oracle and the small restatements of the cases module alone.  If a case stops reaching it -- no tie in a later lane, a block that no
longer straddles two images, a kept fraction outside 10..90 %, fewer than 9 kept boxes in the overflow cell, a copy with two
suppressors, A <= 65536 in round4096, a tie run outside the prefix -- a test here fails."""
import numpy as np
import pytest
import torch

from oracle import effdet_oracle as O
from oracle import pipeline_oracle as PO
from tests import detect_out_cases as DC


# --------------------------------------------------------------------------- anchors
def test_anchor_sizes_round_up_and_the_count_is_the_oracles():
    for H, W in DC.ANCHOR_SIZES:
        assert O.anchors_for_image(H, W).shape == (1, DC.num_anchors_restated(H, W), 4)
    assert DC.num_anchors_restated(1, 1) == 45                                         # one cell per level
    # no size is a multiple of any stride: ceil(H / stride) and ceil(W / stride) round up at every level
    assert all(H % 8 and W % 8 for H, W in DC.ANCHOR_SIZES)
    assert any(H < 8 for H, _ in DC.ANCHOR_SIZES) and any(H > 128 > W for H, W in DC.ANCHOR_SIZES)      # a sub-stride side; 2 x 1 cells at level 7
    for H, W in DC.ANCHOR_SIZES:
        assert DC.num_anchors_restated(H, W) > sum(9 * (H // (1 << l)) * (W // (1 << l)) for l in range(3, 8))


# --------------------------------------------------------------------------- decode_score
def test_torch_cpu_max_returns_the_first_maximal_index():
    v, k = torch.tensor([[0.25, 0.5, 0.5, 0.125, 0.5]]).max(dim=1)
    assert float(v) == 0.5 and int(k) == 1
    v, k = torch.tensor([[0.0, 0.0, 0.0]]).max(dim=1)
    assert int(k) == 0


def test_decode_shapes_cover_the_quad_and_the_block_edges():
    ncs = [nc for _, _, nc in DC.DECODE_SHAPES]
    assert sum(nc < DC.QUAD for nc in ncs) >= 3 and 1 in ncs                           # rows shorter than the quad
    assert sum(nc % DC.QUAD != 0 for nc in ncs) >= 5 and sum(nc % DC.QUAD == 0 for nc in ncs) >= 2
    assert {nc % DC.QUAD for nc in ncs} == {0, 1, 2, 3}
    straddle = [(B, A) for B, A, _ in DC.DECODE_SHAPES if B > 1 and A % DC.DECODE_BLOCK]  # a 64-anchor block holds two images' anchors
    assert (3, 65) in straddle and (2, 63) in straddle
    assert any(B * A % DC.DECODE_BLOCK for B, A, _ in DC.DECODE_SHAPES) and any(B * A > DC.DECODE_BLOCK for B, A, _ in DC.DECODE_SHAPES)
    assert (1, 64, 20) in DC.DECODE_SHAPES                                             # exactly one full block
    assert DC.IMG_H != DC.IMG_W


@pytest.mark.parametrize('shape', DC.DECODE_SHAPES, ids=lambda s: 'B%d_A%d_nc%d' % s)
def test_decode_case_families_and_the_oracles_own_error(shape):
    B, A, nc = shape
    cases = {f: DC.decode_case(B, A, nc, f) for f in DC.FAMILIES}
    for f, c in cases.items():
        assert c['anc'].shape == (1, A, 4) and c['reg'].shape == (B, A, 4) and c['cls'].shape == (B, A, nc)
        assert all(c[k].dtype == torch.float32 and c[k].is_contiguous() for k in ('anc', 'reg', 'cls'))
        assert bool(((c['cls'] >= 0) & (c['cls'] <= 1)).all())
    a = cases['distinct']['cls']
    assert all(len(torch.unique(r)) == nc for r in a.reshape(-1, nc))                  # (a) no tie anywhere in a row
    b = cases['eighths']['cls']
    assert bool((b * 8 == (b * 8).round()).all())
    if nc > DC.QUAD:                                                                   # a later index in an EARLIER lane needs k2 >= 4
        frac = float(DC.later_lane_tie_rows(b).float().mean())
        assert frac >= 0.1, frac
        assert bool((b.max(dim=2)[1][DC.later_lane_tie_rows(b)] % DC.QUAD != 0).all())
    elif nc > 1:                                                                       # short rows still tie (first lane wins)
        m = b.max(dim=2, keepdim=True)[0]
        assert int(((b == m).sum(dim=2) > 1).sum()) > 0
    z = cases['zeros_last']['cls'].reshape(-1, nc)
    assert float(z[0::2].abs().max()) == 0.0                                           # (c) all-zero rows: label 0, score 0
    if B * A > 1:
        assert bool((z[1::2, nc - 1] > 0).all()) and (nc == 1 or float(z[1::2, :nc - 1].abs().max()) == 0.0)
        assert bool((z[1::2].max(dim=1)[1] == nc - 1).all())
    # regression rows: exp far out of the image, underflow to a point, all-zero deltas
    c = cases['distinct']
    rows = DC.special_rows(B * A)
    if B * A >= 50:
        assert len(rows) == 8 and {p for _, p in rows} == set(DC.REG_PATTERNS)
    ref = DC.decode_clip_f64(c['anc'], c['reg'], DC.IMG_H, DC.IMG_W)
    assert bool(torch.isfinite(ref).all())
    flat, anc = ref.view(-1, 4), c['anc'][0].double()
    for r, pat in rows:
        box, an = flat[r], anc[r % A]
        if pat is None:                                                                # the anchor itself, clipped
            want = torch.stack([an[0].clamp(min=0), an[1].clamp(min=0), an[2].clamp(max=DC.IMG_W), an[3].clamp(max=DC.IMG_H)])
            assert bool((box - want).abs().max() < 1e-9)
        else:
            assert abs(float(np.float32(pat[0]) * np.float32(0.2))) == 40.0
            if pat[0] > 0:
                assert float(box[0]) == 0.0 and float(box[2]) == DC.IMG_W
            else:
                assert float(box[2].float()) == float(box[0].float())                  # a point in fp32 (or clipped to one)
            if pat[1] > 0:
                assert float(box[1]) == 0.0 and float(box[3]) == DC.IMG_H
            else:
                assert float(box[3].float()) == float(box[1].float())
    # the fp32 oracle's own error against float64 in assert_close's metric: a quarter of the bound the device tier holds the kernel to
    worst = 0.0
    for f, cc in cases.items():
        err = DC.close_metric(O.decode_clip(cc['anc'], cc['reg'], DC.IMG_H, DC.IMG_W), DC.decode_clip_f64(cc['anc'], cc['reg'], DC.IMG_H, DC.IMG_W))
        print('decode B%d A%d nc%d %-10s oracle fp32 vs float64: %.3g' % (B, A, nc, f, err))
        worst = max(worst, err)
    assert worst < 1e-5                                                                # (inside the 1e-5 parity bound itself)


# --------------------------------------------------------------------------- greedy NMS
@pytest.mark.parametrize('name', sorted(DC.NMS_CASES))
def test_nms_case_is_well_formed(name):
    c = DC.NMS_CASES[name]()
    B, A = c['score'].shape
    assert c['boxes'].shape == (B, A, 4) and c['label'].shape == (B, A) and c['label'].dtype == torch.int32
    assert c['boxes'].dtype == torch.float32 and c['score'].dtype == torch.float32
    assert len(torch.unique(c['label'])) > 1 or A == 1
    assert c['thr'] == DC.THR and all(0.0 < i < 1.0 for i in c['ious'])
    for b in range(B):
        s = c['score'][b][c['score'][b] > c['thr']]
        assert len(torch.unique(s)) == len(s)                                          # distinct scores: the order is the scores' alone


@pytest.mark.parametrize('n', DC.COUNTS_N)
def test_counts_sit_on_the_boundaries_and_keep_a_share(n):
    name = 'counts_n%d' % n
    c = DC.NMS_CASES[name]()
    A = c['score'].shape[1]
    assert A == n + 9 and int((c['score'][0] > DC.THR).sum()) == n
    assert int((c['score'][0] == np.float32(DC.THR)).sum()) == 1                       # exactly on the threshold: not a candidate
    assert c['ious'] == ((0.5, 0.3) if n in (2048, 2049, 4097) else (0.5,))
    pos = torch.nonzero(c['score'][0] > DC.THR).flatten()
    if n > 1:
        assert not torch.equal(pos, torch.arange(n))                                   # candidates scattered between non-candidates
    for iou in c['ious']:
        kept = len(DC.nms_reference(name, iou)[0])
        print('%s IoU %.1f: oracle keeps %d of %d' % (name, iou, kept, n))
        if n >= 63:
            assert 0.1 * n <= kept <= 0.9 * n, (n, iou, kept)
    R = DC.round_size(A)
    assert R == 2048 and set(DC.COUNTS_N) >= {R - 1, R, R + 1, 2 * R - 1, 2 * R, 2 * R + 1, 63, 64, 65, 255, 256, 257}
    if n > R and 0.3 in c['ious']:                                                     # the brute-force cross phase has work in round 1
        order = DC.sorted_candidates(c['score'][0])
        keep = DC.nms_reference(name, 0.3)[0]
        early = keep[torch.isin(keep, order[:R])]
        late = order[R:]
        hit = (DC.iou_matrix(c['boxes'][0][late], c['boxes'][0][early]) > np.float32(0.3)).any(axis=1)
        assert hit.any() and (n == R + 1 or not hit.all())


def test_all_survive_fills_every_round():
    c = DC.all_survive_full_rounds()
    A = c['score'].shape[1]
    assert A == 2 * DC.round_size(A) == 4096 and int((c['score'][0] > DC.THR).sum()) == A
    iou = DC.iou_matrix(c['boxes'][0], c['boxes'][0])
    np.fill_diagonal(iou, 0.0)
    assert float(iou.max()) == 0.0                                                     # pairwise disjoint
    order = DC.sorted_candidates(c['score'][0])
    for t in c['ious']:
        assert torch.equal(DC.nms_reference('all_survive_full_rounds', t)[0], order)
    assert c['ious'] == (0.5, 0.3)


def test_all_identical_keeps_one_and_has_a_second_round():
    c = DC.all_identical()
    A = c['score'].shape[1]
    assert A == 2100 and A - DC.round_size(A) == 52 and bool((c['boxes'][0] == c['boxes'][0, 0]).all())
    for t in c['ious']:
        keep = DC.nms_reference('all_identical', t)[0]
        assert keep.tolist() == [int(c['score'][0].argmax())]


def test_overflow_case_hangs_every_copy_on_one_kept_box_of_the_full_cell():
    c, group = DC.overflow_single_suppressor()
    boxes, score = c['boxes'][0], c['score'][0]
    assert c['ious'] == (DC.OVF_IOU,) and DC.OVF_IOU >= 0.5                             # the grid path
    keep = DC.nms_reference('overflow_single_suppressor', DC.OVF_IOU)[0]
    # (1) 2164 kept: every anchor, every filler, no copy
    assert len(keep) == 2164 == DC.OVF_ANCHORS + DC.OVF_FILLERS
    assert sorted(keep.tolist()) == sorted(torch.nonzero(group != 2).flatten().tolist())
    # (2) all 64 kept anchors are filed under ONE (octave, cell): all but KG_CAP of them live in the overflow list
    anchors = torch.nonzero(group == 0).flatten()
    cells = {DC.grid_cell(boxes[i]) for i in anchors}
    assert len(cells) == 1 and next(iter(cells)) == (12, 31, 31)
    assert len(anchors) - DC.KG_CAP == 56 and len(anchors) >= 9
    assert DC.inv_cell(12) == 1.0 / 32.0 and DC.octave(4096.0) == 12 and DC.octave(4095.9) == 11 and DC.octave(1.0) == DC.SB_MIN
    fillers = torch.nonzero(group == 1).flatten()
    assert not ({DC.grid_cell(boxes[i]) for i in fillers[::50]} & cells)
    # (3) every copy has exactly one suppressor among the kept boxes -- and it is an anchor
    copies = torch.nonzero(group == 2).flatten()
    sup = DC.iou_matrix(boxes[copies], boxes[keep]) > np.float32(DC.OVF_IOU)
    assert bool((sup.sum(axis=1) == 1).all())
    assert bool((group[keep[sup.argmax(axis=1)]] == 0).all()) and len(set(sup.argmax(axis=1).tolist())) == 64
    # (4) every copy sorts behind all kept boxes: at position >= 2164, i.e. in round 1, after the anchors were filed in round 0
    order = DC.sorted_candidates(score)
    rank = torch.empty_like(order); rank[order] = torch.arange(len(order))
    assert int(rank[copies].min()) >= 2164 > DC.round_size(len(score)) and int(rank[anchors].max()) == DC.OVF_ANCHORS - 1
    assert not torch.equal(group, group.sort()[0])                                     # the groups are interleaved over the anchor axis


def test_round4096_uses_the_large_round_and_its_cross_phase():
    c = DC.round4096()
    B, A = c['score'].shape
    assert A > 65536 and B == 2 and DC.round_size(A) == 4096
    n = [int((c['score'][b] > DC.THR).sum()) for b in range(B)]
    assert n == [9000, 4097]
    ref = DC.nms_reference('round4096', 0.5)
    for b in range(B):
        print('round4096 image %d: oracle keeps %d of %d' % (b, len(ref[b]), n[b]))
        assert 0.1 * n[b] <= len(ref[b]) <= 0.9 * n[b]
    boxes, score = c['boxes'][0], c['score'][0]
    order = DC.sorted_candidates(score)
    rank = torch.full((A,), -1, dtype=torch.int64); rank[order] = torch.arange(len(order))
    kr = rank[ref[0]]
    assert int((kr >= 4096).sum()) > 0 and int((kr >= 8192).sum()) > 0                # boxes kept from the second and the third round
    early, late = ref[0][kr < 4096], order[4096:]
    sup_early = (DC.iou_matrix(boxes[late], boxes[early]) > np.float32(0.5)).any(axis=1)
    sup_late = (DC.iou_matrix(boxes[late], boxes[ref[0][kr >= 4096]]) > np.float32(0.5))
    sup_late &= (rank[ref[0][kr >= 4096]][None, :] < rank[late][:, None]).numpy()
    assert int(sup_early.sum()) > 0                                                    # the cross phase at RND = 4096 has victims ...
    only = sup_early & ~sup_late.any(axis=1)
    print('round4096: %d late candidates die by an earlier round, %d of them ONLY by an earlier round' % (int(sup_early.sum()), int(only.sum())))
    assert int(only.sum()) > 0                                                         # ... that nothing in their own round would catch
    order1 = DC.sorted_candidates(c['score'][1])
    assert len(order1) == 4097                                                         # image 1: a second round of ONE candidate
    low = DC.round4096_low_iou()
    assert low['ious'] == (0.3,) and low['score'].shape == (1, A) and torch.equal(low['score'][0], score)
    k3 = DC.nms_reference('round4096_low_iou', 0.3)[0]
    assert 0.1 * 9000 <= len(k3) <= 0.9 * 9000 and int((rank[k3] >= 4096).sum()) > 0


def test_batch_mixed_counts_and_small_A():
    c = DC.batch_mixed_counts()
    B, A = c['score'].shape
    assert (B, A) == (5, 5000) and [int((c['score'][b] > DC.THR).sum()) for b in range(B)] == [5000, 0, 1, 2049, 300]
    rounds = [-(-n // DC.round_size(A)) for n in DC.MIXED_N]
    assert rounds == [3, 0, 1, 2, 1]                                                   # the images finish in different rounds
    for t in c['ious']:
        ref = DC.nms_reference('batch_mixed_counts', t)
        assert len(ref[1]) == 0 and len(ref[2]) == 1 and all(0.1 * n <= len(r) <= 0.9 * n for n, r in zip(DC.MIXED_N, ref) if n >= 63)
    for a, ns in DC.SMALL_N.items():
        c = DC.small_A(a)
        assert c['score'].shape == (2, a) and [int((c['score'][b] > DC.THR).sum()) for b in range(2)] == list(ns)
    assert set(DC.SMALL_N) == {1, 7}


# --------------------------------------------------------------------------- finalize_dets
def test_finalize_case_shape_and_the_stride_boundaries():
    c = DC.finalize_case()
    assert c['score'].shape == (6, 600) and c['count'].tolist() == [0, 1, 255, 256, 257, 600] and c['count'].dtype == torch.int32
    assert c['label'].dtype == torch.int64 and int(c['label'].min()) >= 0 and int(c['label'].max()) <= 90
    assert c['scale'].dtype == torch.float32 and c['scale'].tolist() == [float(np.float32(s)) for s in (0.3, 1.0, 1.7, 2.5, 1 / 3, 0.8125)]
    assert bool((c['score'][:, 1:] <= c['score'][:, :-1]).all())                       # descending over all 600 rows
    assert float(c['score'].min()) > DC.FIN_THRESHOLDS['below'] and float(c['score'].max()) < DC.FIN_THRESHOLDS['above']
    S = DC.FIN_STRIDE
    assert {S - 1, S, S + 1} <= set(c['count'].tolist()) and {S, S + 1} <= set(DC.FIN_MAX_DET)
    assert DC.FIN_MAX_DET == (1, 100, 256, 257, 1000) and max(DC.FIN_MAX_DET) > 600 > min(DC.FIN_MAX_DET)   # max_det above and below the count
    for b, p in DC.FIN_RUN.items():
        assert c['score'][b, p:p + 3].tolist() == [DC.FIN_TIE] * 3
        assert int((c['score'][b] == DC.FIN_TIE).sum()) == 3
    assert DC.FIN_RUN[4] < S <= DC.FIN_RUN[4] + 2                                      # a run that spans the 256-thread stride
    assert DC.FIN_RUN[3] + 3 == 100                                                    # a run that ends exactly at max_det = 100


@pytest.mark.parametrize('max_det', DC.FIN_MAX_DET)
def test_finalize_restatement_is_the_reference_and_the_tie_splits_the_two_rules(max_det):
    c = DC.finalize_case()
    for tname, thr in DC.FIN_THRESHOLDS.items():
        out, oc = DC.finalize_restated(c['score'], c['label'], c['boxes'], c['count'], c['scale'], thr, max_det, False)
        outw, ocw = DC.finalize_restated(c['score'], c['label'], c['boxes'], c['count'], c['scale'], thr, max_det, True)
        for b in range(DC.FIN_B):
            n = int(c['count'][b])
            ref = PO.finalize_reference(c['score'][b, :n].numpy(), c['label'][b, :n].numpy(), c['boxes'][b, :n].numpy(),
                                        float(c['scale'][b]), float(np.float32(thr)), max_det)
            assert oc[b] == len(ref) and np.array_equal(out[b, :oc[b]].view(np.int32), ref.astype(np.float32).view(np.int32)), (tname, b)
            pad = out[b, oc[b]:]
            assert bool((pad[:, :5] == 0).all()) and bool((pad[:, 5] == -1).all())
            lim = min(n, max_det)
            if tname == 'below':
                assert oc[b] == ocw[b] == lim
            elif tname == 'above':
                assert oc[b] == ocw[b] == 0
            else:
                p = DC.FIN_RUN.get(b)
                if p is not None and p + 3 <= lim:                                     # the run lies inside the prefix both rules look at
                    assert oc[b] == p and ocw[b] == p + 3, (b, max_det)                # `>` stops before the run, `>=` ends after it
            # xywh: widths and heights of the very same rows
            k = int(ocw[b])
            if k:
                w = out if oc[b] >= k else DC.finalize_restated(c['score'], c['label'], c['boxes'], c['count'], c['scale'], -1.0, max_det, False)[0]
                assert np.array_equal(outw[b, :k, 2], w[b, :k, 2] - w[b, :k, 0]) and np.array_equal(outw[b, :k, :2], w[b, :k, :2])
    # the tied threshold bites at this max_det for at least one image (max_det = 1 can only hold image 1's single tied row)
    _, oc = DC.finalize_restated(c['score'], c['label'], c['boxes'], c['count'], c['scale'], DC.FIN_TIE, max_det, False)
    _, ocw = DC.finalize_restated(c['score'], c['label'], c['boxes'], c['count'], c['scale'], DC.FIN_TIE, max_det, True)
    inside = [b for b, p in DC.FIN_RUN.items() if p + 3 <= min(DC.FIN_COUNT[b], max_det)]
    assert len(inside) >= (1 if max_det >= 100 else 0) and int((ocw - oc != 0).sum()) >= 1
    if max_det == 256:
        assert int(ocw[4]) == 256 and int(oc[4]) == 254                                # max_det cuts the run of image 4 after two rows


# --------------------------------------------------------------------------- head_out_bwd
def test_head_out_bwd_shapes_reach_vector_tail_and_shared_workgroups():
    assert DC.HOB_SHAPES[-1] == (3074, 1025)
    inside, on_edge = [], []
    for ncls, nreg in DC.HOB_SHAPES:
        gc, gr = -(-ncls // 4), -(-nreg // 4)
        if gc + gr > DC.HOB_WG:                                                        # a multi-workgroup launch
            (inside if gc % DC.HOB_WG else on_edge).append((ncls, nreg))
    # the class / box boundary inside a workgroup (one workgroup serves both regions) -- and, for contrast, exactly between two
    assert (1025, 1023) in inside and (3074, 1025) in inside and (1024, 1024) in on_edge and (1023, 1025) in on_edge
    assert any(ncls < 4 * DC.HOB_WG and ncls + nreg <= 8 for ncls, nreg in DC.HOB_SHAPES)      # single workgroup serving both
    for region in (0, 1):
        sizes = [s[region] for s in DC.HOB_SHAPES]
        assert 0 in {n % 4 for n in sizes} and len({n % 4 for n in sizes} - {0}) >= 2 and any(n < 4 for n in sizes)      # vector groups and scalar tails


@pytest.mark.parametrize('shape', DC.HOB_SHAPES, ids=lambda s: 'ncls%d_nreg%d' % s)
def test_head_out_bwd_case_values(shape):
    ncls, nreg = shape
    c = DC.head_out_bwd_case(ncls, nreg)
    assert c['dprob'].shape == c['prob'].shape == (ncls,) and c['dreg'].shape == (nreg,)
    m = c['marks']
    if ncls >= 8:
        assert set(m) == {'zero', 'one', 'nan', 'inf', '-inf', 'inf_times_zero'}
        assert float(c['prob'][m['zero']]) == 0.0 and float(c['prob'][m['one']]) == 1.0
        assert bool(torch.isnan(c['dprob'][m['nan']])) and float(c['dprob'][m['inf']]) == float('inf') and float(c['dprob'][m['-inf']]) == -float('inf')
        assert (m['one'] >= ncls // 4 * 4) == (ncls % 4 != 0)                          # the exact 1 sits in the scalar tail when there is one
    for dtype in (torch.float32, torch.bfloat16):
        dl, dr = DC.head_out_bwd_reference(c, dtype)
        assert dl.dtype == dr.dtype == dtype
        if 'zero' in m:
            assert float(dl[m['zero']]) == 0.0 or bool(torch.isnan(dl[m['zero']]))
        if 'one' in m:
            assert float(dl[m['one']]) == 0.0
        if 'inf_times_zero' in m:
            assert bool(torch.isnan(dl[m['inf_times_zero']])) and bool(torch.isnan(dl[m['nan']]))
            assert float(dl[m['inf']]) == float('inf') and float(dl[m['-inf']]) == -float('inf')
            assert int(torch.isfinite(dl.float()).sum()) >= ncls - 5
    if nreg >= 5:                                                                      # round-to-nearest-EVEN is visible in dreg
        dr = c['dreg'].bfloat16().float()
        assert float(dr[1]) == 1.0 and float(dr[2]) == 1.015625 and float(dr[3]) == -1.0
        assert nreg < 8 or float(dr[nreg - 1]) == 1.015625                             # ... and in the last element (the tail, if any)
        trunc = (c['dreg'].view(torch.int32) & -65536).view(torch.float32)
        assert not torch.equal(trunc, dr)
