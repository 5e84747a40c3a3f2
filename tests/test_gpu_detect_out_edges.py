"""GPU parity of the output path -- anchors, decode_score, greedy NMS rounds, gather_dets, finalize_dets -- and of head_out_bwd on the
edge cases of tests/detect_out_cases.py (what each case reaches is proven on the CPU by tests/test_detect_out_cases_host.py).  Calls
ops.* only.  Keep lists, labels, scores, the eval consumer's rows and the head gradient are held bit for bit / index for index;
decoded boxes to the 1e-5 of test_gpu_post_loss against the fp32 oracle and to 4 x the oracle's own error against float64."""
import numpy as np
import pytest
import torch

from oracle import effdet_oracle as O
from tests import detect_out_cases as DC
from tests.gpu_util import assert_close

pytestmark = pytest.mark.gpu


# --------------------------------------------------------------------------- anchors
@pytest.mark.parametrize('size', DC.ANCHOR_SIZES, ids=lambda s: '%dx%d' % s)
def test_anchors_at_sizes_that_round_up(size):
    from efficientdet.pytorch_amd import ops
    H, W = size
    ref = O.anchors_for_image(H, W).numpy()
    got = ops.anchors(H, W, 'cuda').cpu().numpy()
    assert ops.num_anchors(H, W) == ref.shape[1] == got.shape[1] == DC.num_anchors_restated(H, W)
    assert np.array_equal(got, ref)


# --------------------------------------------------------------------------- decode_score
@pytest.mark.parametrize('family', DC.FAMILIES)
@pytest.mark.parametrize('shape', DC.DECODE_SHAPES, ids=lambda s: 'B%d_A%d_nc%d' % s)
def test_decode_score_edges(shape, family):
    from efficientdet.pytorch_amd import ops
    B, A, nc = shape
    c = DC.decode_case(B, A, nc, family)
    boxes, score, label = ops.decode_score(c['anc'].cuda(), c['reg'].cuda(), c['cls'].cuda(), DC.IMG_H, DC.IMG_W)
    boxes, score, label = boxes.cpu(), score.cpu(), label.cpu()
    ms, ml = c['cls'].max(dim=2)                                                       # CPU max: the FIRST maximal index
    assert torch.equal(score, ms)
    assert torch.equal(label.long(), ml), 'first differing row %s' % torch.nonzero(label.long() != ml)[:1].tolist()
    ref32 = O.decode_clip(c['anc'], c['reg'], DC.IMG_H, DC.IMG_W)
    ref64 = DC.decode_clip_f64(c['anc'], c['reg'], DC.IMG_H, DC.IMG_W)
    oracle_err = DC.close_metric(ref32, ref64)                                         # from the two references, never from the kernel
    kernel_err = DC.close_metric(boxes, ref64)
    print('decode B%d A%d nc%d %s: kernel vs float64 %.3g, oracle vs float64 %.3g, kernel vs oracle %.3g' % (
        B, A, nc, family, kernel_err, oracle_err, DC.close_metric(boxes, ref32)))
    assert bool(torch.isfinite(boxes).all())
    assert_close(boxes, ref32, 1e-5, 'decode vs the fp32 oracle')
    assert kernel_err <= 4.0 * oracle_err, (kernel_err, oracle_err)


# --------------------------------------------------------------------------- greedy NMS + gather_dets
def _check_nms(name, iou):
    from efficientdet.pytorch_amd import ops
    c = DC.NMS_CASES[name]()
    ref = DC.nms_reference(name, iou)
    boxes, score, label = c['boxes'].cuda(), c['score'].cuda(), c['label'].cuda()
    idx, cnt = ops.nms(boxes, score, c['thr'], iou)
    gs, gl, gb = ops.gather_dets(boxes, score, label, idx, cnt)
    idx, cnt, gs, gl, gb = idx.cpu(), cnt.cpu(), gs.cpu(), gl.cpu(), gb.cpu()
    assert cnt.tolist() == [len(r) for r in ref], (name, iou, cnt.tolist(), [len(r) for r in ref])
    assert gl.dtype == torch.int64
    for b, r in enumerate(ref):
        n = len(r)
        got = idx[b, :n].long()
        if not torch.equal(got, r):
            k = int(torch.nonzero(got != r)[0])
            raise AssertionError('%s IoU %g image %d: keep lists differ from position %d of %d on (got anchor %d, oracle %d)' % (
                name, iou, b, k, n, int(got[k]), int(r[k])))
        # gather_dets of EVERY image against plain indexing
        assert torch.equal(gs[b, :n], c['score'][b][r]), (name, b)
        assert torch.equal(gl[b, :n], c['label'][b][r].long()), (name, b)
        assert torch.equal(gb[b, :n], c['boxes'][b][r]), (name, b)
    return cnt


@pytest.mark.parametrize('n,iou', [(n, 0.5) for n in DC.COUNTS_N] + [(n, 0.3) for n in DC.COUNTS_LOW_IOU])
def test_nms_counts_on_the_round_boundaries(n, iou):
    _check_nms('counts_n%d' % n, iou)


@pytest.mark.parametrize('iou', [0.5, 0.3])
def test_nms_all_survive_full_rounds(iou):
    assert int(_check_nms('all_survive_full_rounds', iou)[0]) == 4096


@pytest.mark.parametrize('iou', [0.5, 0.3])
def test_nms_all_identical(iou):
    assert int(_check_nms('all_identical', iou)[0]) == 1


def test_nms_overflow_single_suppressor():
    """Each of the 64 copies is suppressed by exactly one kept box, and 56 of those sit in the grid's overflow list."""
    assert int(_check_nms('overflow_single_suppressor', DC.OVF_IOU)[0]) == DC.OVF_ANCHORS + DC.OVF_FILLERS


def test_nms_round4096():
    _check_nms('round4096', 0.5)


def test_nms_round4096_low_iou():
    _check_nms('round4096_low_iou', 0.3)


@pytest.mark.parametrize('iou', [0.5, 0.3])
def test_nms_batch_mixed_counts(iou):
    _check_nms('batch_mixed_counts', iou)


@pytest.mark.parametrize('iou', [0.5, 0.3])
@pytest.mark.parametrize('A', sorted(DC.SMALL_N))
def test_nms_small_A(A, iou):
    _check_nms('small_A%d' % A, iou)


# --------------------------------------------------------------------------- finalize_dets
@pytest.mark.parametrize('xywh', [False, True])
@pytest.mark.parametrize('max_det', DC.FIN_MAX_DET)
def test_finalize_dets_edges(max_det, xywh):
    from efficientdet.pytorch_amd import ops
    c = DC.finalize_case()
    dev = {k: v.cuda() for k, v in c.items()}
    for tname, thr in DC.FIN_THRESHOLDS.items():
        ref, ref_n = DC.finalize_restated(c['score'], c['label'], c['boxes'], c['count'], c['scale'], thr, max_det, xywh)
        out, oc = ops.finalize_dets(dev['score'], dev['label'], dev['boxes'], dev['count'], dev['scale'], thr, max_det, xywh)
        out, oc = out.cpu().numpy(), oc.cpu().numpy()
        what = 'threshold %s max_det %d xywh %s' % (tname, max_det, xywh)
        assert oc.dtype == np.int32 and oc.tolist() == ref_n.tolist(), (what, oc.tolist(), ref_n.tolist())
        assert out.shape == (DC.FIN_B, max_det, 6)
        for b in range(DC.FIN_B):
            k = int(ref_n[b])
            assert np.array_equal(out[b, :k].view(np.int32), ref[b, :k].view(np.int32)), (what, b)          # bit for bit
            pad = out[b, k:]
            assert np.array_equal(pad.view(np.int32), ref[b, k:].view(np.int32)), (what, b)                 # (0, 0, 0, 0, 0, -1)
            assert bool((pad[:, :5] == 0).all()) and bool((pad[:, 5] == -1).all())


# --------------------------------------------------------------------------- head_out_bwd
def _same_bits(got, ref, what):
    """Bitwise on the finite lanes; equal NaN masks; equal +Inf and -Inf masks."""
    assert got.dtype == ref.dtype and got.shape == ref.shape, what
    g, r = got.float(), ref.float()                                                    # (bf16 -> fp32 is exact)
    assert torch.equal(torch.isnan(g), torch.isnan(r)), what + ': NaN mask'
    for inf in (float('inf'), -float('inf')):
        assert torch.equal(g == inf, r == inf), what + ': Inf mask'
    fin = torch.isfinite(r)
    gi, ri = g[fin].view(torch.int32), r[fin].view(torch.int32)
    if not torch.equal(gi, ri):
        k = int(torch.nonzero(gi != ri)[0])
        raise AssertionError('%s: %d of %d finite lanes differ (first: got %r, torch %r)' % (
            what, int((gi != ri).sum()), gi.numel(), float(g[fin][k]), float(r[fin][k])))


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('shape', DC.HOB_SHAPES, ids=lambda s: 'ncls%d_nreg%d' % s)
def test_head_out_bwd_edges(shape, dtype):
    from efficientdet.pytorch_amd import ops
    c = DC.head_out_bwd_case(*shape)
    ref_dl, ref_dr = DC.head_out_bwd_reference(c, dtype)
    dl, dr = ops.head_out_bwd(c['dprob'].cuda(), c['prob'].cuda(), c['dreg'].cuda(), dtype)
    _same_bits(dl.cpu(), ref_dl, 'dlogit %s %s' % (shape, dtype))
    _same_bits(dr.cpu(), ref_dr, 'dreg %s %s' % (shape, dtype))
