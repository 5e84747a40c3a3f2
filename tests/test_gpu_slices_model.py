"""GPU: sliced inference at the model level (D0, 20 classes, seeded weights, fp32), in the manner of tests/test_gpu_tta_scales.py.

B = 2 images of 600 x 850 -- multiples of nothing -- under SliceOptions(slice=(256, 256), overlap=(0.25, 0.25), tile_batch=8,
merge=SliceMergeOptions(top_n=200, max_det=300)): 3 x 5 tiles and the full view, 16 lists per image, 3200 candidates.

The expectation is built without the ops under test: the tiles by torch indexing, permuted to NHWC with a zero fourth channel and wrapped
as PackedImages, grouped into the product's chunks of 8 flat tiles, each chunk through forward_raw + evaluate.postprocess; the full view
is ops.resample_images(batch, (256, 256)) (which has its own tests) through one pass of batch 2; the lists are merged on the host by
the fp32 restatement (tests/slices_restated.merge).  detect() must equal that in labels, score bits and box bits.

The seeded weights score nearly every anchor above the model's threshold, so the model runs with set_nms(NMSOptions(max_det=200)): every
list then holds at most 200 = top_n rows and the merge's top_n cuts nothing, which the fixture asserts -- together with a death across
two tiles and a grown hull in both images (tests/test_slices_host.py shows the same on the CPU with the oracle)."""
import numpy as np
import pytest
import torch

from oracle import effdet_oracle as O
from tests import slices_restated as R
from tests.slices_cases import MODEL_CASE as M

pytestmark = pytest.mark.gpu
H, W = 600, 850
S = 256


def _options():
    from efficientdet.pytorch_amd import SliceMergeOptions, SliceOptions
    return SliceOptions(slice=M['slice'], overlap=M['overlap'], tile_batch=M['tile_batch'], merge=SliceMergeOptions(top_n=M['top_n'], max_det=M['max_det']))


def _own_lists(m, img, table, run):
    """The per-tile lists of model m on the batch, built without ops.slice_images -> (score [B,16,200], label, boxes, count [B,16]) on the
    host.  run(x) -> model_nms's tuple for a PackedImages batch x of 256 x 256."""
    from efficientdet.pytorch_amd import PackedImages, ops
    B, T = img.shape[0], len(table) - 1
    flat = []
    for b in range(B):
        for y0, x0, h, w, _, _ in table[:T]:
            t = img[b, :, y0:y0 + h, x0:x0 + w].permute(1, 2, 0)
            flat.append(torch.cat([t, torch.zeros(h, w, 1, device=img.device)], dim=2))
    parts = []
    for t0 in range(0, B * T, M['tile_batch']):
        x = torch.stack(flat[t0:t0 + M['tile_batch']]).contiguous()
        parts.append(run(PackedImages(ops.Map.of(x))))
    whole = run(ops.resample_images(img, (S, S)))
    n = M['top_n']
    out = []
    for i in range(3):
        t = torch.cat([p[i][:, :n] for p in parts])
        t = t.reshape((B, T) + tuple(t.shape[1:]))
        out.append(torch.cat([t, whole[i][:, None, :n]], dim=1).cpu().numpy())
    cnt = torch.cat([torch.cat([p[3] for p in parts]).reshape(B, T), whole[3][:, None]], dim=1).cpu().numpy()
    return out[0], out[1], out[2], cnt


def _restated(lists, table, b):
    s, l, bx, c = lists
    return R.merge(s[b], l[b], bx[b], c[b], table, float(W), float(H), max_det=M['max_det'])


def _assert_is_restated(dets, lists, table, need_cross=True):
    assert len(dets) == 2
    for b, (s, l, bx) in enumerate(dets):
        r = _restated(lists, table, b)
        cross = sum(1 for k, a in zip(r.keepers, r.absorbed) for t, _ in a if t != k[0])
        grown = int(((r.boxes[:, 2] - r.boxes[:, 0]) * (r.boxes[:, 3] - r.boxes[:, 1]) > (r.own[:, 2] - r.own[:, 0]) * (r.own[:, 3] - r.own[:, 1])).sum())
        print('image %d: %d rows -> %d keepers, %d deaths across tiles, %d grown hulls' % (b, int(lists[3][b].sum()), len(r.keepers), cross, grown))
        assert not need_cross or (cross > 0 and grown > 0)
        assert len(s) == len(r.score) and np.array_equal(l.cpu().numpy(), r.label)
        assert np.array_equal(s.cpu().numpy().view(np.uint32), r.score.view(np.uint32))
        assert np.array_equal(bx.cpu().numpy().view(np.uint32), r.boxes.view(np.uint32))


@pytest.fixture(scope='module')
def setup():
    from efficientdet.pytorch_amd import EfficientDet, EFFICIENTDET, NMSOptions, evaluate, ops
    net, nc = 'efficientdet-d0', 20
    c = EFFICIENTDET[net]
    m = EfficientDet(nc, network=net, W_bifpn=c['W_bifpn'], D_bifpn=c['D_bifpn'], D_class=c['D_class'], is_training=False,
                     compute_dtype=torch.float32)
    m.load_state_dict(O.make_state_dict(net, nc, seed=0)); m = m.cuda().eval()
    m.set_nms(NMSOptions(method='hard', pre_nms_top_n=1000, max_det=200))
    img = M['images']().cuda()
    assert tuple(img.shape) == (2, 3, H, W)
    small = img[:, :, 100:100 + S, 300:300 + S].contiguous()
    with torch.no_grad():
        before = (m.detect(small), m.detect(img[:, :, :512, :768].contiguous()))            # a plain model, before any SlicedDetector exists
    table = ops.slice_plan(H, W, _options())
    assert table == R.plan(H, W, M['slice'], M['overlap']) and len(table) == 16

    def run(x):
        cls, reg, anc = m.forward_raw(x)
        return evaluate.postprocess(m, cls, reg, anc, S, S)
    with torch.no_grad():
        lists = _own_lists(m, img, table, run)
    print('counts per list:', lists[3].tolist())
    assert lists[0].shape == (2, 16, 200) and 0 < lists[3].min() and lists[3].max() <= 200           # top_n cuts nothing
    for b in range(2):
        r = _restated(lists, table, b)
        assert any(t != k[0] for k, a in zip(r.keepers, r.absorbed) for t, _ in a)                     # a death across two tiles
        assert ((r.boxes[:, 2] - r.boxes[:, 0]) * (r.boxes[:, 3] - r.boxes[:, 1]) > (r.own[:, 2] - r.own[:, 0]) * (r.own[:, 3] - r.own[:, 1])).any()
    return m, img, small, table, lists, before


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def test_detect_is_the_restated_merge_of_independently_built_tiles(setup):
    from efficientdet.pytorch_amd import SlicedDetector, evaluate
    m, img, small, table, lists, before = setup
    d = SlicedDetector(m, _options())
    dets = d.detect(img)
    _assert_is_restated(dets, lists, table)
    assert all(len(x[0]) <= 300 for x in dets)
    out, oc = evaluate.detections_batched(d, img, [1.0, 1.0], score_threshold=0.0, max_detections=100)
    assert oc.tolist() == [min(len(x[0]), 100) for x in dets]
    for i, n in enumerate(oc.tolist()):
        assert np.array_equal(out[i, :n, 4], dets[i][0][:n].cpu().numpy()) and np.array_equal(out[i, :n, :4], dets[i][2][:n].cpu().numpy())
        assert np.array_equal(out[i, :n, 5], dets[i][1][:n].cpu().numpy().astype(np.float32))


def test_a_model_with_flip_tta_is_sliced_per_tile(setup):
    from efficientdet.pytorch_amd import SlicedDetector, TTAOptions, ops
    m, img, small, table, lists, before = setup
    try:
        m.set_tta(TTAOptions(hflip=True))

        def run(x):
            return ops.model_detections(m, x, S, S)                  # the model's own per-tile output, flip TTA included
        with torch.no_grad():
            tta_lists = _own_lists(m, img, table, run)
        assert 0 < tta_lists[3].min() and not np.array_equal(tta_lists[0], lists[0])
        _assert_is_restated(SlicedDetector(m, _options()).detect(img), tta_lists, table, need_cross=False)
    finally:
        m.set_tta(None)


def test_one_tile_is_the_inner_models_detect(setup):
    from efficientdet.pytorch_amd import SlicedDetector, ops
    m, img, small, table, lists, before = setup
    assert ops.slice_plan(S, S, _options()) == [(0, 0, S, S, 1.0, 1.0)]
    got, want = SlicedDetector(m, _options()).detect(small), m.detect(small)
    assert len(got) == 2 and all(len(w[0]) > 0 for w in want)
    assert all(_same(g, w) for g, w in zip(got, want))               # the merge does not change the model's own NMS output


def test_an_image_smaller_than_the_slice_is_refused_before_any_forward(setup):
    from efficientdet.pytorch_amd import SlicedDetector
    m, img, small, table, lists, before = setup
    calls = []
    orig = m.forward_raw
    try:
        m.forward_raw = lambda x: calls.append(1) or orig(x)
        with pytest.raises(ValueError, match='height 200 is smaller than the slice height 256'):
            SlicedDetector(m, _options()).detect(img[:, :, :200].contiguous())
        assert not calls
    finally:
        del m.forward_raw


def test_other_paths_are_untouched(setup):
    from efficientdet.pytorch_amd import SlicedDetector
    m, img, small, table, lists, before = setup
    SlicedDetector(m, _options()).detect(img)
    after = (m.detect(small), m.detect(img[:, :, :512, :768].contiguous()))
    for a, b in zip(after, before):
        assert len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
