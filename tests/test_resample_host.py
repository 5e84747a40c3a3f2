"""CPU tier of the model-input resampler and of what hangs off it: the NumPy restatement (tests/resample_restated.py) on the hand-derived
cases of its docstring and against torch's CPU bilinear interpolate under the derived bound of tests/resample_cases.py, the mirror, the
binding's table and struct against include/effdet_resample.h, the host-side refusals of the entry point, TTAOptions with scales,
ops.tta_view_plan, and the constructor checks of EnsembleDetector(scales=)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import resample_cases as K
from tests import resample_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _one(a):
    """[H, W] -> [1, H, W, 3] float32, the three channels a, -a and 2 a"""
    a = np.asarray(a, dtype=np.float32)
    return np.stack([a, -a, 2 * a], -1)[None]


def _got(a, size, flip=False):
    out = R.resample(_one(a), size, flip)
    assert np.array_equal(out[..., 1], -out[..., 0]) and np.array_equal(out[..., 2], 2 * out[..., 0])      # exact scalings commute
    return out[0, :, :, 0].tolist()


def test_restatement_on_the_hand_derived_cases():
    assert _got([[0, 4], [8, 12]], (4, 4)) == [[0, 1, 3, 4], [2, 3, 5, 6], [6, 7, 9, 10], [8, 9, 11, 12]]
    assert _got(np.arange(16).reshape(4, 4), (2, 2)) == [[2.5, 4.5], [10.5, 12.5]]
    assert _got(np.arange(8).reshape(1, 8), (1, 2)) == [[1.5, 5.5]]                                      # no antialiasing
    assert _got([[3, 1, 4, 1.5]], (3, 4)) == [[3, 1, 4, 1.5]] * 3                                          # edge-clamped rows
    assert _got([[3], [1], [4], [1.5]], (4, 3)) == [[3] * 3, [1] * 3, [4] * 3, [1.5] * 3]                   # a 1-pixel-wide source
    assert _got([[7]], (3, 2)) == [[7, 7]] * 3
    # the axis rule itself: clamps at both edges with f = 0
    i0, i1, f = R.axis(2, 4)
    assert i0.tolist() == [0, 0, 0, 1] and i1.tolist() == [1, 1, 1, 1] and f.tolist() == [0, 0.25, 0.75, 0] and f.dtype == np.float32
    i0, i1, f = R.axis(1, 5)
    assert not i0.any() and not i1.any() and not f.any()
    i0, i1, f = R.axis(5, 5)                                                                            # the same size: every f is 0
    assert i0.tolist() == [0, 1, 2, 3, 4] and i1.tolist() == [1, 2, 3, 4, 4] and not f.any()
    # the coordinate is the float64 expression rounded once: 256 -> 384 at o = 1 is (1.5 * (256 / 384) - 0.5) = 0.5 exactly in fp64
    assert R.coords(256, 384)[1] == np.float32(0.5) and R.coords(256, 384)[0] == np.float32(0.5 * (256.0 / 384.0) - 0.5)


def test_flip_is_the_mirror_image_bit_for_bit_and_pad_channels_are_zero():
    x = K.torch_input((37, 53), seed=3, B=2)
    for size in ((50, 91), (37, 53), (20, 30)):
        a, b = R.resample(x, size, False), R.resample(x, size, True)
        assert np.array_equal(b.view(np.uint32), a[:, :, ::-1].view(np.uint32))
    assert np.array_equal(R.resample(x, (37, 53), True), x[:, :, ::-1])                # the same size: an exact mirror
    p = R.resample_f32_packed(x, (50, 91), True)
    assert p.shape == (2, 50, 91, 4) and not p[..., 3].any() and np.array_equal(p[..., :3], R.resample(x, (50, 91), True))
    bits = R.bf16_bits(x)
    q = R.resample_bf16_packed(bits, (50, 91))
    assert q.shape == (2, 50, 91, 8) and q.dtype == np.uint16 and not q[..., 3:].any()
    # bf16: exact widening, round to nearest even
    assert R.bf16_bits(np.float32([1.0, 1.00390625, 1.01171875, -1.00390625, 1.005])).tolist() == [0x3f80, 0x3f80, 0x3f82, 0xbf80, 0x3f81]
    assert np.array_equal(R.bf16_bits(R.bf16_widen(bits)), bits)


def test_non_finite_taps_propagate_as_the_header_says():
    inf = np.inf
    with np.errstate(all='ignore'):
        # 2 x 2 -> 4 x 4: output (1, 1) has fx = fy = 0.25 and all four taps; (0, 0) has fx = fy = 0 and reads (0, 0) four times
        for pos, want_11 in (((0, 0), 'nan'), ((0, 1), 'nan'), ((1, 0), 'nan'), ((1, 1), 'inf')):
            a = np.zeros((2, 2)); a[pos] = inf
            out = R.resample(_one(a), (4, 4))[0, :, :, 0]
            assert (np.isnan(out[1, 1]) if want_11 == 'nan' else out[1, 1] == inf), pos
        a = np.zeros((2, 2)); a[0, 0] = inf
        out = R.resample(_one(a), (4, 4))[0, :, :, 0]
        assert np.isnan(out[0, 0])                                      # Inf - Inf at the clamped corner, even with f = 0
        assert out[3, 3] == 0                                           # taps (1, 1) only: the Inf is not read
        a[0, 0] = np.nan
        assert np.isnan(R.resample(_one(a), (4, 4))[0, 1, 1, 0])


@pytest.mark.parametrize('hw,size', K.TORCH_CASES)
def test_restatement_against_torch_bilinear_within_the_derived_bound(hw, size):
    import torch
    import torch.nn.functional as F
    x = K.torch_input(hw, seed=0)
    ref = F.interpolate(torch.from_numpy(x).permute(0, 3, 1, 2).contiguous(), size=size, mode='bilinear', align_corners=False,
                        antialias=False).permute(0, 2, 3, 1).numpy()
    got = R.resample(x, size)
    p00, p01, p10, p11, fx, fy = R.taps(x, size)
    bnd = K.bound(p00, p01, p10, p11, hw[0], hw[1])
    # the floors agree: every coordinate that is not clamped stays further from an integer than the coordinate error
    for n_src, n_dst in ((hw[0], size[0]), (hw[1], size[1])):
        s = R.coords(n_src, n_dst).astype(np.float64)
        inner = (s >= 0) & (np.floor(s) < n_src - 1)
        assert inner.sum() >= n_dst - 2 and np.abs(s[inner] - np.rint(s[inner])).min() >= 1.0 / 6 - 1e-4 > 4 * K.U * n_src
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    ratio = float((err / bnd).max())
    print('%s -> %s: largest |ours - torch| = %.3g, largest ratio to the bound = %.3g (bound: median %.3g)'
          % (hw, size, err.max(), ratio, float(np.median(bnd))))
    assert bnd.min() > 0 and ratio <= 1.0
    assert err.max() > 0 or size[0] in (2 * hw[0], hw[0] // 2)     # (power-of-two ratios may agree exactly: every coordinate is exact)


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'effdet_resample.h')).read(), flags=re.S)


def test_signature_and_struct_match_the_header():
    from efficientdet.pytorch_amd import build, _lib
    h = _header()
    protos = re.findall(r'^([a-z][a-z ]*?)\s*\b(effdet_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', h, flags=re.M)
    assert [(r.strip(), n) for r, n, _ in protos] == [('int', 'effdet_resample_images')]
    params = [' '.join(p.split()) for p in protos[0][2].split(',')]
    assert params == ['const effdet_resample_t* p', 'effdet_stream_t stream'] and _lib.RESAMPLE_SIGNATURES == {'effdet_resample_images': 'i:ps'}
    others = [getattr(_lib, n) for n in dir(_lib) if n.endswith('SIGNATURES') and n != 'RESAMPLE_SIGNATURES']
    assert len(others) >= 13 and not any('effdet_resample_images' in t for t in others)
    # the struct, field by field in the header's order
    body = re.search(r'typedef struct \{(.*?)\}\s*effdet_resample_t;', h, flags=re.S).group(1)
    fields = []
    for decl in [d.strip() for d in body.split(';') if d.strip()]:
        typ, names = re.match(r'(const void\*|void\*|int|long long)\s+(.*)$', decl).groups()
        ct = {'const void*': C.c_void_p, 'void*': C.c_void_p, 'int': C.c_int, 'long long': C.c_longlong}[typ]
        fields += [(n.strip(), ct) for n in names.split(',')]
    assert fields == list(_lib.Resample._fields_), fields
    assert re.search(r'enum\s*\{\s*EFFDET_RESAMPLE_NCHW = 0,\s*EFFDET_RESAMPLE_NHWC = 1\s*\}', h) and (_lib.RESAMPLE_NCHW, _lib.RESAMPLE_NHWC) == (0, 1)
    build.build(verbose=False)
    f = _lib.require('effdet_resample_images').effdet_resample_images
    assert f.restype is C.c_int and list(f.argtypes) == [C.c_void_p, C.c_void_p]
    assert '-ffp-contract=off' in build.PER_FILE['resample.hip']    # three separately rounded blend steps: no FMA contraction
    assert _lib.ABI_VERSION == 11 and 'effdet_resample_images' not in _lib.SIGNATURES
    src = open(os.path.join(ROOT, 'efficientdet', 'pytorch_amd', 'csrc', 'resample.hip')).read()
    assert '#include "resize_u8.h"' in src and 'lin_axis_ratio(' in src and 'floorf' not in src           # the axis rule is included, not restated
    doc = open(os.path.join(ROOT, 'include', 'effdet_resample.h')).read()
    for phrase in ('rounded ONCE', 'NO antialiasing', 'round-to-nearest-even', 'nothing contracted', 'resample first, then', 'Inf tap', 'written as +0'):
        assert phrase in doc, phrase


def test_refusals_are_decided_on_the_host_and_launch_nothing():
    from efficientdet.pytorch_amd import build, _lib
    build.build(verbose=False)
    f = _lib.require('effdet_resample_images').effdet_resample_images
    buf = np.zeros(4096, dtype=np.uint8)
    p = buf.ctypes.data + (-buf.ctypes.data) % 16

    def desc(**kw):
        d = _lib.Resample()
        d.src, d.dst, d.src_layout, d.dtype, d.B, d.H, d.W, d.Ho, d.Wo, d.C, d.flip, d.src_ld, d.src_bstride = p, p, 1, 0, 2, 8, 8, 4, 4, 4, 0, 4, 256
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    assert f(None, None) == -1
    for kw in (dict(src=None), dict(dst=None), dict(dst=p + 4), dict(dst=p + 8)):
        assert f(C.byref(desc(**kw)), None) == -1, kw
    for kw in (dict(src_layout=2), dict(src_layout=-1), dict(dtype=2), dict(dtype=-1), dict(src_layout=0, dtype=1), dict(flip=2), dict(flip=-1),
               dict(B=0), dict(B=65536), dict(H=0), dict(W=0), dict(Ho=0), dict(Wo=0), dict(H=32769), dict(W=32769), dict(Ho=32769),
               dict(Wo=32769), dict(C=2), dict(src_ld=3), dict(src_bstride=-1)):
        assert f(C.byref(desc(**kw)), None) == -3, kw
    assert not buf.any()


def test_tta_options_with_scales():
    from efficientdet.pytorch_amd import ops
    t = ops.TTAOptions()
    # the default is what it was: key, repr, hash, equality
    assert t.scales == () and t.key() == (True, None, (0.55, 0.0, 'avg', 1000)) and hash(t) == hash((True, None, (0.55, 0.0, 'avg', 1000)))
    assert repr(t) == "TTAOptions(hflip=True, weights=None, fusion=WBFOptions(iou_thr=0.55, skip_box_thr=0.0, conf_type='avg', top_n=1000))"
    assert t == ops.TTAOptions(True) == ops.TTAOptions(scales=()) == ops.TTAOptions(scales=[]) and t.num_views == 2
    assert ops.TTAOptions(weights=(1, 2)).key() == (True, (1.0, 2.0), (0.55, 0.0, 'avg', 1000))
    f = ops.WBFOptions(top_n=600)
    s = ops.TTAOptions(scales=(0.5, 1.5), fusion=f)
    assert s.scales == (0.5, 1.5) and s.num_views == 6 and s.key() == (True, None, f.key(), (0.5, 1.5)) and 'scales=(0.5, 1.5)' in repr(s)
    assert s == ops.TTAOptions(True, None, f, (0.5, 1.5)) and hash(s) == hash(ops.TTAOptions(scales=[0.5, 1.5], fusion=f))
    assert s != ops.TTAOptions(scales=(1.5, 0.5), fusion=f) and s != ops.TTAOptions(fusion=f) and s != ops.TTAOptions(scales=(0.5,), fusion=f)
    assert ops.TTAOptions(hflip=False, scales=(0.5,)).num_views == 2 and ops.TTAOptions(hflip=False, scales=(0.5, 2, 3, 4, 5, 6, 7), fusion=ops.WBFOptions(top_n=512)).num_views == 8
    assert ops.TTAOptions(scales=(0.5, 1.5, 2.0), fusion=ops.WBFOptions(top_n=512)).num_views == 8
    assert ops.TTAOptions(hflip=False, scales=(2.0,), weights=(1, 3)).weights == (1.0, 3.0)
    for bad, match in ((dict(scales=(1.0,)), 'scale of 1'), (dict(scales=(0.5, 1)), 'scale of 1'), (dict(scales=(0.5, 0.5)), 'distinct'),
                       (dict(scales=(float('nan'),)), 'positive and finite'), (dict(scales=(float('inf'),)), 'positive and finite'),
                       (dict(scales=(0.0,)), 'positive and finite'), (dict(scales=(-0.5,)), 'positive and finite'),
                       (dict(scales=(0.5, 1.5, 2.0, 3.0), fusion=ops.WBFOptions(top_n=100)), r'10 views .* limit of 8'),
                       (dict(hflip=False, scales=(2, 3, 4, 5, 6, 7, 8, 9), fusion=ops.WBFOptions(top_n=100)), r'9 views .* limit of 8'),
                       (dict(scales=(0.5, 1.5)), r'<= 4096, got 6 \* 1000'), (dict(hflip=False, scales=(0.5,), fusion=ops.WBFOptions(top_n=2049)), r'got 2 \* 2049'),
                       (dict(scales=(0.5,), weights=(1, 1)), '2 weights for 4 views')):
        with pytest.raises(ValueError, match=match):
            ops.TTAOptions(**bad)


def test_tta_view_plan():
    from efficientdet.pytorch_amd import ops
    two_thirds = float(np.float32(2.0 / 3.0))
    plan = ops.tta_view_plan(256, 256, ops.TTAOptions(hflip=True, scales=(0.5, 1.5), fusion=ops.WBFOptions(top_n=600)))
    assert plan == [(256, 256, False, 1.0, 1.0), (256, 256, True, 1.0, 1.0), (128, 128, False, 2.0, 1.0), (128, 128, True, 2.0, 1.0),
                    (384, 384, False, two_thirds, 1.0), (384, 384, True, two_thirds, 1.0)]
    assert two_thirds != 2.0 / 3.0
    plan = ops.tta_view_plan(256, 384, ops.TTAOptions(hflip=False, scales=(2.0,), weights=(3, 0.5)))
    assert plan == [(256, 384, False, 1.0, 3.0), (512, 768, False, 0.5, 0.5)]
    assert ops.tta_view_plan(128, 128, ops.TTAOptions()) == [(128, 128, False, 1.0, 1.0), (128, 128, True, 1.0, 1.0)]
    assert ops.tta_view_plan(100, 100, ops.TTAOptions(hflip=False)) == [(100, 100, False, 1.0, 1.0)]      # the base view takes any size
    assert ops.tta_view_plan(384, 384, ops.TTAOptions(hflip=False, scales=(1.0 / 3.0,)))[1][:2] == (128, 128)   # whole within 1e-6
    for H, W, s in ((256, 256, 0.75), (256, 384, 0.5), (256, 256, 0.25), (256, 256, 1.0001), (384, 256, 1.5)):
        with pytest.raises(ValueError, match=r'H = %d, W = %d at scale s = %s' % (H, W, re.escape(repr(float(s))))):
            ops.tta_view_plan(H, W, ops.TTAOptions(hflip=False, scales=(s,)))
    with pytest.raises(TypeError):
        ops.tta_view_plan(256, 256, None)


def test_model_detections_refuses_a_bad_scale_before_any_launch():
    from efficientdet.pytorch_amd import ops

    class Model:
        tta_options = ops.TTAOptions(hflip=False, scales=(0.75,))

        def forward_raw(self, images):
            raise AssertionError('a view was run')
    with pytest.raises(ValueError, match='multiples of 128'):
        ops.model_detections(Model(), object(), 256, 256)


def test_ensemble_scales_validate_without_a_device():
    from efficientdet.pytorch_amd import EfficientDet, evaluate
    m = EfficientDet(3, is_training=False)
    assert evaluate.EnsembleDetector([m, m]).scales is None and evaluate.EnsembleDetector([m, m], scales=None).scales is None
    assert evaluate.EnsembleDetector([m, m], scales=(None, 1.0)).scales is None and evaluate.EnsembleDetector([m, m], scales=[1, 1]).scales is None
    assert evaluate.EnsembleDetector([m, m], weights=(1, 1), scales=(None, 0.5)).scales == (None, 0.5)
    assert evaluate.EnsembleDetector([m, m, m], scales=(1.25, 1, 2)).scales == (1.25, None, 2.0)
    for bad, match in ((dict(scales=(0.5,)), '1 scales for 2 members'), (dict(scales=(None, 0.5, 2.0)), '3 scales for 2 members'),
                       (dict(scales=()), '0 scales for 2 members'), (dict(scales=(0.0, None)), 'positive and finite'),
                       (dict(scales=(None, float('nan'))), 'positive and finite'), (dict(scales=(float('inf'), 1)), 'positive and finite')):
        with pytest.raises(ValueError, match=match):
            evaluate.EnsembleDetector([m, m], **bad)
    e = evaluate.EnsembleDetector([m, m], scales=(None, 0.75))

    class NoLaunch:
        shape = (2, 3, 256, 256)
    with pytest.raises(ValueError, match=r'EnsembleDetector: H = 256, W = 256 at scale s = 0.75'):
        e.detections(NoLaunch(), 256, 256)
