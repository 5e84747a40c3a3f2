"""GPU: ops.resample_images against the NumPy restatement of include/effdet_resample.h (tests/resample_restated.py), bit for bit, every
output element, for every case of tests/resample_cases.GPU_CASES (B = 2): the three kinds of source, down- and upscales, a
non-square size, the mirror, arena slices, strided and unaligned maps, one-row and one-column sources.  The output of every case lies
between two guard regions of a sentinel that must be untouched, and its pad channels must be +0.  Non-finite taps, the Python-level
refusals, and the eager / captured agreement follow."""
import numpy as np
import pytest
import torch

from tests import resample_cases as K
from tests import resample_restated as R

pytestmark = pytest.mark.gpu
GUARD = 1024                     # bytes of sentinel on either side of the output
SENTINEL = 0xA5


def _bf16_tensor(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(torch.bfloat16)


def _device_source(c, x):
    """The case's source on the device from channels-last values x [B, H, W, 3] -> an NCHW tensor or a PackedImages over an arena."""
    from efficientdet.pytorch_amd import PackedImages, ops
    B, (H, W) = x.shape[0], c['hw']
    if c['src'] == 'nchw':
        return torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2))).cuda()
    Cc, ld, off, gap = c['layout']
    n, bstride = K.arena_layout(c, B)
    host = np.full(n, 7.0, dtype=np.float32)                    # what lies between the pixels is never a tap: a value that would show
    for b in range(B):
        img = host[off + b * bstride: off + b * bstride + H * W * ld].reshape(H * W, ld)
        img[:, :Cc] = 9.0                                       # channels past the third are read at most, never used
        img[:, :3] = x[b].reshape(H * W, 3)
    arena = torch.from_numpy(host).cuda() if c['src'] == 'f32' else _bf16_tensor(R.bf16_bits(host)).cuda()
    return PackedImages(ops.Map(arena, B, H, W, Cc, ld=ld, bstride=bstride, off=off))


def _run(c, src, B=2):
    """resample_images into a map between two guard regions -> (the output's bytes as [B, Ho, Wo, ce] uint32 / uint16, the result)."""
    from efficientdet.pytorch_amd import ops
    dtype = torch.bfloat16 if c['src'] == 'bf16' else torch.float32
    ce, isz = (8, 2) if c['src'] == 'bf16' else (4, 4)
    Ho, Wo = c['out']
    n = B * Ho * Wo * ce
    raw = torch.full((2 * GUARD + n * isz,), SENTINEL, dtype=torch.uint8, device='cuda')
    arena = raw.view(dtype)
    out = ops.Map(arena, B, Ho, Wo, ce, off=GUARD // isz)
    res = ops.resample_images(src, (Ho, Wo), c['flip'], out=out)
    torch.cuda.synchronize()
    host = raw.cpu().numpy()
    assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + n * isz:] == SENTINEL).all(), 'a guard region was written'
    assert res.map is out and tuple(res.shape) == (B, 3, Ho, Wo) and res.dtype == dtype
    return host[GUARD:GUARD + n * isz].view(np.uint16 if isz == 2 else np.uint32).reshape(B, Ho, Wo, ce)


@pytest.mark.parametrize('c', K.GPU_CASES, ids=[c['name'] for c in K.GPU_CASES])
def test_resample_equals_the_restatement_bit_for_bit(c):
    x = K.source(c, seed=11)
    got = _run(c, _device_source(c, x))
    if c['src'] == 'bf16':
        want = R.resample_bf16_packed(R.bf16_bits(x), c['out'], c['flip'])
    else:
        want = R.resample_f32_packed(x, c['out'], c['flip']).view(np.uint32)
    assert not got[..., 3:].any()                                # pad channels: +0, bit for bit
    bad = got != want
    assert not bad.any(), '%s: %d of %d elements differ, first at %s' % (c['name'], bad.sum(), bad.size, np.argwhere(bad)[0].tolist())
    if c['name'] == 'nchw_mirror_only':
        assert np.array_equal(got[..., :3].view(np.float32), x[:, :, ::-1])


def test_allocated_output_is_the_stem_layout_and_equals_the_guarded_run():
    from efficientdet.pytorch_amd import ops
    by = {c['name']: c for c in K.GPU_CASES}
    for name in ('nchw_256_384_flip', 'bf16_256_128'):
        c = by[name]
        x = K.source(c, seed=11)
        src = _device_source(c, x)
        res = ops.resample_images(src, c['out'], c['flip'])
        m = res.map
        ce = 8 if c['src'] == 'bf16' else 4
        assert (m.B, m.H, m.W, m.C, m.ld, m.bstride, m.off) == (2, c['out'][0], c['out'][1], ce, ce, c['out'][0] * c['out'][1] * ce, 0)
        assert m.t.is_contiguous() and m.t.data_ptr() % 16 == 0
        raw = m.t.view(torch.int16 if ce == 8 else torch.int32).cpu().numpy().view(np.uint16 if ce == 8 else np.uint32)
        assert np.array_equal(raw, _run(c, src))


def test_non_finite_taps_propagate_as_the_restatement():
    c = K._case('nonfinite', 'f32', (16, 24), (40, 36), False)
    x = K.source(c, seed=5)
    x[0, 3, 4, 0] = np.inf; x[0, 9, 20, 1] = -np.inf; x[1, 0, 0, 2] = np.nan; x[1, 15, 23, 0] = np.inf; x[1, 7, 7, :] = np.inf
    got = _run(c, _device_source(c, x))[..., :3].view(np.float32)
    want = R.resample(x, c['out'])
    assert np.isnan(want).sum() > 20 and np.isinf(want).sum() > 0
    assert np.array_equal(np.isnan(got), np.isnan(want))         # sign and payload of a NaN are not part of the contract
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32))


def test_python_level_refusals():
    from efficientdet.pytorch_amd import PackedImages, ops
    img = torch.zeros(2, 3, 128, 128, device='cuda')
    with pytest.raises(ValueError, match='size of the batch'):
        ops.resample_images(img, (128, 128))
    with pytest.raises(ValueError, match='size of the batch'):
        ops.resample_images(PackedImages(ops.Map.of(torch.zeros(2, 128, 128, 4, device='cuda'))), (128, 128), flip=False)
    with pytest.raises(TypeError, match='float32'):
        ops.resample_images(img.to(torch.bfloat16), (256, 256))
    with pytest.raises(TypeError, match='float32'):
        ops.resample_images(img.half(), (256, 256))
    with pytest.raises(TypeError):
        ops.resample_images(torch.zeros(2, 4, 128, 128, device='cuda'), (256, 256))
    with pytest.raises(TypeError, match='float32 or bfloat16'):
        ops.resample_images(PackedImages(ops.Map.of(torch.zeros(2, 128, 128, 8, device='cuda', dtype=torch.float16))), (256, 256))
    with pytest.raises(ValueError, match='contiguous'):
        ops.resample_images(torch.zeros(2, 128, 128, 3, device='cuda').permute(0, 3, 1, 2), (256, 256))
    with pytest.raises(ValueError, match='out must be'):
        ops.resample_images(img, (256, 256), out=ops.Map.new(2, 256, 256, 8, torch.float32, 'cuda'))
    with pytest.raises(RuntimeError, match='EFFDET_EUNSUPPORTED'):
        ops.resample_images(PackedImages(ops.Map.of(torch.zeros(2, 128, 128, 2, device='cuda'))), (256, 256))


def test_captured_resample_replays_bit_equal():
    from efficientdet.pytorch_amd import ops
    x = torch.from_numpy(K.torch_input((128, 128), seed=2, B=2).transpose(0, 3, 1, 2).copy()).cuda()
    eager = ops.resample_images(x, (256, 256), True).map.t.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = ops.resample_images(x, (256, 256), True)
    for _ in range(2):
        res.map.t.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(res.map.t, eager)
