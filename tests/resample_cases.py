"""Cases of the model-input resampler (include/effdet_resample.h), shared by the CPU tier (tests/test_resample_host.py) and the GPU
tier (tests/test_gpu_resample.py).

1. TORCH_CASES: the restatement against torch's CPU F.interpolate(mode='bilinear', align_corners=False, antialias=False).

   The two are not bit-equal, for two reasons, and the bound is derived from them -- nothing in it is fitted to an observed figure.

   (a) The source coordinate.  Ours is ((double)o + 0.5) * ((double)n_src / (double)n_dst) - 0.5 rounded ONCE to fp32: off the exact
       s by at most u |s|, u = 2^-24.  torch forms scale = (float)n_src / n_dst (relative error <= u), t = scale * (o + 0.5)
       (exact product off by <= u (s + 0.5), rounded: another u (s + 0.5)), then t - 0.5 (rounded: u |s|).  Both coordinates are
       therefore within
           e_axis = 4 u n_src = 2^-22 n_src
       of each other (s + 0.5 <= n_src for every output index).  Where both clamp (s < 0, or floor(s) >= n_src - 1) both read the
       edge pixel alone, and the value does not depend on the coordinate.
       The blend is a piecewise-linear, continuous function of (sx, sy); inside one cell its slope along x is a convex mix of
       p01 - p00 and p11 - p10 and along y of p10 - p00 and p11 - p01, so moving the coordinates by (ex, ey) moves the value by at
       most (ex + ey) * D, D = the largest absolute difference between two adjacent taps of that pixel.  Where the two floors differ
       by one the coordinates lie on either side of a cell border, within e_axis of it; the function is continuous there, and the
       sizes below never come near one: their coordinates are o / 2 - 1 / 4, 2 o + 1 / 2 and (4 o - 1) / 6, at least 1 / 6 from an
       integer (the test asserts it from the restatement's own coordinates), so the floors are the same and D is the same cell's.
   (b) The blend form.  Ours is three steps p + f * (q - p); torch weights the taps, h0 * (w0 * p00 + w1 * p01) + h1 * (w0 * p10 + w1 *
       p11) with w0 = 1 - w1.  With M = the largest |tap| of the pixel, every intermediate of either form is at most 2 M, and every
       operation rounds by at most u times its result.  Ours: q - p <= 2 u M, times f <= 2 u M more, the sum u M: 5 u M for top and
       for bot; bot - top carries 10 u M and adds 2 u M, the product 2 u M, the last sum 5 u M + u M: 20 u M.  torch's: w0 off by u,
       each product u M (+ u M for w0), the row sum u M: <= 4 u M per row; times h (u M for h0, u M for the product): 6 u M; two rows
       and the last sum: 13 u M.  Together 33 u M; the bound takes
           e_blend = 40 u M.
       It scales with the taps, not with the result: a result that cancels to nearly zero still carries the rounding of its taps.

   bound(pixel) = (e_axis(W) + e_axis(H)) * D + e_blend.

2. GPU_CASES: what tests/test_gpu_resample.py runs, bit for bit against the restatement.  The launch grid is NOT capped -- one thread
   per output pixel, grid (ceil(Ho * Wo / 256), B) -- so there is no second round of a cap to reach; the cases with Ho * Wo no multiple
   of 256 ('odd_*') end in a partly filled workgroup, and every case has more than one workgroup per image and B = 2.
   Fields: name, src ('nchw' | 'f32' | 'bf16': NCHW fp32 tensor, PackedImages fp32, PackedImages bf16), (H, W), (Ho, Wo), flip, and
   for a PackedImages source its map (C, ld, off, gap): channels, pixel stride, offset of the map inside its arena and elements between
   the images, all in elements -- (CE, CE, 0, 0) is the dense tensor; `path` names the loads the kernel takes for it."""
import numpy as np

U = 2.0 ** -24


def bound(p00, p01, p10, p11, H, W):
    """The per-pixel bound of section 1 from the restatement's taps [B, Ho, Wo, 3] -> float64 [B, Ho, Wo, 3]."""
    t = [np.asarray(p, dtype=np.float64) for p in (p00, p01, p10, p11)]
    D = np.max([np.abs(t[1] - t[0]), np.abs(t[3] - t[2]), np.abs(t[2] - t[0]), np.abs(t[3] - t[1])], axis=0)
    M = np.max([np.abs(x) for x in t], axis=0)
    return (4 * U * W + 4 * U * H) * D + 40 * U * M


TORCH_CASES = (((128, 128), (256, 256)), ((256, 256), (128, 128)), ((256, 256), (384, 384)), ((128, 256), (256, 512)))


def torch_input(hw, seed=0, B=1):
    """Seeded uniform in [-2.5, 2.5], channels last [B, H, W, 3] float32."""
    return np.random.RandomState(seed).uniform(-2.5, 2.5, size=(B,) + tuple(hw) + (3,)).astype(np.float32)


def _case(name, src, hw, out, flip, layout=None, path=None):
    ce = {'nchw': 3, 'f32': 4, 'bf16': 8}[src]
    return dict(name=name, src=src, hw=hw, out=out, flip=flip, layout=layout or (ce, ce, 0, 0),
                path=path or ('planes' if src == 'nchw' else 'vector'))


GPU_CASES = [
    _case('nchw_256_128', 'nchw', (256, 256), (128, 128), False),
    _case('nchw_256_384_flip', 'nchw', (256, 256), (384, 384), True),
    _case('nchw_128x256_256x512', 'nchw', (128, 256), (256, 512), False),
    _case('f32_256_128_flip', 'f32', (256, 256), (128, 128), True),
    _case('f32_256_384', 'f32', (256, 256), (384, 384), False),
    _case('f32_128x256_256x512_flip', 'f32', (128, 256), (256, 512), True),
    _case('bf16_256_128', 'bf16', (256, 256), (128, 128), False),
    _case('bf16_256_384_flip', 'bf16', (256, 256), (384, 384), True),
    _case('bf16_128x256_256x512', 'bf16', (128, 256), (256, 512), False),
    # an arena slice with a non-zero offset (aligned: still one 16-byte load per tap) and room between the images
    _case('f32_arena_slice', 'f32', (256, 256), (128, 128), False, (4, 4, 64, 32)),
    _case('bf16_arena_slice_flip', 'bf16', (256, 256), (384, 384), True, (8, 8, 24, 8)),
    # strided pixels: ld > C, aligned
    _case('f32_strided', 'f32', (37, 53), (50, 91), False, (4, 8, 16, 0)),
    _case('bf16_strided', 'bf16', (37, 53), (50, 91), True, (8, 16, 8, 0)),
    # maps that the vector loads cannot take: an offset or a pixel stride off the alignment, or only three channels in memory
    _case('odd_f32_unaligned_off', 'f32', (37, 53), (50, 91), True, (4, 4, 6, 0), 'element'),
    _case('odd_f32_ld5', 'f32', (37, 53), (50, 91), False, (4, 5, 0, 3), 'element'),
    _case('odd_f32_three_channels', 'f32', (37, 53), (50, 91), False, (3, 3, 0, 0), 'element'),
    _case('odd_bf16_unaligned_off', 'bf16', (37, 53), (50, 91), False, (8, 8, 3, 0), 'element'),
    _case('odd_bf16_ld9', 'bf16', (37, 53), (50, 91), True, (8, 9, 0, 5), 'element'),
    _case('odd_nchw', 'nchw', (37, 53), (50, 91), True),
    # the same size mirrored: every fx and fy is 0 and the result is the exact mirror image
    _case('nchw_mirror_only', 'nchw', (128, 128), (128, 128), True),
    # a one-row and a one-column source: every tap of an axis is the same element
    _case('f32_one_row', 'f32', (1, 40), (128, 128), False),
    _case('bf16_one_column', 'bf16', (40, 1), (128, 128), True),
]


def arena_layout(c, B=2):
    """-> (arena elements, bstride): image b of the case's map starts at off + b * bstride."""
    C, ld, off, gap = c['layout']
    H, W = c['hw']
    bstride = H * W * ld + gap
    return off + B * bstride, bstride


def vector_path(c):
    """What csrc/resample.hip decides for the case's map in a 16-byte aligned arena (`path` of the cases restates it): one load of
    four elements per tap needs a fourth channel in memory and the base and both strides on that load's alignment."""
    C, ld, off, gap = c['layout']
    return C >= 4 and off % 4 == 0 and ld % 4 == 0 and arena_layout(c)[1] % 4 == 0


def source(c, seed, B=2):
    """The case's input, channels last: float32 values [B, H, W, 3] (for 'bf16' exactly representable in bfloat16)."""
    x = torch_input(c['hw'], seed, B)
    if c['src'] == 'bf16':
        from tests import resample_restated as R
        x = R.bf16_widen(R.bf16_bits(x))
    return x
