"""NumPy restatement of the model-input resampler (include/effdet_resample.h: effdet_resample_images): the axis rule with its float64
coordinate rounded once to float32, the three blend steps in np.float32 in the header's order (IEEE subtract, multiply, add; NumPy
contracts nothing), the mirror applied to the finished result, bf16 as exact widening and round-to-nearest-even.  The device must
equal it bit for bit, every output element.

Hand-derived pins (tests/test_resample_host.py checks them):

  2 x 2 -> 4 x 4, source [[0, 4], [8, 12]].  ratio = 0.5, s = (o + 0.5) / 2 - 0.5 = -0.25, 0.25, 0.75, 1.25.  o = 0: floor -1 < 0, so
    i0 = 0, f = 0.  o = 1: i0 = 0, f = 0.25.  o = 2: i0 = 0, f = 0.75.  o = 3: floor 1 >= n - 1, so i0 = 1, f = 0.  Along x the top row
    gives 0, 0 + 0.25 * 4 = 1, 0 + 0.75 * 4 = 3, 4 and the bottom row 8, 9, 11, 12; along y the same weights between them:
        [[0, 1, 3, 4], [2, 3, 5, 6], [6, 7, 9, 10], [8, 9, 11, 12]]
  4 x 4 -> 2 x 2, source arange(16).  ratio = 2, s = 2 o + 0.5 = 0.5, 2.5: i0 = 0 and 2, f = 0.5.  Each output is the mean of a 2 x 2
    block: (0 + 1 + 4 + 5) / 4 = 2.5, (2 + 3 + 6 + 7) / 4 = 4.5, (8 + 9 + 12 + 13) / 4 = 10.5, (10 + 11 + 14 + 15) / 4 = 12.5.
  1 x 8 -> 1 x 2, source arange(8).  ratio = 4, s = 1.5, 5.5: taps (1, 2) and (5, 6), outputs 1.5 and 5.5 -- the pixels 0, 3, 4, 7 are
    never read: no antialiasing.
  An edge-clamped row: 1 x 4 -> 3 x 4 (H = 1: every i0 >= n - 1 = 0, so y0 = y1 = 0 and fy = 0) repeats the row three times.
  A 1-pixel-wide source: 4 x 1 -> 4 x 3 repeats the column three times.
"""
import numpy as np

f32 = np.float32


def axis(n_src, n_dst):
    """-> (i0 [n_dst] int64, i1 [n_dst] int64, f [n_dst] float32): lin_axis_ratio of csrc/resize_u8.h for every output index."""
    o = np.arange(n_dst, dtype=np.float64)
    s = ((o + 0.5) * (np.float64(n_src) / np.float64(n_dst)) - 0.5).astype(f32)           # float64 throughout, rounded once
    fl = np.floor(s)
    i0 = fl.astype(np.int64)
    f = s - fl.astype(f32)
    lo = i0 < 0
    i0[lo] = 0; f[lo] = 0
    hi = i0 >= n_src - 1
    i0[hi] = n_src - 1; f[hi] = 0
    return i0, np.minimum(i0 + 1, n_src - 1), f.astype(f32)


def coords(n_src, n_dst):
    """The fp32 source coordinate of every output index before the clamps (for the tests' reasoning about floors)."""
    o = np.arange(n_dst, dtype=np.float64)
    return ((o + 0.5) * (np.float64(n_src) / np.float64(n_dst)) - 0.5).astype(f32)


def taps(x, size):
    """x [B, H, W, 3] float32 -> (p00, p01, p10, p11 [B, Ho, Wo, 3], fx [1, 1, Wo, 1], fy [1, Ho, 1, 1])."""
    x = np.ascontiguousarray(x, dtype=f32)
    Ho, Wo = size
    y0, y1, fy = axis(x.shape[1], Ho)
    x0, x1, fx = axis(x.shape[2], Wo)
    ra, rb = x[:, y0], x[:, y1]
    return ra[:, :, x0], ra[:, :, x1], rb[:, :, x0], rb[:, :, x1], fx.reshape(1, 1, Wo, 1), fy.reshape(1, Ho, 1, 1)


def resample(x, size, flip=False):
    """x [B, H, W, 3] float32 (channels last) -> [B, Ho, Wo, 3] float32."""
    p00, p01, p10, p11, fx, fy = taps(x, size)
    with np.errstate(all='ignore'):
        top = p00 + fx * (p01 - p00)
        bot = p10 + fx * (p11 - p10)
        out = top + fy * (bot - top)
    assert out.dtype == f32
    return np.ascontiguousarray(out[:, :, ::-1]) if flip else out          # resample first, then mirror


def bf16_bits(v):
    """float32 -> bfloat16 bit patterns (uint16), round to nearest even (finite values and infinities)."""
    b = np.ascontiguousarray(v, dtype=f32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7fff + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_widen(bits):
    """bfloat16 bit patterns (uint16) -> the float32 values they stand for, exactly."""
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(f32)


def packed(out, ce):
    """[B, Ho, Wo, 3] -> the stem layout [B, Ho, Wo, ce]: the pad channels are +0."""
    full = np.zeros(out.shape[:3] + (ce,), dtype=out.dtype)
    full[..., :3] = out
    return full


def resample_f32_packed(x, size, flip=False):
    """The device's fp32 output for channels-last fp32 input x: [B, Ho, Wo, 4] float32."""
    return packed(resample(x, size, flip), 4)


def resample_bf16_packed(bits, size, flip=False):
    """The device's bf16 output for channels-last bf16 input given as bit patterns [B, H, W, 3] uint16: [B, Ho, Wo, 8] uint16."""
    return packed(bf16_bits(resample(bf16_widen(bits), size, flip)), 8)
