"""Helpers shared by the host-only (no GPU) tests."""


def wgrad_desc(dtype, B, cin, cout, sizes, k=1, stride=1, pad=0, ldx=None, lddz=None, image_splits=0, want_bias=True, separate=False):
    """effdet_wgrad_t over fake device pointers (planning entry points do no device work).  separate: every level in its own
    'allocation' (offsets from a common base, 4 KiB apart beyond the tensor), as the grouped BiFPN launch passes them."""
    from efficientdet.pytorch_amd import _lib as L
    d = L.WgradDesc()
    d.x, d.dz, d.dw = 0x10000000, 0x50000000, None
    d.dbias = 1 if want_bias else None
    d.dtype, d.B, d.Cin, d.Cout, d.KH, d.KW, d.stride, d.pad_t, d.pad_l = dtype, B, cin, cout, k, k, stride, pad, pad
    d.ldx, d.lddz, d.nseg, d.image_splits = ldx or cin, lddz or cout, len(sizes), image_splits
    ox = oz = 0
    for i, (h, w) in enumerate(sizes):
        s = d.seg[i]
        ho, wo = (h + stride - 1) // stride, (w + stride - 1) // stride
        s.H, s.W, s.Ho, s.Wo = h, w, ho, wo
        s.in_off, s.in_bstride, s.out_off, s.out_bstride = ox, h * w * d.ldx, oz, ho * wo * d.lddz
        ox += B * h * w * d.ldx + (1024 * (i + 1) if separate else 0)
        oz += B * ho * wo * d.lddz + (1024 * (i + 1) if separate else 0)
    return d
