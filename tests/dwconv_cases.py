"""Multi-tile workgroup runs of the depthwise kernels (csrc/dwconv.hip): the case table, its float64 reference, and the benchmark
geometries the table has to cover.  Shared by tests/test_dwconv_cases_host.py (CPU) and tests/test_gpu_dwconv_runs.py (GPU).

A workgroup of the forward, data-gradient, weight-gradient, fused-backward and fused expand->depthwise kernels walks a run of `ppt`
consecutive tiles of one image.  The planner gives ppt > 1 only from ~2048 workgroups up (weight gradient: ~768; fused backward: a
cost loop over 768 / 512 resident workgroups), so the shapes here are the smallest that get there -- which is why they are two orders
of magnitude larger than those of tests/test_gpu_backbone_ops.py, whose tables plan ppt = 1 and keep the single-tile paths.

Every case carries the class it is meant to reach per kernel family, (CQ, nbuf, ppt, ragged):
    CQ      16-byte channel chunks per slab: 4 or 8 (with k, stride and the element type: the template instance)
    nbuf    2 = the next tile is prefetched into a second LDS buffer under the taps, 1 = restaged behind an extra barrier
    ppt     tiles per workgroup
    ragged  tiles per image % ppt != 0: the last run of an image is shorter (t1 = min(tpi, t0 + ppt))
tests/test_dwconv_cases_host.py holds them against effdet_dwconv_plan_info, i.e. against the planner the launches use.

Shapes: H / W leave partial edge tiles in both directions for the forward tile (16 x 8 outputs at stride 1, 8 x 8 at stride 2) and the
data-gradient tile (16 x 8 inputs, 16 x 16 at stride 2); the stride-2 maps are even, so TF-"same" pads asymmetrically (k3: 0 | 1,
k5: 1 | 2); C = 228 / 456 end in a slab with a single live chunk, C = 40 / 144 / 672 in a partial one.
"""
import collections
import functools
import json
import os
import re

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16 = torch.float32, torch.bfloat16
FAMILIES = ('fwd', 'dgrad', 'wgrad')

Case = collections.namedtuple('Case', 'B H W C k s dtype pre expect')
BwdCase = collections.namedtuple('BwdCase', 'B H W C k s expect')
ExpandCase = collections.namedtuple('ExpandCase', 'B H W Cin k s expect')


def _c(B, H, W, C, k, s, dtype, fwd, dgrad, wgrad, pre=False):
    return Case(B, H, W, C, k, s, dtype, pre, {'fwd': fwd, 'dgrad': dgrad, 'wgrad': wgrad})


# forward / data gradient / weight gradient: every instance (k, stride, CQ, element type) with ppt >= 2 and a ragged last run in all
# three families.  pre=True: also run with in_act = SWISH from the pre-activation (two nbuf = 2 and two nbuf = 1 forward instances).
RUN_CASES = [
    # fp32, 8-chunk slabs
    _c(9, 72, 100, 240, 3, 1, F32, (8, 2, 2, True), (8, 2, 2, True), (8, 1, 6, True), pre=True),
    _c(9, 72, 100, 240, 5, 1, F32, (8, 2, 2, True), (8, 2, 2, True), (8, 1, 6, True)),
    _c(8, 360, 40, 228, 3, 2, F32, (8, 2, 2, True), (8, 2, 2, True), (8, 1, 5, True)),
    _c(8, 360, 40, 228, 5, 2, F32, (8, 1, 2, True), (8, 2, 2, True), (8, 1, 5, True), pre=True),     # forward: two tiles > 80 KiB
    # fp32, 4-chunk slabs (the stride-2 one runs 3 / 3 / 9 tiles per workgroup)
    _c(9, 104, 196, 40, 3, 1, F32, (4, 2, 2, True), (4, 2, 2, True), (4, 1, 6, True)),
    _c(9, 104, 196, 40, 5, 1, F32, (4, 2, 2, True), (4, 2, 2, True), (4, 1, 6, True)),
    _c(8, 264, 260, 40, 3, 2, F32, (4, 2, 3, True), (4, 2, 3, True), (4, 1, 9, True)),
    _c(8, 264, 260, 40, 5, 2, F32, (4, 2, 3, True), (4, 2, 3, True), (4, 1, 9, True)),
    # bf16, 8-chunk slabs (stride 2: the forward restages one buffer for k3 and k5)
    _c(6, 40, 196, 672, 3, 1, BF16, (8, 2, 2, True), (8, 2, 2, True), (8, 1, 6, True)),
    _c(6, 40, 196, 672, 5, 1, BF16, (8, 2, 2, True), (8, 2, 2, True), (8, 1, 6, True)),
    _c(8, 360, 40, 456, 3, 2, BF16, (8, 1, 2, True), (8, 2, 2, True), (8, 1, 5, True), pre=True),
    _c(8, 360, 40, 456, 5, 2, BF16, (8, 1, 2, True), (8, 2, 2, True), (8, 1, 5, True)),
    # bf16, 4-chunk slabs
    _c(5, 200, 100, 144, 3, 1, BF16, (4, 2, 2, True), (4, 2, 2, True), (4, 1, 5, True)),
    _c(5, 200, 100, 144, 5, 1, BF16, (4, 2, 2, True), (4, 2, 2, True), (4, 1, 5, True), pre=True),
    _c(5, 200, 196, 144, 3, 2, BF16, (4, 2, 2, True), (4, 2, 2, True), (4, 1, 5, True)),
    _c(5, 200, 196, 144, 5, 2, BF16, (4, 2, 2, True), (4, 2, 2, True), (4, 1, 5, True)),
]

# One tile per workgroup, where the benchmark takes a single-tile class that the tables of tests/test_gpu_backbone_ops.py do not: the
# LDS weight gradient of bf16 k3 / stride 2 at 8-chunk slabs (their bf16 k3 / stride-2 cases are a 4-chunk one and two on the direct
# kernel; D4 @ 1024 runs it at 16 x 16 x 1632).  It runs through the same tests as the runs above.
SINGLE_TILE_CASES = [
    _c(2, 20, 12, 64, 3, 2, BF16, (8, 1, 1, False), (8, 1, 1, False), (8, 1, 1, False)),
]

# fused data + weight gradient (fp32): its 8 instances at the smallest maps whose cost loop picks ppt = 2 with a ragged last run (the
# separate kernels still plan one tile per workgroup there, except the weight gradient of the last), and one run of 3 tiles
BWD_CASES = [
    BwdCase(4, 68, 100, 40, 3, 1, (4, 2, 2, True)), BwdCase(5, 84, 52, 64, 3, 1, (8, 2, 2, True)),
    BwdCase(4, 196, 68, 40, 3, 2, (4, 2, 2, True)), BwdCase(4, 36, 100, 144, 3, 2, (8, 2, 2, True)),
    BwdCase(5, 68, 52, 40, 5, 1, (4, 2, 2, True)), BwdCase(5, 20, 52, 144, 5, 1, (8, 2, 2, True)),
    BwdCase(5, 68, 100, 40, 5, 2, (4, 2, 2, True)), BwdCase(4, 68, 100, 64, 5, 2, (8, 2, 2, True)),
    BwdCase(8, 68, 100, 40, 3, 1, (4, 2, 3, True)),
]

# fused expand -> depthwise forward (fp32, 32-channel slabs, one tile buffer): the four (k, stride) pairs, one Cin = 16 / 24 / 32 / 40
# (4 / 6 / 8 / 10 MFMA k-steps) each
EXPAND_CASES = [
    ExpandCase(8, 100, 196, 16, 3, 1, (8, 1, 2, True)), ExpandCase(5, 196, 196, 24, 3, 2, (8, 1, 2, True)),
    ExpandCase(4, 100, 196, 32, 5, 1, (8, 1, 2, True)), ExpandCase(8, 68, 196, 40, 5, 2, (8, 1, 2, True)),
]


def case_id(c):
    dt = ('-' + str(c.dtype).replace('torch.', '')) if hasattr(c, 'dtype') else ''
    return '%dx%dx%dx%d-k%ds%d%s' % (c.B, c.H, c.W, c.C if hasattr(c, 'C') else c.Cin, c.k, c.s, dt)


def tf_same(n, k, s):
    """TF-'same' padding of one dimension -> (pad before, pad after, outputs)."""
    o = -(-n // s)
    total = max((o - 1) * s + k - n, 0)
    return total // 2, total - total // 2, o


def geometry(c):
    """-> (H, W, C, k, stride, pad_t, pad_l, Ho, Wo) of a case: the arguments the entry points take behind (dtype, B)."""
    (pt, _, Ho), (pl, _, Wo) = tf_same(c.H, c.k, c.s), tf_same(c.W, c.k, c.s)
    return (c.H, c.W, c.C if hasattr(c, 'C') else 6 * c.Cin, c.k, c.s, pt, pl, Ho, Wo)


def plan(kind, c, B=None):
    """The library's own plan for a case (ops.dwconv_plan_info: no device work); B overrides the batch."""
    from efficientdet.pytorch_amd import ops
    return ops.dwconv_plan_info(kind, getattr(c, 'dtype', F32), c.B if B is None else B, *geometry(c), Cin=getattr(c, 'Cin', 0))


def reached(info):
    """(CQ, nbuf, ppt, ragged) of a plan: the form the cases are tagged in."""
    return (info['cq'], info['nbuf'], info['ppt'], info['tpi'] % info['ppt'] != 0)


def plan_class(kind, dtype, k, s, info):
    """The class of a planned launch for the closure over the benchmark geometries."""
    return (kind, str(dtype).replace('torch.', ''), k, s, info['cq'], info['nbuf'], info['ppt'] > 1, bool(info['direct']))


# ----------------------------------------------------------------------------- float64 reference
def pad_same(x, k, s):
    (pt, pb, _), (pl, pr, _) = tf_same(x.shape[2], k, s), tf_same(x.shape[3], k, s)
    return F.pad(x, [pl, pr, pt, pb])


def dwconv64(x, w, k, s):
    """Depthwise conv of the explicitly TF-'same'-padded NCHW float64 x with w [C][1][k][k]."""
    return F.conv2d(pad_same(x, k, s), w, None, s, 0, 1, x.shape[1])


def dwconv64_transposed(dz, w, k, s, H, W):
    """sum over taps of dz * w back onto the H x W input (the data gradient of dwconv64; used on absolute values for the bound)."""
    full = F.conv_transpose2d(dz, w, None, s, 0, 0, dz.shape[1])           # (Ho - 1) s + k rows = H + both pads (or fewer: unused tail)
    pt, pl = tf_same(H, k, s)[0], tf_same(W, k, s)[0]
    full = F.pad(full, [0, max(0, pl + W - full.shape[3]), 0, max(0, pt + H - full.shape[2])])
    return full[:, :, pt:pt + H, pl:pl + W]


def naive_dwconv(x, w, k, s):
    """Nested loops over every output element and tap: what dwconv64 is checked against on tiny shapes."""
    B, C, H, W = x.shape
    (pt, _, Ho), (pl, _, Wo) = tf_same(H, k, s), tf_same(W, k, s)
    out = torch.zeros(B, C, Ho, Wo, dtype=torch.float64)
    for b in range(B):
        for c in range(C):
            for ho in range(Ho):
                for wo in range(Wo):
                    acc = 0.0
                    for kh in range(k):
                        for kw in range(k):
                            h, ww = ho * s + kh - pt, wo * s + kw - pl
                            if 0 <= h < H and 0 <= ww < W:
                                acc += float(x[b, c, h, ww]) * float(w[c, 0, kh, kw])
                    out[b, c, ho, wo] = acc
    return out


def swish64(t):
    return t * torch.sigmoid(t)


def swish_grad64(t):
    sg = torch.sigmoid(t)
    return sg * (1 + t * (1 - sg))


Reference = collections.namedtuple('Reference', 'x w scale shift dz zprev z y dx g dsum z_abs dx_abs')


def inputs(c, seed=1):
    """fp32 operands of a case, NCHW on the CPU: x and dz and zprev already rounded to the storage type."""
    g = torch.Generator().manual_seed(seed)
    q = (lambda t: t.to(c.dtype).float())
    (_, _, Ho), (_, _, Wo) = tf_same(c.H, c.k, c.s), tf_same(c.W, c.k, c.s)
    x = q(torch.randn(c.B, c.C, c.H, c.W, generator=g))
    w = torch.randn(c.C, 1, c.k, c.k, generator=g) * (2.0 / (c.k * c.k)) ** 0.5
    scale = 0.5 + torch.rand(c.C, generator=g)
    shift = torch.randn(c.C, generator=g) * 0.2
    dz = q(torch.randn(c.B, c.C, Ho, Wo, generator=g))
    zprev = q(torch.randn(c.B, c.C, c.H, c.W, generator=g))
    return x, w, scale, shift, dz, zprev


def reference(c, seed=1):
    """float64 on the CPU: z = scale * dwconv(x, w) + shift, y = swish(z), and by autograd of sum(z * dz): dx, g = dw / scale (the
    unscaled rows [k*k][C] the kernels leave), dsum.  z_abs / dx_abs: the same sums on absolute values, the scale of the error bounds."""
    x, w, scale, shift, dz, zprev = inputs(c, seed)
    xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
    sd, hd, dzd = scale.double().view(1, -1, 1, 1), shift.double().view(1, -1, 1, 1), dz.double()
    z = dwconv64(xd, wd, c.k, c.s) * sd + hd
    z.backward(dzd)
    with torch.no_grad():
        z = z.detach()
        g = (wd.grad / scale.double().view(-1, 1, 1, 1)).reshape(c.C, c.k * c.k).t().contiguous()
        z_abs = dwconv64(x.double().abs(), w.double().abs(), c.k, c.s) * sd.abs() + hd.abs()
        dx_abs = dwconv64_transposed(dzd.abs(), (w.double() * scale.double().view(-1, 1, 1, 1)).abs(), c.k, c.s, c.H, c.W)
    return Reference(x, w, scale, shift, dz, zprev, z, swish64(z), xd.grad, g, dzd.sum(dim=(0, 2, 3)), z_abs, dx_abs)


def value_bound(c, scale_abs, ref):
    """Per-element bound of forward z / data gradient dx against float64.  fp32 arithmetic: k*k FMAs, one scale and one shift (the data
    gradient: one rounding of w * scale instead) -- the first-order bound is (k*k + 2) u times the same sum on absolute values, u =
    2^-24; 2 (k*k + 3) u leaves a factor 2 over it.  bf16 storage rounds the fp32 result once more, to 8 significant bits: at most
    2^-8 of its magnitude, so + 2^-8 |ref|, the exact unit roundoff (the 2^-8 of the fp32 error it adds on top is second order and
    sits in the factor 2 of the first term; a kernel that truncated instead of rounding to nearest would show at twice the bound)."""
    b = 2.0 * (c.k * c.k + 3) * 2.0 ** -24 * scale_abs
    return b + 2.0 ** -8 * ref.abs() if c.dtype == BF16 else b


# ----------------------------------------------------------------------------- the benchmark geometries
def benchmark_configs():
    """(backbone, batch per device, image size) of the GPU configs of BASELINE.json, each in both storage types."""
    from efficientdet.pytorch_amd.config import MODEL_MAP
    out = []
    for line in json.load(open(os.path.join(ROOT, 'BASELINE.json')))['configs']:
        if 'MI355X' not in line:
            continue                                                         # the CPU plumbing config launches nothing
        net = 'efficientdet-d%s' % re.search(r'EfficientDet-D(\d)', line).group(1)
        m = re.search(r'batch (\d+) @ (\d+)', line)
        batch, size = int(m.group(1)), int(m.group(2))
        n = re.search(r'on (\d+)×MI355X', line)
        if 'global batch' in line:
            batch //= int(n.group(1))
        out += [(MODEL_MAP[net], batch, size, dt) for dt in (F32, BF16)]
    return sorted(set(out), key=str)


@functools.lru_cache(None)
def benchmark_geometries():
    """Every depthwise geometry of those configs: (dtype, B, H, W, Cexp, k, stride, pad_t, pad_l, Ho, Wo, Cin), walked with
    config.backbone_plan / conv_out like tests/test_host_logic.py::test_depthwise_planning_entry_points.  Cin = 0 for the blocks without
    an expand conv, which the fused expand -> depthwise forward cannot serve."""
    from efficientdet.pytorch_amd.config import backbone_plan, conv_out
    geos = []
    for backbone, batch, size, dt in benchmark_configs():
        _, stem_pad, blocks, _, _ = backbone_plan(backbone)
        hw = conv_out(size, 3, 2, stem_pad)
        for b in blocks:
            ho = conv_out(hw, b.k, b.stride, b.pad)
            geos.append((dt, batch, hw, hw, b.cexp, b.k, b.stride, b.pad[0], b.pad[0], ho, ho, b.cin if b.expand != 1 else 0))
            hw = ho
    return sorted(set(geos), key=str)
