"""Dense-conv launches beyond one round of workgroups (csrc/conv_igemm.hip): the case table, its float64 reference and its error bounds.
Shared by tests/test_conv_plan_cases_host.py (CPU) and tests/test_gpu_conv_large.py (GPU).

plan_conv picks the kernel instance from the problem size, and the op-level tables of tests/test_gpu_conv.py, test_gpu_split.py,
test_gpu_hsplit.py and test_gpu_sparse_reg_grad.py are small enough that it never picks what the benchmark runs there:
  * the persistent kernels launch min(tiles, compute units) workgroups and a workgroup walks tiles b, b + workgroups, ...; with at most
    16 tiles no workgroup ever takes a second one, so the hand-over (the next tile's addressing and first DMA stages issued ahead of the
    finished tile's epilogue, which runs on the saved tile coordinates) never executes, let alone into another pyramid level;
  * the 128-pixel-tile kernel's two-stage instances at 128 / 64 channels are taken from 257 tiles up, its four-stage ones between 129
    and 256 -- below that a long K loop goes to the narrow 32-channel tile -- so their steady state only ever ran 1-5 K-steps;
  * the flagged launch of the split-layout kernel deals pixel tiles out in groups of eight; with 9 pixel tiles only group 0 exists.
Every case carries the class it is meant to reach, (arith, tile_m, tile_n, stages, persistent), and the least K-steps / walk rounds it
must have; tests/test_conv_plan_cases_host.py holds them against effdet_conv2d_plan_info, i.e. against the plan the launch reads.

All cases are 3x3 'same' convs over NHWC maps in the head's level-major pyramid buffers, with bias and ReLU or no activation (the
flagged launches: neither, the kernel takes flags only then).
"""
import collections
import contextlib

import torch
import torch.nn.functional as F

F32, BF16 = torch.float32, torch.bfloat16
MI355X_CUS = 256                                       # compute units of the device the walking cases are sized for
PYRAMID = [(64 >> i, 64 >> i) for i in range(5)]        # the head's levels at a 512 x 512 input

# arith: 'f32' exact fp32 | 'bf16' | 'bf16x3' fp32 storage split in registers | 'split' split-layout operands | 'hsplit' the f16x3 form
# out:   'same' (the operand's own storage: fp32, bf16, split layout, H-split layout) | 'f32' plain fp32 rows from a bf16 / split form
# mask:  ReLU-mask residual (the forward activation in the output's layout)        flagged: also run with per-tile liveness flags
# tune:  tuning knobs (name of _lib.TUNE_* -> value) the case needs; big: the persistent bf16 variant it asks of the big_igemm fixture
Case = collections.namedtuple('Case', 'name B sizes Cin Cout arith out act bias mask flagged tune big expect min_ksteps min_rounds')


def _c(name, B, sizes, Cin, Cout, arith, expect, out='same', act=1, bias=True, mask=False, flagged=False, tune=None, big=0,
       min_ksteps=18, min_rounds=0):
    return Case(name, B, sizes, Cin, Cout, arith, out, act, bias, mask, flagged, tune or {}, big, expect, min_ksteps, min_rounds)


def _big(v):
    return {'TUNE_IGEMM_BIG': v, 'TUNE_IGEMM_BIG_MIN_M': 0}


CASES = [
    # (a) 128-pixel tile, two stages, 128 channels: 133 x 2 = 266 tiles (> 256), a partial last pixel tile, 18 K-steps
    _c('a-f32', 2, [(92, 92)], 64, 256, 'f32', ('f32', 128, 128, 2, False)),
    _c('a-bf16', 2, [(92, 92)], 128, 256, 'bf16', ('bf16', 128, 128, 2, False), act=0),
    _c('a-bf16x3', 2, [(92, 92)], 64, 256, 'bf16x3', ('bf16x3', 128, 128, 2, False)),
    _c('a-f32-cout200', 2, [(92, 92)], 64, 200, 'f32', ('f32', 128, 128, 2, False), act=0),       # partial channel tile (128 + 72)
    # (b) the same kernel at 64 channels: 265 tiles
    _c('b-f32', 2, [(130, 130)], 64, 64, 'f32', ('f32', 128, 64, 2, False), act=0),
    _c('b-bf16', 2, [(130, 130)], 128, 64, 'bf16', ('bf16', 128, 64, 2, False)),
    _c('b-bf16x3', 2, [(130, 130)], 64, 64, 'bf16x3', ('bf16x3', 128, 64, 2, False)),
    # (c) four stages with a long K loop: 134 / 133 tiles (more than the 128 that go to the narrow tile, at most 256)
    _c('c128-f32', 1, [(92, 92)], 64, 256, 'f32', ('f32', 128, 128, 4, False)),
    _c('c128-bf16x3', 1, [(92, 92)], 64, 256, 'bf16x3', ('bf16x3', 128, 128, 4, False), act=0),
    _c('c64-f32', 1, [(130, 130)], 64, 64, 'f32', ('f32', 128, 64, 4, False)),
    _c('c64-bf16x3', 1, [(130, 130)], 64, 64, 'bf16x3', ('bf16x3', 128, 64, 4, False), act=0),
    # (d) persistent split-layout kernel over the head's pyramid in one grouped launch: 171 x 3 = 513 tiles = 2 * 256 + 1, the last
    # channel tile 208 wide; then split-layout output under a ReLU mask: 278 x 2 = 556 tiles, the last channel tile 64 wide
    _c('d-split-f32out', 8, PYRAMID, 256, 720, 'split', ('split', 256, 256, 2, True), out='f32', act=0, min_ksteps=72, min_rounds=3),
    _c('d-split-mask', 13, PYRAMID, 256, 320, 'split', ('split', 256, 256, 2, True), act=0, mask=True, tune={'TUNE_SPLIT_PERS': 1},
       min_ksteps=72, min_rounds=3),
    # (e) persistent bf16 kernels over the same pyramid: the default planner's own choice at 70928 pixels, then each variant by knob
    _c('e-442-default', 13, PYRAMID, 256, 720, 'bf16', ('bf16', 256, 256, 2, True), min_ksteps=36, min_rounds=3),
    _c('e-442', 8, PYRAMID, 256, 720, 'bf16', ('bf16', 256, 256, 2, True), tune=_big(442), big=442, min_ksteps=36, min_rounds=3),
    _c('e-242', 8, PYRAMID, 256, 720, 'bf16', ('bf16', 128, 256, 2, True), tune=_big(242), big=242, min_ksteps=36, min_rounds=3),
    _c('e-243', 8, PYRAMID, 256, 720, 'bf16', ('bf16', 128, 256, 3, True), out='f32', act=0, tune=_big(243), big=243, min_ksteps=36,
       min_rounds=3),
    _c('e-423', 8, PYRAMID, 256, 720, 'bf16', ('bf16', 256, 128, 3, True), tune=_big(423), big=423, min_ksteps=36, min_rounds=3),
    # (f) split-layout and f16x3 128-pixel kernels, one launch of more than 256 tiles over the five levels each; the split-layout ones
    # dense and flagged (171 and 341 pixel tiles: 21 / 42 whole groups of eight and a tail of 3 / 5)
    _c('f-split128-flagged', 4, PYRAMID, 256, 256, 'split', ('split', 128, 128, 2, False), act=0, bias=False, mask=True, flagged=True,
       min_ksteps=72),
    _c('f-split64-flagged', 8, PYRAMID, 256, 64, 'split', ('split', 128, 64, 2, False), out='f32', act=0, bias=False, flagged=True,
       min_ksteps=72),
    _c('f-hsplit128', 4, PYRAMID, 64, 256, 'hsplit', ('hsplit', 128, 128, 2, False)),
    _c('f-hsplit64', 8, PYRAMID, 64, 64, 'hsplit', ('hsplit', 128, 64, 2, False), act=0),
]

# every class (a)-(f) ask for: (arith, tile_m, tile_n, stages, persistent)
REQUIRED_CLASSES = {
    ('f32', 128, 128, 2, False), ('bf16', 128, 128, 2, False), ('bf16x3', 128, 128, 2, False),                      # a
    ('f32', 128, 64, 2, False), ('bf16', 128, 64, 2, False), ('bf16x3', 128, 64, 2, False),                         # b
    ('f32', 128, 128, 4, False), ('bf16x3', 128, 128, 4, False), ('f32', 128, 64, 4, False), ('bf16x3', 128, 64, 4, False),      # c
    ('split', 256, 256, 2, True),                                                                                  # d
    ('bf16', 256, 256, 2, True), ('bf16', 128, 256, 2, True), ('bf16', 128, 256, 3, True), ('bf16', 256, 128, 3, True),          # e
    ('split', 128, 128, 2, False), ('split', 128, 64, 2, False), ('hsplit', 128, 128, 2, False), ('hsplit', 128, 64, 2, False),  # f
}


def case_id(c):
    return c.name


def storage_dtype(c):
    return BF16 if c.arith == 'bf16' else F32


def out_dtype(c):
    return F32 if c.out == 'f32' else storage_dtype(c)


def out_kind(c):
    """How the output values are stored: 'f32', 'bf16', 'split' (bf16 hi | lo) or 'hsplit' (f16 hi | scaled lo)."""
    if c.out == 'f32' or c.arith in ('f32', 'bf16x3'):
        return 'f32'
    return c.arith


@contextlib.contextmanager
def tuned(c):
    """The case's tuning knobs and arithmetic for the launches (and plan queries) inside; what was there before is put back."""
    from efficientdet.pytorch_amd import ops, _lib as L
    old = [(k, ops.tuning_set(getattr(L, k), v)) for k, v in c.tune.items()]
    arith = ops.set_f32_arith('bf16x3' if c.arith in ('bf16x3', 'split') else 'f32')
    try:
        yield
    finally:
        ops.set_f32_arith(arith)
        for k, v in reversed(old):
            ops.tuning_set(getattr(L, k), v)


def conv_kwargs(c, shift=None, res=None, live=None):
    kw = dict(Cin=c.Cin, Cout=c.Cout, KH=3, KW=3, pad_t=1, pad_l=1, act=c.act, shift=shift, out_f32=c.out == 'f32' and c.arith != 'f32',
              split=c.arith == 'split', hsplit=c.arith == 'hsplit', live=live)
    if c.mask:
        kw.update(res=res, res_mode=2)                                     # RES_RELU_MASK
    return kw


def plan(c, device='cpu'):
    """The library's own plan for a case (ops.conv2d_plan_info on the descriptor ops.conv2d would launch; no device work: the buffers
    only lend their addresses)."""
    from efficientdet.pytorch_amd import ops, functional as Fn
    _, xm = Fn.pyramid_alloc(c.B, c.sizes, c.Cin, storage_dtype(c), device)
    _, ym = Fn.pyramid_alloc(c.B, c.sizes, c.Cout, out_dtype(c), device)
    rm = Fn.pyramid_alloc(c.B, c.sizes, c.Cout, out_dtype(c), device)[1] if c.mask else None
    wp = torch.empty(c.Cout * 9 * c.Cin + c.Cout, dtype=storage_dtype(c), device=device)
    shift = torch.empty(c.Cout, device=device) if c.bias else None
    with tuned(c):
        return ops.conv2d_plan_info(xm, wp, ym, **conv_kwargs(c, shift, rm))


def reached(c, info):
    """(arith, tile_m, tile_n, stages, persistent) of a plan: the form the cases are tagged in."""
    arith = {'plain': 'bf16' if c.arith == 'bf16' else 'f32'}.get(info['form'], info['form'])
    return (arith, info['tile_m'], info['tile_n'], info['stages'], info['persistent'])


# ----------------------------------------------------------------------------- the persistent kernels' tile walk
def xcd_remap(bid, nwg):
    """common.h xcd_remap: the bijection of [0, nwg) that hands each of the 8 XCDs a contiguous range of logical tiles."""
    q, r = nwg >> 3, nwg & 7
    xcd, idx = bid & 7, bid >> 3
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + idx


def level_of_tile(c, info, tile):
    """Pyramid level of a logical tile (channel tile fastest, levels back to back in units of tile_m pixels)."""
    mt, start = tile // info['ntiles'], 0
    for lvl, (h, w) in enumerate(c.sizes):
        start += -(-c.B * h * w // info['tile_m'])
        if mt < start:
            return lvl
    raise AssertionError('tile %d beyond the launch' % tile)


def walk(c, info, cus):
    """Per workgroup of a persistent launch on a device of `cus` compute units: the levels of the tiles it walks, in order."""
    total = info['mtiles'] * info['ntiles']
    grid = min(total, cus)
    return [[level_of_tile(c, info, xcd_remap(t, total)) for t in range(b, total, grid)] for b in range(grid)]


def walk_facts(c, info, cus):
    """-> dict: rounds (most tiles one workgroup walks), remainder (tiles % cus), partial_n (last channel tile narrower than tile_n),
    level_changes (workgroups with two consecutive tiles in different levels)."""
    runs = walk(c, info, cus)
    return {'rounds': max(len(r) for r in runs), 'remainder': (info['mtiles'] * info['ntiles']) % cus,
            'partial_n': c.Cout % info['tile_n'] != 0,
            'level_changes': sum(any(a != b for a, b in zip(r, r[1:])) for r in runs)}


# ----------------------------------------------------------------------------- the flagged launch's live map
def live_pixels(c):
    """Per level the [B, H, W] bool map of pixels that carry non-zero input channels in a flagged case: every fifth image, in bands of
    eight rows out of sixteen -- whole images dead, live and dead tiles side by side inside the others."""
    out = []
    for (h, w) in c.sizes:
        m = torch.zeros(c.B, h, w, dtype=torch.bool)
        rows = (torch.arange(h) // 8) % 2 == 0
        m[0::5] = rows.view(1, h, 1)
        out.append(m)
    return out


def tile_flags(c, pixels):
    """One byte per 128-pixel tile over all levels: 0 = every input tap of every pixel of the tile is zero (the non-zero pixels dilated by
    the 3x3 window's radius inside each image, then ORed over each run of 128 of the level's (b, h, w) pixel index)."""
    parts = []
    for m in pixels:
        dil = F.max_pool2d(m.float().unsqueeze(1), 3, 1, 1).reshape(-1) > 0
        n = -(-dil.numel() // 128)
        pad = torch.zeros(n * 128, dtype=torch.bool)
        pad[:dil.numel()] = dil
        parts.append(pad.view(n, 128).any(dim=1))
    return torch.cat(parts).to(torch.uint8)


def deal(mtiles, ntiles):
    """conv_igemm_kernel's round-robin deal of a flagged launch: workgroup -> (pixel tile, channel tile, group j or -1 for the tail past
    the last whole group of eight pixel tiles)."""
    whole = (mtiles >> 3) << 3
    out = []
    for b in range(mtiles * ntiles):
        if b < whole * ntiles:
            i = b >> 3
            j = i // ntiles
            out.append((j * 8 + (b & 7), i - j * ntiles, j))
        else:
            out.append((b // ntiles, b % ntiles, -1))
    return out


# ----------------------------------------------------------------------------- float64 reference
def conv64_unfold(x, w, bias, pads=(1, 1, 1, 1), stride=1):
    """x [B, H, W, Cin] and w [Cout, Cin, KH, KW] in float64 (any device), pads = (top, bottom, left, right) -> (ref, S), both
    [B, Ho, Wo, Cout]: ref = conv + bias as im2col (F.unfold) times the weight matrix, one image at a time; S = sum |x| |w| + |bias|, the
    same product on absolute values -- the scale of the error bounds."""
    Cout, Cin, KH, KW = w.shape
    pt, pb, pl, pr = pads
    w2 = w.reshape(Cout, Cin * KH * KW)
    b = bias if bias is not None else torch.zeros(Cout, dtype=x.dtype, device=x.device)
    refs, Ss = [], []
    for i in range(x.shape[0]):
        xp = F.pad(x[i:i + 1].permute(0, 3, 1, 2), [pl, pr, pt, pb])
        Ho, Wo = (xp.shape[2] - KH) // stride + 1, (xp.shape[3] - KW) // stride + 1
        cols = F.unfold(xp, (KH, KW), stride=stride)[0]                   # [Cin * KH * KW, Ho * Wo]
        refs.append((torch.addmm(b.view(-1, 1), w2, cols)).t().reshape(Ho, Wo, Cout))
        Ss.append((torch.addmm(b.abs().view(-1, 1), w2.abs(), cols.abs())).t().reshape(Ho, Wo, Cout))
    return torch.stack(refs), torch.stack(Ss)


def naive_conv(x, w, bias, pads=(1, 1, 1, 1), stride=1):
    """Nested loops over every output element, tap and channel: what conv64_unfold is checked against on tiny shapes."""
    B, H, W, Cin = x.shape
    Cout, _, KH, KW = w.shape
    pt, pb, pl, pr = pads
    Ho, Wo = (H + pt + pb - KH) // stride + 1, (W + pl + pr - KW) // stride + 1
    out = torch.zeros(B, Ho, Wo, Cout, dtype=torch.float64)
    for b in range(B):
        for ho in range(Ho):
            for wo in range(Wo):
                for n in range(Cout):
                    acc = float(bias[n]) if bias is not None else 0.0
                    for kh in range(KH):
                        for kw in range(KW):
                            h, ww = ho * stride + kh - pt, wo * stride + kw - pl
                            if 0 <= h < H and 0 <= ww < W:
                                for ci in range(Cin):
                                    acc += float(x[b, h, ww, ci]) * float(w[n, ci, kh, kw])
                    out[b, ho, wo, n] = acc
    return out


def conv64_cpu(x, w, bias, pads=(1, 1, 1, 1), stride=1):
    """F.conv2d in float64 on the explicitly padded input, NHWC in and out: the reference of the small cases."""
    pt, pb, pl, pr = pads
    return F.conv2d(F.pad(x.permute(0, 3, 1, 2), [pl, pr, pt, pb]), w, bias, stride).permute(0, 2, 3, 1)


def from_split64(t):
    """[..., C] fp32-typed tensor holding the split layout ([32 x bf16 hi | 32 x bf16 lo] per 32 channels) -> float64 values hi + lo."""
    C = t.shape[-1]
    raw = t.contiguous().view(torch.bfloat16).view(-1, C // 32, 2, 32).double()
    return (raw[:, :, 0] + raw[:, :, 1]).reshape(t.shape)


def from_hsplit64(t):
    """[..., C] fp32-typed tensor holding the H-split layout ([32 x f16 hi | 32 x f16 lo * 2^11]) -> float64 values hi + lo / 2^11."""
    C = t.shape[-1]
    raw = t.contiguous().view(torch.float16).view(-1, C // 32, 2, 32).double()
    return (raw[:, :, 0] + raw[:, :, 1] / 2048.0).reshape(t.shape)


def decode(c, t):
    kind = out_kind(c)
    return from_split64(t) if kind == 'split' else from_hsplit64(t) if kind == 'hsplit' else t.double()


# ----------------------------------------------------------------------------- bounds
U32, U_BF16 = 2.0 ** -24, 2.0 ** -8        # unit roundoffs: fp32 (24 significant bits), bf16 (8)
X3_PER_PRODUCT = 2.0 ** -14


def value_bound(c, S, ref):
    """Per-element bound of the conv output against float64, for operands as stored (bf16 cases: the bf16 values; split forms: the plain
    fp32 values the split was made from).  K = 9 * Cin products per output, S = sum |x| |w| + |bias| in float64.

    Accumulation, every form: the products enter an fp32 accumulator (exact-fp32 form: a chain of K fused multiply-adds; the bf16
    forms: exact 16-bit products, summed by the matrix pipe into fp32), then one bias add -- at most K + 1 roundings of at most
    u = 2^-24 of a partial sum that never exceeds S: first order (K + 1) u S.  2 (K + 3) u S leaves a factor 2 over it.  ReLU and the
    ReLU mask do not grow an error (|relu(a) - relu(b)| <= |a - b|), so the bound holds behind them with ref taken behind them.

    Storage of the result: bf16 rounds once more to 8 significant bits, + 2^-8 |ref| (exact unit roundoff; its product with the fp32
    error is second order and sits in the factor 2).  The split layout stores hi = bf16(v) and lo = bf16(v - hi): |v - hi| <= 2^-8 |v|
    and the second rounding leaves 2^-8 of that, + 2^-16 |ref|.

    Three-product forms (register split and split layout): an operand is x = xh + xl + ex with xh = bf16(x), xl = bf16(x - xh):
    |xl| <= 2^-8 (1 + 2^-8) |x|, |ex| <= 2^-16 |x|; likewise w.  The kernel sums xh wh + xh wl + xl wh
    = (x - ex)(w - ew) - xl wl = x w - x ew - ex w + ex ew - xl wl, so per product the error is at most
    (2^-16 + 2^-16 + 2^-32 + 2^-16 (1 + 2^-8)^2) |x| |w| < 3 * 2^-16 (1 + 2^-7) |x| |w| = 0.756 * 2^-14 |x| |w|: + 2^-14 S, the next power
    of two.  (Their accumulation stays inside the first term on the assumption that a matrix instruction rounds into the accumulator once
    per block of products it sums, not once per product: the three 16x16x32 instructions of 32 reduction elements, 8 products per lane
    and pass, then round 12 times where the chain of the exact form rounds 32 times.)"""
    K = 9 * c.Cin
    b = 2.0 * (K + 3) * U32 * S
    if c.arith in ('bf16x3', 'split'):
        b = b + X3_PER_PRODUCT * S
    kind = out_kind(c)
    if kind == 'bf16':
        b = b + U_BF16 * ref.abs()
    elif kind == 'split':
        b = b + 2.0 ** -16 * ref.abs()
    return b


# the f16x3 form has no simple per-element bound (its lo half is a scaled fp16 number with its own range): tests/test_gpu_hsplit.py's
# criterion for it -- at most twice as far from float64 as the exact-fp32 kernel, relative to the tensor's scale, plus the 22 bits of an
# H-split output; never beyond 3e-6 of the scale (K <= 2304); every element within 1e-4 of max(|ref|, 1e-2 max |ref|)
HSPLIT_VS_EXACT, HSPLIT_OUT_BITS, HSPLIT_SCALE_CAP, HSPLIT_ELEMENT_TOL = 2.0, 2.5e-7, 3e-6, 1e-4
