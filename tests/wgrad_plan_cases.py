"""Weight-gradient launches at multi-range split-K plans (csrc/conv_wgrad.hip): the case table, its float64 reference and its error bounds.
Shared by tests/test_wgrad_plan_cases_host.py (CPU) and tests/test_gpu_wgrad_plan_cases.py (GPU).

The planner cuts every pyramid level into ranges of `mchunk` pixels, one workgroup per (tile, range), and every workgroup writes its
partial tile into the slab of its range.  The op-level tables of tests/test_gpu_split.py, test_gpu_conv.py, test_gpu_wgrad_pair.py and
test_gpu_sparse_reg_grad.py either plan to one range per level, or compare a launch with another launch of the same kernel body, or
look at the sum of the slabs only -- where a pixel dropped from one range and counted in its neighbour cancels.  The cases here plan to
several ranges per level and every slab is held against a float64 reference of its own pixel range:
  * ranges that begin in the middle of an image (m_begin > 0 seeds the kernels' scalar pixel cursor) and, for odd widths, of a row;
  * ranges that cross an image boundary, the short last range of a level, later levels whose ranges start at split_start > 0;
  * ranges of more than 64 steps of 32 pixels: the flagged walk of the split-layout kernel refetches its 64-step flag window;
  * grids of more than one round of the 512 resident workgroups;
  * the paired launch's block map, with both problems' slabs in one caller-owned workspace that is NaN before the launch.
Every case carries the class it is meant to reach -- (arith, path, launches, form) -- and the facts its plan must have;
tests/test_wgrad_plan_cases_host.py holds them against effdet_conv2d_wgrad_plan_info, i.e. against the plan the launch reads.

Reference.  For a level with x [B, H, W, Cin] and dz [B, H, W, Cout] in float64 -- the operands AS STORED: the bf16 values of a bf16
case, the decoded hi + lo values of a split-layout case -- and a range [m0, m1) of the level's (b, h, w) pixel index,
    G[n][tap][c] = sum_m dz[m][n] x[pix(m) + tap][c],  bias[n] = sum_m dz[m][n],
    S[n][tap][c] = sum_m |dz[m][n]| |x[pix(m) + tap][c]|,  Sb[n] = sum_m |dz[m][n]|
one image at a time: the columns of F.unfold (im2col of the zero-padded image) restricted to the range's pixels of that image, times
the dz rows of the same pixels.  tests/test_wgrad_plan_cases_host.py checks it against nested loops.

Bounds (conv_plan_cases.value_bound's model and constants, with the pixel index as the reduction index).  A slab element is a sum of n
products (n = the pixels of its range) in an fp32 accumulator whose partial sums never exceed S: the exact-fp32 form is a chain of n
multiply-adds (at most 2 n roundings of u = 2^-24 if product and sum round separately), the bf16 forms sum exact 16-bit products in the
matrix pipe -- first order n u S, and 2 (n + 3) u S leaves a factor 2 over it.  The three-product forms (bf16x3 in registers, the split
layout) drop the lo * lo term and, in registers, what two bf16 halves cannot hold of an fp32 value: + 2^-14 S (value_bound's docstring
derives the constant).  bf16 products of bf16-stored operands are exact: nothing is added.  The unpacked gradient is the fp32 sum of
the slabs: at most M + nslabs roundings over all M pixels, 2 (M + nslabs + 3) u S with S over all pixels.  A bias row is the same sum
with every x = 1: the same formulas on Sb.  An element with S = 0 (every product an exact zero) must be exactly zero.
No bound is taken from a run of the kernels.  (Measured afterwards on an MI355X: every slab, bias row and unpacked gradient of every
case holds them; the worst slab sits at 0.19 of its bound -- a flagged range with one live pixel, where the whole error is the dropped
lo * lo term -- and the dense slabs at 0.01 - 0.16.)"""
import collections
import contextlib

import torch
import torch.nn.functional as F

from tests.conv_plan_cases import U32, X3_PER_PRODUCT, from_split64

F32, BF16 = torch.float32, torch.bfloat16
RESIDENT = 512                                         # workgroups resident at once on the device the planner plans for (2 x 256 CUs)

# kind:    'split' level-major pyramid buffers in the split layout | 'tiled' plain fp32 / bf16 storage
# arith:   'split' | 'f32' exact fp32 | 'bf16x3' fp32 storage split in registers | 'bf16'
# layout:  'pyramid' the levels of one level-major buffer, one shared weight | 'group' separately allocated levels, independent problems
#          (conv2d_wgrad(group=True)) | 'image' one map with image_splits
# forms:   the launches the GPU test makes: 'dense' | 'flagged' (live32) | 'pair-dense' | 'pair-flagged' (conv2d_wgrad_pair; problem b flagged)
# expect:  (arith, path, launches, layout-or-form class) -- see reached(); need: the facts of the plan, see facts()
Case = collections.namedtuple('Case', 'name kind B sizes Cin Cout lddz k arith layout forms launches need')

SPLIT3 = ('dense', 'flagged', 'pair-dense', 'pair-flagged')
S3, S5 = [(64, 64), (32, 32), (16, 16)], [(64, 64), (32, 32), (16, 16), (8, 8), (4, 4)]
D4 = [(32, 32), (16, 16), (8, 8), (4, 4)]
P5 = [(32, 32), (16, 16), (8, 8), (4, 4), (2, 2)]
P5_1 = [(32, 32), (16, 16), (8, 8), (4, 4), (1, 1)]     # the fp32 forms take 2 x 2 on the DMA-staged kernel: a 1 x 1 level instead


def _s(name, B, sizes, Cin, Cout, lddz, forms, **need):
    return Case(name, 'split', B, sizes, Cin, Cout, lddz, 3, 'split', 'pyramid', forms, 'fast', need)


def _t(name, B, sizes, Cin, Cout, k, arith, layout='pyramid', launches='fast', **need):
    return Case('%s-%s' % (name, arith), 'tiled', B, sizes, Cin, Cout, Cout, k, arith, layout, ('dense',), launches, need)


def _three(name, B, sizes, Cin, Cout, k, need32, need64, layout='pyramid', launches='fast', sizes32=None):
    """one case per arithmetic: exact fp32 and bf16x3 (32-pixel stages, fp32 elements) and bf16 (64-pixel stages)"""
    la = (launches,) * 3 if isinstance(launches, str) else launches
    return [_t(name, B, sizes32 or sizes, Cin, Cout, k, 'f32', layout, la[0], **need32),
            _t(name, B, sizes32 or sizes, Cin, Cout, k, 'bf16x3', layout, la[1], **need32),
            _t(name, B, sizes, Cin, Cout, k, 'bf16', layout, la[2], **need64)]


CASES = [
    # ---- split-layout kernel, 3x3 'same', level-major pyramid buffers
    # ranges of 84 steps (a second flag window), 10 + 3 + 1 ranges, a 12-step last range of level 0, 504 blocks
    _s('s-long', 6, S3, 256, 256, 256, SPLIT3, count=[10, 3, 1], mchunk=2688, stages=84, blocks=504, rounds=1, allr=True, partial=True,
       cross=True),
    # the regression output layer: 36 channels in a 64-wide row, one channel tile
    _s('s-reg', 6, S3, 256, 36, 64, SPLIT3, count=[20, 5, 2], mchunk=1280, stages=40, blocks=486, rounds=1, allr=True, partial=True,
       cross=True),
    # two rounds of workgroups over five levels
    _s('s-rounds', 7, S5, 256, 256, 256, ('dense',), count=[19, 5, 2, 1, 1], mchunk=1536, stages=48, blocks=1008, rounds=2, allr=True,
       partial=True, cross=True),
    # the other template instance (ALLR 0).  The planner takes it below 64 input channels (it compares the doubled channel count of the
    # bf16 view with 128), so the case has 32: a 64-channel pyramid plans to ALLR 1 like the cases above
    _s('s-d0', 5, D4, 32, 64, 64, SPLIT3, count=[9, 3, 1, 1], mchunk=576, stages=18, blocks=42, rounds=1, allr=False, partial=True,
       cross=True),
    # the classification output layer on the 64-channel pyramid: 720 channels in a 768-wide row, 6 channel tiles, the last one partial
    _s('s-cls', 3, D4, 64, 720, 768, ('dense',), count=[6, 2, 1, 1], mchunk=512, stages=16, blocks=300, rounds=1, allr=True, cross=True,
       partial_n=True),
    # rows of 24 and 40 pixels: ranges that start inside a row (ALLR 0 again)
    _s('s-odd', 3, [(20, 24), (6, 40)], 32, 64, 64, ('dense', 'flagged'), count=[3, 2], mchunk=576, allr=False, midrow=True, cross=True,
       partial=True),
] + _three(
    # ---- tiled kernels
    't-long', 6, S3, 256, 256, 3, dict(count=[10, 3, 1], mchunk=2688, stages=84, blocks=504, rounds=1, partial=True, cross=True),
    dict(count=[10, 3, 1], mchunk=2688, stages=42, blocks=504, rounds=1, partial=True, cross=True)
) + _three(
    # five levels; the last one goes to the register-transpose launch (nfast < splits)
    't-pyr', 5, P5, 64, 64, 3, dict(count=[18, 5, 2, 1, 1], slow_levels=[4], partial=True, cross=True),
    dict(count=[9, 3, 1, 1, 1], slow_levels=[4], partial=True, cross=True), launches='both', sizes32=P5_1
) + _three(
    # the BiFPN's grouped pointwise form: five separately allocated levels, each one long row, several ranges per level (bf16: the 20
    # pixels of the 2 x 2 level are no whole 8-pixel pieces and go to the register-transpose launch)
    't-bifpn', 5, P5, 64, 64, 1, dict(count=[15, 4, 1, 1, 1], slow_levels=[], partial=True, cross=True),
    dict(count=[6, 2, 1, 1, 1], slow_levels=[4], partial=True, cross=True), layout='group', launches=('fast', 'fast', 'both')
) + _three(
    # the backbone's widest project conv: per-image slabs, a second round of workgroups, two / one stage per range
    't-mb-rounds', 32, [(8, 8)], 1152, 192, 1, dict(count=[32], mchunk=64, stages=2, blocks=576, rounds=2, q=1),
    dict(count=[32], mchunk=64, stages=1, blocks=576, rounds=2, q=1), layout='image'
) + _three(
    # per-image slabs, several per image, two j tiles
    't-mb-q', 4, [(32, 32)], 240, 40, 1, dict(count=[16], q=4, jtiles=2), dict(count=[8], q=2, jtiles=2), layout='image'
) + _three(
    # 30-wide rows, 1080-pixel images: ranges start inside rows and cross images (bf16: rows of 30 are no whole 8-pixel pieces, the
    # register-transpose launch alone)
    't-odd', 3, [(36, 30)], 64, 64, 3, dict(count=[12], mchunk=288, stages=9, partial=True, cross=True, midrow=True),
    dict(count=[6], mchunk=576, stages=9, partial=True, cross=True, midrow=True), launches=('fast', 'fast', 'slow')
)

# every class the table is written for: (arith, path, launches, form)
REQUIRED_CLASSES = {('split', 'split', 'fast', f) for f in SPLIT3} | \
    {(a, 'tiled', 'fast', 'pyramid') for a in ('f32', 'bf16x3', 'bf16')} | \
    {(a, 'tiled', 'both', 'pyramid') for a in ('f32', 'bf16x3', 'bf16')} | \
    {('f32', 'tiled', 'fast', 'group'), ('bf16x3', 'tiled', 'fast', 'group'), ('bf16', 'tiled', 'both', 'group'),
     ('bf16', 'tiled', 'slow', 'pyramid')} | \
    {(a, 'tiled', 'fast', 'image') for a in ('f32', 'bf16x3', 'bf16')}

VARIANTS = [(c, f) for c in CASES for f in c.forms]


def case_id(c):
    return c.name


def variant_id(v):
    return '%s-%s' % (v[0].name, v[1])


def storage_dtype(c):
    return BF16 if c.arith == 'bf16' else F32


@contextlib.contextmanager
def tuned(c):
    """The case's arithmetic for the launches (and plan queries) inside; what was there before is put back."""
    from efficientdet.pytorch_amd import ops
    arith = ops.set_f32_arith('bf16x3' if c.arith in ('bf16x3', 'split') else 'f32')
    try:
        yield
    finally:
        ops.set_f32_arith(arith)


def wgrad_kwargs(c):
    pad = (c.k - 1) // 2
    return dict(Cin=c.Cin, Cout=c.Cout, KH=c.k, KW=c.k, pad_t=pad, pad_l=pad, split=c.kind == 'split', image_splits=c.layout == 'image')


def alloc(c, device):
    """-> (x maps, dz maps) of a case, uninitialised: level-major pyramid buffers, or (layout 'group') one allocation per level"""
    from efficientdet.pytorch_amd import functional as Fn
    from efficientdet.pytorch_amd.ops import Map
    dt = storage_dtype(c)
    if c.layout == 'group':
        return ([Map.new(c.B, h, w, c.Cin, dt, device) for h, w in c.sizes], [Map.new(c.B, h, w, c.lddz, dt, device) for h, w in c.sizes])
    return Fn.pyramid_alloc(c.B, c.sizes, c.Cin, dt, device)[1], Fn.pyramid_alloc(c.B, c.sizes, c.lddz, dt, device)[1]


def plan(c, device='cpu'):
    """The library's own plan for a case (ops.conv2d_wgrad_plan_info on the descriptor ops.conv2d_wgrad would launch; no device work: the
    buffers only lend their addresses)."""
    from efficientdet.pytorch_amd import ops
    xm, zm = alloc(c, device)
    with tuned(c):
        return ops.conv2d_wgrad_plan_info(xm, zm, **wgrad_kwargs(c))


def reached(c, info, form):
    """(arith, path, launches, form) of a plan: the form the cases are tagged in.  launches: 'fast' = one launch of the DMA-staged /
    split-layout kernel, 'both' = that and the register-transpose kernel, 'slow' = the latter alone."""
    launches = 'fast' if info['nfast'] == info['splits'] else 'both' if info['nfast'] > 0 else 'slow'
    return (c.arith, info['path'], launches, form if c.kind == 'split' else c.layout)


def level_pixels(c):
    return [c.B * h * w for h, w in c.sizes]


def ranges(c, info):
    """-> list over slabs (in slab order) of (level, m0, m1): slab first[l] + r holds level l's pixels [r mchunk, min(M_l, (r + 1) mchunk))"""
    out = [None] * info['splits']
    for l, M in enumerate(level_pixels(c)):
        for r in range(info['count'][l]):
            assert out[info['first'][l] + r] is None
            out[info['first'][l] + r] = (l, r * info['mchunk'], min(M, (r + 1) * info['mchunk']))
    assert all(o is not None for o in out)
    return out


def facts(c, info):
    """What the plan of a case looks like, in the words of the cases' `need`:
    count, mchunk, allr, jtiles   as planned
    stages      pipeline stages of a whole range (mchunk / stage_pixels, rounded up)
    blocks      workgroups (both launches of a tiled plan together); rounds: blocks in units of the 512 resident workgroups
    partial     the last range of level 0 is shorter than mchunk
    cross       a range holds pixels of two images
    midrow      a range starts inside an image row
    partial_n   the last channel tile is narrower than the tile
    slow_levels levels of the register-transpose launch
    q           image_splits: slabs per image"""
    tiles = info['ntiles'] * info['jtiles']
    rg = ranges(c, info)
    hw = [h * w for h, w in c.sizes]
    f = {'count': info['count'], 'mchunk': info['mchunk'], 'allr': info['allr'], 'jtiles': info['jtiles'],
         'stages': -(-info['mchunk'] // info['stage_pixels']),
         'blocks': tiles * info['splits'], 'rounds': -(-tiles * info['splits'] // RESIDENT),
         'partial': level_pixels(c)[0] % info['mchunk'] != 0,
         'cross': any((m1 - 1) // hw[l] != m0 // hw[l] for l, m0, m1 in rg),
         'midrow': any(m0 % c.sizes[l][1] != 0 for l, m0, m1 in rg),
         'partial_n': c.Cout % 128 != 0 and info['ntiles'] > 1,
         'slow_levels': [l for l in range(len(c.sizes)) if info['first'][l] >= info['nfast']],
         'q': info['count'][0] // c.B if c.layout == 'image' else 0}
    return f


def holds(need, f):
    """the facts a case declares, against facts(): -> list of the names that do not hold"""
    return [(k, v, f[k]) for k, v in need.items() if f[k] != v]


# ----------------------------------------------------------------------------- the pair kernel's block map
def eighth(n, x):
    """conv_wgrad_pair_kernel's eighth(): first block of XCD x in xcd_remap's partition of n blocks"""
    return x * (n >> 3) + min(x, n & 7)


def pair_block(bid, tiles, ntiles, splits, first, liveb):
    """conv_wgrad_pair_kernel's block -> (problem, channel tile, j tile, split) map.  tiles = ntiles * jtiles, splits = (a's, b's),
    first = the problem whose blocks come first, liveb: problem 1 carries flags (split-fastest, descending)."""
    grid = tiles * (splits[0] + splits[1])
    xcd, idx = bid & 7, bid >> 3
    f0 = eighth(tiles * splits[first], xcd)
    nf = eighth(tiles * splits[first], xcd + 1) - f0
    prob = first if idx < nf else first ^ 1
    l = f0 + idx if idx < nf else eighth(grid, xcd) - f0 + (idx - nf)
    if liveb and prob == 1:
        tile = l // splits[1]
        split = splits[1] - 1 - (l - tile * splits[1])
    else:
        split = l // tiles
        tile = l - split * tiles
    return prob, tile % ntiles, tile // ntiles, split


# ----------------------------------------------------------------------------- the flagged launches' live steps
def live_steps(c, info):
    """The 32-pixel steps of problem b that carry a non-zero dz pixel in a flagged launch: per level a sorted list of the level's own step
    indices.  By range r of n = mchunk / 32 steps (a short last range: what it has):
      level 0   r = 0: steps 0, 63, 64, 65 and the last (both sides of the 64-step flag window, where the range is that long)
                r = 1: one step past the first window (step 70, or the last but one of a shorter range): dead in steps 0-63
                r = 2: dead
                r = 3: every step
                the last range: its last step only; every other range: dead
      level l   r % 3 == 0: step 1 and the last one;  r % 3 == 1: every step;  r % 3 == 2: dead"""
    per = info['mchunk'] // 32
    out = []
    for l, M in enumerate(level_pixels(c)):
        live = []
        for r in range(info['count'][l]):
            n = min(per, -(-(M - r * info['mchunk']) // 32))
            if l == 0:
                if r == 0:
                    s = {0, 63, 64, 65, n - 1}
                elif r == 1:
                    s = {70 if n > 71 else n - 2}
                elif r == 3 and r != info['count'][0] - 1:
                    s = set(range(n))
                elif r == info['count'][0] - 1 and r > 1:
                    s = {n - 1}
                else:
                    s = set()
            else:
                s = {1, n - 1} if r % 3 == 0 else set(range(n)) if r % 3 == 1 else set()
            live += sorted(r * per + i for i in s if 0 <= i < n)
        out.append(live)
    return out


def live_pixel_masks(c, info):
    """Per level the [B * H * W] bool mask of problem b's non-zero dz pixels: ONE pixel in every live step, at offset (7 step) % 32 of the
    step (the last pixel of the level where the step is cut short)."""
    out = []
    for M, steps in zip(level_pixels(c), live_steps(c, info)):
        m = torch.zeros(M, dtype=torch.bool)
        for s in steps:
            m[min(32 * s + (7 * s) % 32, M - 1)] = True
        out.append(m)
    return out


def step_flags(masks):
    """One byte per 32-pixel step, levels concatenated, each rounded up to whole steps: 1 = a pixel of the step is set"""
    parts = []
    for m in masks:
        n = -(-m.numel() // 32)
        pad = torch.zeros(n * 32, dtype=torch.bool, device=m.device)
        pad[:m.numel()] = m
        parts.append(pad.view(n, 32).any(dim=1))
    return torch.cat(parts).to(torch.uint8)


# ----------------------------------------------------------------------------- float64 reference
def range_refs(x, dz, k, rngs):
    """x [B, H, W, Cin], dz [B, H, W, Cout] in float64 (any device), a k x k 'same' conv (k = 1 or 3), rngs = [(m0, m1)] over the level's
    (b, h, w) pixel index -> (G, S, bias, Sb): [R][Cout][k k][Cin] twice and [R][Cout] twice, see the module docstring."""
    B, H, W, Cin = x.shape
    Cout, hw, kk, pad = dz.shape[3], H * W, k * k, (k - 1) // 2
    R = len(rngs)
    G = torch.zeros(R, Cout, Cin * kk, dtype=x.dtype, device=x.device)
    S = torch.zeros_like(G)
    bias = torch.zeros(R, Cout, dtype=x.dtype, device=x.device)
    Sb = torch.zeros_like(bias)
    for b in range(B):
        mine = [(i, max(m0, b * hw) - b * hw, min(m1, (b + 1) * hw) - b * hw) for i, (m0, m1) in enumerate(rngs)
                if m0 < (b + 1) * hw and m1 > b * hw]
        if not mine:
            continue
        cols = F.unfold(F.pad(x[b:b + 1].permute(0, 3, 1, 2), [pad, pad, pad, pad]), (k, k))[0]       # [Cin k k, H W], row = (c, kh, kw)
        acols = cols.abs()
        zb = dz[b].reshape(hw, Cout)
        for i, lo, hi in mine:
            zt = zb[lo:hi].t()
            G[i] += zt @ cols[:, lo:hi].t()
            S[i] += zt.abs() @ acols[:, lo:hi].t()
            bias[i] += zt.sum(dim=1)
            Sb[i] += zt.abs().sum(dim=1)
    to_slab = lambda t: t.view(R, Cout, Cin, kk).permute(0, 1, 3, 2).contiguous()
    return to_slab(G), to_slab(S), bias, Sb


def naive_range(x, dz, k, m0, m1):
    """Nested loops over every pixel of the range, tap, channel and output channel: what range_refs is checked against on tiny shapes"""
    B, H, W, Cin = x.shape
    Cout, pad = dz.shape[3], (k - 1) // 2
    G, S = torch.zeros(Cout, k * k, Cin, dtype=torch.float64), torch.zeros(Cout, k * k, Cin, dtype=torch.float64)
    bias, Sb = torch.zeros(Cout, dtype=torch.float64), torch.zeros(Cout, dtype=torch.float64)
    for m in range(m0, m1):
        b, rem = divmod(m, H * W)
        h, w = divmod(rem, W)
        for n in range(Cout):
            z = float(dz[b, h, w, n])
            bias[n] += z
            Sb[n] += abs(z)
            for kh in range(k):
                for kw in range(k):
                    hh, ww = h + kh - pad, w + kw - pad
                    if 0 <= hh < H and 0 <= ww < W:
                        for ci in range(Cin):
                            G[n, kh * k + kw, ci] += z * float(x[b, hh, ww, ci])
                            S[n, kh * k + kw, ci] += abs(z) * abs(float(x[b, hh, ww, ci]))
    return G, S, bias, Sb


def stored64(c, t):
    """the float64 values a stored operand holds: the bf16 / fp32 values, or (split layout) the decoded hi + lo"""
    return from_split64(t) if c.kind == 'split' else t.double()


# ----------------------------------------------------------------------------- bounds
def sum_bound(c, n, S):
    """Bound of an fp32 sum of n products (or of n dz values: a bias row) against float64, S = the same sum on absolute values"""
    b = 2.0 * (n + 3) * U32 * S
    if c.arith in ('bf16x3', 'split'):
        b = b + X3_PER_PRODUCT * S
    return b
