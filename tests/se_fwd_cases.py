"""Case tables of the squeeze-excite forward / streaming-helper tests, and a plain-Python restatement of the partitions those kernels
walk (csrc/se.hip, csrc/pack.hip), made from the kernels' text.  Shared by tests/test_se_fwd_cases_host.py (CPU: the tables reach every
branch and loop exit they are meant to reach, so that they cannot be trimmed into shallowness) and tests/test_gpu_se_fwd_ops.py (GPU).

pool_reduce<NT> (se.hip): the sum of the depthwise forward's partial rows [G][C] of one image.  G <= 4: one thread per channel adds the
rows in order.  G > 4: NSL = NT / 64 slices of per = ceil(G / NSL) groups, slice sl = [min(G, sl per), min(G, sl per + per)); a thread
walks its slice with four chains (g, g+1, g+2, g+3 while g + 3 < g1) and a scalar tail on the first chain, folds them as
(s0 + s1) + (s2 + s3), and the slices meet in LDS and are added in slice order; channels in rounds of 64.  NT = 1024 (16 slices) in the
one-workgroup-per-image kernel, NT = 256 (4 slices) in phase 1 of the split form (Cse >= 8 and B <= 16).

se_dgate (se.hip): slabs = min(64, ceil(HW / 16)) workgroups per image, slab s covers the pixels [HW s / slabs, HW (s + 1) / slabs);
tcols = min(C / CE, 256) threads across the 16-byte chunks of a pixel row (CE = 4 fp32 / 8 bf16 elements per chunk), rpp = 256 / tcols
row groups that meet in LDS, ceil((C / CE) / tcols) column passes.

The grid-stride elementwise kernels (channel_scale, se_bwd_apply, act_bwd, add_inplace) run min(4096, ceil(n / 256)) workgroups of 256
threads over n 16-byte chunks; the layout converters of pack.hip min(2048, ceil(n / 256)) over n items (output elements; pixels on the
image path).
"""
import torch

F32, BF16 = torch.float32, torch.bfloat16


def ce(dtype):
    """Elements per 16-byte chunk."""
    return 4 if dtype == F32 else 8


# ----------------------------------------------------------------------------- pool_reduce
POOL_G = (1, 4, 5, 16, 17, 28, 33, 64, 65, 144)     # (28: four slices of 7 -- a tail of three behind a whole 4-chain pass)
POOL_C = (32, 144, 672, 1152)
NSL = {'one': 16, 'split': 4}               # slices of pool_reduce<1024> / pool_reduce<256>
POOL_FORMS = {'one': 4, 'split': 8}         # the Cse that selects the form (below 8 the split entry point forwards to one workgroup)
SPLIT_MAX_B = 16                            # above it the split entry point forwards too


def gate_form(B, Cse):
    """The kernel effdet_se_gate_fwd_split runs: 'split' (8 workgroups per image, pool_reduce<256>) or 'one' (pool_reduce<1024>)."""
    return 'one' if (B > SPLIT_MAX_B or Cse < 8) else 'split'


def pool_slices(G, nsl):
    """[(g0, g1)] of the nsl slices for G > 4; None on the direct branch."""
    if G <= 4:
        return None
    per = -(-G // nsl)
    out = []
    for sl in range(nsl):
        g0 = min(G, sl * per)
        out.append((g0, min(G, g0 + per)))
    return out


def slice_walk(n):
    """(passes of the 4-chain loop, rows left to the scalar tail) of a slice of n groups."""
    return n // 4, n % 4


def pool_reduce_restated(part, nsl):
    """The fp32 sum of part [G][C] (a float32 CPU tensor) in the kernel's own order: bit for bit what pool_reduce stores as the pooled sum
    (only additions, each rounded once; a chain starts from 0.0, which is exact)."""
    G, C = part.shape
    assert part.dtype == torch.float32
    sl = pool_slices(G, nsl)
    if sl is None:
        t = part[0].clone()
        for g in range(1, G):
            t = t + part[g]
        return t
    acc = None
    for g0, g1 in sl:
        s = [torch.zeros(C) for _ in range(4)]
        g = g0
        while g + 3 < g1:
            for u in range(4):
                s[u] = s[u] + part[g + u]
            g += 4
        while g < g1:
            s[0] = s[0] + part[g]
            g += 1
        v = (s[0] + s[1]) + (s[2] + s[3])
        acc = v if acc is None else acc + v
    return acc


# (b) the gate MLP on many partial rows: (G, C, Cse, B).  Cse 4 / 6: one workgroup per image whatever B; Cse 8 / 48 / 112: the split
# form at B = 2, one workgroup at B = 17.  The one-workgroup kernel runs squeezed channels j0, j0 + 16, j0 + 32 per wave in rounds of 48
# (Cse 48: one whole round, 112: two whole rounds and a third of 16), the split one j = slice + 8 wave in rounds of 32.
GATE_CSE = (4, 6, 8, 48, 112)
GATE_B = (2, 17)
GATE_CASES = [
    (1, 144, 4, 2), (5, 32, 4, 2), (17, 672, 4, 17), (144, 1152, 4, 2),
    (4, 672, 6, 17), (33, 144, 6, 2), (65, 1152, 6, 17), (16, 32, 6, 2),
    (1, 672, 8, 2), (5, 144, 8, 2), (17, 1152, 8, 2), (64, 32, 8, 2),
    (4, 1152, 48, 2), (33, 672, 48, 2), (144, 144, 48, 2),
    (16, 672, 112, 2), (65, 144, 112, 2), (5, 1152, 112, 2),
    (5, 672, 8, 17), (64, 32, 8, 17), (33, 1152, 48, 17), (4, 144, 48, 17), (17, 144, 112, 17), (144, 1152, 112, 17),
]
GATE_INV_HW = 1.0 / 49


# ----------------------------------------------------------------------------- se_dgate
DGATE_HW = (1, 16, 17, 1008, 1009, 1089, 1600)
DGATE_CH = ((F32, 32), (F32, 144), (F32, 1152), (F32, 2688), (BF16, 240), (BF16, 1152))
DGATE_B = 2


def dgate_slabs(HW):
    return min(64, max(1, -(-HW // 16)))


def dgate_partition(HW, C, dtype):
    """-> (slabs, [(p0, p1)] per slab, tcols, rpp, column passes)."""
    slabs = dgate_slabs(HW)
    cpr = C // ce(dtype)
    tcols = min(cpr, 256)
    return slabs, [(HW * s // slabs, HW * (s + 1) // slabs) for s in range(slabs)], tcols, 256 // tcols, -(-cpr // tcols)


# ----------------------------------------------------------------------------- grid-stride elementwise kernels
ELEMWISE_BLOCK, ELEMWISE_CAP, PACK_CAP = 256, 4096, 2048
ELEMWISE_ROUND = ELEMWISE_CAP * ELEMWISE_BLOCK          # chunks one round of the capped grid covers
PACK_ROUND = PACK_CAP * ELEMWISE_BLOCK

# (dtype, B, H, W, C): 5 x 63 x 65 pixels of 58 chunks = 1 187 550 chunks (~19 MB a tensor): the second round, a partial last
# workgroup, and a pixel row that no power of two divides (H x W = 4095 so that the count is no multiple of 256)
ELEMWISE_CASES = [(F32, 5, 63, 65, 232), (BF16, 5, 63, 65, 464)]


def elemwise_chunks(dtype, B, H, W, C):
    """-> (chunks, chunks per pixel row, chunks per image, rounds of the capped grid)."""
    cpr = C // ce(dtype)
    n = B * H * W * cpr
    grid = min(ELEMWISE_CAP, max(1, -(-n // ELEMWISE_BLOCK)))
    return n, cpr, H * W * cpr, -(-n // (grid * ELEMWISE_BLOCK))


# ----------------------------------------------------------------------------- layout converters
# nchw_to_nhwc: (dtype, B, C, H, W, cpad); 'image' = the per-pixel path (C <= CE channels padded to exactly one chunk: items are pixels),
# 'generic' = one item per output element
TO_NHWC_CASES = [
    ('image', F32, 3, 3, 420, 420, 4), ('image', BF16, 3, 3, 420, 420, 8),
    ('generic', F32, 3, 3, 149, 149, 8), ('generic', F32, 3, 40, 67, 67, 40), ('generic', BF16, 3, 40, 67, 67, 40),
]
# nhwc_to_nchw: (dtype, B, H, W, C)
TO_NCHW_CASES = [(F32, 2, 64, 64, 88), (BF16, 2, 64, 64, 88)]


def to_nhwc_path(dtype, C, cpad):
    return 'image' if (cpad == ce(dtype) and C <= ce(dtype)) else 'generic'


def pack_items(path, B, H, W, cpad):
    """-> (items, rounds of the 2048-workgroup grid)."""
    n = B * H * W * (1 if path == 'image' else cpad)
    grid = min(PACK_CAP, max(1, -(-n // ELEMWISE_BLOCK)))
    return n, -(-n // (grid * ELEMWISE_BLOCK))


# ----------------------------------------------------------------------------- colsum
# thread (column lane, sl = 0..3) walks rows sl, sl + 4, ... two at a time (p and p + 4 while p + 4 < rows), then one more if p < rows
COLSUM_ROWS = (1, 3, 4, 5, 8, 9, 12, 13, 1000)
COLSUM_C = (40, 64, 65)
COLSUM_LD_EXTRA = (0, 24)


def colsum_walk(rows, sl):
    """(two-row passes, whether the single-row tail runs) of row slice sl."""
    p, passes = sl, 0
    while p + 4 < rows:
        p += 8
        passes += 1
    return passes, p < rows


# ----------------------------------------------------------------------------- producer -> consumer chain
# (B, H, W): dwconv_fwd(pool=True) at C = 96, k = 3, stride 1 and expand_dw_fwd at Cin = 16 (Cexp = 96), k = 3, stride 1
CHAIN_GEOMETRY = (2, 64, 64)
CHAIN_C, CHAIN_CIN, CHAIN_K = 96, 16, 3
CHAIN_CSE = (4, 8)                      # one workgroup per image / the split form at B = 2
