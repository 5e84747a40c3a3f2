"""The persistent MFMA streaming kernels of the MBConv backward (csrc/pw_bwd.hip: effdet_pw_bwd, csrc/pw_dgrad.hip: effdet_pw_dgrad_se):
case tables, input builders and float64 references.  Shared by tests/test_pw_stream_cases_host.py (CPU) and tests/test_gpu_pw_stream.py
(GPU); imports torch only, every builder and reference takes the device to work on.

Both kernels run persistent workgroups of four waves, grid-stride over 64-pixel tiles (a wave owns 16 pixels of a tile): workgroup w
owns the tiles w, w + nwg, ...; nwg = min(tiles, resident slots), slots = 768 (pw_bwd at Cin = 16, pw_dgrad_se) or 512 (pw_bwd at Cin =
24 / 32).  The tables below hold the smallest shapes that are served at all (pw_bwd from M = 64 * 2048, pw_dgrad_se from M = 65536) and
reach, per template instance, the classes named in bwd_classes / dgrad_classes; the host test asserts the coverage over the tables.

pw_bwd leaves dx [M][Cin], one slab [Cexp][Cin] and one dsum row [Cexp] per workgroup; pw_dgrad_se leaves dz_d [M][Ce]:
    dx[p][ci]   = sum_ce dz[p][ce] fl32(s0[ce] W[ce][ci]) (+ res[p][ci])
    slab[w]     = sum over tiles t = w mod nwg of dz_t^T x_t,   dsum[w] = column sums of those dz_t
    dz_d[p][ce] = (rs[b] (sum_co dy[p][co] fl32(s2[co] W[co][ce])) gate[b][ce] + dpool[b][ce]) swish'(z_d[p][ce]),   b = p / HW

EXACT inputs: small integers from a hash of (row, column), powers of two for the scales, quarters for res / dpool -- every product and
every partial sum is a multiple of 2^-7 below 2^15 (pw_dgrad_se) or of 2^-2 far below 2^24 (pw_bwd; the largest: the whole-M weight
gradient, <= 16 M ~ 2^21), so fp32 arithmetic is exact in any order and the kernels must be torch.equal to the float64 reference.  The
powers of two are 2^-2 .. 2^2 by the hash of the channel / image -- they differ from neighbour to neighbour, but a wider range would
cost the exactness of the sums.  RANDOM inputs: randn with per-channel magnitudes spread over 2^-6 .. 2^6, held per element to the
any-order summation bound gamma(n + 2) * sum |a_i b_i|.
"""
import collections

import torch

TP = 64                                         # pixels per tile
WAVE_PIX = 16                                   # pixels of a tile per wave
PWB_MIN_M = 64 * 2048                           # effdet_pw_bwd_slabs: below it the two separate launches serve the map
PWB_SLOTS = {16: 768, 24: 512, 32: 512}         # resident workgroups of pw_bwd (EFFDET_PWB_SLOTS unset)
PWD_MIN_M = 65536
PWD_SLOTS = 768                                 # ... of pw_dgrad_se (EFFDET_PWD_SLOTS unset)
PWD_UNROLL = 3                                  # channel tiles of z_d / gate / dpool requested ahead
PWD_LDS_BYTES = 65536                           # the scaled project weights [Co][Ce + 4] live in LDS
DESCRIPTOR_LIMIT = 0xFFFF0000                   # bytes a 32-bit buffer descriptor covers
EUNSUPPORTED = -3

U32 = 2.0 ** -24                                # unit roundoff of fp32

# Relative error of the device's Swish' factor, |dy * swish_gradf_(z) (fp32, __expf and v_rcp inside) - dy * swish'(z) (float64)| over
# dy * m(z), m(z) = sig(z) (1 + |z| (1 - sig(z))): the magnitude of Swish' without the cancellation of 1 + z (1 - sig(z)) that takes
# the function through zero at z = -1.2785 (m = |swish'| for z >= 0; no relative bound holds at that root for any implementation).
# Measured through effdet_act_bwd (ACT_SWISH; it shares swish_gradf_ of csrc/common.h with pw_dgrad_se) on 2^22 points z in [-30, 30],
# dy in [1, 2): 1.74e-6 (with dy = 1, the factor alone: 1.72e-6; for |z| <= 8: 6.9e-7).  The constant is twice the measured value --
# headroom against another instruction schedule;
# tests/test_gpu_pw_stream.py::test_swish_grad_factor_error_is_within_the_constant re-measures it on every run.
SWISH_GRAD_E = 3.5e-6

PwBwdCase = collections.namedtuple('PwBwdCase', 'B H W Cin skip scale')
PwDgradCase = collections.namedtuple('PwDgradCase', 'B H W Co Ce rowscale scale')

# (B, H, W, Cin, identity-skip gradient given, BN scale given); Cexp = 6 Cin.  M = 131072 (the threshold: 2048 whole tiles), 131521
# (M % 64 = 1: one live pixel in wave 0 of the last tile), 133457 = 131072 + 64 * 37 + 17 (one live pixel in wave 1; 2086 tiles: 38 of
# the 512 workgroups own 5 tiles, the rest 4), 131327 (M % 64 = 63: one dead pixel).
PW_BWD_CASES = [
    PwBwdCase(2, 256, 256, 16, True, True), PwBwdCase(13, 67, 151, 16, False, True),
    PwBwdCase(1, 317, 421, 16, True, False), PwBwdCase(7, 73, 257, 16, True, True),
    PwBwdCase(2, 256, 256, 24, False, True), PwBwdCase(13, 67, 151, 24, False, True),
    PwBwdCase(1, 317, 421, 24, True, False), PwBwdCase(7, 73, 257, 24, False, True),
    PwBwdCase(2, 256, 256, 32, True, True), PwBwdCase(13, 67, 151, 32, False, False),
    PwBwdCase(1, 317, 421, 32, True, True), PwBwdCase(7, 73, 257, 32, True, True),
]

# (B, H, W, Co, Ce, per-image row scale given, BN scale given).  Geometries: 4 x 128 x 128 = 65536 exactly; 7 x 97 x 97 (M % 64 = 7, a
# wave's 16 pixels straddle two images); 7300 x 3 x 3 (every 16-pixel fragment spans two or three images).  (Co, Ce): (16, 48) the
# minimum Ce; (16, 64) NJ % 3 = 1; (24, 80) NJ % 3 = 2; (40, 112) NJ % 3 = 1 with the 8-channel K tail; (40, 400) and (24, 672) the
# largest Ce the LDS rule admits (64640 / 64896 bytes).
PW_DGRAD_CASES = [
    PwDgradCase(4, 128, 128, 16, 48, True, True), PwDgradCase(7, 97, 97, 16, 64, False, True), PwDgradCase(7300, 3, 3, 16, 64, True, False),
    PwDgradCase(7300, 3, 3, 16, 48, True, True),
    PwDgradCase(7, 97, 97, 24, 80, True, True), PwDgradCase(7300, 3, 3, 24, 80, False, False), PwDgradCase(4, 128, 128, 24, 672, True, True),
    PwDgradCase(4, 128, 128, 40, 112, True, False), PwDgradCase(7300, 3, 3, 40, 112, True, True), PwDgradCase(7, 97, 97, 40, 400, False, True),
]

BWD_CLASSES = ('threshold', 'tail1', 'tail17', 'tail63', 'tail+skip', 'tail-skip', 'ragged', 'scale_none')
DGRAD_PAIRS = ((16, 48), (16, 64), (24, 80), (40, 112), (40, 400), (24, 672))
DGRAD_GEOMETRIES = ('exact65536', 'straddle', 'tiny_images')
DGRAD_OPTIONS = ('rowscale_none', 'scale_none', 'both_given')


def bwd_id(c):
    return '%dx%dx%d-Cin%d%s%s' % (c.B, c.H, c.W, c.Cin, '-skip' if c.skip else '', '' if c.scale else '-noscale')


def dgrad_id(c):
    return '%dx%dx%d-Co%d-Ce%d%s%s' % (c.B, c.H, c.W, c.Co, c.Ce, '' if c.rowscale else '-nors', '' if c.scale else '-noscale')


def ownership(M, slots):
    """-> (tiles, workgroups, fewest and most tiles a workgroup owns) of the grid-stride walk."""
    ntiles = -(-M // TP)
    nwg = min(ntiles, slots)
    return ntiles, nwg, ntiles // nwg, -(-ntiles // nwg)


def bwd_geometry(c):
    M = c.B * c.H * c.W
    ntiles, nwg, tmin, tmax = ownership(M, PWB_SLOTS[c.Cin])
    return dict(M=M, Cexp=6 * c.Cin, ntiles=ntiles, nwg=nwg, tiles_min=tmin, tiles_max=tmax, tail=M % TP, dz_bytes=M * 6 * c.Cin * 4)


def bwd_classes(c):
    """The classes of BWD_CLASSES a case reaches."""
    g = bwd_geometry(c)
    out = set()
    if g['M'] == PWB_MIN_M:
        out.add('threshold')
    if g['tail'] in (1, 17, 63):
        out.add('tail%d' % g['tail'])
    if g['tail']:
        out.add('tail+skip' if c.skip else 'tail-skip')
    if g['ntiles'] % g['nwg']:
        out.add('ragged')
    if not c.scale:
        out.add('scale_none')
    return out


def dgrad_lds_bytes(Co, Ce):
    return Co * (Ce + 4) * 4


def dgrad_geometry(c):
    M, HW = c.B * c.H * c.W, c.H * c.W
    ntiles, nwg, tmin, tmax = ownership(M, PWD_SLOTS)
    # images the 16 pixels of a wave's fragment fall into, over all whole fragments: (fewest, most)
    spans = [(p0 + WAVE_PIX - 1) // HW - p0 // HW + 1 for p0 in range(0, M - WAVE_PIX + 1, WAVE_PIX)]
    return dict(M=M, HW=HW, ntiles=ntiles, nwg=nwg, tiles_min=tmin, tiles_max=tmax, tail=M % TP, nj=c.Ce // 16, nj_mod=(c.Ce // 16) % PWD_UNROLL,
                k_tail=(c.Co % 16) // 8, lds=dgrad_lds_bytes(c.Co, c.Ce), span_min=min(spans), span_max=max(spans), z_bytes=M * c.Ce * 4)


def dgrad_classes(c):
    """-> (geometry class or None, option class) of a case."""
    g = dgrad_geometry(c)
    geo = None
    if g['M'] == PWD_MIN_M and g['tail'] == 0:
        geo = 'exact65536'
    elif g['HW'] < WAVE_PIX and g['span_min'] >= 2 and g['span_max'] >= 3:
        geo = 'tiny_images'
    elif g['tail'] == 7 and g['span_max'] == 2 and g['HW'] % WAVE_PIX:
        geo = 'straddle'
    opts = set()
    if not c.rowscale:
        opts.add('rowscale_none')
    if not c.scale:
        opts.add('scale_none')
    if c.rowscale and c.scale:
        opts.add('both_given')
    return geo, opts


# ----------------------------------------------------------------------------- inputs
def hash32(rows, cols, salt, device):
    """[rows][cols] int64 in [0, 2^32): a multiply-xorshift hash of (row, column, salt)."""
    r = torch.arange(rows, dtype=torch.int64, device=device).view(-1, 1)
    c = torch.arange(cols, dtype=torch.int64, device=device).view(1, -1)
    m = 0xFFFFFFFF
    x = (r * 0x9E3779B1 + c * 0x85EBCA6B + salt * 0xC2B2AE35 + 0x27D4EB2F) & m
    x = x ^ (x >> 15)
    x = (x * 0x2C1B3C6D) & m
    x = x ^ (x >> 12)
    x = (x * 0x297A2D39) & m
    return x ^ (x >> 15)


def hash_ints(rows, cols, lim, salt, device='cpu'):
    """[rows][cols] fp32 integers in [-lim, lim] that depend on row and column."""
    return (hash32(rows, cols, salt, device) % (2 * lim + 1) - lim).float()


def hash_pow2(rows, cols, salt, device='cpu'):
    """[rows][cols] fp32 powers of two 2^-2 .. 2^2."""
    return torch.pow(2.0, (hash32(rows, cols, salt, device) % 5 - 2).float())


def hash_choice(rows, cols, a, b, salt, device='cpu'):
    """[rows][cols] fp32, a or b."""
    pick = (hash32(rows, cols, salt, device) >> 7) % 2 == 0
    return torch.where(pick, torch.tensor(float(a), device=device), torch.tensor(float(b), device=device))


BwdInputs = collections.namedtuple('BwdInputs', 'dz x w scale res')
DgradInputs = collections.namedtuple('DgradInputs', 'dy w scale rowscale gate dpool zd')
Z_PASS, Z_BLOCK = 40.0, -100.0          # swish_gradf_ is exactly 1 at 40 (__expf(-40) vanishes against 1) and +-0 at -100 (rcp(inf))


def bwd_exact_inputs(c, device='cpu', M=None):
    """|dz|, |x| <= 4, |w| <= 2, scale a power of two per expanded channel, res in quarters."""
    M = c.B * c.H * c.W if M is None else M
    Ci, Ce = c.Cin, 6 * c.Cin
    return BwdInputs(hash_ints(M, Ce, 4, 1, device), hash_ints(M, Ci, 4, 2, device), hash_ints(Ce, Ci, 2, 3, device),
                     hash_pow2(Ce, 1, 4, device).view(-1) if c.scale else None,
                     hash_ints(M, Ci, 15, 5, device) / 4 if c.skip else None)


def _spread(n, g):
    """n magnitudes 2^e, e uniform in [-6, 6]."""
    return torch.pow(2.0, torch.rand(n, generator=g) * 12 - 6)


def bwd_random_inputs(c, device='cpu', M=None, seed=0):
    M = c.B * c.H * c.W if M is None else M
    Ci, Ce = c.Cin, 6 * c.Cin
    g = torch.Generator().manual_seed(1000 + 7 * c.Cin + seed)
    dz = torch.randn(M, Ce, generator=g) * _spread(Ce, g)
    x = torch.randn(M, Ci, generator=g) * _spread(Ci, g)
    w = torch.randn(Ce, Ci, generator=g) * _spread(Ce, g).view(-1, 1) / Ci ** 0.5
    scale = 0.5 + torch.rand(Ce, generator=g) if c.scale else None
    res = torch.randn(M, Ci, generator=g) if c.skip else None
    return BwdInputs(*(None if t is None else t.to(device) for t in (dz, x, w, scale, res)))


def dgrad_exact_inputs(c, device='cpu', zd=None):
    """|dy| <= 4, |w| <= 2, scale / rowscale / gate powers of two per channel / image / (image, channel), dpool in quarters, z_d in
    {Z_PASS, Z_BLOCK} by the hash (or the zd given)."""
    M, Co, Ce = c.B * c.H * c.W, c.Co, c.Ce
    return DgradInputs(hash_ints(M, Co, 4, 11, device), hash_ints(Co, Ce, 2, 12, device),
                       hash_pow2(Co, 1, 13, device).view(-1) if c.scale else None,
                       hash_pow2(c.B, 1, 14, device).view(-1) / 2 if c.rowscale else None,
                       hash_pow2(c.B, Ce, 15, device), hash_ints(c.B, Ce, 15, 16, device) / 4,
                       hash_choice(M, Ce, Z_PASS, Z_BLOCK, 17, device) if zd is None else zd)


def dgrad_random_inputs(c, device='cpu', seed=0):
    M, Co, Ce = c.B * c.H * c.W, c.Co, c.Ce
    g = torch.Generator().manual_seed(2000 + 3 * Ce + Co + seed)
    dy = torch.randn(M, Co, generator=g) * _spread(Co, g)
    w = torch.randn(Co, Ce, generator=g) * _spread(Co, g).view(-1, 1) / Ce ** 0.5
    scale = 0.5 + torch.rand(Co, generator=g) if c.scale else None
    rs = 0.5 + torch.rand(c.B, generator=g) if c.rowscale else None
    gate = torch.rand(c.B, Ce, generator=g)
    dpool = torch.randn(c.B, Ce, generator=g) * 1e-2
    zd = torch.randn(M, Ce, generator=g) * 2
    return DgradInputs(*(None if t is None else t.to(device) for t in (dy, w, scale, rs, gate, dpool, zd)))


# ----------------------------------------------------------------------------- float64 references
def gamma(k):
    """k u / (1 - k u): the bound factor of k fp32 roundings."""
    return k * U32 / (1 - k * U32)


def scaled_weight(w, scale):
    """fl32(w * scale[row]) as both kernels form it when they fill LDS, then exact: float64."""
    return (w.float() * scale.float().view(-1, 1) if scale is not None else w.float()).double()


def by_owner(t, nwg):
    """[M][C] -> [nwg][K * 64][C]: the rows of the tiles w, w + nwg, ... of every workgroup w, zero rows behind M."""
    M, C = t.shape
    ntiles = -(-M // TP)
    K = -(-ntiles // nwg)
    pad = torch.zeros(K * nwg * TP, C, dtype=t.dtype, device=t.device)
    pad[:M] = t
    return pad.view(K, nwg, TP, C).permute(1, 0, 2, 3).reshape(nwg, K * TP, C)


BwdReference = collections.namedtuple('BwdReference', 'dx slabs dsum')


def bwd_reference(i, nwg, absolute=False):
    """float64 dx [M][Cin], slabs [nwg][Cexp][Cin], dsum [nwg][Cexp] of BwdInputs i.  absolute: the same sums on absolute values (the
    scale of the error bounds; res left out of dx)."""
    a = (lambda t: t.double().abs()) if absolute else (lambda t: t.double())
    ws = scaled_weight(i.w, i.scale)
    dz, x = a(i.dz), a(i.x)
    dx = dz @ (ws.abs() if absolute else ws)
    if i.res is not None and not absolute:
        dx = dx + i.res.double()
    dzo = by_owner(dz, nwg)
    return BwdReference(dx, dzo.transpose(1, 2) @ by_owner(x, nwg), dzo.sum(1))


def owned_pixels(M, nwg, device='cpu'):
    """[nwg] live pixels in the tiles of every workgroup: the terms of an element of its slab."""
    return by_owner(torch.ones(M, 1, dtype=torch.float64, device=device), nwg).sum(1).view(-1)


def bwd_bounds(i, nwg, ref):
    """Per-element bounds of (dx, slabs, dsum) against ref: gamma(n + 2) * sum |a_i b_i| with n = Cexp for dx, n = the pixels a workgroup
    owns for its slab and dsum row; with res, dx is rounded once more: + u |ref|."""
    ab = bwd_reference(i, nwg, absolute=True)
    Ce = i.dz.shape[1]
    dx = gamma(Ce + 2) * ab.dx
    if i.res is not None:
        dx = dx + U32 * ref.dx.abs()
    n = owned_pixels(i.dz.shape[0], nwg, i.dz.device)
    gn = (n + 2) * U32 / (1 - (n + 2) * U32)
    return BwdReference(dx, gn.view(-1, 1, 1) * ab.slabs, gn.view(-1, 1) * ab.dsum)


def sigmoid64(z):
    return torch.sigmoid(z.double())


def swish_grad64(z):
    s = sigmoid64(z)
    return s * (1 + z.double() * (1 - s))


def swish_grad_magnitude(z):
    """m(z) = sig(z) (1 + |z| (1 - sig(z))): see SWISH_GRAD_E."""
    s = sigmoid64(z)
    return s * (1 + z.double().abs() * (1 - s))


def _per_pixel(t, B, HW):
    """[B][...] -> one row per pixel."""
    return t.repeat_interleave(HW, dim=0)


def dgrad_pre(i, B, HW, absolute=False):
    """float64 (rs (dy @ fl32(w s2)) gate + dpool) [M][Ce]: what the Swish' factor multiplies; absolute: on absolute values."""
    a = (lambda t: t.double().abs()) if absolute else (lambda t: t.double())
    v = a(i.dy) @ a(scaled_weight(i.w, i.scale))
    if i.rowscale is not None:
        v = v * _per_pixel(a(i.rowscale).view(B, 1), B, HW)
    v = v.view(B, HW, -1) * a(i.gate).view(B, 1, -1) + a(i.dpool).view(B, 1, -1)
    return v.view(B * HW, -1)


def dgrad_reference(i, B, HW):
    return dgrad_pre(i, B, HW) * swish_grad64(i.zd)


def dgrad_exact_reference(i, B, HW):
    """For z_d in {Z_PASS, Z_BLOCK}: the factor is exactly 1 / 0 on the device (float64 Swish' is 1 + 4e-16 / -4e-42 there)."""
    return dgrad_pre(i, B, HW) * (i.zd == Z_PASS).double()


def dgrad_bound(i, B, HW, ref):
    """Per-element bound against dgrad_reference.  v = the value in front of Swish' takes n = Co roundings in the MFMA chain, one by the
    row scale and one by the fused gate multiply-add: |v^ - v| <= gamma(n + 2) S, S = dgrad_pre on absolute values.  The factor f^ =
    swish_gradf_(z) and the last product err by at most E m(z) (SWISH_GRAD_E), so
        |v^ f^ - v f| <= gamma(n + 2) S (|f| + E m) + E |v| m
    -- E |v| m is E |ref| wherever Swish' does not cancel (z >= 0) and stays a bound where it does."""
    f, m = swish_grad64(i.zd).abs(), swish_grad_magnitude(i.zd)
    S, v = dgrad_pre(i, B, HW, absolute=True), dgrad_pre(i, B, HW).abs()
    return gamma(i.dy.shape[1] + 2) * S * (f + SWISH_GRAD_E * m) + SWISH_GRAD_E * v * m
