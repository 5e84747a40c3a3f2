"""Explicit forward / backward of the EfficientDet components over the HIP kernels.

Each component has a ``*_fwd`` that returns (outputs, saved) and a ``*_bwd`` that maps output gradients
to input + parameter gradients.  PyTorch only owns memory, streams and the outer autograd graph
(efficientdet.py wraps these in autograd.Function nodes); every numeric op is a kernel of
libeffdet_hip.so.  Reference lines cited are relative to the reference repository root.

Frozen-BN backward without re-reading the conv output: for y = act(s*c + t), c = conv(x, W),
s = gamma*invstd:   dz = dy*act'(z);  dx = dgrad(dz, W*s);  G = x^T dz;  dW = s*G;
dgamma = invstd*(sum_k W*G - mean*sum dz);  dbeta = sum dz.
"""
import collections
import contextlib
import os

import torch

from . import ops
from .config import BN_EPS, conv_out
from .ops import ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_SWISH, RES_ADD, RES_NONE, RES_RELU_MASK, Map

DW_SAVE_Y = os.environ.get('EFFDET_DW_SAVE_Y', '0') == '1'      # A/B switch: also store the depthwise Swish output in training
BIFPN_WGRAD_GROUP = os.environ.get('EFFDET_BIFPN_WGRAD_GROUP', '1') != '0'     # A/B switch: grouped BiFPN weight gradients
EXPAND_Z_ONLY = os.environ.get('EFFDET_EXPAND_Z_ONLY', '1') == '1'   # training: the expand conv stores its pre-activation only
SE_FUSED = os.environ.get('EFFDET_SE_FUSED', '1') == '1'             # squeeze-excite backward fused into the project conv's gradients
DW_BWD_FUSED = os.environ.get('EFFDET_DW_BWD_FUSED', '1') == '1'       # training, fp32, k = 3, or k = 5 at H*W >= 1024 (stride 1) / 4096 (stride 2), EFFDET_DW_BWD_FUSED_K5 overrides: depthwise data + weight gradient in one kernel
PW_BWD_FUSED = os.environ.get('EFFDET_PW_BWD_FUSED', '1') == '1'       # training, fp32, Cin 16 / 24 / 32: expand conv data + weight gradient in one kernel
PW_DGRAD_SE = os.environ.get('EFFDET_PW_DGRAD_SE', '1') == '1'         # training, fp32, Co 16 / 24 / 40: project-conv data gradient + SE backward epilogue as a streaming MFMA kernel
FUSE_EXPAND_DW = os.environ.get('EFFDET_FUSE_EXPAND_DW', '1') == '1'  # inference, fp32 storage: expand conv inside the depthwise kernel
FUSE_CIN = tuple(int(v) for v in os.environ.get('EFFDET_FUSE_CIN', '16,24,32').split(','))     # block input widths that take it (A/B)
# f16x3 BiFPN convs from this much work per launch (output pixels x C^2; x 18 = FLOPs): below ~2 GFLOP the launch is a handful of tiles behind a
# DMA round trip and the exact kernel's deep-staged narrow tiles win (measured, D4 B = 8 @1024, 224 -> 224: M = 8192 87 -> 63 us, M = 2048
# 56 -> 61, M = 512 55 -> 61; D0 B = 32 @512, 64 -> 64: M = 131072 97 -> 59, M = 32768 35 -> 27, M = 8192 22 -> 27)
BIFPN_F16X3_MIN_WORK = float(os.environ.get('EFFDET_BIFPN_F16X3_MIN_WORK', '1.2e8'))
GATE_IN_WEIGHTS = os.environ.get('EFFDET_GATE_IN_WEIGHTS', '1') == '1'  # the SE gate folded into per-image project weights (no channel_scale pass)
# ... in training too (fp32 storage, fused SE backward): built, tested, and OFF.  The depthwise forward then stores its Swish output
# next to the pre-activation, which costs about what channel_scale's pass did: 27.65 / 27.97 ms (off) vs 27.72 / 27.62 ms (on) in round 4;
# round 6, alternating in one GPU call: 28.79 / 28.75 (off) vs 28.66 / 28.62 (on), 16 launches fewer -- but W diag(gate) is another
# rounding of the project conv's products, and with it the D1 and D6 train goldens leave their `1e-3 + s_k` gates (the single ReLU /
# max-pool ties of those fixtures fall the other way): 0.4 % of the step is not worth a parity gate
GATE_IN_WEIGHTS_TRAIN = os.environ.get('EFFDET_GATE_IN_WEIGHTS_TRAIN', '0') == '1'
# The gate in the project conv's OPERAND (training, fp32 storage, exact-fp32 forward, z-only depthwise storage): the conv and its per-image
# weight gradient read the depthwise pre-activation and form swish(z_d) * gate[b][c] in their operand registers (ops.conv2d /
# conv2d_wgrad a_gate=), the very statements channel_scale runs -- every MFMA gets the operand it got, losses and gradients are
# torch.equal to the channel_scale path's (tests/test_gpu_gate_operand.py), and xs is neither written, read twice nor kept for the
# backward.  Unlike GATE_IN_WEIGHTS_TRAIN above, which changes the products.
GATE_IN_OPERAND = os.environ.get('EFFDET_GATE_IN_OPERAND', '1') == '1'
# ... for maps of at least this many pixels per image (Ho * Wo).  Per block, D0 B = 32 @512, channel_scale + project forward + per-image
# weight gradient against the two gated launches (tools/gate_operand_timing.py, profiles/gate_operand_launch_timing.json; us):
#   block   0 (256^2)  1 (128^2)  2 (128^2)  3 (64^2)  4 (64^2)  5 (32^2)  6 (32^2)  7 (32^2) |  8 (16^2)  9 (16^2)  10 (16^2)
#   old       273.3      192.4      287.2      95.6     147.0      56.8      87.5      87.6   |    65.0      50.9       50.5
#   gated     193.3      130.6      202.2      76.3     109.1      52.6      82.2      82.1   |    68.5      52.4       52.7
# The consumers pay 5-30 % for the Swish they now run (forward +0 .. +8 us, weight gradient +3 .. +23 us per launch): that stays below
# channel_scale's pass down to the 32 x 32 maps and exceeds it on the 16 x 16 ones, whose 8.6 us pass was mostly launch latency.
# Blocks 11 .. 15 (8 x 8, 4 x 4) are no whole 128-pixel tiles per image: the planners refuse them.  Hence 1024.
GATE_OPERAND_MIN_HW = int(os.environ.get('EFFDET_GATE_OPERAND_MIN_HW', '1024'))


def chunk_elems(dtype):
    return 8 if dtype == torch.bfloat16 else 4


class ZeroArena:
    """One zero-filled fp32 allocation carved into gradient accumulators (one memset instead of dozens)."""

    def __init__(self, nfloats, device):
        self.buf = ops.zeros(max(int(nfloats), 1), device)
        self.pos = 0

    def take(self, *shape):
        n = 1
        for s in shape:
            n *= s
        v = self.buf[self.pos:self.pos + n].view(*shape)
        self.pos += (n + 63) // 64 * 64
        assert self.pos <= self.buf.numel() + 64
        return v

    @staticmethod
    def need(*sizes):
        return sum((n + 63) // 64 * 64 for n in sizes)


def as_map(t):
    return Map.of(t)


# ------------------------------------------------------------------------------------------ stem
def stem_fwd(img, w, gamma, beta, mean, var, pad, dtype, train, z_only=False):
    """models/efficientnet.py:193  swish(bn0(conv_stem(img)))  (3x3 s2, static same pad).
    z_only (training, consumer = an expand-1 MBConv block handed `xpre`): only the PRE-activation is stored and returned -- the
    block's depthwise kernels Swish their staged tiles (one 256 x 256 x 32 write stream less)."""
    ce = chunk_elems(dtype)
    B, _, H, W = img.shape
    if hasattr(img, 'map'):       # efficientdet.PackedImages: already NHWC / compute dtype / one chunk of channels
        x = img.map
    else:
        x = ops.nchw_to_nhwc(img.contiguous().float(), dtype, cpad=ce)
    s, t, inv = ops.bn_fold(gamma, beta, mean, var, BN_EPS)
    wp = ops.pack_weight(w, dtype, cin_pad=ce)
    Cout = w.shape[0]
    Ho, Wo = conv_out(H, 3, 2, pad), conv_out(W, 3, 2, pad)
    if z_only and train:
        z = Map.new(B, Ho, Wo, Cout, dtype, img.device)
        ops.conv2d(x, wp, z, Cin=ce, Cout=Cout, KH=3, KW=3, stride=2, pad_t=pad[0], pad_l=pad[0], scale=s, shift=t, act=ACT_NONE)
        return z, (x, z, s, inv, mean, w, pad)
    y = Map.new(B, Ho, Wo, Cout, dtype, img.device)
    z = Map.new(B, Ho, Wo, Cout, dtype, img.device) if train else None
    ops.conv2d(x, wp, y, Cin=ce, Cout=Cout, KH=3, KW=3, stride=2, pad_t=pad[0], pad_l=pad[0], scale=s, shift=t,
               act=ACT_SWISH, zs=z)
    return y, (x, z, s, inv, mean, w, pad)


def stem_bwd(saved, dy, dy_is_dz=False):
    """dy_is_dz: the incoming gradient already went through the stem's Swish' (fused into block 0's depthwise data gradient)."""
    x, z, s, inv, mean, w, pad = saved
    Cout, ce = w.shape[0], x.C
    dz = dy if dy_is_dz else ops.act_bwd(dy, z, ACT_SWISH)
    G, dsum = ops.conv2d_wgrad(x, dz, Cin=ce, Cout=Cout, KH=3, KW=3, stride=2, pad_t=pad[0], pad_l=pad[0])
    dw, dg, db = ops.unpack_wgrad_bn(G, w, s, dsum, mean, inv, cin_pad=ce)     # + frozen-BN gamma/beta grads, one launch
    return dw, dg, db


# ------------------------------------------------------------------------------------------ MBConv
# A block's path is chosen once, by mbconv_path (forward) and mbconv_bwd_path (backward): nothing else reads the switches above, and the
# stages below branch on the records alone.  DESIGN.md section 3 has the table of gate forms and the backward's reaction to each.
# MBConvPath.expand -- how the expand conv runs
EXPAND_NONE = 'none'      # expand == 1: the depthwise conv reads the block input
EXPAND_IN_DW = 'in_dw'    # inference: inside the depthwise kernel (ops.expand_dw_fwd)
EXPAND_Z = 'z'            # training: it stores its pre-activation only, the depthwise kernels Swish their staged tiles
EXPAND_YZ = 'yz'          # it stores its output and, in training, its pre-activation
# MBConvPath.gate -- what the depthwise forward stores and how the squeeze-excite gate reaches the project conv
GATE_WEIGHTS = 'weights'          # x_d (+ z_d in training) stored; the gate rides in per-image project weights
GATE_OPERAND = 'operand'          # z_d stored; the project conv and its weight gradient form swish(z_d) * gate in their operand registers
GATE_XS_FROM_ZD = 'xs_from_zd'    # z_d stored; xs = channel_scale(z_d, gate, swish) is materialised
GATE_XS_FROM_XD = 'xs_from_xd'    # x_d (+ z_d in training) stored; xs = channel_scale(x_d, gate) is materialised
# the forward path of one block.  dw_in_act: ACT_SWISH = the depthwise conv's input is a pre-activation that it Swishes itself
MBConvPath = collections.namedtuple('MBConvPath', 'expand dw_in_act gate')
# the backward's choices.  se_fused: the fused squeeze-excite backward, else the se_dgate / se_bwd_apply chain; gate: the form the project
# conv's weight gradient takes (GATE_OPERAND: if its planner accepts); xs_from: None = the forward kept xs, 'xd' / 'zd' = a switch changed
# since the forward (or the chain runs) and xs is materialised first, from that tensor; ask_*: whether to ask the fused kernel at all
MBConvBwdPath = collections.namedtuple('MBConvBwdPath', 'se_fused gate xs_from ask_pw_dgrad_se ask_dw_bwd ask_pw_bwd')
# what mbconv_fwd hands mbconv_bwd.  A field that a path does not produce is None (s0 / i0 / ze with expand == 1, xd with z-only storage,
# xs where it was never materialised, xpre without a producer's pre-activation)
MBConvSaved = collections.namedtuple('MBConvSaved', 'path blk P x rowscale xpre s0 i0 ze xe s1 i1 wk xd zd pool gate mid xs s2 i2 inv_hw')


def mbconv_path(blk, x, dtype, train, in_act):
    """The forward path of one block -- the only reader of the forward switches.  GATE_OPERAND is subject to the two planners, which
    need the operands: mbconv_gate_settled, in the project stage."""
    hw = conv_out(x.H, blk.k, blk.stride, blk.pad) * conv_out(x.W, blk.k, blk.stride, blk.pad)
    f32 = dtype == torch.float32
    if blk.expand == 1:
        expand, dw_in_act = EXPAND_NONE, in_act      # ACT_SWISH: the producer (the stem) handed its pre-activation ONLY (stem_fwd z_only)
    elif not train and FUSE_EXPAND_DW and f32 and blk.k == 3 and blk.cin in FUSE_CIN and x.ld == x.C and x.off == 0:
        # (measured per block, D0 B = 32 @512, expand + depthwise -> fused: k3/s2 Cin 16 492 -> 335 us, k3/s1 Cin 24 267 -> 216; but
        #  k5/s2 Cin 24 224 -> 333, k5/s1 Cin 40 157 -> 168, k3/s2 Cin 40 107 -> 143: the k = 5 tiles leave one workgroup per CU and at
        #  Cin = 40 the expand's MFMA work outweighs the bytes saved -- so only the k = 3, Cin <= 32 blocks take it)
        expand, dw_in_act = EXPAND_IN_DW, ACT_NONE
    elif train and EXPAND_Z_ONLY and hw > 64:          # (<= 8x8 maps: the direct weight-gradient kernel would Swish every tap load)
        # training stores ONE tensor for the expand conv, its pre-activation: the depthwise forward / weight-gradient kernels
        # Swish their staged tiles (the two streams y_e, z_e were 35 % of the backbone's forward writes)
        expand, dw_in_act = EXPAND_Z, ACT_SWISH
    else:
        expand, dw_in_act = EXPAND_YZ, ACT_NONE
    # training stores the depthwise pre-activation ONLY (the step is bound by HBM write bandwidth, ~2.5 TB/s measured):
    # the gate multiply and the backward of the gate recompute Swish from it
    # gate in per-image project weights (round 4): inference always; training when the fused SE backward applies (it takes the
    # project conv's weight gradient per image, which is where the gate re-enters) -- the depthwise conv then stores BOTH its
    # pre-activation (backward) and its Swish output (the project conv's operand) and channel_scale's read + write pass is gone
    if GATE_IN_WEIGHTS and hw % 128 == 0 and (not train or (GATE_IN_WEIGHTS_TRAIN and SE_FUSED and f32 and hw % 32 == 0)):
        gate = GATE_WEIGHTS
    elif not train or DW_SAVE_Y:
        gate = GATE_XS_FROM_XD
    elif GATE_IN_OPERAND and f32 and SE_FUSED and hw >= GATE_OPERAND_MIN_HW:
        gate = GATE_OPERAND
    else:
        gate = GATE_XS_FROM_ZD
    return MBConvPath(expand, dw_in_act, gate)


def mbconv_gate_settled(path, zd, wpp, y, gate, pkw):
    """`path` with the planners' answer in it: the gate stays in the operand only if both readers of xs take the form (exact-fp32 launch,
    whole 128-pixel tiles per image, per-image splits on the thin / DMA-staged weight-gradient kernels), else xs is materialised as
    before.  pkw: the project conv's keyword arguments."""
    if path.gate != GATE_OPERAND or (ops.conv2d_gated_ok(zd, wpp, y, gate, ACT_SWISH, **pkw)
                                     and ops.conv2d_wgrad_gated_ok(zd, y, gate, ACT_SWISH, Cin=pkw['Cin'], Cout=pkw['Cout'])):
        return path
    return path._replace(gate=GATE_XS_FROM_ZD)


def mbconv_bwd_path(path, dtype, hw):
    """The backward's choices for a block whose forward took `path`, on maps of `hw` pixels per image -- the only reader of the backward
    switches, read when the backward runs (a switch may have changed since the forward: tests do that)."""
    f32 = dtype == torch.float32
    se_fused = SE_FUSED and hw % (64 if dtype == torch.bfloat16 else 32) == 0
    if path.gate == GATE_WEIGHTS:         # the forward ran on W diag(gate_b) and x_d; only the fused form takes the gate back in its unpack
        gate, xs_from = (GATE_WEIGHTS, None) if se_fused else (GATE_XS_FROM_XD, 'xd')
    elif path.gate == GATE_OPERAND:       # the forward kept no xs: the fused form takes z_d + the gate, anything else the same values as xs
        gate, xs_from = (GATE_OPERAND if GATE_IN_OPERAND and se_fused else GATE_XS_FROM_ZD), 'zd'
    else:
        gate, xs_from = path.gate, None
    return MBConvBwdPath(se_fused, gate, xs_from, ask_pw_dgrad_se=se_fused and PW_DGRAD_SE and f32,
                         ask_dw_bwd=DW_BWD_FUSED and path.dw_in_act == ACT_SWISH and f32,
                         ask_pw_bwd=path.expand != EXPAND_NONE and PW_BWD_FUSED and f32)


def _mbconv_expand_fwd(path, x, blk, P, dtype, train):
    """-> (xe, ze, s0, t0, i0): the depthwise conv's input, the expand conv's stored pre-activation, its folded BN"""
    if path.expand == EXPAND_NONE:
        return x, None, None, None, None
    s0, t0, i0 = ops.bn_fold(P['bn0.weight'], P['bn0.bias'], P['bn0.running_mean'], P['bn0.running_var'], BN_EPS)
    if path.expand == EXPAND_IN_DW:
        return None, None, s0, t0, i0       # (the 6x-expanded map exists only tile by tile, in LDS: see ops.expand_dw_fwd)
    dev = x.t.device
    if path.expand == EXPAND_Z:
        ze = Map.new(x.B, x.H, x.W, blk.cexp, dtype, dev)
        ops.conv2d(x, ops.pack_weight(P['expand.weight'], dtype), ze, Cin=blk.cin, Cout=blk.cexp, KH=1, KW=1,
                   scale=s0, shift=t0, act=ACT_NONE)
        return ze, ze, s0, t0, i0
    xe = Map.new(x.B, x.H, x.W, blk.cexp, dtype, dev)
    ze = Map.new(x.B, x.H, x.W, blk.cexp, dtype, dev) if train else None
    ops.conv2d(x, ops.pack_weight(P['expand.weight'], dtype), xe, Cin=blk.cin, Cout=blk.cexp, KH=1, KW=1,
               scale=s0, shift=t0, act=ACT_SWISH, zs=ze)
    return xe, ze, s0, t0, i0


def _mbconv_dw_se_fwd(path, x, xe, s0, t0, blk, P, train):
    """Depthwise conv (with the expand conv inside it on EXPAND_IN_DW) + squeeze-excite gate
    -> (xd, zd, wk, s1, i1, gate, mid, pool, inv_hw)"""
    Ho, Wo = conv_out(x.H, blk.k, blk.stride, blk.pad), conv_out(x.W, blk.k, blk.stride, blk.pad)
    s1, t1, i1 = ops.bn_fold(P['bn1.weight'], P['bn1.bias'], P['bn1.running_mean'], P['bn1.running_var'], BN_EPS)
    wk = ops.dw_pack_weight(P['dw.weight'])
    if path.expand == EXPAND_IN_DW:
        xd, pool_part = ops.expand_dw_fwd(x, P['expand.weight'], s0, t0, wk, s1, t1, blk.k, blk.stride, blk.pad[0], blk.pad[0], Ho, Wo)
        zd = None
    else:
        xd, zd, pool_part = ops.dwconv_fwd(xe, wk, s1, t1, blk.k, blk.stride, blk.pad[0], blk.pad[0], Ho, Wo, save_z=train, pool=True,
                                           save_y=path.gate in (GATE_WEIGHTS, GATE_XS_FROM_XD), in_act=path.dw_in_act)
    inv_hw = 1.0 / (Ho * Wo)
    w1 = P['se_reduce.weight'].view(blk.cse, blk.cexp); w2 = P['se_expand.weight'].view(blk.cexp, blk.cse)
    gate, mid, pool = ops.se_gate_fwd(pool_part, w1, P['se_reduce.bias'], w2, P['se_expand.bias'], inv_hw, save_mid=train)
    return xd, zd, wk, s1, i1, gate, mid, pool, inv_hw


def _mbconv_project_fwd(path, x, xd, zd, gate, blk, P, dtype, rowscale):
    """Project conv with the gate in the form `path` names (+ drop_connect scale and identity skip in its epilogue)
    -> (y, xs, s2, i2, path with the planners' answer)"""
    Ho, Wo = conv_out(x.H, blk.k, blk.stride, blk.pad), conv_out(x.W, blk.k, blk.stride, blk.pad)
    s2, t2, i2 = ops.bn_fold(P['bn2.weight'], P['bn2.bias'], P['bn2.running_mean'], P['bn2.running_var'], BN_EPS)
    y = Map.new(x.B, Ho, Wo, blk.cout, dtype, x.t.device)
    pkw = dict(Cin=blk.cexp, Cout=blk.cout, KH=1, KW=1, scale=s2, shift=t2, act=ACT_NONE, rowscale=rowscale if blk.skip else None,
               res=x if blk.skip else None, res_mode=RES_ADD if blk.skip else RES_NONE)
    if path.gate == GATE_WEIGHTS:
        # y = (W diag(gate_b)) x_d -- the gate rides in per-image project weights (a few MB for the whole batch) instead of
        # a read + write pass over the expanded map (16 channel_scale launches moved 3.2 GB per D0 B = 32 forward: 5 % of it)
        wpb, wstride = ops.scale_pack_weight(P['project.weight'], gate, dtype)
        ops.conv2d(xd, wpb, y, w_image_stride=wstride, **pkw)
        return y, None, s2, i2, path
    wpp = ops.pack_weight(P['project.weight'], dtype)
    path = mbconv_gate_settled(path, zd, wpp, y, gate, pkw)
    if path.gate == GATE_OPERAND:
        xs = None
        ops.conv2d(zd, wpp, y, a_gate=gate, a_act=ACT_SWISH, **pkw)
    else:
        xs = ops.channel_scale(zd, gate, ACT_SWISH) if path.gate == GATE_XS_FROM_ZD else ops.channel_scale(xd, gate)
        ops.conv2d(xs, wpp, y, **pkw)
    return y, xs, s2, i2, path


def mbconv_fwd(x, blk, P, dtype, train, rowscale=None, xpre=None, in_act=ACT_NONE):
    """models/efficientnet.py:75-105.  P: dict of parameter / buffer tensors of the block.
    rowscale: optional [B] fp32 = drop_connect keep-mask / keep_prob (models/utils.py:79-90).
    in_act=ACT_SWISH (expand == 1 blocks only, with xpre = x): x is the producer's PRE-activation (stem_fwd z_only) -- stated by the
    caller, never inferred.  -> (y Map, MBConvSaved)"""
    assert in_act == ACT_NONE or (blk.expand == 1 and xpre is x)
    path = mbconv_path(blk, x, dtype, train, in_act)
    xe, ze, s0, t0, i0 = _mbconv_expand_fwd(path, x, blk, P, dtype, train)
    xd, zd, wk, s1, i1, gate, mid, pool, inv_hw = _mbconv_dw_se_fwd(path, x, xe, s0, t0, blk, P, train)
    y, xs, s2, i2, path = _mbconv_project_fwd(path, x, xd, zd, gate, blk, P, dtype, rowscale)
    return y, MBConvSaved(path, blk, P, x, rowscale, xpre, s0, i0, ze, xe, s1, i1, wk, xd, zd, pool, gate, mid, xs, s2, i2, inv_hw)


def _mbconv_project_se_bwd(bp, sv, dy):
    """Project conv (+ drop_connect scale on the branch) + squeeze-excite backward -> (dz_d Map, their gradients keyed like P)"""
    blk, P = sv.blk, sv.P
    dtype, dev = sv.x.dtype, sv.x.t.device
    B, Ce, Co, Cs = sv.x.B, blk.cexp, blk.cout, blk.cse
    g = {}
    rs = sv.rowscale if blk.skip else None
    wp = P['project.weight']
    w1 = P['se_reduce.weight'].view(Cs, Ce); w2 = P['se_expand.weight'].view(Ce, Cs)
    form, xs = bp.gate, sv.xs
    if form == GATE_OPERAND and not ops.conv2d_wgrad_gated_ok(sv.zd, dy, sv.gate, ACT_SWISH, Cin=Ce, Cout=Co):
        form = GATE_XS_FROM_ZD
    if bp.xs_from is not None and form != GATE_OPERAND:       # the same values as the forward's xs either way
        xs = ops.channel_scale(sv.xd, sv.gate) if bp.xs_from == 'xd' else ops.channel_scale(sv.zd, sv.gate, ACT_SWISH)
    if bp.se_fused:
        # Fused form (no pass over the activations for the gate gradient, dxs never materialised):
        #   per-image partial weight gradients M_b = dy_b^T xs_b (split-K on image boundaries)
        #   dW = sum_b rs_b M_b (slab scale in the unpack);  (dgate*gate)[b][c] = rs_b sum_n W'[n][c] M_b[n][c]
        #   dz_d = (rs_b (dy W') gate[b][c] + dpool[b][c]) * swish'(z_d)   in the epilogue of the project conv's data gradient
        # -- se_dgate (2 tensor reads), se_bwd_apply (2 reads + 1 write) and the drop_connect act_bwd become one extra read of z_d.
        # (giw: the forward ran on W diag(gate_b) and x_d; the slabs are then M'_b = dy_b^T x_d,b -- the gate re-enters as a per-(image,
        #  channel) factor of the unpack, and sum_n W'[n][c] M'_b[n][c] is d(loss)/d(gate) itself, not yet times the gate)
        giw = form == GATE_WEIGHTS
        if form == GATE_OPERAND:
            G2, dsum2 = ops.conv2d_wgrad(sv.zd, dy, Cin=Ce, Cout=Co, KH=1, KW=1, image_splits=True, a_gate=sv.gate, a_act=ACT_SWISH)
        else:
            G2, dsum2 = ops.conv2d_wgrad(sv.xd if giw else xs, dy, Cin=Ce, Cout=Co, KH=1, KW=1, image_splits=True)
        g['project.weight'], g['bn2.weight'], g['bn2.bias'] = ops.unpack_wgrad_bn(G2, wp, sv.s2, dsum2, P['bn2.running_mean'], sv.i2,
                                                                                 slab_scale=rs, slab_cscale=sv.gate if giw else None)
        dgg = ops.se_dgate_from_wgrad(G2, wp, sv.s2, rs, B)
        dpool, dw1, db1, dw2, db2 = ops.se_gate_bwd(dgg, sv.gate, sv.mid, sv.pool, w1, P['se_reduce.bias'], w2, sv.inv_hw,
                                                    times_gate=not giw)
        # the high-resolution blocks (Co 16 / 24 / 40 over >= 64 k pixels): a streaming kernel of its own (round 6)
        dzd = ops.pw_dgrad_se(dy, wp, sv.s2, rs, sv.gate, dpool, sv.zd) if bp.ask_pw_dgrad_se else None
        if dzd is None:
            dzd = Map.new(B, dy.H, dy.W, Ce, dtype, dev)
            ops.conv2d(dy, ops.pack_weight(wp, dtype, mode=1, scale=sv.s2), dzd, Cin=Co, Cout=Ce, KH=1, KW=1, rowscale=rs,
                       bc_scale=sv.gate, bc_shift=dpool, res=sv.zd, res_mode=ops.RES_SWISH_GRAD)
    else:
        dz2 = ops.act_bwd(dy, None, ACT_NONE, rowscale=rs) if rs is not None else dy
        G2, dsum2 = ops.conv2d_wgrad(xs, dz2, Cin=Ce, Cout=Co, KH=1, KW=1)
        g['project.weight'], g['bn2.weight'], g['bn2.bias'] = ops.unpack_wgrad_bn(G2, wp, sv.s2, dsum2, P['bn2.running_mean'], sv.i2)
        dxs = Map.new(B, dy.H, dy.W, Ce, dtype, dev)
        ops.conv2d(dz2, ops.pack_weight(wp, dtype, mode=1, scale=sv.s2), dxs, Cin=Co, Cout=Ce, KH=1, KW=1)
        dgate = ops.se_dgate(dxs, sv.xd) if form == GATE_XS_FROM_XD else ops.se_dgate(dxs, sv.zd, ACT_SWISH)
        dpool, dw1, db1, dw2, db2 = ops.se_gate_bwd(dgate, sv.gate, sv.mid, sv.pool, w1, P['se_reduce.bias'], w2, sv.inv_hw)
        dzd = ops.se_bwd_apply(dxs, sv.gate, dpool, sv.zd)
    g['se_reduce.weight'], g['se_reduce.bias'] = dw1.view(Cs, Ce, 1, 1), db1
    g['se_expand.weight'], g['se_expand.bias'] = dw2.view(Ce, Cs, 1, 1), db2
    return dzd, g


def _mbconv_dw_bwd(bp, sv, dzd):
    """Depthwise conv backward -> (dz_e Map: the gradient of the depthwise conv's input, through the Swish of `zprev` where there is one,
    its gradients keyed like P)"""
    blk, P = sv.blk, sv.P
    # (expand == 1, i.e. block 0: the depthwise conv reads the block input itself; given the pre-activation `xpre` of the producer --
    #  the stem's z -- its Swish' is applied here, in the data gradient's epilogue, instead of a separate pass in the stem's backward)
    zprev = sv.ze if blk.expand != 1 else sv.xpre
    fused = None
    if bp.ask_dw_bwd:
        # z-only storage: the depthwise input IS swish(zprev) -- one kernel reads dz_d and zprev once for both gradients (round 6)
        assert zprev is sv.xe
        fused = ops.dwconv_bwd(dzd, sv.wk, sv.s1, zprev, blk.k, blk.stride, blk.pad[0], blk.pad[0])
    if fused is not None:
        dze, gk, dsum1 = fused
    else:
        gk, dsum1 = ops.dwconv_wgrad(sv.xe, dzd, blk.k, blk.stride, blk.pad[0], blk.pad[0], in_act=sv.path.dw_in_act)
        dze = ops.dwconv_dgrad(dzd, sv.wk, sv.s1, zprev, sv.x.H, sv.x.W, blk.k, blk.stride, blk.pad[0], blk.pad[0])
    g = {}
    g['dw.weight'], g['bn1.weight'], g['bn1.bias'] = ops.dw_unpack_wgrad_bn(gk, sv.s1, P['dw.weight'], dsum1, P['bn1.running_mean'], sv.i1)
    return dze, g


def _mbconv_expand_bwd(bp, sv, dze, dy):
    """Expand conv backward; the identity-skip gradient is added in the data-gradient epilogue -> (dx Map, its gradients keyed like P).
    expand == 1 (block 0, no skip): the depthwise conv acted on the block input directly, dz_e is dx."""
    if sv.path.expand == EXPAND_NONE:
        return dze, {}
    blk, P, x = sv.blk, sv.P, sv.x
    Ce, Ci = blk.cexp, blk.cin
    g = {}
    we = P['expand.weight']
    fusedp = ops.pw_bwd(dze, x, we, sv.s0, dy if blk.skip else None) if bp.ask_pw_bwd else None
    if fusedp is not None:
        # the high-resolution blocks (Cin 16 / 24 / 32): both gradients of the expand conv from ONE read of the 6x-expanded gradient (round 6)
        dx, G0, dsum0 = fusedp
    else:
        G0, dsum0 = ops.conv2d_wgrad(x, dze, Cin=Ci, Cout=Ce, KH=1, KW=1)
    g['expand.weight'], g['bn0.weight'], g['bn0.bias'] = ops.unpack_wgrad_bn(G0, we, sv.s0, dsum0, P['bn0.running_mean'], sv.i0)
    if fusedp is None:
        dx = Map.new(x.B, x.H, x.W, Ci, x.dtype, x.t.device)
        ops.conv2d(dze, ops.pack_weight(we, x.dtype, mode=1, scale=sv.s0), dx, Cin=Ce, Cout=Ci, KH=1, KW=1,
                   res=dy if blk.skip else None, res_mode=RES_ADD if blk.skip else RES_NONE)
    return dx, g


def mbconv_bwd(sv, dy):
    """sv: the MBConvSaved of mbconv_fwd -> (dx Map, grads dict keyed like P)."""
    bp = mbconv_bwd_path(sv.path, sv.x.dtype, dy.H * dy.W)
    dzd, g2 = _mbconv_project_se_bwd(bp, sv, dy)
    dze, g1 = _mbconv_dw_bwd(bp, sv, dzd)
    dx, g0 = _mbconv_expand_bwd(bp, sv, dze, dy)
    return dx, {**g2, **g1, **g0}


# ------------------------------------------------------------------------------------------ BiFPN
def lateral_fwd(feats, weights, biases, W, dtype):
    """models/bifpn.py:100-103: 1x1 conv + bias per level (different Cin / weights per level)."""
    outs = []
    for f, w, b in zip(feats, weights, biases):
        y = Map.new(f.B, f.H, f.W, W, dtype, f.t.device)
        ops.conv2d(f, ops.pack_weight(w, dtype), y, Cin=f.C, Cout=W, KH=1, KW=1, shift=b)
        outs.append(y)
    return outs


def lateral_bwd(feats, weights, douts, dtype):
    dfs, dws, dbs = [], [], []
    for f, w, dy in zip(feats, weights, douts):
        W, Cin = w.shape[0], w.shape[1]
        G, dbp = ops.conv2d_wgrad(f, dy, Cin=Cin, Cout=W, KH=1, KW=1)
        dw = torch.empty_like(w)
        db = ops.unpack_wgrad(G, dw, dbias_part=dbp)
        df = Map.new(f.B, f.H, f.W, Cin, dtype, w.device)
        ops.conv2d(dy, ops.pack_weight(w, dtype, mode=1), df, Cin=W, Cout=Cin, KH=1, KW=1)
        dfs.append(df); dws.append(dw); dbs.append(db)
    return dfs, dws, dbs


def _conv3_fwd(x, w, b, dtype, xh=None):
    """xh: the same input in the H-split layout -> the conv runs in the f16x3 arithmetic (plain fp32 output)."""
    src = x if xh is None else xh
    y = Map.new(src.B, src.H, src.W, w.shape[0], dtype, src.t.device)
    if xh is not None:
        ops.conv2d(xh, ops.pack_weight(w, dtype, h3=True), y, Cin=w.shape[1], Cout=w.shape[0], KH=3, KW=3, pad_t=1, pad_l=1, shift=b,
                   hsplit=True, out_f32=True)
    else:
        ops.conv2d(x, ops.pack_weight(w, dtype), y, Cin=w.shape[1], Cout=w.shape[0], KH=3, KW=3, pad_t=1, pad_l=1, shift=b)
    return y


def bifpn_module_fwd(p, w1, w2, cw, cb, dtype, train):
    """models/bifpn.py:172-203.  p: 5 Maps (fine -> coarse); cw/cb: the 8 conv weights / biases.
    Node order and aliasing follow the reference exactly: top-down results overwrite p[3..0], the
    bottom-up pass reads those plus the ORIGINAL inputs (its `inputs_clone`)."""
    L_ = len(p)
    t_in = list(p)
    cur = list(p)
    nodes = []            # (mode, col, wsel, a_name, b_name, c_name, out_name, fused Map)
    names = {('in', l): t_in[l] for l in range(L_)}
    c = 0
    # f16x3 (ops.F32_ARITH_HEAD, the headline mode): the node's 3x3 conv reads the fused map in the H-split layout, which the fusion kernel
    # writes itself (inference: instead of the plain map; training: next to it -- the conv's weight gradient reads the plain one)
    hs = head_uses_f16x3(cw[0].shape[0], dtype) and cw[0].shape[1] == cw[0].shape[0]

    def fuse(a, b, cc, w, col, mode):
        if not hs or a.B * a.H * a.W * a.C * a.C < BIFPN_F16X3_MIN_WORK:
            return ops.bifpn_fuse_fwd(a, b, cc, w, col, mode), None
        return ops.bifpn_fuse_fwd(a, b, cc, w, col, mode, plain=train, hsplit=True)
    for i in range(L_ - 1, 0, -1):                                  # top-down, bifpn.py:188-192
        a_n = ('in', i - 1); b_n = ('in', i) if i == L_ - 1 else ('td', i)
        f, fh = fuse(names[a_n], names[b_n], None, w1, i - 1, 0)
        out_n = ('td', i - 1); names[out_n] = _conv3_fwd(f, cw[c], cb[c], dtype, fh)
        nodes.append((0, i - 1, 1, a_n, b_n, None, out_n, f, c)); c += 1
    for i in range(0, L_ - 2):                                      # bottom-up, bifpn.py:194-198
        a_n = ('td', i + 1); b_n = ('td', 0) if i == 0 else ('bu', i); c_n = ('in', i + 1)
        f, fh = fuse(names[a_n], names[b_n], names[c_n], w2, i, 1)
        out_n = ('bu', i + 1); names[out_n] = _conv3_fwd(f, cw[c], cb[c], dtype, fh)
        nodes.append((1, i, 2, a_n, b_n, c_n, out_n, f, c)); c += 1
    a_n = ('in', L_ - 1); b_n = ('bu', L_ - 2)                      # top node, bifpn.py:200-202
    f, fh = fuse(names[a_n], names[b_n], None, w1, L_ - 1, 2)
    out_n = ('top', L_ - 1); names[out_n] = _conv3_fwd(f, cw[c], cb[c], dtype, fh)
    nodes.append((2, L_ - 1, 1, a_n, b_n, None, out_n, f, c))
    out_names = [('td', 0)] + [('bu', l) for l in range(1, L_ - 1)] + [out_n]
    outs = [names[n] for n in out_names]
    cur = outs
    saved = (nodes, names, out_names, w1, w2, cw) if train else None
    return cur, saved


def bifpn_module_bwd(saved, douts, dtype, own=False):
    """-> (d_inputs [5 Maps], dw1, dw2, dcw [8], dcb [8]).  own: `douts` are private buffers of the caller (the d_inputs of the next
    module's backward) and may be accumulated into; gradients handed over by autograd are copied first."""
    nodes, names, out_names, w1, w2, cw = saved
    dev = w1.device
    Wc = cw[0].shape[0]
    grads = {}                                   # tensor name -> Map (private, safe to accumulate into)
    for n, d in zip(out_names, douts):
        grads[n] = d if own else Map.of(d.tensor().clone())    # never write into autograd's grad_outputs
    n1, n2 = ops.fuse_dn_floats(w1.shape[1]), ops.fuse_dn_floats(w2.shape[1])
    ar = ZeroArena(ZeroArena.need(n1, n2), dev)
    dn1, dn2 = ar.take(n1), ar.take(n2)     # per-workgroup partial rows of d loss / d n_r (zeroed: a column without a launch adds nothing)
    dcw, dcb = [None] * 8, [None] * 8

    def target(name):
        like = names[name]
        if name in grads:
            return grads[name], True
        grads[name] = Map.new(like.B, like.H, like.W, like.C, dtype, dev)
        return grads[name], False

    pending = []                                                     # (M, f, dz, conv index): weight gradients, leaf work
    for (mode, col, wsel, a_n, b_n, c_n, out_n, f, ci) in reversed(nodes):
        dz = grads[out_n]                                            # conv has bias only: dz = dy (final: its consumers ran first)
        if BIFPN_WGRAD_GROUP:
            pending.append((f.B * f.H * f.W, f, dz, ci))
        else:
            G, dbp = ops.conv2d_wgrad(f, dz, Cin=Wc, Cout=Wc, KH=3, KW=3, pad_t=1, pad_l=1)
            dw = torch.empty_like(cw[ci]); db = ops.unpack_wgrad(G, dw, dbias_part=dbp)
            dcw[ci], dcb[ci] = dw, db
        df = Map.new(f.B, f.H, f.W, Wc, dtype, dev)
        ops.conv2d(dz, ops.pack_weight(cw[ci], dtype, mode=1), df, Cin=Wc, Cout=Wc, KH=3, KW=3, pad_t=1, pad_l=1)
        da, da_acc = target(a_n); dbm, db_acc = target(b_n)
        dc, dc_acc = target(c_n) if c_n is not None else (None, False)
        ops.bifpn_fuse_bwd(df, names[a_n], names[b_n], names[c_n] if c_n else None, da, dbm, dc, da_acc, db_acc, dc_acc,
                           w1 if wsel == 1 else w2, dn1 if wsel == 1 else dn2, col, mode)
    # The 8 weight gradients of the module as TWO launches of independent problems (one pyramid level each, own weights): launched
    # one by one they are 19-89 us apiece -- the 4x4 .. 16x16 levels are 5-160 workgroups walking one dependent chain -- 268 us
    # per module for 27 GFLOP.  The largest level shares its launch with the four smallest, the 32x32 / 16x16 ones share the other.
    if pending:
        pending.sort(key=lambda t: -t[0])
        chunks = [pending[:1] + pending[4:], pending[1:4]] if len(pending) > 5 else [pending]
        for ch in chunks:
            if not ch:
                continue
            outs = ops.conv2d_wgrad([t[1] for t in ch], [t[2] for t in ch], Cin=Wc, Cout=Wc, KH=3, KW=3, pad_t=1, pad_l=1, group=True)
            for (_, _, _, ci), (G, dbp) in zip(ch, outs):
                dw = torch.empty_like(cw[ci]); dcb[ci] = ops.unpack_wgrad(G, dw, dbias_part=dbp); dcw[ci] = dw
    dw1 = ops.zeros(tuple(w1.shape), w1.device); dw2 = ops.zeros(tuple(w2.shape), w2.device)
    ops.bifpn_weight_bwd(w1, dn1, dw1); ops.bifpn_weight_bwd(w2, dn2, dw2)
    dins = [grads[('in', l)] for l in range(len(out_names))]
    return dins, dw1, dw2, dcw, dcb


# ------------------------------------------------------------------------------------------ RetinaHead
def _pyramid_alloc_n(n, B, sizes, C, dtype, device):
    """n pyramids of one geometry (one activation of n towers of the head) in ONE flat buffer, tower-major then level-major, so that
    grouped launches can address every pyramid tensor of the same channel count with identical relative offsets: outputs, split copies
    and ReLU-mask residuals of all n towers from one base each.  -> (flat, [maps of tower 0, ...])"""
    flat = torch.empty(n * sum(B * h * w * C for (h, w) in sizes), dtype=dtype, device=device)
    out, off = [], 0
    for _ in range(n):
        maps = []
        for (h, w) in sizes:
            maps.append(Map(flat, B, h, w, C, off=off)); off += B * h * w * C
        out.append(maps)
    return flat, out


def pyramid_alloc(B, sizes, C, dtype, device):
    """All levels of one activation in ONE flat buffer (level-major).  -> (flat, maps)"""
    flat, (maps,) = _pyramid_alloc_n(1, B, sizes, C, dtype, device)
    return flat, maps


def pyramid_alloc_pair(B, sizes, C, dtype, device):
    """The same layer of the head's two towers in ONE flat buffer.  -> (flat, maps of tower A, maps of tower B)"""
    flat, (a, b) = _pyramid_alloc_n(2, B, sizes, C, dtype, device)
    return flat, a, b


def level_tensor(m):
    n = m.B * m.H * m.W * m.C
    return m.t[m.off:m.off + n].view(m.B, m.H, m.W, m.C)


def head_out_maps(buf, B, sizes, per_anchor):
    """Views of a [B, A, per_anchor] output buffer as per-level NHWC maps with 9*per_anchor channels
    (models/retinahead.py:119-127: NHWC permute + view(B, -1, C) is free in this layout)."""
    A = sum(h * w for (h, w) in sizes) * 9
    maps, aoff = [], 0
    for (h, w) in sizes:
        maps.append(Map(buf, B, h, w, 9 * per_anchor, ld=9 * per_anchor, bstride=A * per_anchor, off=aoff * per_anchor))
        aoff += h * w * 9
    return maps


# The two towers of the RetinaHead are independent chains of equal launches.  A 256 -> 256 tower conv is 2728 tiles on 512 workgroup slots =
# 5.33 rounds: the last round runs a third full, i.e. ~11 % of every launch is a draining tail (PMC: MFMA busy 0.82 = 0.89 of quantisation x
# 0.92 in the loop).  On two streams (one graph branch each under capture) the regression tower's workgroups fill the classification
# tower's tail and vice versa.  Fork / join discipline instead of record_stream: the side stream starts behind everything the main stream
# has enqueued, and the main stream waits for it before anything the side stream touched can be freed or reused.
HEAD_TWO_STREAMS = os.environ.get('EFFDET_HEAD_TWO_STREAMS', '0') == '1'
_side_streams = {}


class _Fork:
    """with _Fork(device, on) as f: ...main-stream work...; with f.side(): ...side-stream work...   (joined at exit; on=False: one stream)"""

    def __init__(self, device, on):
        self.on = on
        if on:
            key = (device.index, torch.cuda.current_stream(device).cuda_stream)
            if key not in _side_streams:
                _side_streams[key] = torch.cuda.Stream(device)
            self.main, self.s = torch.cuda.current_stream(device), _side_streams[key]

    def __enter__(self):
        if self.on:
            self.s.wait_stream(self.main)
        return self

    def side(self):
        return torch.cuda.stream(self.s) if self.on else contextlib.nullcontext()

    def join(self):
        if self.on:
            self.main.wait_stream(self.s)
            self.on = False

    def __exit__(self, et, ev, tb):
        self.join()
        return False


HEAD_PAIR_TOWERS = os.environ.get('EFFDET_HEAD_PAIR_TOWERS', '1') == '1'     # A/B switch: layer t of both towers as one launch (f16x3 forward, split-layout data gradients)
HEAD_SPLIT = os.environ.get('EFFDET_HEAD_SPLIT', '1') == '1'     # A/B switch: split-layout head activations in the bf16x3 arithmetic
# A/B switch: the regression tower's backward pass skips the tiles / steps its gradient cannot reach (head_bwd).  The smooth-L1 gradient
# is an exact zero everywhere but at the positive anchors and every layer behind it is a 3x3 conv without bias, so after k data-gradient
# layers the gradient is confined to Chebyshev distance k of those pixels: ops.live_tiles flags the units, the split-layout kernels skip
# the rest.  Bit for bit the dense pass (DESIGN.md section 3 names the one exception: non-finite weights / activations under a zero gradient).
HEAD_SPARSE_REG = os.environ.get('EFFDET_HEAD_SPARSE_REG', '1') == '1'
# A/B switch: the forward counterpart.  In training the regression output is read at the positive anchors only, and those follow from
# anchors and annotations alone: ops.needed_tiles flags, ahead of the head, the tiles of every regression-tower layer whose output can
# reach a positive anchor (the same geometry, read forwards); the f16x3 kernels write zeros into the rest.  Losses and gradients are bit
# for bit the dense ones (include/effdet_needed_tiles.h).
HEAD_SPARSE_REG_FWD = os.environ.get('EFFDET_HEAD_SPARSE_REG_FWD', '1') == '1'
# A/B switch: the flagged forward and data-gradient launches of the regression tower in the gathered form (include/effdet_unit_lists.h):
# the flagged 32-pixel units, four to a 128-pixel tile, instead of every tile that holds a flagged pixel -- 0.53 - 0.80 of the computed
# tiles on the benchmark's batch (profiles/unit_count_b32_512.json).  One more small launch per pass builds the lists; the weight
# gradients (which walk the 32-pixel flags already) do not change.  Bit for bit the tile flags' results where anything reads them.
HEAD_SPARSE_UNITS = os.environ.get('EFFDET_HEAD_SPARSE_UNITS', '1') == '1'
# A/B switch: in the paired head backward, the weight gradients of layer t of BOTH towers as one launch (ops.conv2d_wgrad_pair).  The
# regression tower's flagged launch lasts as long as its few almost entirely live ranges, which are dispatched last; in one grid with the
# classification tower's dense launch they start first and the dense blocks fill the slots behind them.  Same plans, same slabs: bit for
# bit the separate launches.  Off: one launch per (tower, layer).
HEAD_PAIR_WGRAD = os.environ.get('EFFDET_HEAD_PAIR_WGRAD', '1') == '1'
_split_ok = {}


def head_uses_split(B, sizes, Wc, dtype, arith=None):
    """bf16x3 arithmetic on fp32 storage: the RetinaHead's activations and gradients live in the SPLIT layout (every 32 channels
    as [32 x bf16 hi | 32 x bf16 lo], same 4 bytes per element) so that the head's convs and weight gradients -- 95 % of the
    step's FLOPs -- read ready-made MFMA operands instead of splitting fp32 values in registers in every K-step.  Needs pyramid
    levels the split weight-gradient kernel can take (whole 8-pixel runs per row); otherwise the plain-fp32 path stays.
    arith: the arithmetic asked about (default: the one the launches use now)."""
    if not (HEAD_SPLIT and dtype == torch.float32 and (arith or ops.F32_ARITH) == 'bf16x3' and Wc % 32 == 0):
        return False
    key = (B, tuple(sizes), Wc)
    if key not in _split_ok:
        _split_ok[key] = ops.wgrad_split_supported(B, sizes, 256, 256, 256) and ops.wgrad_split_supported(B, sizes, Wc, 256, 256)
    return _split_ok[key]


def _pyramid_to_split(src_maps, B, sizes, C_, dtype, dev, bf=True, h=False):
    """A pyramid activation (plain fp32, one tensor per level) -> fresh flat level-major buffers holding it in the split layout (bf) and /
    or the H-split layout of the f16x3 forward convs (h), written by ONE pass per level.  -> (split maps or None, H-split maps or None)"""
    dst = pyramid_alloc(B, sizes, C_, dtype, dev)[1] if bf else None
    dsth = pyramid_alloc(B, sizes, C_, dtype, dev)[1] if h else None
    for i, s_ in enumerate(src_maps):
        ops.to_split2(s_.tensor(), dst[i].addr() if bf else None, dsth[i].addr() if h else None, s_.B * s_.H * s_.W * s_.C,
                      ops.range_flag(dev) if h else None)
    return dst, dsth


def head_uses_f16x3(Wc, dtype):
    """The f16x3 forward head (ops.F32_ARITH_HEAD): fp32 storage, exact-fp32 arithmetic around it, whole 32-channel groups."""
    return HEAD_SPLIT and dtype == torch.float32 and ops.F32_ARITH == 'f32' and ops.F32_ARITH_HEAD == 'f16x3' and Wc % 32 == 0


def _head_forms(B, sizes, Wc, dtype, train):
    """The form head_fwd runs in -> (split, split_bwd, hs).  split: the all-bf16x3 head on split-layout activations.  split_bwd: an exact
    or f16x3 forward whose backward runs the split-layout gradient kernels (their operands / masks ride along as `ysplit`).  hs: the
    f16x3 forward (fp32-equivalent three-product fp16 form) -- every conv reads H-split operands and writes H-split outputs; training
    geometries the split gradient kernels cannot take keep the exact-fp32 head."""
    split = head_uses_split(B, sizes, Wc, dtype)
    split_bwd = (not split) and train and ops.F32_ARITH_BWD == 'bf16x3' and head_uses_split(B, sizes, Wc, dtype, 'bf16x3')
    hs = (not split) and head_uses_f16x3(Wc, dtype) and (split_bwd or not train)
    return split, split_bwd, hs


def head_fwd_takes_needed(p, dtype, train):
    """Will head_fwd(p, ..., dtype, train) honour reg_needed?  The training f16x3 forward with the split-layout backward, switch on."""
    _, split_bwd, hs = _head_forms(p[0].B, [(m.H, m.W) for m in p], p[0].C, dtype, train)
    return bool(HEAD_SPARSE_REG_FWD and train and hs and split_bwd)


_K3 = dict(KH=3, KW=3, pad_t=1, pad_l=1)       # every conv of the head, forward and backward: 3x3, stride 1, same-padded
# what head_fwd hands head_bwd: the pyramid as the weight gradients read it, {tower: its four layer outputs in that form}, the level
# sizes, the parameter dict, the class count, whether all of it is in the split layout, and whether the forward ran the towers as a pair
HeadSaved = collections.namedtuple('HeadSaved', 'pyramid acts sizes HP num_classes split paired')


def _tower_layer(group, xs, wp, geo, Cin, shift=None, ysplit=False, res=None, **kw):
    """The 3x3 conv to 256 channels of every tower of `group` (a tuple of tower names, in segment order) as ONE launch: a forward layer
    or its data gradient.  xs / wp / shift / res: {tower: input maps / packed weight / bias / residual maps}; geo: (B, sizes, dtype,
    device, 128-pixel tiles of one pyramid); kw: ops.conv2d's other arguments, needed= / live= being the REGRESSION tower's flags.
    -> ({tower: output maps}, {tower: maps of the split copy} or None), each set in one flat tower-major buffer.
    The towers are independent chains of identical launches: two run concatenated, with per-segment weights / bias (effdet_conv_t.seg_w
    / seg_shift) and the flags starting at the regression tower's first tile -- 2 x 2728 tiles on the 512 workgroup slots = 10.66 rounds
    instead of twice 5.33: the draining third of a round is paid once per layer, not twice.  Same tiles, same K walk: bit for bit the
    separate launches.  A single tower passes no per-segment operands (the planner takes those for another kind of launch)."""
    B, sizes, dtype, dev, ntile = geo
    first = group[0]
    ys = dict(zip(group, _pyramid_alloc_n(len(group), B, sizes, 256, dtype, dev)[1]))
    ss = dict(zip(group, _pyramid_alloc_n(len(group), B, sizes, 256, dtype, dev)[1])) if ysplit else None
    if len(group) > 1:
        L = len(sizes)
        kw['seg_w'] = [wp[tw] for tw in group for _ in range(L)]
        if shift is not None:
            kw['seg_shift'] = [shift[tw] for tw in group for _ in range(L)]
    for flags in ('needed', 'live'):
        if kw.get(flags) is not None:
            kw[flags + '_tile0'] = ntile * group.index('reg')

    def cat(d):
        return [m for tw in group for m in d[tw]] if d is not None else None
    ops.conv2d(cat(xs), wp[first], cat(ys), Cin=Cin, Cout=256, **_K3, shift=shift[first] if shift is not None else None, ysplit=cat(ss),
               res=cat(res), **kw)
    return ys, ss


def head_fwd(p, HP, num_classes, dtype, train, reg_needed=None, reg_units=None):
    """models/retinahead.py:109-132 for all 5 levels per launch (weights are shared across levels).
    p: 5 Maps; HP: dict of head parameter tensors.  -> classification [B,A,nc] fp32 (probabilities),
    regression [B,A,4] fp32.
    Arithmetic 'f32_bwd_bf16x3' (forward exact, gradients in the three-product form): the forward below runs on plain fp32
    activations with exact-fp32 products, and every activation the BACKWARD will read -- the pyramid and the eight tower outputs,
    operands of the weight gradients and ReLU masks of the data gradients -- is stored a second time in the split layout by the
    conv that produces it (`ysplit`: the epilogue writes both forms; the plain copy dies with the next layer), so that head_bwd
    runs the split-layout gradient kernels unchanged.
    reg_needed (uint8 [radius][tiles], ops.needed_tiles; f16x3 forward only): the caller reads the regression output at the flagged
    pixels alone, so layer t of the regression tower computes the tiles of row 4 - t and retina_reg those of row 0; the rest of `reg`
    and of the tower's activations is zeros.  None: dense.
    reg_units (ops.UnitLists of the same flags, or None): those launches in the gathered form."""
    dev = p[0].t.device
    B, Wc = p[0].B, p[0].C
    sizes = [(m.H, m.W) for m in p]
    A = sum(h * w for (h, w) in sizes) * 9
    split, split_bwd, hs = _head_forms(B, sizes, Wc, dtype, train)
    if not (hs and split_bwd):
        reg_needed = None
    if reg_needed is None or not HEAD_SPARSE_UNITS:
        reg_units = None
    geo = (B, sizes, dtype, dev, sum((B * h * w + 127) // 128 for (h, w) in sizes))

    def need(towers, r):
        return reg_needed[r] if (reg_needed is not None and 'reg' in towers) else None

    def need_units(towers, r):
        return reg_units.row(r) if (reg_units is not None and 'reg' in towers) else None

    def pack(w):
        return ops.pack_weight(w, dtype, x3=split, h3=hs)
    pin, pin_h = p, None
    if split or split_bwd or hs:    # the pyramid once in the split layout(s): operand of both towers' first conv and of their weight gradients
        pin, pin_h = _pyramid_to_split(p, B, sizes, Wc, dtype, dev, bf=split or split_bwd, h=hs)
        if pin is None:
            pin = p
    acts = {'cls': [], 'reg': []}
    cls = torch.empty((B, A, num_classes), dtype=torch.float32, device=dev)
    reg = torch.empty((B, A, 4), dtype=torch.float32, device=dev)
    out = {'cls': (cls, num_classes, ACT_SIGMOID), 'reg': (reg, 4, ACT_NONE)}

    def towers_fwd(group):
        """the four layers of the group's towers, one launch per layer, then the output conv of each tower"""
        cur = dict.fromkeys(group, pin_h if hs else (p if split_bwd else pin))
        for t in range(4):
            w = {tw: HP[f'{tw}_convs.{t}.weight'] for tw in group}
            cur, ysp = _tower_layer(group, cur, {tw: pack(w[tw]) for tw in group}, geo, w[group[0]].shape[1],
                                    shift={tw: HP[f'{tw}_convs.{t}.bias'] for tw in group}, ysplit=split_bwd, act=ACT_RELU, split=split,
                                    hsplit=hs, needed=need(group, 4 - t), units=need_units(group, 4 - t))
            for tw in group:          # (split_bwd: `cur` stays plain fp32 / H-split and is not kept for backward)
                acts[tw].append(ysp[tw] if split_bwd else cur[tw])
        for tw in group:
            buf, per, act = out[tw]
            ops.conv2d(cur[tw], pack(HP[f'retina_{tw}.weight']), head_out_maps(buf, B, sizes, per), Cin=256, Cout=9 * per, **_K3,
                       shift=HP[f'retina_{tw}.bias'], act=act, out_f32=True, split=split, hsplit=hs, needed=need((tw,), 0),
                       units=need_units((tw,), 0))
    paired = hs and HEAD_PAIR_TOWERS         # layer t of both towers as one launch
    if paired:
        towers_fwd(('cls', 'reg'))
    else:
        with _Fork(dev, HEAD_TWO_STREAMS and ops.PROFILE is None) as fk:
            with fk.side():
                towers_fwd(('reg',))
            towers_fwd(('cls',))
    saved = HeadSaved(pin, acts, sizes, HP, num_classes, split or split_bwd, paired and split_bwd) if train else None
    return cls, reg, saved


def _split_rows(maps, Cfp, dtype):
    """plain fp32 gradient maps (possibly strided views of a [B, A, per] buffer) -> fresh contiguous maps of Cfp (% 32 == 0)
    channels per pixel in the split layout."""
    out = []
    for m in maps:
        padded = ops.pad_rows(m, Cfp) if (m.C != Cfp or m.ld != Cfp or m.bstride != m.H * m.W * Cfp or m.off) else m
        out.append(Map.of(ops.to_split(padded.tensor())))
    return out


def head_bwd(saved, dcls_logit, dreg, dtype, dcls_ld=0, cls_gscale=None, dreg_ld=0, in_split=False):
    """dcls_logit [B,A,nc] (or, with dcls_ld, pixel-major and channel-padded [B,A/9,dcls_ld]: ops.focal_loss_bwd_pix),
    dreg [B,A,4] (or, with dreg_ld, pixel-major [B,A/9,dreg_ld]): gradients wrt the cls LOGITS and box deltas, in `dtype` -- when
    the head was run in the split layout (saved.split) they are needed in the split layout too: in_split says the pixel-major forms
    already are (the loss kernels write it directly), anything else is converted here.  -> (dp: 5 Maps, grads dict keyed like HP).
    cls_gscale (fp32 tensor [1]): dcls_logit was computed for an upstream gradient of one (ops.focal_loss_fwd_grad); the
    real scalar enters here where the chain is linear: as the per-image output scale of retina_cls's data-gradient conv
    and as a factor on retina_cls's own parameter gradients."""
    p, acts, sizes, HP, nc, split, paired = saved
    dev = p[0].t.device
    B, Wc = p[0].B, p[0].C
    g = {}
    apix = sum(h * w for (h, w) in sizes)
    last = {}
    # liveness flags of the regression tower (row r: units within distance r of a non-zero d(reg) pixel), from the pixel-major rows
    # the loss kernel wrote; retina_reg's gradients read d(reg) itself (r = 0 / 1), layer t of the tower is 4 - t / 5 - t layers on
    live = None
    if HEAD_SPARSE_REG and split and dreg_ld and (in_split or dreg.dtype == torch.float32):
        live = ops.live_tiles(dreg, B, sizes, dreg_ld, in_split)
    ulists = ops.UnitLists(*live) if (live is not None and HEAD_SPARSE_UNITS) else None      # the data-gradient launches gather their units
    geo = (B, sizes, dtype, dev, sum((B * h * w + 127) // 128 for (h, w) in sizes))
    douts = {'cls': (dcls_logit, nc, dcls_ld), 'reg': (dreg, 4, dreg_ld)}      # tower -> (gradient, values per anchor, its pixel-major ld)

    def lv(towers, kind, r):
        return live[kind][r] if (live is not None and 'reg' in towers) else None

    def lu(towers, r):
        return ulists.row(r) if (ulists is not None and 'reg' in towers) else None

    def tower_final(tower, dout, per, pix_ld):
        """retina_cls / retina_reg: weight gradient + data gradient back into the tower (ReLU mask of its last layer fused) -> dz maps"""
        fin = f'retina_{tower}'
        wf = HP[fin + '.weight']
        Cf = wf.shape[0]
        ce = 32 if split else chunk_elems(dtype)
        if pix_ld:
            # the loss kernel already wrote rows of pix_ld channels per pixel (zeros past 9*per): aligned 128-B K-slices
            Cfp, poff, dzmaps = pix_ld, 0, []
            for (h, w) in sizes:
                dzmaps.append(Map(dout, B, h, w, Cfp, ld=Cfp, bstride=apix * Cfp, off=poff * Cfp)); poff += h * w
            if split and not in_split:
                assert Cfp % 32 == 0
                dzmaps = _split_rows(dzmaps, Cfp, dtype)
        else:
            dzmaps = head_out_maps(dout, B, sizes, per)
            Cfp = (Cf + ce - 1) // ce * ce
            if split:
                dzmaps = _split_rows(dzmaps, Cfp, dtype)
            elif Cfp != Cf:          # 9*num_classes (or 36) channels are not whole 16-byte chunks: zero-pad the rows
                dzmaps = [ops.pad_rows(m, Cfp) for m in dzmaps]
        G, dbp = ops.conv2d_wgrad(acts[tower][3], dzmaps, Cin=256, Cout=Cf, **_K3, split=split, live32=lv((tower,), 0, 0))
        # (cls_gscale: the class-loss gradient was written for an upstream gradient of one -- the upstream scalar multiplies the
        #  slabs and bias partial rows inside the unpack, and the rows of the data gradient)
        gs = cls_gscale if tower == 'cls' else None
        dw = torch.empty_like(wf); db = ops.unpack_wgrad(G, dw, dbias_part=dbp, slab_scale=gs)
        rows = gs.expand(B).contiguous() if gs is not None else None
        g[fin + '.weight'], g[fin + '.bias'] = dw, db
        # data gradient with the ReLU mask of the producing tower layer fused into the epilogue
        _, dz = pyramid_alloc(B, sizes, 256, dtype, dev)
        ops.conv2d(dzmaps, ops.pack_weight(wf, dtype, mode=1, cin_pad=Cfp, x3=split), dz, Cin=Cfp, Cout=256, **_K3, res=acts[tower][3],
                   res_mode=RES_RELU_MASK, rowscale=rows, split=split, live=lv((tower,), 1, 1), units=lu((tower,), 1))
        return dz

    def layer_wgrads(group, t, dz):
        """weight gradients of layer t of the group's towers, `reg` first; both towers with HEAD_PAIR_WGRAD: the dense classification
        problem and the (flagged) regression problem in one launch, unpacked in the order of the separate launches"""
        w = {tw: HP[f'{tw}_convs.{t}.weight'] for tw in group}
        xin = {tw: acts[tw][t - 1] if t > 0 else p for tw in group}
        both = None
        if len(group) == 2 and HEAD_PAIR_WGRAD:
            a, b = group
            both = dict(zip(group, ops.conv2d_wgrad_pair(xin[a], dz[a], xin[b], dz[b], Cin=w[a].shape[1], Cout=256, **_K3,
                                                         live32_b=lv((b,), 0, 4 - t))))
        for tw in reversed(group):
            G, dbp = both[tw] if both else ops.conv2d_wgrad(xin[tw], dz[tw], Cin=w[tw].shape[1], Cout=256, **_K3, split=split,
                                                            live32=lv((tw,), 0, 4 - t))
            dw = torch.empty_like(w[tw]); db = ops.unpack_wgrad(G, dw, dbias_part=dbp)
            g[f'{tw}_convs.{t}.weight'], g[f'{tw}_convs.{t}.bias'] = dw, db

    def towers_bwd(group):
        """the output convs of the group's towers, `reg` first, then per layer the weight gradient(s) and ONE data-gradient launch"""
        dz = {tw: tower_final(tw, *douts[tw]) for tw in reversed(group)}
        for t in range(3, -1, -1):
            layer_wgrads(group, t, dz)
            wd = {tw: ops.pack_weight(HP[f'{tw}_convs.{t}.weight'], dtype, mode=1, x3=split) for tw in group}
            if t > 0:
                dz, _ = _tower_layer(group, dz, wd, geo, 256, res={tw: acts[tw][t - 1] for tw in group}, res_mode=RES_RELU_MASK,
                                     split=split, live=lv(group, 1, 5 - t), units=lu(group, 5 - t))
            else:
                for tw in group:
                    last[tw] = (dz[tw], wd[tw])     # 256 -> Wc back to the neck: after the join (the towers' sum)

    if paired and split:          # the forward laid both towers' activations out pairwise: both towers in lockstep
        towers_bwd(('cls', 'reg'))
    else:
        # (the two towers on two streams, see HEAD_TWO_STREAMS: the deferred unpack jobs of both leave in the node's ONE tail launch, on
        #  the main stream, after the join -- hence no early flush in between)
        two = HEAD_TWO_STREAMS and ops.PROFILE is None
        ops.hold_tail_flush(two)
        try:
            with _Fork(dev, two) as fk:
                with fk.side():
                    towers_bwd(('reg',))
                towers_bwd(('cls',))
        finally:
            ops.hold_tail_flush(False)
    # back to plain fp32 for the neck (out_f32 in the split form): the first tower writes, the second accumulates onto it
    _, dp_maps = pyramid_alloc(B, sizes, Wc, dtype, dev)
    dz, wd = last['cls']
    ops.conv2d(dz, wd, dp_maps, Cin=256, Cout=Wc, **_K3, split=split, out_f32=split)
    dz, wd = last['reg']
    ops.conv2d(dz, wd, dp_maps, Cin=256, Cout=Wc, **_K3, res=dp_maps, res_mode=RES_ADD, split=split, out_f32=split, live=lv(('reg',), 1, 5),
               units=lu(('reg',), 5))
    return dp_maps, g
