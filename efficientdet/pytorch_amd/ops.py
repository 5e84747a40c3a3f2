"""Thin Python wrappers over the C ABI (raw device tensors in, raw device tensors out).

Plumbing only: PyTorch owns the memory and the stream; every numeric op is a HIP kernel in
libeffdet_hip.so.  No function here has a CPU path.
"""
import ctypes as C
import os
import threading

import numpy as np
import torch

from . import _lib as L
from ._lib import (ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_SWISH, RES_ADD, RES_NONE,  # noqa: F401
                   RES_RELU_MASK, RES_SWISH_GRAD)


class LaunchProfile:
    """Optional per-launch HIP-event timing of the MFMA kernels (bench.py's live roofline measurement).
    Events are recorded on the SAME stream the kernels are launched on (torch's current stream)."""

    def __init__(self):
        self.records = []          # (kernel symbol, algorithmic flops, start event, end event, shape note)

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, flops, e0, e1, _, nbytes in self.records:
            d = out.setdefault(name, {'launches': 0, 'flops': 0.0, 'ms': 0.0, 'bytes': 0.0})
            d['launches'] += 1; d['flops'] += flops; d['ms'] += e0.elapsed_time(e1); d['bytes'] += nbytes
        return out

    def by_shape(self, name, top=4):
        """The launches of one kernel symbol grouped by shape note, heaviest first (a symbol mixes MFMA-bound head shapes with
        HBM-bound backbone ones; this shows them apart)."""
        torch.cuda.synchronize()
        agg = {}
        for n, flops, e0, e1, note, _ in self.records:
            if n == name:
                d = agg.setdefault(note, {'launches': 0, 'flops': 0.0, 'ms': 0.0})
                d['launches'] += 1; d['flops'] += flops; d['ms'] += e0.elapsed_time(e1)
        rows = sorted(agg.items(), key=lambda kv: -kv[1]['ms'])[:top]
        return {k: {'launches': v['launches'], 'ms': round(v['ms'], 3), 'tflops': round(v['flops'] / (v['ms'] * 1e-3) / 1e12, 1)}
                for k, v in rows}


PROFILE = None     # set to a LaunchProfile() to time every conv launch


def _timed(name, flops, fn, note='', nbytes=0.0):
    """flops: algorithmic FLOPs of an MFMA launch (for the byte-counted kernels, whose notes start with 'BYTES': their algorithmic bytes);
    nbytes: algorithmic bytes of an MFMA launch (operands read once + outputs written once), next to the PMC traffic in the roofline."""
    if PROFILE is None:
        return fn()
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record(); r = fn(); e1.record()
    PROFILE.records.append((name, flops, e0, e1, note, nbytes))
    return r


# Arithmetic of the MFMA kernels on fp32 STORAGE (process-wide; EfficientDet(..., f32_arith=...) sets it):
#   'f32'    v_mfma_f32_16x16x4_f32 -- exact fp32 products (the strict parity mode)
#   'bf16x3' operands split into bf16 hi + lo in registers, 3 bf16 MFMAs per product (~16 mantissa bits), fp32 accumulate
# F32_ARITH is what the launches issued NOW use; F32_ARITH_BWD is what the autograd nodes recorded by the running forward will
# switch to in their backward.  A MODEL names the pair (MODEL_ARITH): 'f32' and 'bf16x3' use one arithmetic throughout;
# 'f32_bwd_bf16x3' computes every forward value -- the (classification, regression, anchors) triple of models/efficientdet.py:64-66,
# the losses, every ReLU / max-pool / IoU decision the backward depends on -- with exact fp32 products, bit for bit what 'f32'
# computes, and takes only the GRADIENT convolutions (data + weight gradients) through the three-product bf16 form: their ~1e-5
# product error lands on gradients whose masks were decided exactly, 100x inside the 1e-3 gradient gate.
# F32_ARITH_HEAD: arithmetic of the RetinaHead's FORWARD convs when F32_ARITH is 'f32' -- 'f32' (exact), or 'f16x3': operands as
# fp16 hi + scaled fp16 lo (22 significand bits), 3 fp16 MFMAs per product into one fp32 accumulator.  Per product ~2^-22 relative --
# below the rounding noise of the fp32 accumulation itself (measured: outputs within 1.2x of the exact mode's distance to a float64
# head) -- at the fp16 matrix rate: "fp32-equivalent", not bit-identical to the exact mode.
# 'f32_hf16x3_bwd_bf16x3' = that forward head + exact fp32 everywhere else in the forward + bf16x3 gradient convs.
F32_ARITH = 'f32'
F32_ARITH_BWD = 'f32'
F32_ARITH_HEAD = 'f32'
MODEL_ARITH = {'f32': ('f32', 'f32', 'f32'), 'bf16x3': ('bf16x3', 'bf16x3', 'f32'), 'f32_bwd_bf16x3': ('f32', 'bf16x3', 'f32'),
               'f32_hf16x3_bwd_bf16x3': ('f32', 'bf16x3', 'f16x3')}


def set_f32_arith(mode, bwd=None):
    """Arithmetic of the launches from now on (and, unless `bwd` says otherwise, of the backward of nodes recorded from now on)."""
    global F32_ARITH, F32_ARITH_BWD
    if mode not in ('f32', 'bf16x3') or (bwd is not None and bwd not in ('f32', 'bf16x3')):
        raise ValueError("f32_arith must be 'f32' or 'bf16x3'")
    old, F32_ARITH = F32_ARITH, mode
    F32_ARITH_BWD = mode if bwd is None else bwd
    return old


def set_model_arith(name):
    """A model's arithmetic by name (MODEL_ARITH): forward arithmetic now, its backward arithmetic for the nodes it records."""
    if name not in MODEL_ARITH:
        raise ValueError('f32_arith must be one of %s' % (sorted(MODEL_ARITH),))
    global F32_ARITH_HEAD
    fwd, bwd, head = MODEL_ARITH[name]
    set_f32_arith(fwd, bwd)
    F32_ARITH_HEAD = head


# Out-of-fp16-range watch of the f16x3 arithmetic: one device int per GPU that every H-split producer (pyramid conversion, BiFPN fusion,
# tower conv epilogues) ORs bit 0 into when a value cannot be held (|v| >= 65520 or NaN).  Created outside stream capture (the model's
# forward asks for it before anything else), never reset by the kernels.
_range_flags = {}


def range_flag(device):
    device = torch.device(device)
    key = device.index if (device.index is not None or device.type != 'cuda') else torch.cuda.current_device()
    t = _range_flags.get(key)
    if t is None:
        t = _range_flags[key] = torch.zeros(1, dtype=torch.int32, device=device)
    return t


def clear_range_flag(device):
    """Start a guarded call (detect(), a GraphedDetect replay) with a clean watch: what the next check reports is then that call's own
    overflow, not one left by a training step in between.  fill_ is an elementwise kernel on the current stream, so it is captured into a
    graph as a kernel node (a memset node did not hold inside captured graphs here, loss.hip zero_stat)."""
    range_flag(device).fill_(0)


def check_range_flag(device, what='f16x3'):
    """Host-side read of the watch (synchronises the current stream): raises -- and clears the flag -- if a value left fp16's range since
    the last check."""
    t = range_flag(device)
    if int(t.item()) != 0:
        t.zero_()
        raise FloatingPointError('%s: an activation of the RetinaHead / BiFPN left the range of the fp16 operand split (|x| >= 65520 or NaN); '
                                 "the outputs of this call are not valid -- use f32_arith='f32_bwd_bf16x3' or 'f32' for this model" % what)


class backward_scope:
    """with backward_scope(ctx.prep, ctx.arith): the body of an autograd node's backward -- this model's parameter arena and its BACKWARD
    arithmetic for the launches inside, and the arithmetic found at entry put back at exit, so that direct ops.conv2d / functional.* calls
    issued between a backward and the next model forward do not silently inherit the gradient arithmetic."""

    def __init__(self, prep, arith):
        self.prep, self.arith = prep, arith

    def __enter__(self):
        self.old = (F32_ARITH, F32_ARITH_BWD, F32_ARITH_HEAD)
        set_prep(self.prep); set_f32_arith(self.arith)
        return self

    def __exit__(self, et, ev, tb):
        global F32_ARITH, F32_ARITH_BWD, F32_ARITH_HEAD
        F32_ARITH, F32_ARITH_BWD, F32_ARITH_HEAD = self.old
        return False


def _mma_dtype_code(dtype, K=None, N=None):
    """dtype code of an MFMA launch.  For the dense conv (K, N given) the bf16x3 form also needs weights packed in its
    pre-split layout, so the SAME rule decides the pack (pack_weight) and the launch (conv2d): reduction length a
    multiple of 32 and long enough for the matrix pipe to be the bound."""
    code = L.dtype_code(dtype)
    if code != L.F32 or F32_ARITH != 'bf16x3':
        return code
    if K is not None and (K % 32 or K < 256 or N < 32):
        return code
    return L.F32_BF16X3


def _igemm_symbol(dtype, desc):
    """Kernel symbol the library will launch for this descriptor (profiling attribution only)."""
    kid = int(L.lib().effdet_conv2d_kernel(C.byref(desc)))
    if kid in (30, 31):
        return 'conv_igemm_kernel<hsplit,%d,f16x3>' % (128, 64)[kid - 30]
    if kid >= 10000:
        return 'conv_igemm_pers_kernel<split,bf16x3>'
    if kid == 20:
        return 'conv_pw_f32_kernel'
    if kid >= 10:
        v = str(kid - 10)
        return 'conv_igemm_pers_kernel<%s,%s,%s>' % (v[0], v[1], v[2])
    if kid in (8, 9):
        return 'conv_igemm_kernel<split,%d,bf16x3>' % (128, 64)[kid - 8]
    if 0 <= kid < 8 and dtype == torch.float32:
        # ids 0..7 name a channel-tile class; the short-tile instances (TUNE_SHORT_TILE) are told apart by the plan's pixel tile
        info = L.ConvPlanInfo()
        if int(L.require('effdet_conv2d_plan_info').effdet_conv2d_plan_info(C.byref(desc), C.byref(info))) == kid and info.tile_m < 128:
            return 'conv_igemm_kernel<f32,%d%s,short%d>' % (info.tile_n, ',bf16x3' if kid >= 4 else '', info.tile_m)
    if 4 <= kid < 8:
        return 'conv_igemm_kernel<f32,%d,bf16x3>' % (128, 64, 32, 16)[kid - 4]
    return 'conv_igemm_kernel<%s,%d>' % ('bf16' if dtype == torch.bfloat16 else 'f32', (128, 64, 32, 16)[max(kid, 0)])


class Map:
    """An NHWC feature-map view: element (b,h,w,c) at  t.data_ptr() + (off + b*bstride + (h*W+w)*ld + c)*itemsize."""
    __slots__ = ('t', 'B', 'H', 'W', 'C', 'ld', 'bstride', 'off')

    def __init__(self, t, B, H, W, C, ld=None, bstride=None, off=0):
        self.t, self.B, self.H, self.W, self.C = t, B, H, W, C
        self.ld = C if ld is None else ld
        self.bstride = H * W * self.ld if bstride is None else bstride
        self.off = off

    @staticmethod
    def new(B, H, W, C, dtype, device, zero=False):
        f = torch.zeros if zero else torch.empty
        return Map(f((B, H, W, C), dtype=dtype, device=device), B, H, W, C)

    @staticmethod
    def of(t):
        assert t.dim() == 4 and t.is_contiguous()
        return Map(t, t.shape[0], t.shape[1], t.shape[2], t.shape[3])

    @property
    def dtype(self):
        return self.t.dtype

    def addr(self):
        return self.t.data_ptr() + self.off * self.t.element_size()

    def tensor(self):
        """The [B,H,W,C] tensor (only for plain contiguous maps)."""
        assert self.ld == self.C and self.bstride == self.H * self.W * self.C and self.off == 0
        return self.t.view(self.B, self.H, self.W, self.C)


def _segs(desc, xs, ys, base_x, base_y, isz_x, isz_y):
    desc.nseg = len(xs)
    for i, (x, y) in enumerate(zip(xs, ys)):
        s = desc.seg[i]
        s.H, s.W, s.Ho, s.Wo = x.H, x.W, y.H, y.W
        dx = x.addr() - base_x
        dy = y.addr() - base_y
        assert dx % isz_x == 0 and dy % isz_y == 0
        s.in_off, s.in_bstride = dx // isz_x, x.bstride
        s.out_off, s.out_bstride = dy // isz_y, y.bstride


# ----------------------------------------------------------------------------- batched parameter preparation
PREP_PACK0, PREP_PACK1, PREP_BNFOLD, PREP_DWPACK = 0, 1, 2, 3

# Writers that change parameters through RAW POINTERS (effdet_clip_adamw_step, every replay of a captured train step) never
# move Tensor._version, which is what the inference-side "packed copies are still fresh" test looks at: they bump this
# process-wide generation instead (ClipAdamW.step, graph.GraphedTrainStep.__call__), and the fingerprint includes it.
_PARAM_GENERATION = 0


def bump_param_generation():
    global _PARAM_GENERATION
    _PARAM_GENERATION += 1



class ParamPrep:
    """Record / replay of the per-step parameter repacks (conv weight packs, frozen-BN folds, depthwise packs).

    The first step of a model runs them one by one (~190 four-microsecond launches for D0) and RECORDS each as a job of
    effdet_prepare_params; from the second step on begin_step() replays the whole table in ONE launch at the start of
    the forward pass and pack_weight / bn_fold / dw_pack_weight return views of its output arena.  Parameter storage
    must be stable (it is under in-place optimizers, load_state_dict and DDP); the owner drops the table when the
    module is moved (nn.Module._apply).  A lookup miss falls back to the single launch and re-records."""

    def __init__(self, f32_arith='f32'):
        self.f32_arith = f32_arith          # the owner's arithmetic by name (MODEL_ARITH; see set_model_arith)
        self.jobs, self.outs, self.bn_src = {}, {}, {}
        self.table, self.dirty, self.replay = None, False, False
        self._n0 = 0                        # jobs of the first build since the last reset (bounds the table's growth)
        self._fresh = None                  # (source version sum, stream) the arena was last refreshed for -- inference only
        self.zbuf, self.zpos, self.zreq, self.zsize = None, 0, 0, 0

    # -- zero-initialised scratch of one step (SE pools, bias / BN / fusion-weight accumulators): ONE memset per step
    #    instead of ~60; sized by what the previous step asked for, a fresh buffer every step (gradients may keep views)
    def _begin_zeros(self, device):
        self.zsize = max(self.zsize, self.zreq)
        self.zbuf = torch.zeros(self.zsize, dtype=torch.float32, device=device) if self.zsize else None
        self.zpos = self.zreq = 0

    def zeros(self, n, device):
        n64 = (n + 63) // 64 * 64
        self.zreq += n64
        if self.zbuf is not None and self.zpos + n64 <= self.zbuf.numel() and self.zbuf.device == device:
            v = self.zbuf[self.zpos:self.zpos + n]
            self.zpos += n64
            return v
        return torch.zeros(n, dtype=torch.float32, device=device)

    def reset(self):
        """Forget every recorded job (the next step records afresh)."""
        self.jobs, self.outs, self.bn_src = {}, {}, {}
        self.table, self.dirty, self.replay, self._fresh, self._n0 = None, False, False, None, 0

    def _sources_moved(self):
        """A recorded source tensor no longer lives where the job table says (p.data = ..., a parameter swapped for another
        tensor, replicas of nn.DataParallel): the device-side table would read stale or foreign memory."""
        for job in self.jobs.values():
            for t, a in zip(job[1], job[7]):
                if t is not None and t.data_ptr() != a:
                    return True
        return False

    def begin_step(self, device=None):
        if device is not None:
            self._begin_zeros(device)
        capturing = torch.cuda.is_current_stream_capturing()
        if self.jobs and not capturing:
            # pointer validation (jobs are keyed on addresses): re-record from scratch when a source moved, and keep the table
            # bounded -- lookups that miss every step (tensors re-created per forward) would otherwise grow it without limit
            if self._sources_moved() or (self.table is not None and len(self.jobs) > 2 * max(self._n0, 64)):
                self.reset()
        if self.dirty:
            self._build()
        self.replay = self.table is not None
        if self.replay:
            # Inference: the packed copies in the arena stay valid while no source tensor was written (torch optimizers,
            # load_state_dict, .copy_ all bump Tensor._version; the raw-pointer writers -- ClipAdamW, graph replays -- bump
            # _PARAM_GENERATION): skip the launch (0.05 ms of a 5 ms D0 forward, 0.2 of 12 for D4).
            # Never under graph capture (a captured forward must refresh them on every replay) nor with autograd on.
            fp = None
            if not torch.is_grad_enabled() and not capturing:
                fp = (self._version_sum(), _PARAM_GENERATION, torch.cuda.current_stream().cuda_stream)
                if fp == self._fresh:
                    return
            jobs, bj, bf, nblocks = self.table[:4]
            L.check(L.lib().effdet_prepare_params(L.ptr(jobs), L.ptr(bj), L.ptr(bf), nblocks, L.stream_ptr()), 'effdet_prepare_params')
            self._fresh = fp

    def _version_sum(self):
        return sum(t._version for job in self.jobs.values() for t in job[1] if t is not None)

    def lookup(self, key):
        return self.outs.get(key) if self.replay else None

    def record(self, key, kind, srcs, dims, dtype, shape, eps=0.0, code=None, work=None):
        """work: number of 1-per-thread work items of the job when it is not the number of output elements (the f16x3 pack: rows + row scales)."""
        if key not in self.jobs:
            self.jobs[key] = (kind, srcs, dims, dtype, shape, eps, L.dtype_code(dtype) if code is None else code,
                              tuple(t.data_ptr() if t is not None else 0 for t in srcs), work)
            self.dirty = True

    def _build(self):
        keys = list(self.jobs)
        dev = self.jobs[keys[0]][1][0].device
        offs, total = [], 0
        for k in keys:
            kind, srcs, dims, dtype, shape, eps = self.jobs[k][:6]
            n = 1
            for d in shape:
                n *= d
            offs.append((total, n)); total += (n * (2 if dtype == torch.bfloat16 else 4) + 255) // 256 * 256
        arena = torch.empty(total, dtype=torch.uint8, device=dev)
        arr = (L.PrepJob * len(keys))()
        block_job, block_first, nb = [], [], 0
        self.outs, self.bn_src = {}, {}      # (drop the pointers of record-time temporaries)
        for i, k in enumerate(keys):
            kind, srcs, dims, dtype, shape, eps, code = self.jobs[k][:7]
            off, n = offs[i]
            out = arena[off:off + n * (2 if dtype == torch.bfloat16 else 4)].view(dtype).view(shape)
            j = arr[i]
            ptrs = [t.data_ptr() if t is not None else None for t in srcs] + [None] * (4 - len(srcs))
            j.a, j.b, j.c, j.d = ptrs[:4]
            j.out, j.kind, j.dtype, j.eps = out.data_ptr(), kind, code, eps
            j.n0, j.n1, j.n2, j.n3, j.n4 = (list(dims) + [0] * 5)[:5]
            blocks = ((self.jobs[k][8] or n) + 255) // 256
            block_first.append(nb); block_job += [i] * blocks; nb += blocks
            self.outs[k] = out
            if kind == PREP_BNFOLD:
                self.bn_src[out[0].data_ptr()] = (srcs[0], srcs[3], eps)
        jobs_dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
        bj = torch.from_numpy(np.asarray(block_job, dtype=np.int32)).to(dev)
        bf = torch.from_numpy(np.asarray(block_first, dtype=np.int32)).to(dev)
        self.table, self.dirty, self._fresh = (jobs_dev, bj, bf, nb, arena), False, None
        if not self._n0:
            self._n0 = len(keys)


_tls = threading.local()     # .prep: the ParamPrep of the model whose forward / backward runs on this thread


def set_prep(p):
    _tls.prep = p
    if p is not None:
        set_model_arith(p.f32_arith)        # the model's forward arithmetic; its nodes' backward sets theirs (ctx.arith)


def get_prep():
    return getattr(_tls, 'prep', None)


def zeros(shape, device):
    """fp32 zeros, from the running model's per-step zero pool when there is one."""
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    n = 1
    for d in shape:
        n *= d
    prep = get_prep()
    device = torch.device(device)
    t = prep.zeros(n, device) if prep is not None else torch.zeros(n, dtype=torch.float32, device=device)
    return t.view(shape)


def pack_weight(w_oihw, dtype, mode=0, scale=None, cin_pad=None, x3=False, h3=False):
    """OIHW fp32 -> packed [Cout][taps][Cin_pad] (mode 0) or data-gradient operand [Cin][taps'][Cout] (mode 1).
    x3=True: always the pre-split bf16x3 operand layout (the convs on split-layout activations need it whatever the size).
    h3=True (mode 0, fp32 storage): the f16x3 forward operand (EFFDET_F32_HSPLIT) -- a flat fp32-typed buffer holding Cout rows of
    row-scaled [32 x f16 hi | 32 x f16 lo] groups followed by the Cout row scales 1 / S_n (conv2d(..., hsplit=True) finds them there)."""
    Cout, Cin, KH, KW = w_oihw.shape
    w = w_oihw.detach()
    assert w.dtype == torch.float32 and w.is_contiguous()
    if cin_pad is None:
        cin_pad = Cin if mode == 0 else Cout
    shape = (Cout, KH * KW, cin_pad) if mode == 0 else (Cin, KH * KW, cin_pad)
    code = L.F32_BF16X3 if x3 else _mma_dtype_code(dtype, KH * KW * cin_pad, shape[0])
    work = None
    if h3:
        assert mode == 0 and dtype == torch.float32 and not x3
        work = Cout * 256                                   # one 256-thread workgroup per output row (it derives the row's scale)
        code, shape = L.F32_HSPLIT, (Cout * KH * KW * cin_pad + Cout,)
    PREP = get_prep()
    if PREP is not None:
        bn = PREP.bn_src.get(scale.data_ptr()) if scale is not None else None
        if scale is None or bn is not None:
            key = ('pack', w.data_ptr(), mode, dtype, cin_pad, scale is not None, code)
            hit = PREP.lookup(key)
            if hit is not None:
                return hit
            PREP.record(key, PREP_PACK1 if mode else PREP_PACK0, (w_oihw, bn[0] if bn else None, bn[1] if bn else None),
                        (Cout, Cin, KH, KW, cin_pad), dtype, shape, bn[2] if bn else 0.0, code, work)
    out = torch.empty(shape, dtype=dtype, device=w.device)
    L.check(L.lib().effdet_pack_conv_weight(L.ptr(w), L.ptr(scale), L.ptr(out), code, mode,
                                            Cout, Cin, KH, KW, cin_pad, L.stream_ptr()), 'effdet_pack_conv_weight')
    return out


def scale_pack_weight(w_oihw, gate, dtype):
    """Per-image 1x1 weights W_b = W * diag(gate_b), packed for conv2d(..., w_image_stride=...): -> (packed [B][Cout][Cin], image
    stride in bytes).  The squeeze-excite gate of an MBConv block applied through the project conv's weights instead of a pass
    over the activations (models/efficientnet.py:86-95)."""
    Cout, Cin = w_oihw.shape[0], w_oihw.shape[1]
    assert w_oihw.shape[2:] == (1, 1) and gate.shape[1] == Cin and gate.dtype == torch.float32 and gate.is_contiguous()
    B = gate.shape[0]
    code = _mma_dtype_code(dtype, Cin, Cout)
    out = torch.empty((B, Cout, Cin), dtype=dtype, device=gate.device)
    L.check(L.lib().effdet_scale_pack_weight(L.ptr(w_oihw.detach()), L.ptr(gate), L.ptr(out), code, B, Cout, Cin, L.stream_ptr()),
            'effdet_scale_pack_weight')
    return out, Cout * Cin * out.element_size()


def _conv_desc(xs, wp, ys, *, Cin, Cout, KH, KW, stride=1, pad_t=0, pad_l=0, scale=None, shift=None, act=ACT_NONE,
               res=None, res_mode=RES_NONE, rowscale=None, zs=None, out_f32=False, split=False, bc_scale=None, bc_shift=None,
               w_image_stride=0, ysplit=None, hsplit=False, seg_w=None, seg_shift=None, live=None, live_tile0=0, needed=None, needed_tile0=0):
    """The effdet_conv_t of a conv2d(...) call -> (descriptor, xs, ys as lists).  The one place it is built: conv2d launches from it and
    conv2d_plan_info asks the planner about it, so the query describes the launch conv2d makes."""
    if isinstance(xs, Map):
        xs, ys = [xs], [ys]
        zs = [zs] if zs is not None else None
        res = [res] if res is not None else None
        ysplit = [ysplit] if ysplit is not None else None
    d = L.ConvDesc()
    x0, y0 = xs[0], ys[0]
    isx, isy = x0.t.element_size(), y0.t.element_size()
    base_x = min(x.addr() for x in xs)
    base_y = min(y.addr() for y in ys)
    d.x, d.w, d.y = base_x, wp.data_ptr(), base_y
    d.z = d.res = None
    if zs is not None:
        # z/res share the output addressing: same relative offsets as ys
        bz = min(z.addr() for z in zs)
        for y, z in zip(ys, zs):
            assert (z.addr() - bz) * isy == (y.addr() - base_y) * z.t.element_size() and z.ld == y.ld and z.bstride == y.bstride
        d.z = bz
    if res is not None:
        br = min(r.addr() for r in res)
        for y, r in zip(ys, res):
            assert (r.addr() - br) * isy == (y.addr() - base_y) * r.t.element_size() and r.ld == y.ld and r.bstride == y.bstride
        d.res = br
    d.y_split = None
    d.range_flag = range_flag(x0.t.device).data_ptr() if (hsplit and not out_f32) else None
    for i in range(len(xs)):
        d.seg_w[i] = seg_w[i].data_ptr() if (seg_w is not None and seg_w[i] is not None) else None
        d.seg_shift[i] = seg_shift[i].data_ptr() if (seg_shift is not None and seg_shift[i] is not None) else None
    if ysplit is not None:
        bs = min(q.addr() for q in ysplit)
        for y, q in zip(ys, ysplit):
            assert (q.addr() - bs) == (y.addr() - base_y) and q.t.element_size() == isy and q.ld == y.ld and q.bstride == y.bstride
        d.y_split = bs
    d.scale, d.shift, d.rowscale = (t.data_ptr() if t is not None else None for t in (scale, shift, rowscale))
    d.bc_scale, d.bc_shift = (t.data_ptr() if t is not None else None for t in (bc_scale, bc_shift))     # [B][Cout] fp32, after rowscale, before res
    assert not (hsplit and (split or scale is not None))
    d.dtype, d.out_f32 = (L.F32_HSPLIT if hsplit else (L.F32_SPLIT if split else _mma_dtype_code(x0.dtype, KH * KW * Cin, Cout))), int(out_f32)
    d.B, d.Cin, d.Cout, d.KH, d.KW = x0.B, Cin, Cout, KH, KW
    d.stride, d.pad_t, d.pad_l = stride, pad_t, pad_l
    d.ldx, d.ldy = x0.ld, y0.ld
    d.act, d.res_mode = act, res_mode
    d.w_image_stride = int(w_image_stride)       # bytes; image b reads its own packed weights (scale_pack_weight)
    _segs(d, xs, ys, base_x, base_y, isx, isy)
    # live / needed are one (kind, tile flags, first tile) triple from here on: checked once, and what conv2d launches from
    assert live is None or needed is None
    kind, flags, tile0 = ('live', live, live_tile0) if live is not None else ('needed', needed, needed_tile0) if needed is not None else (None, None, 0)
    if kind is not None:
        assert flags.dtype == torch.uint8 and flags.is_contiguous()
        ntile = sum((y.B * y.H * y.W + 127) // 128 for y in ys)
        assert 0 <= tile0 <= ntile and flags.numel() == ntile - tile0, (flags.numel(), ntile, tile0)
    d.tile_flags = (kind, flags, tile0)          # (a Python attribute of the descriptor object: not part of effdet_conv_t)
    return d, xs, ys


def conv2d(xs, wp, ys, *, Cin, Cout, KH, KW, stride=1, pad_t=0, pad_l=0, scale=None, shift=None, act=ACT_NONE,
           res=None, res_mode=RES_NONE, rowscale=None, zs=None, out_f32=False, split=False, bc_scale=None, bc_shift=None,
           w_image_stride=0, ysplit=None, hsplit=False, seg_w=None, seg_shift=None, live=None, live_tile0=0, needed=None, needed_tile0=0,
           a_gate=None, a_act=ACT_NONE, units=None):
    """Grouped implicit-GEMM conv: xs/ys (and optional zs/res) are lists of Map, one per pyramid level.
    a_gate ([B][Cin] fp32, with a_act = ACT_NONE or ACT_SWISH): the conv runs on act(xs) * a_gate[image][channel], formed in the kernel's
    operand registers (effdet_conv2d_gated) -- bit for bit conv2d(channel_scale(xs, a_gate, a_act), ...) without that pass.  Exact-fp32
    1x1 convs on one map whose images are whole 128-pixel tiles (conv2d_gated_ok); anything else raises.
    split=True (EFFDET_F32_SPLIT): xs hold the split layout ([32 x bf16 hi | 32 x bf16 lo] per 32 channels, 4 B per element), wp
    is packed for bf16x3; ys are written split too unless out_f32 (then plain fp32; res, if any, is plain and ADDed).
    ysplit (exact-fp32 and f16x3 convs only): Maps addressed like ys that receive the output a second time in the split layout.
    hsplit=True (EFFDET_F32_HSPLIT, the f16x3 forward arithmetic): xs hold the H-split layout ([32 x f16 hi | 32 x f16 lo * 2^11] per 32
    channels), wp = pack_weight(..., h3=True); ys are written H-split too unless out_f32; no scale / res / rowscale.
    seg_w / seg_shift (lists, one entry per map, None = wp / shift): the maps are INDEPENDENT convs of one geometry with their own packed
    weights / bias rows -- the same layer of the head's two towers in one launch (<= 10 maps).  Same values as separate launches.
    live (uint8 tensor, one byte per 128-pixel tile from tile live_tile0 on: live_tiles()[1][r]): a 0 marks a tile whose every input
    tap is zero; the split-layout kernels without bias / affine / activation skip it (zeros out, or nothing under an in-place RES_ADD),
    every other launch ignores the flags.  Same values as without, but 0 where the dense launch would give 0 * Inf = NaN.
    needed (uint8 tensor, one byte per 128-pixel tile from tile needed_tile0 on: needed_tiles()[r]): a 0 marks a tile whose result
    nobody reads; the f16x3 kernels (hsplit) do not compute it and write zeros into every output stream (ys, ysplit) instead, every
    other launch ignores the flags.  The needed tiles hold what the dense launch gives them.
    units (with live or needed; UnitLists.row(r) of the same radius): the gathered form of the flagged launch (include/effdet_unit_lists.h)
    -- the flagged 32-pixel units, four to a tile, are computed and every other row is zero bytes.  Where the planner or the device-side
    count declines it the launch is the one with the tile flags; a launch that takes no flags at all raises."""
    d, xs, ys = _conv_desc(xs, wp, ys, Cin=Cin, Cout=Cout, KH=KH, KW=KW, stride=stride, pad_t=pad_t, pad_l=pad_l, scale=scale, shift=shift,
                           act=act, res=res, res_mode=res_mode, rowscale=rowscale, zs=zs, out_f32=out_f32, split=split, bc_scale=bc_scale,
                           bc_shift=bc_shift, w_image_stride=w_image_stride, ysplit=ysplit, hsplit=hsplit, seg_w=seg_w, seg_shift=seg_shift,
                           live=live, live_tile0=live_tile0, needed=needed, needed_tile0=needed_tile0)
    x0, y0 = xs[0], ys[0]
    isx, isy = x0.t.element_size(), y0.t.element_size()
    flops = 2.0 * KH * KW * Cin * Cout * sum(y.B * y.H * y.W for y in ys)
    # algorithmic bytes: the input map, the packed weights, every output stream (y, the pre-activation copy, the split copy), the residual
    nbytes = isx * Cin * sum(x.B * x.H * x.W for x in xs) + wp.numel() * wp.element_size() + \
        (4 if out_f32 else isy) * Cout * sum(y.B * y.H * y.W for y in ys) * (1 + (zs is not None) + (ysplit is not None) + (res is not None))
    kind, flags, tile0 = d.tile_flags
    key = (a_gate is not None, kind, units is not None)
    assert key in _CONV_CALLS, key
    name, args = _CONV_CALLS[key], []        # the entry point's own arguments, between descriptor and stream
    if a_gate is not None:
        assert a_gate.dtype == torch.float32 and a_gate.is_contiguous() and a_gate.shape == (x0.B, Cin)
        args = [a_gate.data_ptr(), int(a_act)]
    if units is not None:
        f32, ulist, ucount = units
        assert f32.dtype == torch.uint8 and f32.is_contiguous() and ulist.dtype == torch.int32 and ulist.is_contiguous()
        assert ucount.dtype == torch.int32 and ucount.is_contiguous() and ucount.numel() == L.UNIT_COUNTS
        nstep, t_ = 0, 0                       # steps of the flagged segments: those from tile tile0 on
        for y in ys:
            if t_ >= tile0:
                nstep += (y.B * y.H * y.W + 31) // 32
            t_ += (y.B * y.H * y.W + 127) // 128
        assert f32.numel() == nstep and ulist.numel() == nstep, (f32.numel(), ulist.numel(), nstep)
        args = [f32.data_ptr(), ulist.data_ptr(), ucount.data_ptr()]
        UNIT_LAUNCHES[0] += 1
    if kind is not None:
        args = [flags.data_ptr()] + args + [int(tile0)]          # (tile flags, [unit lists,] first tile)
        NEEDED_LAUNCHES[0] += kind == 'needed'

    def run():
        L.check(getattr(L.require(name), name)(C.byref(d), *args, L.stream_ptr()), name)
        GATE_OPERAND_LAUNCHES[0] += a_gate is not None
    # (flops stay those of the dense launch: a flagged launch reports an EFFECTIVE rate)
    _timed(_igemm_symbol(x0.dtype, d) if PROFILE is not None else '', flops, run,
           'k%d s%d Cin%d Cout%d M%d' % (KH, stride, Cin, Cout, sum(y.B * y.H * y.W for y in ys)), nbytes=float(nbytes))


NEEDED_LAUNCHES = [0]        # conv2d(..., needed=...) calls made so far (tests: which path a step took)
UNIT_LAUNCHES = [0]          # conv2d(..., units=...) calls made so far
GATE_OPERAND_LAUNCHES = [0, 0]     # conv2d(..., a_gate=...) / conv2d_wgrad(..., a_gate=...) calls made so far (tests: which path a step took)
# conv2d's library call by (a_gate given, kind of tile flags, units given); every other combination is refused
_CONV_CALLS = {(False, None, False): 'effdet_conv2d', (True, None, False): 'effdet_conv2d_gated',
               (False, 'live', False): 'effdet_conv2d_live', (False, 'needed', False): 'effdet_conv2d_needed',
               (False, 'live', True): 'effdet_conv2d_live_units', (False, 'needed', True): 'effdet_conv2d_needed_units'}


def conv2d_gated_plan_info(xs, wp, ys, a_gate, a_act=ACT_NONE, **kw):
    """conv2d_plan_info for conv2d(xs, wp, ys, a_gate=a_gate, a_act=a_act, **kw) (effdet_conv2d_gated_plan_info: no device work) -> its
    dict plus 'gate' (the form the launch takes: 1 = x * gate, 2 = swish(x) * gate), or None where the planner answers
    EFFDET_EUNSUPPORTED; other refusals raise."""
    d, _, _ = _conv_desc(xs, wp, ys, **kw)
    info = L.ConvPlanInfo()
    rc = int(L.require('effdet_conv2d_gated_plan_info').effdet_conv2d_gated_plan_info(C.byref(d), a_gate.data_ptr(), int(a_act), C.byref(info)))
    if rc == -3:
        return None
    if rc < 0:
        L.check(rc, 'effdet_conv2d_gated_plan_info')
    return dict(_plan_info_dict(info), gate=int(info.reserved[0]))


def conv2d_gated_ok(xs, wp, ys, a_gate, a_act=ACT_NONE, **kw):
    """Does the planner accept conv2d(xs, wp, ys, a_gate=a_gate, a_act=a_act, **kw)?  False: the caller materialises channel_scale's
    output instead."""
    info = conv2d_gated_plan_info(xs, wp, ys, a_gate, a_act, **kw)
    return info is not None and info['gate'] == (2 if a_act == ACT_SWISH else 1)


def conv2d_wgrad_gated_ok(x, dz, a_gate, a_act=ACT_NONE, *, Cin, Cout, KH=1, KW=1, image_splits=True):
    """Does the planner accept conv2d_wgrad(x, dz, ..., a_gate=a_gate, a_act=a_act)?  (effdet_conv2d_wgrad_gated_kernel: no device work.)"""
    rc = _wgrad_gated_kernel(_wgrad_desc([x], [dz], None, None, Cin, Cout, KH, KW, 1, 0, 0, True, False, image_splits), a_gate, a_act)
    if rc < 0 and rc != -3:
        L.check(rc, 'effdet_conv2d_wgrad_gated_kernel')
    return rc >= 0


def _wgrad_gated_kernel(d, a_gate, a_act):
    """effdet_conv2d_wgrad_gated_kernel on a descriptor: the path of the operand-gate launch, or the (negative) code it is refused with"""
    return int(L.require('effdet_conv2d_wgrad_gated_kernel').effdet_conv2d_wgrad_gated_kernel(C.byref(d), a_gate.data_ptr(), int(a_act)))


def conv2d_plan_info(xs, wp, ys, **kw):
    """What conv2d(xs, wp, ys, **kw) would launch, asked of the library's own planner without device work (effdet_conv2d_plan_info) on the
    descriptor conv2d builds (_conv_desc; the tensors only lend their addresses and may live on the host) -> dict of id, form ('plain',
    'bf16x3', 'split', 'hsplit', 'skinny'), persistent, tile_m, tile_n, stages, threads, mtiles, ntiles, grid (a persistent kernel: its
    tile count before the cap at the device's compute units), ksteps, kord, lds_bytes, m32.  Raises where conv2d would."""
    d, _, _ = _conv_desc(xs, wp, ys, **kw)
    info = L.ConvPlanInfo()
    rc = int(L.require('effdet_conv2d_plan_info').effdet_conv2d_plan_info(C.byref(d), C.byref(info)))
    if rc < 0:
        L.check(rc, 'effdet_conv2d_plan_info')
    return _plan_info_dict(info)


def _plan_info_dict(info):
    """effdet_conv_plan_info_t -> the dict of conv2d_plan_info / conv2d_gated_plan_info"""
    out = {n: int(getattr(info, n)) for n, _ in L.ConvPlanInfo._fields_ if n != 'reserved'}
    out['form'] = L.CONV_FORMS[out['form']]
    out['persistent'], out['m32'] = bool(out['persistent']), bool(out['m32'])
    return out


def _wgrad_desc(xs, dzs, dw, dbias, Cin, Cout, KH, KW, stride, pad_t, pad_l, want_bias, split, image_splits):
    d = L.WgradDesc()
    x0, z0 = xs[0], dzs[0]
    isz = x0.t.element_size()
    base_x = min(x.addr() for x in xs)
    base_z = min(z.addr() for z in dzs)
    d.x, d.dz = base_x, base_z
    d.dw = dw.data_ptr() if dw is not None else None
    d.dbias = dbias.data_ptr() if dbias is not None else (1 if (want_bias and dw is None) else None)    # dw None: only a request flag
    d.dtype = L.F32_SPLIT if split else _mma_dtype_code(x0.dtype)     # split: both operands in the split layout (see conv2d)
    d.B, d.Cin, d.Cout, d.KH, d.KW = x0.B, Cin, Cout, KH, KW
    d.stride, d.pad_t, d.pad_l = stride, pad_t, pad_l
    d.ldx, d.lddz = x0.ld, z0.ld
    d.image_splits = int(image_splits)        # split-K boundaries on image boundaries: slabs [B*q], slab s = image s // q (one level only)
    _segs(d, xs, dzs, base_x, base_z, isz, z0.t.element_size())
    return d


def conv2d_wgrad_kernel_id(x, dz, *, Cin, Cout, KH, KW, stride=1, pad_t=0, pad_l=0, split=False, image_splits=False, a_gate=None,
                           a_act=ACT_NONE):
    """Which kernel conv2d_wgrad would launch for one map pair (effdet_conv2d_wgrad_kernel): 0 tiled, 1 thin pointwise, 2 split;
    with a_gate: the operand-gate launch's (effdet_conv2d_wgrad_gated_kernel), negative where it is refused."""
    d = _wgrad_desc([x], [dz], None, None, Cin, Cout, KH, KW, stride, pad_t, pad_l, True, split, image_splits)
    return _wgrad_gated_kernel(d, a_gate, a_act) if a_gate is not None else int(L.lib().effdet_conv2d_wgrad_kernel(C.byref(d)))


def conv2d_wgrad_plan_info(xs, dzs, dw=None, dbias=None, *, Cin, Cout, KH, KW, stride=1, pad_t=0, pad_l=0, want_bias=True, split=False,
                           image_splits=False, **_launch_only):
    """What conv2d_wgrad(xs, dzs, ...) would launch, asked of the library's own planner without device work
    (effdet_conv2d_wgrad_plan_info) on the descriptor conv2d_wgrad builds (_wgrad_desc; the tensors only lend their addresses and may live
    on the host; group / live32 do not change the plan) -> dict of path ('tiled', 'thin', 'split', 'stem'), splits, nfast, mchunk, ntiles,
    jtiles, stage_pixels, allr, thin_ns, gate, first and count (lists, one entry per map).  Raises where conv2d_wgrad would."""
    if isinstance(xs, Map):
        xs, dzs = [xs], [dzs]
    return _wgrad_plan(_wgrad_desc(xs, dzs, dw, dbias, Cin, Cout, KH, KW, stride, pad_t, pad_l, want_bias, split, image_splits))


def _wgrad_plan(d, refused=None):
    """The library's plan for a descriptor, asked once (effdet_conv2d_wgrad_plan_info) -> the dict of conv2d_wgrad_plan_info.  A refused
    plan raises RuntimeError(refused), or (refused None) the library's code as L.check words it."""
    info = L.WgradPlanInfo()
    rc = int(L.require('effdet_conv2d_wgrad_plan_info').effdet_conv2d_wgrad_plan_info(C.byref(d), C.byref(info)))
    if rc < 0:
        if refused is not None:
            raise RuntimeError(refused)
        L.check(rc, 'effdet_conv2d_wgrad_plan_info')
    out = {n: int(getattr(info, n)) for n, _ in L.WgradPlanInfo._fields_ if n not in ('first', 'count', 'reserved', 'nseg')}
    out['path'], out['allr'] = L.WGRAD_PATHS[out['path']], bool(out['allr'])
    out['first'], out['count'] = list(info.first[:info.nseg]), list(info.count[:info.nseg])
    return out


def _wgrad_views(ws, splits, Cout, taps, Cin, bias, first=0, count=None):
    """The head of a workspace in effdet_conv2d_wgrad's layout -> (slabs [splits][Cout][taps][Cin], bias partial rows [splits][Cout] or
    None); first, count: that slab range only (one problem of a grouped launch)."""
    n, r = Cout * taps * Cin, slice(first, splits if count is None else first + count)
    return ws[:splits * n].view(splits, Cout, taps, Cin)[r], (ws[splits * n:splits * (n + Cout)].view(splits, Cout)[r] if bias else None)


def _wgrad_workspace(ws, floats, device):
    """The caller's workspace (a contiguous fp32 tensor of at least `floats` elements, e.g. pre-filled by a test) or a fresh one."""
    if ws is None:
        return torch.empty(floats, dtype=torch.float32, device=device)
    assert ws.dtype == torch.float32 and ws.is_contiguous() and ws.dim() == 1 and ws.numel() >= floats and ws.device == torch.device(device)
    return ws[:floats]


def conv2d_wgrad(xs, dzs, dw=None, dbias=None, *, Cin, Cout, KH, KW, stride=1, pad_t=0, pad_l=0, want_bias=True, split=False,
                 image_splits=False, group=False, live32=None, a_gate=None, a_act=ACT_NONE, ws=None):
    """Weight gradient -> (slabs [splits][Cout][taps][Cin] fp32, bias partial rows [splits][Cout] fp32 or None): the UNREDUCED
    split-K partials for unpack_wgrad / unpack_wgrad_bn to sum, in slab order, while unpacking (no float atomics anywhere: two
    runs are bitwise equal).  With dw given (packed [Cout][taps][Cin] fp32) the library reduces itself: dw += ..., dbias += ...
    group=True (dw None, <= 5 maps): the maps are INDEPENDENT problems of the same conv geometry (different tensors, different
    weights) sharing one launch -> a list of (slabs_i, parts_i), one per map (the plan's first / count).
    live32 (split only; uint8 tensor, one byte per 32-pixel step of dzs: live_tiles()[0][r]): a 0 marks a step whose dz pixels are all
    zero; every split-K block walks only its live steps.  Same slabs and bias rows as without.
    a_gate ([B][Cin] fp32, with a_act = ACT_NONE or ACT_SWISH; image_splits, one 1x1 map pair): the gradient against
    act(xs) * a_gate[image][channel], formed in the kernels' operand registers (effdet_conv2d_wgrad_gated) -- bit for bit
    conv2d_wgrad(channel_scale(xs, a_gate, a_act), ...) without that pass; raises where the planner refuses (conv2d_wgrad_gated_ok).
    ws (default: a fresh torch.empty): the caller's own fp32 workspace of at least splits * (Cout * taps * Cin + Cout) floats; the
    results are views of its head (tests pre-fill it, so that a slab no workgroup wrote shows)."""
    if isinstance(xs, Map):
        xs, dzs = [xs], [dzs]
    x0 = xs[0]
    d = _wgrad_desc(xs, dzs, dw, dbias, Cin, Cout, KH, KW, stride, pad_t, pad_l, want_bias, split, image_splits)
    flops = 2.0 * KH * KW * Cin * Cout * sum(z.B * z.H * z.W for z in dzs)
    plan = _wgrad_plan(d, 'effdet_conv2d_wgrad: unsupported geometry')
    splits, n = plan['splits'], Cout * KH * KW * Cin
    ws = _wgrad_workspace(ws, splits * (n + Cout), x0.t.device)
    name, args = 'effdet_conv2d_wgrad', (L.ptr(ws), ws.numel() * 4)
    if a_gate is not None:
        assert live32 is None and not group and a_gate.dtype == torch.float32 and a_gate.is_contiguous() and a_gate.shape == (x0.B, Cin)
        name, args = 'effdet_conv2d_wgrad_gated', (a_gate.data_ptr(), int(a_act)) + args
    elif live32 is not None:
        assert split and live32.dtype == torch.uint8 and live32.is_contiguous()
        assert live32.numel() == sum((z.B * z.H * z.W + 31) // 32 for z in dzs)
        name, args = 'effdet_conv2d_wgrad_live', args + (live32.data_ptr(),)

    def run():
        L.check(getattr(L.require(name), name)(C.byref(d), *args, L.stream_ptr()), name)
        GATE_OPERAND_LAUNCHES[1] += a_gate is not None
    # (bf16: DMA + LDS-transpose-read kernel, fp32: DMA + direct-operand kernel; levels neither can take use the register-transpose kernel)
    _timed('conv_wgrad_tr_kernel<8>' if x0.dtype == torch.bfloat16 else
           'conv_wgrad_split_kernel' if split else
           'conv_wgrad_thin_kernel' if plan['path'] in ('thin', 'stem') else
           'conv_wgrad_f32dma_kernel<4,bf16x3>' if d.dtype == L.F32_BF16X3 else 'conv_wgrad_f32dma_kernel<8>', flops,
           run,
           'k%d s%d Cin%d Cout%d M%d' % (KH, stride, Cin, Cout, sum(z.B * z.H * z.W for z in dzs)),
           nbytes=float(x0.t.element_size() * Cin * sum(x.B * x.H * x.W for x in xs) +
                        dzs[0].t.element_size() * Cout * sum(z.B * z.H * z.W for z in dzs) + 4.0 * splits * (n + Cout)))
    if group:
        assert dw is None and not image_splits
        return [_wgrad_views(ws, splits, Cout, KH * KW, Cin, d.dbias, f, c) for f, c in zip(plan['first'], plan['count'])]
    return _wgrad_views(ws, splits, Cout, KH * KW, Cin, d.dbias)


def conv2d_wgrad_pair(xs_a, dzs_a, xs_b, dzs_b, *, Cin, Cout, KH, KW, stride=1, pad_t=0, pad_l=0, want_bias=True, live32_b=None, ws=None):
    """conv2d_wgrad(xs_a, dzs_a, split=True) and conv2d_wgrad(xs_b, dzs_b, split=True, live32=live32_b) as ONE launch
    (effdet_conv2d_wgrad_pair: two split-layout problems of one geometry, e.g. the same layer of the RetinaHead's two towers)
    -> ((slabs_a, parts_a), (slabs_b, parts_b)), views of one workspace, bit for bit what the two separate launches leave.
    live32_b: problem b's step flags (see conv2d_wgrad) or None for two dense problems; problem a is always dense.
    ws: the caller's own workspace for both problems (see conv2d_wgrad)."""
    if isinstance(xs_a, Map):
        xs_a, dzs_a = [xs_a], [dzs_a]
    if isinstance(xs_b, Map):
        xs_b, dzs_b = [xs_b], [dzs_b]
    lib_ = L.require('effdet_conv2d_wgrad_pair')
    ds = [_wgrad_desc(xs, dzs, None, None, Cin, Cout, KH, KW, stride, pad_t, pad_l, want_bias, True, False)
          for xs, dzs in ((xs_a, dzs_a), (xs_b, dzs_b))]
    splits = [_wgrad_plan(d, 'effdet_conv2d_wgrad_pair: unsupported geometry')['splits'] for d in ds]
    n = Cout * KH * KW * Cin
    ws = _wgrad_workspace(ws, sum(splits) * (n + Cout), xs_a[0].t.device)
    nbytes = ws.numel() * 4
    if live32_b is not None:
        assert live32_b.dtype == torch.uint8 and live32_b.is_contiguous()
        assert live32_b.numel() == sum((z.B * z.H * z.W + 31) // 32 for z in dzs_b)
    run = lambda: L.check(lib_.effdet_conv2d_wgrad_pair(C.byref(ds[0]), C.byref(ds[1]), L.ptr(ws), nbytes, L.ptr(live32_b), L.stream_ptr()),
                          'effdet_conv2d_wgrad_pair')
    # (flops stay those of the two dense launches: a flagged half reports an EFFECTIVE rate)
    pix = sum(z.B * z.H * z.W for z in dzs_a) + sum(z.B * z.H * z.W for z in dzs_b)
    _timed('conv_wgrad_split_kernel', 2.0 * KH * KW * Cin * Cout * pix, run, 'pair k%d s%d Cin%d Cout%d M%d' % (KH, stride, Cin, Cout, pix),
           nbytes=float(xs_a[0].t.element_size() * Cin * (sum(x.B * x.H * x.W for x in xs_a) + sum(x.B * x.H * x.W for x in xs_b)) +
                        dzs_a[0].t.element_size() * Cout * pix + 4.0 * sum(splits) * (n + Cout)))
    return (_wgrad_views(ws, splits[0], Cout, KH * KW, Cin, want_bias),
            _wgrad_views(ws[splits[0] * (n + Cout):], splits[1], Cout, KH * KW, Cin, want_bias))


class _TailBatch:
    """Deferred leaf work of one backward node (effdet_backward_tail): inside ``with unpack_batch():`` unpack_wgrad /
    unpack_wgrad_bn / dw_unpack_wgrad_bn / the parameter-gradient half of se_gate_bwd only record a job (outputs are allocated
    right away, inputs stay referenced here) and the whole list goes out as one launch per 24 jobs when the block exits.
    Nothing inside the block may READ these outputs."""

    def __init__(self):
        self.jobs, self.keep, self.bytes = [], [], 0

    def add(self, kind, job, *tensors):
        t = L.TailJob()
        t.kind = kind
        if kind == L.TAIL_UNPACK:
            t.u.conv = job
        elif kind == L.TAIL_SE_PARAMS:
            t.u.se = job
        else:
            t.u.dw = job
        self.jobs.append(t); self.keep.append(tensors)
        # the deferred jobs pin their split-K slab workspaces (tens of MB per head conv): bound the lifetime, not only the launch
        # size -- past the byte budget the jobs recorded so far leave now and their inputs go back to the allocator
        self.bytes += sum(x.numel() * x.element_size() for x in tensors if isinstance(x, torch.Tensor))
        if self.bytes > TAIL_KEEP_BYTES and not getattr(_tls, 'hold_tail', False):
            self.flush()

    def flush(self):
        if self.jobs:
            arr = (L.TailJob * len(self.jobs))(*self.jobs)
            L.check(L.lib().effdet_backward_tail(arr, len(self.jobs), L.stream_ptr()), 'effdet_backward_tail')
        self.jobs, self.keep, self.bytes = [], [], 0


UNPACK_BATCHED = os.environ.get('EFFDET_UNPACK_BATCH', '1') != '0'      # A/B switch: 0 = every tail job is its own launch
TAIL_KEEP_BYTES = int(os.environ.get('EFFDET_TAIL_KEEP_MB', '2048')) << 20  # flush early once the deferred jobs pin this much workspace (256 MB split the
# D0 head's ten unpacks over three launches: 515 -> 704 us of tail time per step; the chains of few jobs do not fill the GPU)


def hold_tail_flush(on):
    """While on, the open tail batch of this thread never flushes early (its jobs were recorded under more than one stream: they may only
    be launched by the owner of the batch, after the streams have joined)."""
    _tls.hold_tail = bool(on)


def _cur_batch():
    """The open tail batch of THIS thread (thread-local like the ParamPrep pointer: replica backwards of a multi-device
    nn.DataParallel run concurrently on per-device autograd threads and must never see each other's batch)."""
    return getattr(_tls, 'unpack_batch', None)


class unpack_batch:
    """Context manager: batch the tail jobs (see _TailBatch) issued inside into one launch at exit (re-entrant: an inner block
    joins the outer one)."""

    def __enter__(self):
        self.owner = _cur_batch() is None and UNPACK_BATCHED
        if self.owner:
            _tls.unpack_batch = _TailBatch()
        return self

    def __exit__(self, et, ev, tb):
        if self.owner:
            b, _tls.unpack_batch = _tls.unpack_batch, None
            if et is None:
                b.flush()
        return False


def _unpack_job(g, dw, Cout, Cin, KH, KW, cin_pad, nslabs, slab_scale, slab_cscale=None, **ptrs):
    j = L.UnpackJob()
    j.g, j.dw_oihw, j.slab_scale = g.data_ptr(), dw.data_ptr(), (slab_scale.data_ptr() if slab_scale is not None else None)
    for k, t in ptrs.items():
        setattr(j, k, t.data_ptr() if t is not None else None)
    j.Cout, j.Cin, j.KH, j.KW, j.Cin_pad, j.nslabs = Cout, Cin, KH, KW, (Cin if cin_pad is None else cin_pad), nslabs
    j.slabs_per_scale = nslabs // slab_scale.numel() if slab_scale is not None else 1
    if slab_cscale is not None:      # [images][Cin_pad] per-input-channel factors (the SE gate): slab s belongs to image s // slabs_per_scale
        assert slab_cscale.dtype == torch.float32 and slab_cscale.is_contiguous() and slab_cscale.shape[1] == j.Cin_pad
        assert nslabs % slab_cscale.shape[0] == 0 and (slab_scale is None or slab_scale.numel() == slab_cscale.shape[0])
        j.slab_cscale = slab_cscale.data_ptr()
        j.slabs_per_scale = nslabs // slab_cscale.shape[0]
    return j


def _unpack_submit(job, *tensors):
    batch = _cur_batch()
    if batch is not None:
        batch.add(L.TAIL_UNPACK, job, *tensors)
    else:
        L.check(L.lib().effdet_unpack_conv_wgrad_batch(C.byref(job), 1, L.stream_ptr()), 'effdet_unpack_conv_wgrad_batch')


def unpack_wgrad(g, dw_oihw, scale=None, w_oihw=None, wsum=None, accumulate=False, cin_pad=None, dbias_part=None, slab_scale=None):
    """g: packed gradient [Cout][taps][Cin_pad] or unreduced slabs [splits][Cout][taps][Cin_pad] (summed here).
    dbias_part ([splits][Cout], from conv2d_wgrad): -> the bias gradient [Cout] (summed in slab order), else None.
    Inside ``with unpack_batch():`` the launch is deferred to the end of the block."""
    Cout, Cin, KH, KW = dw_oihw.shape
    nslabs = g.shape[0] if g.dim() == 4 else 1
    db = torch.empty(Cout, dtype=torch.float32, device=dw_oihw.device) if dbias_part is not None else None
    assert dbias_part is None or dbias_part.shape == (nslabs, Cout)
    assert slab_scale is None or nslabs % slab_scale.numel() == 0
    job = _unpack_job(g, dw_oihw, Cout, Cin, KH, KW, cin_pad, nslabs, slab_scale, scale=scale, w_oihw=w_oihw, wsum=wsum,
                      dsum_part=dbias_part, dbias_out=db)
    job.accumulate = int(accumulate)
    _unpack_submit(job, g, dw_oihw, scale, w_oihw, wsum, dbias_part, db, slab_scale)
    return db


def unpack_wgrad_bn(g, w_oihw, scale, dsum_part, mean, invstd, cin_pad=None, slab_scale=None, slab_cscale=None):
    """unpack_wgrad + bn_param_grad in one launch -> (dw, dgamma, dbeta); dsum_part: the [splits][Cout] rows of conv2d_wgrad.
    slab_scale [B] (per-image slabs of conv2d_wgrad(image_splits=True)): slab s is multiplied by slab_scale[s // (splits / B)].
    slab_cscale [B][Cin]: and, per input channel, by the image's squeeze-excite gate (forward on per-image weights)."""
    Cout, Cin, KH, KW = w_oihw.shape
    nslabs = g.shape[0] if g.dim() == 4 else 1
    if dsum_part.dim() == 1:
        dsum_part = dsum_part.view(1, Cout)
    assert dsum_part.shape == (nslabs, Cout) and dsum_part.is_contiguous()
    assert slab_scale is None or nslabs % slab_scale.numel() == 0
    dw = torch.empty_like(w_oihw)
    dgb = torch.empty((2, Cout), dtype=torch.float32, device=dw.device)
    wd = w_oihw.detach()
    job = _unpack_job(g, dw, Cout, Cin, KH, KW, cin_pad, nslabs, slab_scale, slab_cscale, scale=scale, w_oihw=wd, dsum_part=dsum_part, mean=mean,
                      invstd=invstd, dgamma=dgb[0], dbeta=dgb[1])
    _unpack_submit(job, g, dw, scale, wd, dsum_part, mean, invstd, dgb, slab_scale, slab_cscale)
    return dw, dgb[0], dgb[1]


def wgrad_split_supported(B, sizes, Cin, Cout, lddz, KH=3, KW=3, pad=1):
    """Can the split-operand weight-gradient kernel take these pyramid levels (same-padded stride-1 conv, flat level-major
    buffers)?  Host-side query only (no device work)."""
    d = L.WgradDesc()
    d.x, d.dz, d.dw, d.dbias = 128, 128, None, None
    d.dtype, d.B, d.Cin, d.Cout, d.KH, d.KW = L.F32_SPLIT, B, Cin, Cout, KH, KW
    d.stride, d.pad_t, d.pad_l, d.ldx, d.lddz = 1, pad, pad, Cin, lddz
    d.nseg = len(sizes)
    ox = oz = 0
    for i, (h, w) in enumerate(sizes):
        s = d.seg[i]
        s.H, s.W, s.Ho, s.Wo = h, w, h, w
        s.in_off, s.in_bstride, s.out_off, s.out_bstride = ox, h * w * Cin, oz, h * w * lddz
        ox += B * h * w * Cin; oz += B * h * w * lddz
    return int(L.require('effdet_conv2d_wgrad_plan_info').effdet_conv2d_wgrad_plan_info(C.byref(d), C.byref(L.WgradPlanInfo()))) >= 0


def live_tiles(dreg, B, sizes, reg_ld, split):
    """Liveness flags of the regression tower's backward pass (include/effdet_live_tiles.h) from d(reg) as focal_loss_bwd_reg leaves
    it with reg_ld: [B][sum H*W][reg_ld] rows, fp32 or (split) the split layout.  -> (live32 [6][steps], live128 [6][tiles]) uint8:
    row r flags the 32-pixel steps / 128-pixel tiles (per level over its (b, h, w) pixel index, levels concatenated) that hold a pixel
    within Chebyshev distance r of a non-zero d(reg) pixel of the same image and level.  Three kernel launches, nothing else."""
    lib_ = L.require(*L.LIVE_SIGNATURES)
    n = len(sizes)
    Hs, Ws = (C.c_int * n)(*[h for h, _ in sizes]), (C.c_int * n)(*[w for _, w in sizes])
    steps, tiles = C.c_longlong(), C.c_longlong()
    pixels = int(lib_.effdet_live_tiles_counts(B, n, Hs, Ws, C.byref(steps), C.byref(tiles)))
    if pixels < 0:
        L.check(pixels, 'effdet_live_tiles_counts')
    assert dreg.is_contiguous() and dreg.element_size() == 4 and dreg.numel() == pixels * reg_ld
    S, T, R = steps.value, tiles.value, L.LIVE_RADII
    buf = torch.empty(R * S + R * T + 2 * pixels, dtype=torch.uint8, device=dreg.device)
    l32, l128, scratch = buf[:R * S].view(R, S), buf[R * S:R * (S + T)].view(R, T), buf[R * (S + T):]
    L.check(lib_.effdet_live_tiles(dreg.data_ptr(), L.F32_SPLIT if split else L.F32, reg_ld, B, n, Hs, Ws, scratch.data_ptr(),
                                   l32.data_ptr(), l128.data_ptr(), L.stream_ptr()), 'effdet_live_tiles')
    return l32, l128


def _level_arrays(sizes):
    n = len(sizes)
    return n, (C.c_int * n)(*[h for h, _ in sizes]), (C.c_int * n)(*[w for _, w in sizes])


def positive_pixel_map(anc, annots, sizes):
    """The pixels with at least one positive anchor under the default matcher (include/effdet_needed_tiles.h), from the anchor table
    [1, A, 4] and the annotations [B, N, 5] alone -> uint8 [sum B*H*W], level-major, each level in (b, h, w) order: the layout of
    live_tiles' per-pixel map.  Equal to (assign >= 0) of the loss's assign pass OR-ed over each pixel's 9 anchors.  One launch."""
    B, N = annots.shape[0], annots.shape[1]
    A = anc.numel() // 4
    n, Hs, Ws = _level_arrays(sizes)
    assert anc.dtype == torch.float32 and anc.is_contiguous() and annots.dtype == torch.float32 and annots.is_contiguous()
    out = torch.empty(B * sum(h * w for h, w in sizes), dtype=torch.uint8, device=annots.device)
    L.check(L.require('effdet_positive_pixel_map').effdet_positive_pixel_map(L.ptr(anc), L.ptr(annots), B, A, N, n, Hs, Ws, out.data_ptr(),
                                                                             L.stream_ptr()), 'effdet_positive_pixel_map')
    return out


def live_tiles_from_map(pixmap, B, sizes):
    """live_tiles' flags from a per-pixel byte map (positive_pixel_map's layout; non-zero = non-zero pixel) -> (live32 [6][steps],
    live128 [6][tiles]) uint8.  Two kernel launches, nothing else."""
    lib_ = L.require('effdet_live_tiles_counts', 'effdet_live_tiles_from_map')
    n, Hs, Ws = _level_arrays(sizes)
    steps, tiles = C.c_longlong(), C.c_longlong()
    pixels = int(lib_.effdet_live_tiles_counts(B, n, Hs, Ws, C.byref(steps), C.byref(tiles)))
    if pixels < 0:
        L.check(pixels, 'effdet_live_tiles_counts')
    assert pixmap.dtype == torch.uint8 and pixmap.is_contiguous() and pixmap.numel() == pixels
    S, T, R = steps.value, tiles.value, L.LIVE_RADII
    buf = torch.empty(R * S + R * T + 2 * pixels, dtype=torch.uint8, device=pixmap.device)
    l32, l128, scratch = buf[:R * S].view(R, S), buf[R * S:R * (S + T)].view(R, T), buf[R * (S + T):]
    L.check(lib_.effdet_live_tiles_from_map(pixmap.data_ptr(), B, n, Hs, Ws, scratch.data_ptr(), l32.data_ptr(), l128.data_ptr(),
                                            L.stream_ptr()), 'effdet_live_tiles_from_map')
    return l32, l128


class UnitLists:
    """The flags of one pyramid with their compacted 32-pixel unit lists (include/effdet_unit_lists.h): live32 [6][steps], live128
    [6][tiles] uint8 as live_tiles returns them, units [6][steps] int32 (row r: the indices of live32[r]'s set flags, ascending, in its
    first counts[r][0] entries) and counts [6][4] int32 = {set steps, set tiles, gather, 0} per radius.  One more launch."""

    def __init__(self, live32, live128):
        R, S = live32.shape
        assert live32.dtype == torch.uint8 and live128.dtype == torch.uint8 and live32.is_contiguous() and live128.is_contiguous() and R == L.LIVE_RADII
        self.live32, self.live128 = live32, live128
        buf = torch.empty(R * S + R * L.UNIT_COUNTS, dtype=torch.int32, device=live32.device)
        self.units, self.counts = buf[:R * S].view(R, S), buf[R * S:].view(R, L.UNIT_COUNTS)
        L.check(L.require('effdet_unit_lists').effdet_unit_lists(live32.data_ptr(), live128.data_ptr(), S, live128.shape[1], self.units.data_ptr(),
                                                                 self.counts.data_ptr(), L.stream_ptr()), 'effdet_unit_lists')

    def row(self, r):
        """conv2d's units= for radius r"""
        return self.live32[r], self.units[r], self.counts[r]


def needed_tiles(anc, annots, B, sizes):
    """-> uint8 [6][tiles]: row r flags the 128-pixel tiles holding a pixel within Chebyshev distance r of a pixel with a positive
    anchor -- the tiles of the regression tower's forward pass whose output can reach the loss (conv2d(..., needed=row))."""
    return live_tiles_from_map(positive_pixel_map(anc, annots, sizes), B, sizes)[1]


def to_split(t):
    """plain fp32 tensor (rows of whole 32-channel groups) -> the same shape in the split layout (out of place)."""
    assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() % 32 == 0
    out = torch.empty_like(t)
    L.check(L.lib().effdet_to_split(L.ptr(t), L.ptr(out), t.numel(), L.stream_ptr()), 'effdet_to_split')
    return out


def to_split2(src, dst_split, dst_hsplit, n, flag=None):
    """The first n elements of the plain fp32 tensor src -> the split layout at address dst_split and / or the H-split layout at address
    dst_hsplit (ints; None = that form is not wanted), out of place, in one pass.  flag (range_flag(device) or None): the watch word a
    value that does not fit the H-split layout sets.  Without an H-split destination this is the single-layout pass of to_split."""
    if dst_hsplit is None:
        L.check(L.lib().effdet_to_split(L.ptr(src), dst_split, n, L.stream_ptr()), 'effdet_to_split')
    else:
        L.check(L.lib().effdet_to_split2(L.ptr(src), dst_split, dst_hsplit, n, L.ptr(flag), L.stream_ptr()), 'effdet_to_split2')


def nhwc_to_nchw(m):
    out = torch.empty((m.B, m.C, m.H, m.W), dtype=torch.float32, device=m.t.device)
    L.check(L.lib().effdet_nhwc_to_nchw_f32(L.ptr(m.tensor()), L.ptr(out), L.dtype_code(m.dtype), m.B, m.H, m.W, m.C,
                                            L.stream_ptr()), 'effdet_nhwc_to_nchw_f32')
    return out


def nchw_to_nhwc(x, dtype, cpad=None):
    B, Cc, H, W = x.shape
    assert x.dtype == torch.float32 and x.is_contiguous()
    cpad = Cc if cpad is None else cpad
    m = Map.new(B, H, W, cpad, dtype, x.device)
    L.check(L.lib().effdet_nchw_f32_to_nhwc(L.ptr(x), L.ptr(m.t), L.dtype_code(dtype), B, H, W, Cc, cpad, L.stream_ptr()),
            'effdet_nchw_f32_to_nhwc')
    return m


# ----------------------------------------------------------------------------- frozen BN
def bn_fold(gamma, beta, mean, var, eps=1e-3):
    C_ = gamma.numel()
    PREP = get_prep()
    if PREP is not None:
        key = ('bn', gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(), var.data_ptr(), eps)
        hit = PREP.lookup(key)
        if hit is not None:
            return hit[0], hit[1], hit[2]
        PREP.record(key, PREP_BNFOLD, (gamma, beta, mean, var), (C_,), torch.float32, (3, C_), eps)
    out = torch.empty((3, C_), dtype=torch.float32, device=gamma.device)     # scale | shift | invstd
    L.check(L.lib().effdet_bn_fold(L.ptr(gamma), L.ptr(beta), L.ptr(mean), L.ptr(var), float(eps),
                                   L.ptr(out[0]), L.ptr(out[1]), L.ptr(out[2]), C_, L.stream_ptr()), 'effdet_bn_fold')
    if PREP is not None:
        PREP.bn_src[out[0].data_ptr()] = (gamma, var, eps)
    return out[0], out[1], out[2]


def bn_param_grad(wsum, dsum, mean, invstd):
    C_ = wsum.numel()
    dg = torch.empty(C_, dtype=torch.float32, device=wsum.device); db = torch.empty_like(dg)
    L.check(L.lib().effdet_bn_param_grad(L.ptr(wsum), L.ptr(dsum), L.ptr(mean), L.ptr(invstd), L.ptr(dg), L.ptr(db), C_,
                                         L.stream_ptr()), 'effdet_bn_param_grad')
    return dg, db


# ----------------------------------------------------------------------------- depthwise
def dw_pack_weight(w_c1kk):
    Cc, _, k, _ = w_c1kk.shape
    PREP = get_prep()
    if PREP is not None:
        key = ('dw', w_c1kk.data_ptr())
        hit = PREP.lookup(key)
        if hit is not None:
            return hit
        PREP.record(key, PREP_DWPACK, (w_c1kk,), (Cc, 0, k * k), torch.float32, (k * k, Cc))
    out = torch.empty((k * k, Cc), dtype=torch.float32, device=w_c1kk.device)
    L.check(L.lib().effdet_dw_pack_weight(L.ptr(w_c1kk.detach()), L.ptr(out), Cc, k, L.stream_ptr()), 'effdet_dw_pack_weight')
    return out


def dw_unpack_wgrad(g_kkc, scale, w_c1kk, wsum=None):
    Cc, _, k, _ = w_c1kk.shape
    dw = torch.empty_like(w_c1kk)
    L.check(L.lib().effdet_dw_unpack_wgrad(L.ptr(g_kkc), L.ptr(scale), L.ptr(w_c1kk.detach()), L.ptr(dw), L.ptr(wsum), Cc, k,
                                           L.stream_ptr()), 'effdet_dw_unpack_wgrad')
    return dw


def dw_unpack_wgrad_bn(g_kkc, scale, w_c1kk, dsum, mean, invstd):
    """dw_unpack_wgrad + bn_param_grad in one launch -> (dw, dgamma, dbeta).  Deferred inside ``with unpack_batch():``."""
    Cc, _, k, _ = w_c1kk.shape
    dw = torch.empty_like(w_c1kk)
    dgb = torch.empty((2, Cc), dtype=torch.float32, device=dw.device)
    wd = w_c1kk.detach()
    batch = _cur_batch()
    if batch is not None:
        j = L.DwUnpackJob()
        j.g_kkc, j.scale, j.w_c1kk, j.dw_c1kk, j.dsum, j.mean, j.invstd = (t.data_ptr() for t in (g_kkc, scale, wd, dw, dsum, mean, invstd))
        j.dgamma, j.dbeta, j.C, j.kk = dgb[0].data_ptr(), dgb[1].data_ptr(), Cc, k * k
        batch.add(L.TAIL_DW_UNPACK, j, g_kkc, scale, wd, dw, dsum, mean, invstd, dgb)
    else:
        L.check(L.lib().effdet_dw_unpack_wgrad_bn(L.ptr(g_kkc), L.ptr(scale), L.ptr(wd), L.ptr(dw), L.ptr(dsum), L.ptr(mean),
                                                  L.ptr(invstd), L.ptr(dgb[0]), L.ptr(dgb[1]), Cc, k, L.stream_ptr()),
                'effdet_dw_unpack_wgrad_bn')
    return dw, dgb[0], dgb[1]


def dwconv_fwd(x, w_kkc, scale, shift, k, stride, pad_t, pad_l, Ho, Wo, save_z=False, pool=False, save_y=True, in_act=ACT_NONE):
    """-> (y, z, pool_part); save_y=False (needs save_z) stores the pre-activation only: consumers recompute Swish (act=ACT_SWISH).
    pool=True: pool_part [B][G][C] fp32 = per-(image, tile group) partial sums of the Swish output for se_gate_fwd.
    in_act=ACT_SWISH: x is the pre-activation of the expand conv (z-only storage); Swish is applied to the staged tiles."""
    assert save_y or save_z
    if pool:
        G = int(L.lib().effdet_dwconv_fwd_pool_groups(L.dtype_code(x.dtype), x.B, x.C, stride, Ho, Wo))
        if G < 1:
            raise RuntimeError('effdet_dwconv_fwd_pool_groups: unsupported geometry')
        pool = torch.empty((x.B, G, x.C), dtype=torch.float32, device=x.t.device)
    else:
        pool = None
    y = Map.new(x.B, Ho, Wo, x.C, x.dtype, x.t.device) if save_y else None
    z = Map.new(x.B, Ho, Wo, x.C, x.dtype, x.t.device) if save_z else None
    nbytes = x.t.element_size() * x.B * x.C * (x.H * x.W + Ho * Wo * (int(save_y) + int(save_z)))
    _timed('dw_fwd_lds_kernel', nbytes, lambda: L.check(L.lib().effdet_dwconv_fwd(
        L.ptr(x.tensor()), L.ptr(w_kkc), L.ptr(scale), L.ptr(shift), L.ptr(y.t if y else None), L.ptr(z.t if z else None), L.ptr(pool),
        L.dtype_code(x.dtype), x.B, x.H, x.W, x.C, k, stride, pad_t, pad_l, Ho, Wo, in_act, L.stream_ptr()), 'effdet_dwconv_fwd'),
        'BYTES k%d s%d C%d %dx%d' % (k, stride, x.C, x.H, x.W))
    return y, z, pool


def expand_dw_fwd(x, w_expand, scale0, shift0, w_kkc, scale1, shift1, k, stride, pad_t, pad_l, Ho, Wo):
    """Inference: expand 1x1 + BN + Swish -> depthwise k x k + BN + Swish in ONE kernel (the expanded map stays in LDS).
    x: fp32 Map [B,H,W,Cin], Cin in {16, 24, 32, 40}; w_expand: the OIHW 1x1 weight.  -> (y Map [B,Ho,Wo,Cexp], pool_part [B][G][Cexp])."""
    Cexp, Cin = w_expand.shape[0], w_expand.shape[1]
    assert x.dtype == torch.float32 and x.C == Cin
    G = int(L.lib().effdet_mbconv_expand_dw_pool_groups(x.B, Cexp, stride, Ho, Wo))
    if G < 1:
        raise RuntimeError('effdet_mbconv_expand_dw_pool_groups: unsupported geometry')
    pool = torch.empty((x.B, G, Cexp), dtype=torch.float32, device=x.t.device)
    y = Map.new(x.B, Ho, Wo, Cexp, torch.float32, x.t.device)
    nbytes = 4 * x.B * (x.H * x.W * Cin * ((Cexp + 31) // 32) + Ho * Wo * Cexp)
    _timed('dw_fwd_fused_kernel', nbytes, lambda: L.check(L.lib().effdet_mbconv_expand_dw_fwd(
        L.ptr(x.tensor()), L.ptr(w_expand.detach()), L.ptr(scale0), L.ptr(shift0), L.ptr(w_kkc), L.ptr(scale1), L.ptr(shift1), L.ptr(y.t), L.ptr(pool),
        x.B, x.H, x.W, Cin, Cexp, k, stride, pad_t, pad_l, Ho, Wo, L.stream_ptr()), 'effdet_mbconv_expand_dw_fwd'),
        'BYTES fused k%d s%d Cin%d C%d %dx%d' % (k, stride, Cin, Cexp, x.H, x.W))
    return y, pool


def dwconv_dgrad(dz, w_kkc, scale, zprev, H, W, k, stride, pad_t, pad_l):
    dx = Map.new(dz.B, H, W, dz.C, dz.dtype, dz.t.device)
    nbytes = dz.t.element_size() * dz.B * dz.C * (dz.H * dz.W + H * W * (2 if zprev else 1))
    _timed('dw_dgrad_lds_kernel', nbytes, lambda: L.check(L.lib().effdet_dwconv_dgrad(
        L.ptr(dz.tensor()), L.ptr(w_kkc), L.ptr(scale), L.ptr(zprev.tensor() if zprev else None), L.ptr(dx.t),
        L.dtype_code(dz.dtype), dz.B, H, W, dz.C, k, stride, pad_t, pad_l, dz.H, dz.W, L.stream_ptr()), 'effdet_dwconv_dgrad'),
        'BYTES k%d s%d C%d %dx%d' % (k, stride, dz.C, H, W))
    return dx


def dwconv_wgrad(x, dz, k, stride, pad_t, pad_l, in_act=ACT_NONE):
    g = torch.empty((k * k + 1, x.C), dtype=torch.float32, device=x.t.device)       # taps | dsum (overwritten by the slab reduction)
    geo = (L.dtype_code(x.dtype), x.B, x.H, x.W, x.C, k, stride, pad_t, pad_l, dz.H, dz.W)
    nbytes = int(L.lib().effdet_dwconv_wgrad_workspace_bytes(*geo))
    if nbytes < 0:
        raise RuntimeError('effdet_dwconv_wgrad: unsupported geometry')
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.t.device)
    traffic = x.t.element_size() * x.B * x.C * (x.H * x.W + dz.H * dz.W)
    _timed('dw_wgrad_lds_kernel', traffic, lambda: L.check(L.lib().effdet_dwconv_wgrad(
        L.ptr(x.tensor()), L.ptr(dz.tensor()), L.ptr(g), L.ptr(g[k * k]), L.ptr(ws), nbytes, *geo, in_act, L.stream_ptr()),
        'effdet_dwconv_wgrad'), 'BYTES k%d s%d C%d %dx%d' % (k, stride, x.C, x.H, x.W))
    return g[:k * k], g[k * k]


def dwconv_bwd(dz, w_kkc, scale, zprev, k, stride, pad_t, pad_l):
    """Data + weight gradient of the depthwise conv in one pass (the conv's input was stored as the pre-activation ``zprev`` only).
    -> (dx, g [k*k][C], dsum [C]), or None when the fused kernel does not serve the geometry (callers run dwconv_wgrad + dwconv_dgrad)."""
    H, W = zprev.H, zprev.W
    geo = (L.dtype_code(dz.dtype), dz.B, H, W, dz.C, k, stride, pad_t, pad_l, dz.H, dz.W)
    nbytes = int(L.lib().effdet_dwconv_bwd_workspace_bytes(*geo))
    if nbytes < 0:
        raise RuntimeError('effdet_dwconv_bwd: invalid geometry')
    if nbytes == 0 or zprev.ld != zprev.C or zprev.off != 0 or dz.ld != dz.C or dz.off != 0:
        return None
    dx = Map.new(dz.B, H, W, dz.C, dz.dtype, dz.t.device)
    g = torch.empty((k * k + 1, dz.C), dtype=torch.float32, device=dz.t.device)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dz.t.device)
    traffic = dz.t.element_size() * dz.B * dz.C * (dz.H * dz.W + 2 * H * W)
    _timed('dw_bwd_lds_kernel', traffic, lambda: L.check(L.lib().effdet_dwconv_bwd(
        L.ptr(dz.tensor()), L.ptr(w_kkc), L.ptr(scale), L.ptr(zprev.tensor()), L.ptr(dx.t), L.ptr(g), L.ptr(g[k * k]), L.ptr(ws),
        nbytes, *geo, L.stream_ptr()), 'effdet_dwconv_bwd'), 'BYTES k%d s%d C%d %dx%d' % (k, stride, dz.C, H, W))
    return dx, g[:k * k], g[k * k]


DW_PLAN_KINDS = {'fwd': L.DW_PLAN_FWD, 'dgrad': L.DW_PLAN_DGRAD, 'wgrad': L.DW_PLAN_WGRAD, 'bwd': L.DW_PLAN_BWD, 'expand_fwd': L.DW_PLAN_EXPAND_FWD}


def dwconv_plan_info(kind, dtype, B, H, W, Cch, k, stride, pad_t, pad_l, Ho, Wo, Cin=0):
    """What the depthwise entry point of `kind` ('fwd', 'dgrad', 'wgrad', 'bwd', 'expand_fwd': Cch = Cexp) plans for a geometry, asked of
    the library's own planner without device work (effdet_dwconv_plan_info) -> dict of cq, tpi, ppt, nbuf, groups (per image), nslab,
    direct; or None where the entry point answers EFFDET_EUNSUPPORTED (e.g. the fused backward at a geometry it does not serve)."""
    info = (C.c_int * len(L.DW_INFO))()
    rc = int(L.require('effdet_dwconv_plan_info').effdet_dwconv_plan_info(
        DW_PLAN_KINDS[kind], L.dtype_code(dtype), B, H, W, Cch, k, stride, pad_t, pad_l, Ho, Wo, Cin, info))
    if rc == -3:
        return None
    L.check(rc, 'effdet_dwconv_plan_info')
    return dict(zip(L.DW_INFO, (int(v) for v in info)))


def pw_bwd(dz, x, w_expand, scale, res=None):
    """Data + weight gradient of the MBConv expand conv in one pass over the expanded gradient ``dz`` (effdet_pw_bwd).
    -> (dx Map, slabs [S][Cexp][1][Cin], dsum parts [S][Cexp]) for unpack_wgrad_bn, or None when the fused kernel does not serve the geometry."""
    Cexp, Cin = w_expand.shape[0], w_expand.shape[1]
    M = dz.B * dz.H * dz.W
    dense = all(m is None or (m.ld == m.C and m.off == 0 and m.bstride == m.H * m.W * m.C and m.dtype == torch.float32) for m in (dz, x, res))
    S = int(L.lib().effdet_pw_bwd_slabs(M, Cin, Cexp)) if dense and dz.C == Cexp and x.C == Cin else 0
    if S < 1:
        return None
    dx = Map.new(x.B, x.H, x.W, Cin, torch.float32, x.t.device)
    ws = torch.empty(S * (Cexp * Cin + Cexp), dtype=torch.float32, device=x.t.device)
    slabs, parts = ws[:S * Cexp * Cin].view(S, Cexp, 1, Cin), ws[S * Cexp * Cin:].view(S, Cexp)
    _timed('conv_pw_bwd_kernel', 4.0 * Cin * Cexp * M, lambda: L.check(L.lib().effdet_pw_bwd(
        L.ptr(dz.tensor()), L.ptr(x.tensor()), L.ptr(w_expand.detach()), L.ptr(scale), L.ptr(res.tensor() if res is not None else None), L.ptr(dx.t),
        L.ptr(slabs), L.ptr(parts), M, Cin, Cexp, L.stream_ptr()), 'effdet_pw_bwd'), 'Cin%d Cexp%d M%d' % (Cin, Cexp, M),
        nbytes=4.0 * M * (Cexp + (3 if res is not None else 2) * Cin))
    return dx, slabs, parts


def pw_dgrad_se(dy, w_project, scale, rowscale, gate, dpool, zd):
    """Project-conv data gradient with the squeeze-excite backward + Swish' epilogue (effdet_pw_dgrad_se) -> dz_d Map, or None when the
    kernel does not serve the geometry (callers use conv2d(..., bc_scale=gate, bc_shift=dpool, res=zd, res_mode=RES_SWISH_GRAD))."""
    Cout, Cexp = w_project.shape[0], w_project.shape[1]
    M = dy.B * dy.H * dy.W
    dense = all(m.ld == m.C and m.off == 0 and m.bstride == m.H * m.W * m.C and m.dtype == torch.float32 for m in (dy, zd))
    if not dense or dy.C != Cout or zd.C != Cexp or not int(L.lib().effdet_pw_dgrad_se_supported(M, Cout, Cexp)):
        return None
    dz = Map.new(zd.B, zd.H, zd.W, Cexp, torch.float32, zd.t.device)
    _timed('conv_pw_dgrad_se_kernel', 2.0 * Cout * Cexp * M, lambda: L.check(L.lib().effdet_pw_dgrad_se(
        L.ptr(dy.tensor()), L.ptr(w_project.detach()), L.ptr(scale), L.ptr(rowscale), L.ptr(gate), L.ptr(dpool), L.ptr(zd.tensor()), L.ptr(dz.t),
        M, dy.H * dy.W, dy.B, Cout, Cexp, L.stream_ptr()), 'effdet_pw_dgrad_se'), 'Cout%d Cexp%d M%d' % (Cout, Cexp, M),
        nbytes=4.0 * M * (Cout + 2 * Cexp))
    return dz


# ----------------------------------------------------------------------------- squeeze-excite
def se_gate_fwd(pool_part, w1, b1, w2, b2, inv_hw, save_mid=False):
    """pool_part: [B][G][C] partial sums of dwconv_fwd (or a plain [B][C] pool) -> (gate, mid, pool [B][C] = the pooled SUM)."""
    if pool_part.dim() == 2:
        pool_part = pool_part.unsqueeze(1)
    B, G, Cc = pool_part.shape
    assert pool_part.is_contiguous()
    Cse = w1.shape[0]
    gate = torch.empty((B, Cc), dtype=torch.float32, device=pool_part.device)
    pool = torch.empty((B, Cc), dtype=torch.float32, device=pool_part.device)
    mid = torch.empty((B, Cse), dtype=torch.float32, device=pool_part.device) if save_mid else None
    ws = torch.empty((B, Cse), dtype=torch.float32, device=pool_part.device)
    L.check(L.lib().effdet_se_gate_fwd_split(L.ptr(pool_part), G, L.ptr(pool), L.ptr(w1.detach()), L.ptr(b1.detach()), L.ptr(w2.detach()),
                                             L.ptr(b2.detach()), L.ptr(gate), L.ptr(mid), L.ptr(ws), B, Cc, Cse, float(inv_hw),
                                             L.stream_ptr()), 'effdet_se_gate_fwd_split')
    return gate, mid, pool


def channel_scale(x, gate, act=ACT_NONE):
    """act(x) * gate[b][c]; act=ACT_SWISH when x is the depthwise pre-activation (z-only storage)."""
    y = Map.new(x.B, x.H, x.W, x.C, x.dtype, x.t.device)
    L.check(L.lib().effdet_channel_scale(L.ptr(x.tensor()), L.ptr(gate), L.ptr(y.t), act, L.dtype_code(x.dtype), x.B,
                                         x.H * x.W, x.C, L.stream_ptr()), 'effdet_channel_scale')
    return y


def se_dgate(dy, x, act=ACT_NONE):
    """-> dgate_part [B][slabs][C]: per-pixel-slab partial sums (added in slab order by se_gate_bwd)."""
    dg = torch.empty((x.B, int(L.lib().effdet_se_dgate_slabs(x.H * x.W)), x.C), dtype=torch.float32, device=x.t.device)
    L.check(L.lib().effdet_se_dgate(L.ptr(dy.tensor()), L.ptr(x.tensor()), L.ptr(dg), act, L.dtype_code(x.dtype), x.B,
                                    x.H * x.W, x.C, L.stream_ptr()), 'effdet_se_dgate')
    return dg


def se_dgate_from_wgrad(slabs, w_oc, bn_scale, rowscale, B):
    """(d loss / d gate * gate) [B][Cexp] from the project conv's per-image weight-gradient slabs [B*q][Cout][1][Cexp] (see the header)."""
    S, Co, _, Ce = slabs.shape
    assert S % B == 0
    out = torch.empty((B, Ce), dtype=torch.float32, device=slabs.device)
    L.check(L.lib().effdet_se_dgate_from_wgrad(L.ptr(slabs), L.ptr(w_oc.detach()), L.ptr(bn_scale), L.ptr(rowscale), L.ptr(out), B, S // B,
                                               Co, Ce, L.stream_ptr()), 'effdet_se_dgate_from_wgrad')
    return out


def se_gate_bwd(dgate, gate, mid, pool, w1, b1, w2, inv_hw, times_gate=False):
    """dgate: [B][slabs][C] partial rows of se_dgate (or a plain [B][C] gradient).
    -> (dpool, dw1, db1, dw2, db2); the parameter grads are fresh tensors (overwritten, not accumulated)."""
    if dgate.dim() == 2:
        dgate = dgate.unsqueeze(1)
    assert dgate.is_contiguous()
    B, Cc = pool.shape
    Cse = w1.shape[0]
    dev = pool.device
    dpool = torch.empty_like(pool)
    out = torch.empty(2 * Cc * Cse + Cc + Cse + B * (Cc + 2 * Cse), dtype=torch.float32, device=dev)
    dw1 = out[:Cse * Cc].view(Cse, Cc); o = Cse * Cc
    dw2 = out[o:o + Cc * Cse].view(Cc, Cse); o += Cc * Cse
    db1 = out[o:o + Cse]; o += Cse
    db2 = out[o:o + Cc]; o += Cc
    ws = out[o:]
    assert ws.numel() >= L.lib().effdet_se_gate_bwd_workspace_floats(B, Cc, Cse)
    batch = _cur_batch()
    defer = batch is not None                  # the parameter gradients (phase B) join the node's tail launch
    w1d, b1d, w2d = w1.detach(), b1.detach(), w2.detach()
    L.check(L.lib().effdet_se_gate_bwd(L.ptr(dgate), dgate.shape[1], int(times_gate), L.ptr(gate), L.ptr(mid), L.ptr(pool), L.ptr(w1d), L.ptr(b1d),
                                       L.ptr(w2d), L.ptr(dpool), L.ptr(None if defer else dw1), L.ptr(None if defer else db1),
                                       L.ptr(None if defer else dw2), L.ptr(None if defer else db2), L.ptr(ws),
                                       B, Cc, Cse, float(inv_hw), L.stream_ptr()), 'effdet_se_gate_bwd')
    if defer:
        j = L.SeParamJob()
        j.du, j.dmid, j.sw = ws.data_ptr(), ws.data_ptr() + 4 * B * Cc, ws.data_ptr() + 4 * B * (Cc + Cse)
        j.pool, j.dw1, j.db1, j.dw2, j.db2 = pool.data_ptr(), dw1.data_ptr(), db1.data_ptr(), dw2.data_ptr(), db2.data_ptr()
        j.B, j.C, j.Cse, j.inv_hw = B, Cc, Cse, inv_hw
        batch.add(L.TAIL_SE_PARAMS, j, out, pool)
    return dpool, dw1, db1, dw2, db2


def se_bwd_apply(dy, gate, dpool, z):
    out = Map.new(z.B, z.H, z.W, z.C, z.dtype, z.t.device)
    L.check(L.lib().effdet_se_bwd_apply(L.ptr(dy.tensor()), L.ptr(gate), L.ptr(dpool), L.ptr(z.tensor()), L.ptr(out.t),
                                        L.dtype_code(z.dtype), z.B, z.H * z.W, z.C, L.stream_ptr()), 'effdet_se_bwd_apply')
    return out


def act_bwd(dy, aux, act, rowscale=None, out=None):
    out = out or Map.new(dy.B, dy.H, dy.W, dy.C, dy.dtype, dy.t.device)
    L.check(L.lib().effdet_act_bwd(L.ptr(dy.tensor()), L.ptr(aux.tensor() if aux is not None else None), L.ptr(rowscale),
                                   L.ptr(out.t), L.dtype_code(dy.dtype), act, dy.B, dy.H * dy.W * dy.C,
                                   L.stream_ptr()), 'effdet_act_bwd')
    return out


def add_inplace(y, x):
    """y += x for two same-shaped contiguous tensors / Maps."""
    ty = y.tensor() if isinstance(y, Map) else y
    tx = x.tensor() if isinstance(x, Map) else x
    assert ty.numel() == tx.numel() and ty.dtype == tx.dtype
    L.check(L.lib().effdet_add_inplace(L.ptr(ty), L.ptr(tx), L.dtype_code(ty.dtype), ty.numel(), L.stream_ptr()),
            'effdet_add_inplace')


def colsum(t2d, out):
    rows, Cc = t2d.shape
    L.check(L.lib().effdet_colsum(L.ptr(t2d), L.ptr(out), L.dtype_code(t2d.dtype), rows, Cc, Cc, L.stream_ptr()),
            'effdet_colsum')


# ----------------------------------------------------------------------------- BiFPN fusion
def bifpn_fuse_fwd(a, b, c, wraw, col, mode, plain=True, hsplit=False):
    """-> the fused map (plain Map), or with hsplit=True the pair (plain Map or None, H-split Map): the operand of an f16x3 conv."""
    out = Map.new(a.B, a.H, a.W, a.C, a.dtype, a.t.device) if plain else None
    outh = Map.new(a.B, a.H, a.W, a.C, a.dtype, a.t.device) if hsplit else None
    wr, wc = wraw.shape
    L.check(L.lib().effdet_bifpn_fuse_fwd2(L.ptr(a.tensor()), L.ptr(b.tensor()), L.ptr(c.tensor() if c is not None else None),
                                           L.ptr(out.t if plain else None), L.ptr(outh.t if hsplit else None), L.ptr(wraw.detach()), wr, wc, col, mode,
                                           L.dtype_code(a.dtype), a.B, a.H, a.W, a.C, L.ptr(range_flag(a.t.device) if hsplit else None),
                                           L.stream_ptr()), 'effdet_bifpn_fuse_fwd2')
    return (out, outh) if hsplit else out


FUSE_COL_FLOATS = 4 + 3 * 2048     # EFFDET_FUSE_COL_FLOATS (include/effdet_hip.h): per weight column, [count | per-workgroup partial triples]


def fuse_dn_floats(wcols):
    return wcols * FUSE_COL_FLOATS


def bifpn_fuse_bwd(dout, a, b, c, da, db, dc, da_acc, db_acc, dc_acc, wraw, dn, col, mode):
    wr, wc = wraw.shape
    assert dn.numel() == fuse_dn_floats(wc)
    L.check(L.lib().effdet_bifpn_fuse_bwd(L.ptr(dout.tensor()), L.ptr(a.tensor()), L.ptr(b.tensor()),
                                          L.ptr(c.tensor() if c is not None else None), L.ptr(da.tensor()), L.ptr(db.tensor()),
                                          L.ptr(dc.tensor() if dc is not None else None), int(da_acc), int(db_acc), int(dc_acc),
                                          L.ptr(wraw.detach()), L.ptr(dn), wr, wc, col, mode, L.dtype_code(a.dtype),
                                          a.B, a.H, a.W, a.C, L.stream_ptr()), 'effdet_bifpn_fuse_bwd')


def bifpn_weight_bwd(wraw, dn, dwraw):
    wr, wc = wraw.shape
    L.check(L.lib().effdet_bifpn_weight_bwd(L.ptr(wraw.detach()), L.ptr(dn), L.ptr(dwraw), wr, wc, L.stream_ptr()),
            'effdet_bifpn_weight_bwd')


# ----------------------------------------------------------------------------- anchors / decode / NMS
def num_anchors(H, W):
    return int(L.lib().effdet_num_anchors(H, W))


def anchors(H, W, device):
    A = num_anchors(H, W)
    out = torch.empty((1, A, 4), dtype=torch.float32, device=device)
    L.check(L.lib().effdet_anchors(L.ptr(out), H, W, L.stream_ptr()), 'effdet_anchors')
    return out


def decode_score(anc, reg, cls, img_h, img_w):
    B, A, nc = cls.shape
    boxes = torch.empty((B, A, 4), dtype=torch.float32, device=cls.device)
    score = torch.empty((B, A), dtype=torch.float32, device=cls.device)
    label = torch.empty((B, A), dtype=torch.int32, device=cls.device)
    # algorithmic bytes: probabilities + box deltas read once, boxes / score / label written once (anchors: one [A,4] table for the batch)
    nbytes = 4 * (B * A * (nc + 4) + A * 4 + B * A * 6)
    _timed('decode_score_kernel', nbytes, lambda: L.check(L.lib().effdet_decode_score(
        L.ptr(anc), L.ptr(reg), L.ptr(cls), L.ptr(boxes), L.ptr(score), L.ptr(label), B, A, nc, float(img_w), float(img_h),
        L.stream_ptr()), 'effdet_decode_score'), 'BYTES B%d A%d nc%d' % (B, A, nc))
    return boxes, score, label


def nms(boxes, score, threshold, iou_threshold):
    """-> (idx [B][A] int32 kept anchor indices in order, count [B] int32); all on device, no sync."""
    B, A = score.shape
    nbytes = int(L.lib().effdet_nms_workspace_bytes(B, A))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=score.device)
    idx = torch.empty((B, A), dtype=torch.int32, device=score.device)
    count = torch.empty((B,), dtype=torch.int32, device=score.device)
    # algorithmic bytes of the whole NMS call (sort + greedy rounds = ~90 launches): every candidate's box + score read once, its index
    # written once -- the O(K^2) suppression work is latency / ALU, not bytes, so the GB/s of this entry says how far from a streaming
    # pass the greedy algorithm is, not how well a kernel streams
    _timed('nms (radix sort + cross / matrix / resolve rounds)', 4 * B * A * 6, lambda: L.check(L.lib().effdet_nms(
        L.ptr(boxes), L.ptr(score), float(threshold), float(iou_threshold), L.ptr(idx), L.ptr(count),
        L.ptr(ws), nbytes, B, A, L.stream_ptr()), 'effdet_nms'), 'BYTES B%d A%d' % (B, A))
    return idx, count


def gather_dets(boxes, score, label, idx, count):
    B, A = score.shape
    os_ = torch.empty((B, A), dtype=torch.float32, device=score.device)
    ol = torch.empty((B, A), dtype=torch.int64, device=score.device)
    ob = torch.empty((B, A, 4), dtype=torch.float32, device=score.device)
    L.check(L.lib().effdet_gather_dets(L.ptr(boxes), L.ptr(score), L.ptr(label), L.ptr(idx), L.ptr(count), L.ptr(os_), L.ptr(ol),
                                       L.ptr(ob), B, A, L.stream_ptr()), 'effdet_gather_dets')
    return os_, ol, ob


NMS_METHODS = {'hard': 0, 'linear': 1, 'gaussian': 2}
SOFT_NMS_MAX_TOP_N = 4096          # the kernel holds the top-N candidates of an image in one workgroup's LDS


class _Options:
    """What the options classes share: ``key()`` (each class's own tuple) decides equality, within one class, and the hash."""

    def __eq__(self, other):
        return type(other) is type(self) and self.key() == other.key()

    def __hash__(self):
        return hash(self.key())


class NMSOptions(_Options):
    """The rescoring NMS of EfficientDet.set_nms (effdet_soft_nms): method 'hard' | 'linear' | 'gaussian', gaussian sigma,
    per-class suppression, the top-N candidates per image that take part (<= 4096) and the picks per image."""

    def __init__(self, method='hard', sigma=0.5, class_aware=False, pre_nms_top_n=1000, max_det=100):
        if method not in NMS_METHODS:
            raise ValueError('NMSOptions: method must be one of %s, not %r' % (sorted(NMS_METHODS), method))
        if not float(sigma) > 0.0:
            raise ValueError('NMSOptions: sigma must be > 0')
        if not 1 <= int(pre_nms_top_n) <= SOFT_NMS_MAX_TOP_N:
            raise ValueError('NMSOptions: pre_nms_top_n must be in 1..%d' % SOFT_NMS_MAX_TOP_N)
        if not 1 <= int(max_det) <= int(pre_nms_top_n):
            raise ValueError('NMSOptions: max_det must be in 1..pre_nms_top_n')
        self.method, self.sigma, self.class_aware = method, float(sigma), bool(class_aware)
        self.pre_nms_top_n, self.max_det = int(pre_nms_top_n), int(max_det)

    def key(self):
        return (self.method, self.sigma, self.class_aware, self.pre_nms_top_n, self.max_det)

    def __repr__(self):
        return 'NMSOptions(method=%r, sigma=%r, class_aware=%r, pre_nms_top_n=%d, max_det=%d)' % self.key()


_soft_nms_ws = {}      # (device, B, A, top_n) -> workspace of eager calls (a capture allocates its own, from the graph's pool)


def soft_nms(boxes, score, label, threshold, iou_threshold, method, sigma=0.5, class_aware=False, pre_nms_top_n=1000, max_det=100):
    """Rescoring NMS (include/effdet_soft_nms.h: effdet_soft_nms) -> (idx [B,A] int32 picked anchor indices in pick order,
    new_score [B,A] fp32 their scores when picked, count [B] int32); all on device, no sync.  label is read with class_aware only."""
    lib = L.require('effdet_soft_nms', 'effdet_soft_nms_workspace_bytes')
    B, A = score.shape
    dev = score.device
    nbytes = int(lib.effdet_soft_nms_workspace_bytes(B, A, int(pre_nms_top_n)))
    if torch.cuda.is_current_stream_capturing():
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    else:
        k = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device(), B, A, int(pre_nms_top_n))
        ws = _soft_nms_ws.get(k)
        if ws is None:
            ws = _soft_nms_ws[k] = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    idx = torch.empty((B, A), dtype=torch.int32, device=dev)
    new_score = torch.empty((B, A), dtype=torch.float32, device=dev)
    count = torch.empty((B,), dtype=torch.int32, device=dev)
    m = NMS_METHODS[method] if isinstance(method, str) else int(method)
    # algorithmic bytes as for nms: the sort's traffic + one box / score / label per top-N candidate; the pick loop is LDS / latency
    _timed('soft_nms (radix sort + per-image pick loop)', 4 * B * A * 6, lambda: L.check(lib.effdet_soft_nms(
        L.ptr(boxes), L.ptr(score), L.ptr(label) if class_aware else None, float(threshold), float(iou_threshold), m, float(sigma),
        1 if class_aware else 0, int(pre_nms_top_n), int(max_det), L.ptr(idx), L.ptr(new_score), L.ptr(count), L.ptr(ws), nbytes, B, A,
        L.stream_ptr()), 'effdet_soft_nms'), 'BYTES B%d A%d' % (B, A))
    return idx, new_score, count


def model_nms(model, boxes, score, label):
    """The NMS stage of every detection path (EfficientDet.detect, evaluate.postprocess, graph.GraphedDetect) on decode_score's
    outputs -> (scores [B,A], labels [B,A] int64, boxes [B,A,4], count [B] int32): score-descending rows, count[b] of them valid.
    model.nms_options None: the reference's class-agnostic greedy NMS; an NMSOptions: the rescoring NMS, scores = the rescored ones."""
    opt = getattr(model, 'nms_options', None)
    if opt is None:
        idx, count = nms(boxes, score, float(model.threshold), float(model.iou_threshold))
        s, l, b = gather_dets(boxes, score, label, idx, count)
        return s, l, b, count
    idx, new_score, count = soft_nms(boxes, score, label, float(model.threshold), float(model.iou_threshold), opt.method, opt.sigma,
                                     opt.class_aware, opt.pre_nms_top_n, opt.max_det)
    _, l, b = gather_dets(boxes, score, label, idx, count)
    return new_score, l, b, count


# ----------------------------------------------------------------------------- weighted boxes fusion / test-time augmentation
WBF_CONF_TYPES = {'avg': 0, 'max': 1}                # EFFDET_WBF_AVG, EFFDET_WBF_MAX
WBF_MAX_VIEWS, WBF_MAX_IN = L.WBF_MAX_VIEWS, L.WBF_MAX_IN


class WBFOptions(_Options):
    """Weighted Boxes Fusion of fuse_detections (effdet_wbf): a candidate joins the same-label cluster it overlaps most when that IoU is
    > iou_thr; rows scoring below skip_box_thr take no part; the fused score is the members' mean confidence scaled by how many views
    agreed ('avg') or the largest one ('max'); of every view the first top_n rows per image take part (views * top_n <= 4096)."""

    def __init__(self, iou_thr=0.55, skip_box_thr=0.0, conf_type='avg', top_n=1000):
        if not 0.0 <= float(iou_thr) <= 1.0:
            raise ValueError('WBFOptions: iou_thr must be in [0, 1]')
        if not 0.0 <= float(skip_box_thr) < float('inf'):
            raise ValueError('WBFOptions: skip_box_thr must be finite and >= 0')
        if conf_type not in WBF_CONF_TYPES:
            raise ValueError('WBFOptions: conf_type must be one of %s, not %r' % (sorted(WBF_CONF_TYPES), conf_type))
        if not 1 <= int(top_n) <= WBF_MAX_IN:
            raise ValueError('WBFOptions: top_n must be in 1..%d' % WBF_MAX_IN)
        self.iou_thr, self.skip_box_thr, self.conf_type, self.top_n = float(iou_thr), float(skip_box_thr), conf_type, int(top_n)

    def key(self):
        return (self.iou_thr, self.skip_box_thr, self.conf_type, self.top_n)

    def __repr__(self):
        return 'WBFOptions(iou_thr=%r, skip_box_thr=%r, conf_type=%r, top_n=%d)' % self.key()


def _view_weights(weights, V, what):
    """weights (None: all 1) -> tuple of V positive finite floats."""
    w = (1.0,) * V if weights is None else tuple(float(x) for x in weights)
    if len(w) != V:
        raise ValueError('%s: %d weights for %d views' % (what, len(w), V))
    if not all(0.0 < x < float('inf') for x in w):
        raise ValueError('%s: weights must be positive and finite' % what)
    return w


def _tta_scales(scales):
    """scales -> tuple of distinct positive finite floats, none equal to 1 (the unscaled view is always there)."""
    sc = tuple(float(x) for x in scales)
    if not all(0.0 < x < float('inf') for x in sc):
        raise ValueError('TTAOptions: scales must be positive and finite, got %r' % (sc,))
    if 1.0 in sc:
        raise ValueError('TTAOptions: a scale of 1 is the base view, which is always present; got %r' % (sc,))
    if len(set(sc)) != len(sc):
        raise ValueError('TTAOptions: scales must be distinct, got %r' % (sc,))
    return sc


class TTAOptions(_Options):
    """Test-time augmentation of EfficientDet.set_tta: views of the batch, each through the whole detection path (its own forward of batch
    B at the view's size), the lists merged by fuse_detections.  The views, in this order: the batch as given; with hflip its mirror
    image; then for each s of scales, in the order given, the batch resampled to (H * s, W * s) (resample_images: bilinear, no
    antialiasing) and, with hflip, that view mirrored.  num_views = (1 + len(scales)) * (2 if hflip else 1) <= 8.  weights: one per view
    in that order (None: all 1).  H * s and W * s must be multiples of 128 (tta_view_plan checks it at the call)."""

    def __init__(self, hflip=True, weights=None, fusion=None, scales=()):
        fusion = WBFOptions() if fusion is None else fusion
        if not isinstance(fusion, WBFOptions):
            raise TypeError('TTAOptions: fusion must be a WBFOptions, not %r' % (fusion,))
        self.hflip, self.fusion, self.scales = bool(hflip), fusion, _tta_scales(scales)
        if self.num_views > WBF_MAX_VIEWS:
            raise ValueError('TTAOptions: %d views (%d sizes%s) exceed the limit of %d'
                             % (self.num_views, 1 + len(self.scales), ', each with its mirror image' if self.hflip else '', WBF_MAX_VIEWS))
        self.weights = None if weights is None else _view_weights(weights, self.num_views, 'TTAOptions')
        if self.num_views * fusion.top_n > WBF_MAX_IN:
            raise ValueError('TTAOptions: views * fusion.top_n must be <= %d, got %d * %d' % (WBF_MAX_IN, self.num_views, fusion.top_n))

    @property
    def num_views(self):
        return (1 + len(getattr(self, 'scales', ()))) * (2 if self.hflip else 1)     # (options pickled before scales existed have none)

    def key(self):
        sc = getattr(self, 'scales', ())
        return (self.hflip, self.weights, self.fusion.key()) + ((sc,) if sc else ())

    def __repr__(self):
        sc = getattr(self, 'scales', ())
        return 'TTAOptions(hflip=%r, weights=%r, fusion=%r%s)' % (self.hflip, self.weights, self.fusion, ', scales=%r' % (sc,) if sc else '')


def scaled_size(H, W, s, what='tta_view_plan'):
    """The size (H * s, W * s) of a scaled view: both whole numbers (within 1e-6) and multiples of 128 -- the pyramid halves five times
    and the BiFPN upsamples by exactly 2 -- else ValueError.  Host only."""
    hv, wv = float(H) * float(s), float(W) * float(s)
    Hv, Wv = int(round(hv)), int(round(wv))
    if not (0.0 < float(s) < float('inf')) or abs(hv - Hv) > 1e-6 or abs(wv - Wv) > 1e-6 or Hv < 128 or Wv < 128 or Hv % 128 or Wv % 128:
        raise ValueError('%s: H = %d, W = %d at scale s = %r gives %r x %r; both sides of a scaled view must be whole multiples of 128'
                         % (what, H, W, s, hv, wv))
    return Hv, Wv


def tta_view_plan(H, W, options):
    """The views of TTAOptions `options` on a batch of H x W, in the documented order -> [(H_v, W_v, flip, mul, weight)]: the view's size,
    whether it is mirrored, the factor that takes its boxes back to the batch's frame (H / H_v in fp64, rounded to fp32; both axes scale
    by the same s, so one factor serves x and y) and its fusion weight.  ValueError for a scale whose size is not whole multiples of
    128.  Host only: nothing is launched."""
    if not isinstance(options, TTAOptions):
        raise TypeError('tta_view_plan takes a TTAOptions, not %r' % (options,))
    H, W = int(H), int(W)
    w = options.weights if options.weights is not None else (1.0,) * options.num_views
    plan = []
    for s in (1.0,) + tuple(getattr(options, 'scales', ())):
        Hv, Wv = (H, W) if s == 1.0 else scaled_size(H, W, s)
        mul = float(np.float32(float(H) / float(Hv)))
        for flip in ((False, True) if options.hflip else (False,)):
            plan.append((Hv, Wv, flip, mul, w[len(plan)]))
    return plan


_wbf_ws = {}           # (device, B, V, top_n) -> workspace of eager calls (a capture allocates its own, from the graph's pool)


def fuse_detections(views, weights=None, flips=None, muls=None, options=None):
    """Weighted Boxes Fusion (include/effdet_wbf.h: effdet_wbf) of V <= 8 views of one batch -> (scores [B,N], labels [B,N] int64, boxes
    [B,N,4], count [B] int32) with N = V * options.top_n: fused detections score-descending, count[b] of them valid, zero rows after
    them -- model_nms's layout.  views: (scores [B,A_v], labels [B,A_v] int64, boxes [B,A_v,4], count [B] int32) each, as model_nms
    returns them; weights: one per view (None: all 1); flips: per view None or the width to mirror the boxes about; muls: per view a
    factor applied to every coordinate after the flip (None: 1).  All on device, no sync."""
    lib = L.require('effdet_wbf', 'effdet_wbf_workspace_bytes')
    options = WBFOptions() if options is None else options
    views = list(views)
    V = len(views)
    if not 1 <= V <= WBF_MAX_VIEWS:
        raise ValueError('fuse_detections: 1..%d views, got %d' % (WBF_MAX_VIEWS, V))
    if V * options.top_n > WBF_MAX_IN:
        raise ValueError('fuse_detections: views * top_n must be <= %d, got %d * %d' % (WBF_MAX_IN, V, options.top_n))
    w = _view_weights(weights, V, 'fuse_detections')
    flips = [None] * V if flips is None else list(flips)
    muls = [1.0] * V if muls is None else [float(x) for x in muls]
    if len(flips) != V or len(muls) != V:
        raise ValueError('fuse_detections: flips and muls take one entry per view')
    if not all(0.0 < x < float('inf') for x in muls):
        raise ValueError('fuse_detections: muls must be positive and finite')
    d = L.Wbf()
    B, dev = int(views[0][0].shape[0]), views[0][0].device
    keep = []
    for v, (s, l, b, c) in enumerate(views):
        if s.dim() != 2 or s.shape[0] != B or tuple(l.shape) != tuple(s.shape) or tuple(b.shape) != tuple(s.shape) + (4,) or tuple(c.shape) != (B,):
            raise ValueError('fuse_detections: view %d must be scores [B,A], labels [B,A], boxes [B,A,4], count [B]' % v)
        if (s.dtype, l.dtype, b.dtype, c.dtype) != (torch.float32, torch.int64, torch.float32, torch.int32):
            raise TypeError('fuse_detections: view %d must be (float32, int64, float32, int32) tensors' % v)
        s, l, b, c = s.contiguous(), l.contiguous(), b.contiguous(), c.contiguous()
        keep.append((s, l, b, c))
        d.score[v], d.label[v], d.boxes[v], d.count[v], d.A[v] = L.ptr(s), L.ptr(l), L.ptr(b), L.ptr(c), int(s.shape[1])
        d.weight[v], d.mul[v] = w[v], muls[v]
        d.flip[v], d.width[v] = (0, 0.0) if flips[v] is None else (1, float(flips[v]))
    N = V * options.top_n
    d.V, d.B, d.top_n, d.conf_type = V, B, options.top_n, WBF_CONF_TYPES[options.conf_type]
    d.iou_thr, d.skip_thr = options.iou_thr, options.skip_box_thr
    os_ = torch.empty((B, N), dtype=torch.float32, device=dev)
    ol = torch.empty((B, N), dtype=torch.int64, device=dev)
    ob = torch.empty((B, N, 4), dtype=torch.float32, device=dev)
    count = torch.empty((B,), dtype=torch.int32, device=dev)
    d.out_score, d.out_label, d.out_boxes, d.out_count = L.ptr(os_), L.ptr(ol), L.ptr(ob), L.ptr(count)
    nbytes = int(lib.effdet_wbf_workspace_bytes(B, V, options.top_n))
    ws = None
    if nbytes and torch.cuda.is_current_stream_capturing():
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    elif nbytes:
        k = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device(), B, V, options.top_n)
        ws = _wbf_ws.get(k)
        if ws is None:
            ws = _wbf_ws[k] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    # algorithmic bytes: every view's rows read once (score, label, box: 28 B), the fused rows written once; the clustering is LDS / latency
    _timed('wbf (per-image sort + sequential clustering)', 28 * B * sum(min(int(s.shape[1]), options.top_n) for s, _, _, _ in keep) + 28 * B * N,
           lambda: L.check(lib.effdet_wbf(C.byref(d), L.ptr(ws), nbytes, L.stream_ptr()), 'effdet_wbf'), 'BYTES B%d V%d N%d' % (B, V, N))
    return os_, ol, ob, count


def flip_images(images):
    """The mirror image of a batch: NCHW tensor, or a PackedImages whose map is a dense [B,H,W,C] tensor (TypeError otherwise)."""
    m = getattr(images, 'map', None)
    if m is None:
        return torch.flip(images, (3,))
    if not (m.off == 0 and m.ld == m.C and m.bstride == m.H * m.W * m.C and m.t.numel() == m.B * m.H * m.W * m.C):
        raise TypeError('TTA with hflip needs PackedImages over a dense [B,H,W,C] tensor (this map is strided or an arena slice): '
                        'pass the NCHW batch instead')
    return type(images)(Map.of(torch.flip(m.tensor(), (2,)).contiguous()))


def resample_images(images, size, flip=False, out=None):
    """A batch at another resolution (include/effdet_resample.h: effdet_resample_images): bilinear with half-pixel centres and edge clamp,
    no antialiasing, then mirrored left-right with flip -> a dense PackedImages of size = (H_out, W_out) in the stem conv's layout (NHWC,
    channels zero-padded to one 16-byte chunk).  images: a contiguous NCHW fp32 [B,3,H,W] tensor (the result is fp32) or a PackedImages
    in fp32 / bf16 (the result keeps its dtype) over any map: strided and arena slices included.  size == (H, W) without flip is
    refused: an unscaled view is the batch itself.  out: a dense Map [B, H_out, W_out, one chunk] of the result's dtype to write into
    (an arena slice at a 16-byte aligned address, say); None allocates one."""
    from .efficientdet import PackedImages
    lib = L.require('effdet_resample_images')
    Ho, Wo = (int(v) for v in size)
    d = L.Resample()
    m = getattr(images, 'map', None)
    if m is None:
        if not torch.is_tensor(images) or images.dim() != 4 or images.shape[1] != 3:
            raise TypeError('resample_images takes an NCHW [B,3,H,W] tensor or a PackedImages')
        if images.dtype != torch.float32:
            raise TypeError('resample_images: an NCHW batch must be float32, not %s (pack other dtypes as PackedImages)' % images.dtype)
        if not images.is_contiguous():
            raise ValueError('resample_images: the NCHW batch must be contiguous')
        B, _, H, W = (int(v) for v in images.shape)
        dtype, src_bytes = torch.float32, 12
        d.src, d.src_layout, d.C, d.src_ld, d.src_bstride = L.ptr(images), L.RESAMPLE_NCHW, 3, 0, 0
    else:
        if m.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError('resample_images: PackedImages must be float32 or bfloat16, not %s' % m.dtype)
        B, H, W, dtype, src_bytes = m.B, m.H, m.W, m.dtype, 3 * m.t.element_size()
        d.src, d.src_layout, d.C, d.src_ld, d.src_bstride = m.addr(), L.RESAMPLE_NHWC, m.C, m.ld, m.bstride
    if (Ho, Wo) == (H, W) and not flip:
        raise ValueError('resample_images: size %r is the size of the batch: use the batch itself for an unscaled view' % ((Ho, Wo),))
    ce = 4 if dtype == torch.float32 else 8                          # one 16-byte chunk of channels
    if out is None:
        out = Map.new(B, Ho, Wo, ce, dtype, images.device)
    elif (out.B, out.H, out.W, out.C, out.ld, out.bstride, out.dtype) != (B, Ho, Wo, ce, ce, Ho * Wo * ce, dtype) or out.addr() % 16:
        raise ValueError('resample_images: out must be a dense, 16-byte aligned [%d,%d,%d,%d] %s map' % (B, Ho, Wo, ce, dtype))
    d.dst, d.dtype, d.flip = out.addr(), L.dtype_code(dtype), 1 if flip else 0
    d.B, d.H, d.W, d.Ho, d.Wo = B, H, W, Ho, Wo
    # algorithmic bytes: four taps of three channels read and one 16-byte chunk written per output pixel
    _timed('resample (bilinear, one output pixel per thread)', B * Ho * Wo * (4 * src_bytes + 16),
           lambda: L.check(lib.effdet_resample_images(C.byref(d), L.stream_ptr()), 'effdet_resample_images'),
           'BYTES B%d %dx%d->%dx%d' % (B, H, W, Ho, Wo))
    return PackedImages(out)


def _detections_pass(model, images, H, W):
    cls, reg, anc = model.forward_raw(images)
    boxes, score, label = decode_score(anc, reg, cls, H, W)
    return model_nms(model, boxes, score, label) + (int(cls.shape[-1]),)


def model_detections(model, images, H, W, num_classes=False):
    """THE detection pass of every path (EfficientDet.detect, evaluate.detections_batched / evaluate_voc / evaluate_coco,
    graph.GraphedDetect) -> (scores [B,N], labels [B,N] int64, boxes [B,N,4], count [B] int32), model_nms's layout.  No TTA
    (model.tta_options None): forward_raw -> decode_score -> model_nms.  With TTAOptions: one such pass per view of tta_view_plan --
    separate forwards of batch B, so every launch plan and summation order is the plain pass's at that size -- and fuse_detections over
    them: a mirrored view's boxes flipped back about the view's own width, a scaled view's then multiplied by H / H_v.  The base view and
    its mirror image are the batch and flip_images(batch); a scaled view is resample_images(batch, (H_v, W_v), flip) and decodes
    against its own size.  A model that brings its own pass (evaluate.EnsembleDetector) is asked for it.  num_classes=True appends the
    head's class count to the tuple.  The caller holds no_grad and the f16x3 range watch."""
    own = getattr(model, 'detections', None)
    tta = getattr(model, 'tta_options', None)            # (a model pickled before the option existed has no such attribute)
    if own is not None:
        out = own(images, H, W) + (int(model.num_classes),)
    elif tta is None:
        out = _detections_pass(model, images, H, W)
    else:
        plan = tta_view_plan(H, W, tta)                               # (first: a scale this size cannot take is refused before any launch,
        mirror = flip_images(images) if tta.hflip else None          #  and so is a batch that cannot be mirrored)
        first = _detections_pass(model, images, H, W)
        views, flips = [first[:4]], [None]
        if tta.hflip:
            views.append(_detections_pass(model, mirror, H, W)[:4])
            flips.append(W)
        for Hv, Wv, flip, _, _ in plan[len(views):]:
            views.append(_detections_pass(model, resample_images(images, (Hv, Wv), flip), Hv, Wv)[:4])
            flips.append(Wv if flip else None)
        muls = [p[3] for p in plan] if getattr(tta, 'scales', ()) else None      # (no scales: no multiplier at all, as before)
        out = fuse_detections(views, tta.weights, flips, muls, tta.fusion) + first[4:]
    return out if num_classes else out[:4]


# ----------------------------------------------------------------------------- sliced inference
SLICE_METHODS = {'nms': L.SLICE_NMS, 'nmm': L.SLICE_NMM}          # EFFDET_SLICE_NMS, EFFDET_SLICE_NMM
SLICE_METRICS = {'iou': L.SLICE_IOU, 'ios': L.SLICE_IOS}          # EFFDET_SLICE_IOU, EFFDET_SLICE_IOS
SLICE_MAX_TILES, SLICE_MAX_IN = L.SLICE_MAX_TILES, L.SLICE_MAX_IN


class SliceMergeOptions(_Options):
    """The cross-tile merge of merge_slices (effdet_slice_merge): candidates in score order; a keeper takes every later candidate whose
    metric with the keeper's own box is > thr ('iou', or 'ios': intersection over the smaller box, which is what lets a full box absorb
    one truncated at a tile edge) and, with class_aware, whose label is the keeper's.  'nms' drops what a keeper takes, 'nmm' also
    grows the keeper's box to the hull of what it took.  Rows scoring below skip_thr take no part; of every tile the first top_n rows
    take part (lists * top_n <= 8192); at most max_det detections per image come out."""

    def __init__(self, method='nmm', metric='ios', thr=0.5, class_aware=True, skip_thr=0.0, top_n=256, max_det=300):
        if method not in SLICE_METHODS:
            raise ValueError('SliceMergeOptions: method must be one of %s, not %r' % (sorted(SLICE_METHODS), method))
        if metric not in SLICE_METRICS:
            raise ValueError('SliceMergeOptions: metric must be one of %s, not %r' % (sorted(SLICE_METRICS), metric))
        if not 0.0 <= float(thr) <= 1.0:
            raise ValueError('SliceMergeOptions: thr must be in [0, 1]')
        if not 0.0 <= float(skip_thr) < float('inf'):
            raise ValueError('SliceMergeOptions: skip_thr must be finite and >= 0')
        if not 1 <= int(top_n) <= SLICE_MAX_IN:
            raise ValueError('SliceMergeOptions: top_n must be in 1..%d' % SLICE_MAX_IN)
        if not 1 <= int(max_det) <= SLICE_MAX_IN:
            raise ValueError('SliceMergeOptions: max_det must be in 1..%d' % SLICE_MAX_IN)
        self.method, self.metric, self.thr, self.class_aware = method, metric, float(thr), bool(class_aware)
        self.skip_thr, self.top_n, self.max_det = float(skip_thr), int(top_n), int(max_det)

    def key(self):
        return (self.method, self.metric, self.thr, self.class_aware, self.skip_thr, self.top_n, self.max_det)

    def __repr__(self):
        return 'SliceMergeOptions(method=%r, metric=%r, thr=%r, class_aware=%r, skip_thr=%r, top_n=%d, max_det=%d)' % self.key()


class SliceOptions(_Options):
    """Sliced inference of evaluate.SlicedDetector: the image is cut into tiles of slice = (h, w) (whole multiples of 128: a tile is a
    network input) that overlap by overlap = (ratio_y, ratio_x) of the tile, each in [0, 0.9]; with full_view the whole image resampled
    to (h, w) is one more view; the tiles go through the detector tile_batch at a time; merge: the SliceMergeOptions (None: defaults)."""

    def __init__(self, slice=(512, 512), overlap=(0.2, 0.2), full_view=True, tile_batch=32, merge=None):
        merge = SliceMergeOptions() if merge is None else merge
        if not isinstance(merge, SliceMergeOptions):
            raise TypeError('SliceOptions: merge must be a SliceMergeOptions, not %r' % (merge,))
        try:
            sl, ov = tuple(int(v) for v in slice), tuple(float(v) for v in overlap)
            whole = all(float(v) == int(v) for v in slice)
        except TypeError:
            raise ValueError('SliceOptions: slice and overlap take one entry per axis: (h, w) and (ratio_y, ratio_x)') from None
        if len(sl) != 2 or not whole or not all(v >= 128 and v % 128 == 0 for v in sl):
            raise ValueError('SliceOptions: both sides of slice must be whole multiples of 128, got %r' % (slice,))
        if len(ov) != 2 or not all(0.0 <= v <= 0.9 for v in ov):
            raise ValueError('SliceOptions: overlap ratios must be in [0, 0.9], got %r' % (overlap,))
        if not int(tile_batch) >= 1:
            raise ValueError('SliceOptions: tile_batch must be >= 1')
        self.slice, self.overlap, self.full_view, self.tile_batch, self.merge = sl, ov, bool(full_view), int(tile_batch), merge

    def key(self):
        return (self.slice, self.overlap, self.full_view, self.tile_batch, self.merge.key())

    def __repr__(self):
        return 'SliceOptions(slice=%r, overlap=%r, full_view=%r, tile_batch=%d, merge=%r)' % (self.slice, self.overlap, self.full_view,
                                                                                             self.tile_batch, self.merge)


def _slice_positions(L_, s, ratio, side):
    """Tile origins along an axis of length L_: k * step while the tile ends before L_, then L_ - s (the last tile is shifted back
    into the image, not shrunk)."""
    if L_ < s:
        raise ValueError('slice_plan: the image %s %d is smaller than the slice %s %d: an image smaller than the slice needs no slicing'
                         % (side, L_, side, s))
    step = s - int(np.floor(ratio * s))
    pos, k = [], 0
    while k * step + s < L_:
        pos.append(k * step)
        k += 1
    return pos + [L_ - s]


def slice_plan(H, W, options):
    """The views of SliceOptions `options` on a batch of H x W -> [(y0, x0, h, w, my, mx)], tiles row-major (y outer): origin, size
    and the multipliers that take a view's boxes back to the image's frame (1 for a tile).  With full_view one more record goes last:
    the whole image at (0, 0) as an h x w view, my = fp32(H / h), mx = fp32(W / w) (anisotropic when the image's shape is not the
    tile's); (H, W) == (h, w) is one tile and no full view.  ValueError for an image smaller than the slice and for more candidates
    than the merge holds.  Host only: nothing is launched."""
    if not isinstance(options, SliceOptions):
        raise TypeError('slice_plan takes a SliceOptions, not %r' % (options,))
    H, W = int(H), int(W)
    h, w = options.slice
    ys = _slice_positions(H, h, options.overlap[0], 'height')
    xs = _slice_positions(W, w, options.overlap[1], 'width')
    plan = [(y, x, h, w, 1.0, 1.0) for y in ys for x in xs]
    if options.full_view and (H, W) != (h, w):
        plan.append((0, 0, h, w, float(np.float32(float(H) / float(h))), float(np.float32(float(W) / float(w)))))
    what = '%d x %d at slice %r, overlap %r gives %d x %d tiles%s' % (H, W, options.slice, options.overlap, len(ys), len(xs),
                                                                      ' and the full view' if len(plan) > len(ys) * len(xs) else '')
    if len(plan) > SLICE_MAX_TILES:
        raise ValueError('slice_plan: %s: %d views exceed the limit of %d' % (what, len(plan), SLICE_MAX_TILES))
    if len(plan) * options.merge.top_n > SLICE_MAX_IN:
        raise ValueError('slice_plan: %s; views * merge.top_n = %d * %d exceeds %d: raise the slice, lower the overlap or lower merge.top_n'
                         % (what, len(plan), options.merge.top_n, SLICE_MAX_IN))
    return plan


_slice_tables = {}     # (device, plan) -> the plan's device table: built once, so that a call copies nothing from the host
_slice_ws = {}         # (device, B, TPI, R) -> workspace of eager calls (a capture allocates its own, from the graph's pool)


def slice_table(plan, device):
    """The device tile table (effdet_slice_tile_t records as an int32 [T, 4] tensor: x0, y0 and the bits of mx, my) of a slice_plan
    list, or of any list of (y0, x0, h, w, my, mx); cached per device and plan."""
    device = torch.device(device)
    k = (device.type, device.index if device.index is not None else torch.cuda.current_device(), tuple(tuple(r) for r in plan))
    t = _slice_tables.get(k)
    if t is None:
        rec = np.zeros((len(plan), 4), dtype=np.int32)
        for i, (y0, x0, _, _, my, mx) in enumerate(plan):
            rec[i, 0], rec[i, 1] = int(x0), int(y0)
            rec[i, 2:] = np.asarray([mx, my], dtype=np.float32).view(np.int32)
        t = _slice_tables[k] = torch.from_numpy(rec).to(device)
    return t


def _as_slice_table(plan_or_table, device):
    if torch.is_tensor(plan_or_table):
        t = plan_or_table
        if t.dtype != torch.int32 or t.dim() != 2 or t.shape[1] != 4 or not t.is_contiguous() or t.shape[0] < 1 or t.data_ptr() % 16:
            raise ValueError('a tile table is a contiguous, 16-byte aligned int32 [T, 4] tensor (slice_table makes one)')
        return t
    if not len(plan_or_table):
        raise ValueError('a tile plan needs at least one tile')
    return slice_table(plan_or_table, device)


def slice_images(images, plan_or_table, size, t0, t1, out=None):
    """Tiles of a batch (include/effdet_slices.h: effdet_slice_images) -> a dense PackedImages [t1 - t0, h, w] with size = (h, w) in the
    stem conv's layout (NHWC, channels zero-padded to one 16-byte chunk): the flat tiles t0 <= t < t1 of the image-major order
    t = b * T + j, pixels copied bit for bit, origins outside the image edge-clamped.  images: a contiguous NCHW fp32 [B,3,H,W] tensor
    (the result is fp32) or a PackedImages in fp32 / bf16 (the result keeps its dtype) over any map.  plan_or_table: a slice_plan list
    or a slice_table tensor.  out: a dense Map [t1 - t0, h, w, one chunk] of the result's dtype to write into; None allocates one."""
    from .efficientdet import PackedImages
    lib = L.require('effdet_slice_images')
    h, w = (int(v) for v in size)
    t0, t1 = int(t0), int(t1)
    d = L.SliceImages()
    m = getattr(images, 'map', None)
    if m is None:
        if not torch.is_tensor(images) or images.dim() != 4 or images.shape[1] != 3:
            raise TypeError('slice_images takes an NCHW [B,3,H,W] tensor or a PackedImages')
        if images.dtype != torch.float32:
            raise TypeError('slice_images: an NCHW batch must be float32, not %s (pack other dtypes as PackedImages)' % images.dtype)
        if not images.is_contiguous():
            raise ValueError('slice_images: the NCHW batch must be contiguous')
        B, _, H, W = (int(v) for v in images.shape)
        dtype, src_bytes = torch.float32, 12
        d.src, d.src_layout, d.C, d.src_ld, d.src_bstride = L.ptr(images), L.RESAMPLE_NCHW, 3, 0, 0
    else:
        if m.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError('slice_images: PackedImages must be float32 or bfloat16, not %s' % m.dtype)
        B, H, W, dtype, src_bytes = m.B, m.H, m.W, m.dtype, 3 * m.t.element_size()
        d.src, d.src_layout, d.C, d.src_ld, d.src_bstride = m.addr(), L.RESAMPLE_NHWC, m.C, m.ld, m.bstride
    table = _as_slice_table(plan_or_table, images.device)
    T = int(table.shape[0])
    if not 0 <= t0 < t1 <= B * T:
        raise ValueError('slice_images: the tile range [%d, %d) is not inside [0, %d) (%d images of %d tiles)' % (t0, t1, B * T, B, T))
    n = t1 - t0
    ce = 4 if dtype == torch.float32 else 8                          # one 16-byte chunk of channels
    if out is None:
        out = Map.new(n, h, w, ce, dtype, images.device)
    elif (out.B, out.H, out.W, out.C, out.ld, out.bstride, out.dtype) != (n, h, w, ce, ce, h * w * ce, dtype) or out.addr() % 16:
        raise ValueError('slice_images: out must be a dense, 16-byte aligned [%d,%d,%d,%d] %s map' % (n, h, w, ce, dtype))
    d.dst, d.tiles, d.dtype = out.addr(), L.ptr(table), L.dtype_code(dtype)
    d.B, d.H, d.W, d.T, d.t0, d.t1, d.h, d.w = B, H, W, T, t0, t1, h, w
    # algorithmic bytes: three channels read and one 16-byte chunk written per output pixel
    _timed('slice_images (copy, one output pixel per thread)', n * h * w * (src_bytes + 16),
           lambda: L.check(lib.effdet_slice_images(C.byref(d), L.stream_ptr()), 'effdet_slice_images'),
           'BYTES B%d %dx%d tiles %d..%d of %dx%d' % (B, H, W, t0, t1, h, w))
    return PackedImages(out)


def merge_slices(lists, table, H, W, options=None):
    """The cross-tile merge (include/effdet_slices.h: effdet_slice_merge) of the detection lists of every view of a batch -> (scores
    [B,K], labels [B,K] int64, boxes [B,K,4], count [B] int32) with K = min(options.max_det, TPI * R): detections of the H x W image
    score-descending, count[b] of them valid, zero rows after them -- model_nms's layout.  lists: (scores [B,TPI,R], labels [B,TPI,R]
    int64, boxes [B,TPI,R,4], count [B,TPI] int32), each list (b, j) in tile j's frame as model_nms returns it, narrowed to R columns;
    table: the slice_plan list or slice_table tensor of the TPI views.  options.top_n is not applied here: R is.  All on device, no sync."""
    lib = L.require('effdet_slice_merge', 'effdet_slice_merge_workspace_bytes')
    options = SliceMergeOptions() if options is None else options
    s, l, b, c = lists
    if s.dim() != 3 or tuple(l.shape) != tuple(s.shape) or tuple(b.shape) != tuple(s.shape) + (4,) or tuple(c.shape) != tuple(s.shape[:2]):
        raise ValueError('merge_slices: lists must be scores [B,TPI,R], labels [B,TPI,R], boxes [B,TPI,R,4], count [B,TPI]')
    if (s.dtype, l.dtype, b.dtype, c.dtype) != (torch.float32, torch.int64, torch.float32, torch.int32):
        raise TypeError('merge_slices: lists must be (float32, int64, float32, int32) tensors')
    B, TPI, R = (int(v) for v in s.shape)
    dev = s.device
    table = _as_slice_table(table, dev)
    if int(table.shape[0]) != TPI:
        raise ValueError('merge_slices: %d lists per image but %d tiles in the table' % (TPI, int(table.shape[0])))
    if B < 1 or R < 1 or TPI > SLICE_MAX_TILES or TPI * R > SLICE_MAX_IN:
        raise ValueError('merge_slices: B >= 1, R >= 1, TPI <= %d and TPI * R <= %d, got B = %d, TPI * R = %d * %d'
                         % (SLICE_MAX_TILES, SLICE_MAX_IN, B, TPI, R))
    if not (0.0 < float(H) < float('inf') and 0.0 < float(W) < float('inf')):
        raise ValueError('merge_slices: H and W must be positive and finite')
    s, l, b, c = s.contiguous(), l.contiguous(), b.contiguous(), c.contiguous()
    K = min(options.max_det, TPI * R)
    d = L.SliceMerge()
    d.score, d.label, d.boxes, d.count, d.tiles = L.ptr(s), L.ptr(l), L.ptr(b), L.ptr(c), L.ptr(table)
    d.B, d.TPI, d.R, d.method, d.metric = B, TPI, R, SLICE_METHODS[options.method], SLICE_METRICS[options.metric]
    d.class_aware, d.max_det, d.W, d.H, d.thr, d.skip_thr = int(options.class_aware), K, float(W), float(H), options.thr, options.skip_thr
    os_ = torch.empty((B, K), dtype=torch.float32, device=dev)
    ol = torch.empty((B, K), dtype=torch.int64, device=dev)
    ob = torch.empty((B, K, 4), dtype=torch.float32, device=dev)
    count = torch.empty((B,), dtype=torch.int32, device=dev)
    d.out_score, d.out_label, d.out_boxes, d.out_count = L.ptr(os_), L.ptr(ol), L.ptr(ob), L.ptr(count)
    nbytes = int(lib.effdet_slice_merge_workspace_bytes(B, TPI, R))
    if torch.cuda.is_current_stream_capturing():
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    else:
        k = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device(), B, TPI, R)
        ws = _slice_ws.get(k)
        if ws is None:
            ws = _slice_ws[k] = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    # algorithmic bytes: every list's rows read once (score, label, box: 28 B), the merged rows written once; the greedy pass is LDS / latency
    _timed('slice_merge (keys + radix sort + per-image greedy pass)', 28 * B * TPI * R + 28 * B * K,
           lambda: L.check(lib.effdet_slice_merge(C.byref(d), L.ptr(ws), nbytes, L.stream_ptr()), 'effdet_slice_merge'),
           'BYTES B%d TPI%d R%d' % (B, TPI, R))
    return os_, ol, ob, count


# ----------------------------------------------------------------------------- loss
# Six sets of entry points, one per kind of call.  The calls of a kind take the same arguments in every set, the set's own ones just
# before the stream; each public function below names the call it wants, and _loss_entry alone chooses the set:
#   effdet_focal_loss_*    the reference's constants (no extra argument; the only set with the combined backward _bwd / _bwd_pix)
#   effdet_box_loss_*      the same with an IoU-family box term: kind, weight
#   effdet_loss_opts_*     non-default LossOptions: the options struct, with the box term inside it.  Its backward calls (_bwd_cls,
#                          _bwd_reg) also serve every set below, with the struct even where its values are the defaults
#   effdet_loss_atss_*     a matcher (ATSSOptions), forward calls only: the options struct, then the matcher's
#   effdet_loss_quality_*  a quality loss (QualityLossOptions), forward calls and the class backward: the options struct, the matcher's
#                          or NULL (forward only), its own
#   effdet_loss_tal_*      the task-aligned matcher (TaskAlignedOptions), forward calls only: the options struct, the matcher's, the
#                          quality loss's or NULL; its class backward is the options set's resp. the quality loss's
# Every set has its workspace layout, which effdet_loss[_<set>]_workspace_bytes sizes (the box set shares the reference's).
BOX_LOSS_KINDS = {'smooth_l1': 0, 'iou': 1, 'giou': 2, 'diou': 3, 'ciou': 4}     # EFFDET_BOX_LOSS_* (0: the effdet_focal_loss_* calls)


class BoxLossOptions(_Options):
    """The box regression term of EfficientDet.set_box_loss / FocalLoss(box_loss=) (include/effdet_box_loss.h): kind 'smooth_l1' (the
    reference's, on the encoded deltas) or 'iou' | 'giou' | 'diou' | 'ciou' between the decoded prediction and the assigned annotation,
    in place of smooth-L1; weight multiplies the IoU kinds' loss (and gradient).  smooth_l1 is the reference's term as it is: it takes
    no weight other than 1."""

    def __init__(self, kind='smooth_l1', weight=1.0):
        if kind not in BOX_LOSS_KINDS:
            raise ValueError('BoxLossOptions: kind must be one of %s, not %r' % (sorted(BOX_LOSS_KINDS), kind))
        w = float(weight)
        if not 0.0 <= w < float('inf'):
            raise ValueError('BoxLossOptions: weight must be finite and >= 0')
        if kind == 'smooth_l1' and w != 1.0:
            raise ValueError("BoxLossOptions: kind 'smooth_l1' is the reference's unweighted term (weight 1.0)")
        self.kind, self.weight = kind, w

    def key(self):
        return (self.kind, self.weight)

    def is_default(self):
        return self.kind == 'smooth_l1'

    def __repr__(self):
        return 'BoxLossOptions(kind=%r, weight=%r)' % self.key()


def _box_loss_args(options):
    """-> None for the smooth-L1 path (options None or kind 'smooth_l1'), else (kind code, weight)."""
    if options is None:
        return None
    if not isinstance(options, BoxLossOptions):
        raise TypeError('box loss options must be a BoxLossOptions or None, not %r' % (options,))
    return None if options.is_default() else (BOX_LOSS_KINDS[options.kind], options.weight)


def _f32(v):
    return C.c_float(float(v)).value


LOSS_BETA_DEFAULT = _f32(1.0 / 9.0)                  # the reference's smooth-L1 knee as the fp32 the kernels compare with


class LossOptions(_Options):
    """The options of the training loss of EfficientDet.set_loss / FocalLoss(loss=) (include/effdet_loss_opts.h): focal alpha and gamma,
    label smoothing eps (soft target h (1 - eps) + eps / 2), the smooth-L1 knee beta (Huber delta) and its weight reg_weight, the
    matcher's bands (positive at IoU >= pos_iou, negative below neg_iou, ignored between) and low_quality (every annotation's best
    anchor(s) become positive, torchvision's allow_low_quality_matches).  Values are kept as the fp32 the kernels receive.  The
    defaults are the reference's constants: a LossOptions equal to them is the existing ops.focal_loss_* / box_loss_* calls."""

    _FIELDS = ('alpha', 'gamma', 'label_smoothing', 'beta', 'reg_weight', 'pos_iou', 'neg_iou', 'low_quality')

    def __init__(self, alpha=0.25, gamma=2.0, label_smoothing=0.0, beta=LOSS_BETA_DEFAULT, reg_weight=1.0, pos_iou=0.5, neg_iou=0.4,
                 low_quality=False):
        a, g, e, b, w, hi, lo = (_f32(v) for v in (alpha, gamma, label_smoothing, beta, reg_weight, pos_iou, neg_iou))
        inf = float('inf')
        if not 0.0 < a < 1.0:
            raise ValueError('LossOptions: alpha must lie in (0, 1), not %r' % (alpha,))
        if not 0.0 <= g <= 8.0:
            raise ValueError('LossOptions: gamma must lie in [0, 8], not %r' % (gamma,))
        if not 0.0 <= e < 1.0:
            raise ValueError('LossOptions: label_smoothing must lie in [0, 1), not %r' % (label_smoothing,))
        if not 0.0 < b < inf:
            raise ValueError('LossOptions: beta must be finite and > 0, not %r' % (beta,))
        if not 0.0 <= w < inf:
            raise ValueError('LossOptions: reg_weight must be finite and >= 0, not %r' % (reg_weight,))
        if not 0.0 <= lo <= hi <= 1.0:
            raise ValueError('LossOptions: need 0 <= neg_iou <= pos_iou <= 1, not neg_iou %r, pos_iou %r' % (neg_iou, pos_iou))
        if low_quality not in (False, True, 0, 1):
            raise ValueError('LossOptions: low_quality must be a bool, not %r' % (low_quality,))
        self.alpha, self.gamma, self.label_smoothing, self.beta, self.reg_weight, self.pos_iou, self.neg_iou = a, g, e, b, w, hi, lo
        self.low_quality = bool(low_quality)

    def key(self):
        return tuple(getattr(self, f) for f in self._FIELDS)

    def is_default(self):
        return self.key() == _LOSS_DEFAULT_KEY

    def __repr__(self):
        return 'LossOptions(%s)' % ', '.join('%s=%r' % (f, getattr(self, f)) for f in self._FIELDS)


_LOSS_DEFAULT_KEY = LossOptions().key()


class ATSSOptions(_Options):
    """The ATSS matcher of EfficientDet.set_matcher / FocalLoss(matcher=) (include/effdet_atss.h), in place of the IoU bands: per
    annotation the topk anchors nearest its centre on every pyramid level are candidates, positive where their IoU reaches the
    candidates' mean + standard deviation and their centre lies inside the box."""

    def __init__(self, topk=9):
        if isinstance(topk, bool) or not isinstance(topk, int) or not 1 <= topk <= L.ATSS_MAX_TOPK:
            raise ValueError('ATSSOptions: topk must be an int in [1, %d], not %r' % (L.ATSS_MAX_TOPK, topk))
        self.topk = topk

    def key(self):
        return (self.topk,)

    def __repr__(self):
        return 'ATSSOptions(topk=%r)' % self.topk


class TaskAlignedOptions(_Options):
    """The task-aligned matcher of EfficientDet.set_matcher / FocalLoss(matcher=) (include/effdet_tal.h; TOOD, PP-YOLOE, YOLOv8), in
    place of the IoU bands: per annotation, among the anchors whose centre lies inside its box, the topk with the largest alignment
    metric m = s^alpha u^beta are selected -- s the PREDICTED probability of the annotation's class, u the IoU between the DECODED
    prediction and the annotation -- and an anchor selected by several annotations takes the one with the largest u.  With a quality
    loss and aligned_target the soft target of a positive is m normalised per annotation to its largest IoU (TOOD's target) instead of
    the IoU itself.  Values are kept as the fp32 the kernels receive.  The assignment reads the predictions, so it is usually switched
    on after a few epochs of ATSS (set_matcher plus a new capture of a graphed step); it needs no pyramid levels."""

    def __init__(self, topk=13, alpha=1.0, beta=6.0, aligned_target=True):
        if isinstance(topk, bool) or not isinstance(topk, int) or not 1 <= topk <= L.TAL_MAX_TOPK:
            raise ValueError('TaskAlignedOptions: topk must be an int in [1, %d], not %r' % (L.TAL_MAX_TOPK, topk))
        a, b = _f32(alpha), _f32(beta)
        if not 0.0 <= a <= 4.0:
            raise ValueError('TaskAlignedOptions: alpha must lie in [0, 4], not %r' % (alpha,))
        if not 0.0 <= b <= 16.0:
            raise ValueError('TaskAlignedOptions: beta must lie in [0, 16], not %r' % (beta,))
        if aligned_target not in (False, True, 0, 1):
            raise ValueError('TaskAlignedOptions: aligned_target must be a bool, not %r' % (aligned_target,))
        self.topk, self.alpha, self.beta, self.aligned_target = topk, a, b, bool(aligned_target)

    def key(self):
        return (self.topk, self.alpha, self.beta, self.aligned_target)

    def __repr__(self):
        return 'TaskAlignedOptions(topk=%r, alpha=%r, beta=%r, aligned_target=%r)' % self.key()


MATCHERS = (ATSSOptions, TaskAlignedOptions)


QUALITY_KINDS = {'qfl': L.QUALITY_QFL, 'vfl': L.QUALITY_VFL}     # EFFDET_QUALITY_*


class QualityLossOptions(_Options):
    """The IoU-aware class term of EfficientDet.set_quality_loss / FocalLoss(quality=) (include/effdet_quality_loss.h), in place of the
    hard-target focal loss: the target of a positive anchor's assigned label is q, the IoU between its DECODED prediction and its
    annotation (a constant of the gradient).  kind 'qfl': GFL's quality focal loss |q - p|^beta BCE(p, q); kind 'vfl': the varifocal
    loss, q BCE(p, q) on those elements and alpha p^gamma BCE(p, 0) on every other.  Values are kept as the fp32 the kernels receive
    (each must be in range whatever the kind).  The sums are normalised per image by its number of positives, as every class term
    here (mmdet: one batch-wide normaliser); there is no distribution focal loss and no distribution head."""

    def __init__(self, kind='qfl', beta=2.0, alpha=0.75, gamma=2.0):
        if kind not in QUALITY_KINDS:
            raise ValueError('QualityLossOptions: kind must be one of %s, not %r' % (sorted(QUALITY_KINDS), kind))
        b, a, g = _f32(beta), _f32(alpha), _f32(gamma)
        if not 1.0 <= b <= 8.0:
            raise ValueError('QualityLossOptions: beta must lie in [1, 8], not %r' % (beta,))
        if not 0.0 < a <= 1.0:
            raise ValueError('QualityLossOptions: alpha must lie in (0, 1], not %r' % (alpha,))
        if not 0.0 <= g <= 8.0:
            raise ValueError('QualityLossOptions: gamma must lie in [0, 8], not %r' % (gamma,))
        self.kind, self.beta, self.alpha, self.gamma = kind, b, a, g

    def key(self):
        return (self.kind, self.beta, self.alpha, self.gamma)

    def __repr__(self):
        return 'QualityLossOptions(kind=%r, beta=%r, alpha=%r, gamma=%r)' % self.key()


def check_quality(quality, loss):
    """TypeError on anything but a QualityLossOptions / None; ValueError where loss sets what a quality loss replaces (focal alpha /
    gamma, label smoothing)."""
    if quality is None:
        return
    if not isinstance(quality, QualityLossOptions):
        raise TypeError('quality loss options must be a QualityLossOptions or None, not %r' % (quality,))
    if isinstance(loss, LossOptions) and loss.key()[:3] != _LOSS_DEFAULT_KEY[:3]:
        raise ValueError('%r replaces the focal class term: it cannot be combined with the alpha / gamma / label_smoothing of %r'
                         % (quality, loss))


def _quality_struct(quality):
    return L.QualityLoss(QUALITY_KINDS[quality.kind], quality.beta, quality.alpha, quality.gamma)


def check_matcher(matcher, loss):
    """TypeError on anything but an ATSSOptions / TaskAlignedOptions / None; ValueError where loss sets what a matcher replaces (bands,
    low_quality)."""
    if matcher is None:
        return
    if not isinstance(matcher, MATCHERS):
        raise TypeError('matcher must be an ATSSOptions, a TaskAlignedOptions or None, not %r' % (matcher,))
    if isinstance(loss, LossOptions) and (loss.low_quality or (loss.pos_iou, loss.neg_iou) != _LOSS_DEFAULT_KEY[5:7]):
        raise ValueError('%r replaces the IoU bands: it cannot be combined with the pos_iou / neg_iou / low_quality of %r'
                         % (matcher, loss))


def _atss_struct(matcher, levels, A):
    """-> the effdet_atss_t of matcher on a table of A anchors cut into levels (the anchor count of every level, in table order)."""
    if levels is None:
        raise ValueError('a matcher needs levels: the anchor count of every pyramid level')
    levels = [int(v) for v in levels]
    if not 1 <= len(levels) <= L.ATSS_MAX_LEVELS or min(levels) < 1 or sum(levels) != A:
        raise ValueError('levels must be 1 .. %d positive anchor counts that add up to A = %d, not %r' % (L.ATSS_MAX_LEVELS, A, levels))
    t = L.Atss(matcher.topk, len(levels))
    for i, v in enumerate(levels):
        t.level_start[i + 1] = t.level_start[i] + v
    return t


def _tal_struct(matcher):
    return L.Tal(matcher.topk, matcher.alpha, matcher.beta, 1 if matcher.aligned_target else 0)


def _matcher_struct(matcher, levels, A):
    """-> the host struct of matcher for the forward calls: an effdet_atss_t (it needs levels), an effdet_tal_t, or None."""
    if matcher is None:
        return None
    return _tal_struct(matcher) if isinstance(matcher, TaskAlignedOptions) else _atss_struct(matcher, levels, A)


def _loss_opts_struct(loss, box=None, force=False):
    """-> None where the existing calls apply (loss None or equal to the defaults), else the effdet_loss_opts_t of (loss, box).
    force: the options path although default (a matcher's calls take the struct whatever its values)."""
    if loss is None and force:
        loss = LossOptions()
    if loss is None:
        return None
    if not isinstance(loss, LossOptions):
        raise TypeError('loss options must be a LossOptions or None, not %r' % (loss,))
    if loss.is_default() and not force:
        return None
    kw = _box_loss_args(box)
    kind, weight = (0, 1.0) if kw is None else kw
    return L.LossOpts(loss.alpha, loss.gamma, loss.label_smoothing, loss.beta, loss.reg_weight, loss.pos_iou, loss.neg_iou,
                      1 if loss.low_quality else 0, kind, weight)


def _loss_entry(stem, loss=None, box=None, matcher=None, atss=None, quality=None):
    """-> (the entry point of the call `stem` for (loss, box, matcher, quality), its name, its extra arguments, whether it is of the
    options set, and for a forward call ws_bytes(B, A, nc, N): the size of the workspace the call needs, by its set's own
    *_workspace_bytes).  atss: the matcher's effdet_atss_t resp. effdet_tal_t, for the forward calls.  A quality loss has calls of its own
    for the forward and the class backward (the options struct, the matcher's or NULL on the forward calls, its own); its d(reg) call
    is the options set's, with the options struct even where its values are the defaults.  A TaskAlignedOptions has forward calls of
    its own (the options struct, its own, the quality loss's or NULL)."""
    check_matcher(matcher, loss)
    check_quality(quality, loss)
    o = _loss_opts_struct(loss, box, force=matcher is not None or quality is not None)
    forward = stem in ('fwd', 'fwd_grad')
    ref = lambda s: None if s is None else C.byref(s)      # noqa: E731
    ql = None if quality is None else _quality_struct(quality)
    sized = (ref(atss),)                                   # what the set's workspace-bytes call takes after (B, A, nc, N); None: no N
    if isinstance(atss, L.Tal) and forward:
        family, extra = 'loss_tal', (ref(o), ref(atss), ref(ql))
    elif quality is not None and stem != 'bwd_reg':
        family, extra = 'loss_quality', (ref(o),) + ((ref(atss),) if forward else ()) + (ref(ql),)
    elif atss is not None:
        family, extra = 'loss_atss', (ref(o), ref(atss))
    elif o is not None:
        family, extra, sized = 'loss_opts', (ref(o),), ()
    else:
        kw = _box_loss_args(box)
        family, extra, sized = 'focal_loss' if kw is None else 'box_loss', kw or (), None
    name, wname = 'effdet_%s_%s' % (family, stem), 'effdet_%s_workspace_bytes' % ('loss' if sized is None else family)
    ws_bytes = lambda B, A, nc, N: int(getattr(L.require(wname), wname)(B, A, nc, *(() if sized is None else (N,) + sized)))      # noqa: E731
    return getattr(L.require(name), name), name, extra, o is not None, ws_bytes if forward else None


def _dtype_code(dtype, split):
    return L.F32_SPLIT if split else L.dtype_code(dtype)


def _loss_forward(cls, reg, anc, annots, loss, box, grad=None, matcher=None, levels=None, quality=None):
    """Forward of (loss, box, matcher, quality) -> (losses [2], ws), and with grad = (dtype, dld, split) also dcls_pix [B, A/9, dld]."""
    B, A, nc = cls.shape
    N = annots.shape[1]
    check_matcher(matcher, loss)
    atss = _matcher_struct(matcher, levels, A)
    fn, name, extra, _, ws_bytes = _loss_entry('fwd_grad' if grad else 'fwd', loss, box, matcher, atss, quality)
    nbytes = ws_bytes(B, A, nc, N)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=cls.device)
    losses = torch.empty(2, dtype=torch.float32, device=cls.device)
    out, args = (losses, ws), ()
    if grad:
        dtype, dld, split = grad
        dcls = torch.empty((B, A // 9, dld), dtype=dtype, device=cls.device)
        out, args = (losses, ws, dcls), (L.ptr(dcls), dld, _dtype_code(dtype, split))
    L.check(fn(L.ptr(cls), L.ptr(reg), L.ptr(anc), L.ptr(annots), L.ptr(losses), L.ptr(ws), nbytes, *args, B, A, nc, N, *extra,
               L.stream_ptr()), name)
    return out


def _loss_bwd_reg(reg, anc, annots, gscale, ws, dtype, reg_ld, split, loss, box, matcher=None, quality=None):
    """-> dreg [B, A, 4], or with reg_ld pixel-major and channel-padded [B, A/9, reg_ld] (split=True: in the split layout), from the
    workspace of a forward call with the same (loss, box, matcher, quality)."""
    fn, name, extra = _loss_entry('bwd_reg', loss, box, matcher, quality=quality)[:3]
    B, A, _ = reg.shape
    dreg = torch.empty((B, A // 9, reg_ld) if reg_ld else (B, A, 4), dtype=dtype, device=reg.device)
    L.check(fn(L.ptr(reg), L.ptr(anc), L.ptr(annots), L.ptr(gscale), L.ptr(ws), L.ptr(dreg), reg_ld, _dtype_code(dtype, split), B, A,
               annots.shape[1], *extra, L.stream_ptr()), name)
    return dreg


def focal_loss_fwd(cls, reg, anc, annots):
    return _loss_forward(cls, reg, anc, annots, None, None)


def focal_loss_bwd(cls, reg, anc, annots, gscale, ws, dtype):
    return focal_loss_bwd_pix(cls, reg, anc, annots, gscale, ws, dtype, None)


def focal_loss_bwd_pix(cls, reg, anc, annots, gscale, ws, dtype, dld):
    """focal_loss_bwd with d(cls logits) pixel-major and channel-padded: -> (dcls_pix [B, A/9, dld], dreg [B, A, 4])."""
    # the reference's constants have the combined entry points (dld None: the flat one, d(logits) [B, A, nc]), which also write dreg
    B, A, nc = cls.shape
    dcls = torch.empty((B, A // 9, dld) if dld else (B, A, nc), dtype=dtype, device=cls.device)
    name = 'effdet_focal_loss_bwd' if dld is None else 'effdet_focal_loss_bwd_pix'
    dreg = torch.empty((B, A, 4), dtype=dtype, device=cls.device)
    L.check(getattr(L.lib(), name)(L.ptr(cls), L.ptr(reg), L.ptr(anc), L.ptr(annots), L.ptr(gscale), L.ptr(ws), L.ptr(dcls),
                                   *(() if dld is None else (dld,)), L.ptr(dreg), L.dtype_code(dtype), B, A, nc, annots.shape[1],
                                   L.stream_ptr()), name)
    return dcls, dreg


def focal_loss_fwd_grad(cls, reg, anc, annots, dtype, dld, split=False):
    """Training fast path: -> (losses [2], ws, dcls_pix [B, A/9, dld]) in one pass over cls; dcls_pix is the gradient wrt the
    logits for an upstream gradient of ONE (the caller scales downstream, see effdet_hip.h)."""
    return _loss_forward(cls, reg, anc, annots, None, None, (dtype, dld, split))


def focal_loss_bwd_reg(reg, anc, annots, gscale, ws, dtype, reg_ld=0, split=False):
    """-> dreg [B, A, 4], or with reg_ld pixel-major and channel-padded [B, A/9, reg_ld] (split=True: in the split layout)."""
    return _loss_bwd_reg(reg, anc, annots, gscale, ws, dtype, reg_ld, split, None, None)


def box_loss_fwd(cls, reg, anc, annots, options=None):
    """focal_loss_fwd with the box term of options (None / 'smooth_l1': focal_loss_fwd itself) -> (losses [2], ws)."""
    return _loss_forward(cls, reg, anc, annots, None, options)


def box_loss_fwd_grad(cls, reg, anc, annots, dtype, dld, split=False, options=None):
    """focal_loss_fwd_grad with the box term of options -> (losses [2], ws, dcls_pix [B, A/9, dld])."""
    return _loss_forward(cls, reg, anc, annots, None, options, (dtype, dld, split))


def box_loss_bwd_reg(reg, anc, annots, gscale, ws, dtype, reg_ld=0, split=False, options=None):
    """focal_loss_bwd_reg with the box term of options: d(reg) in the same three layouts, from the workspace of any forward call."""
    return _loss_bwd_reg(reg, anc, annots, gscale, ws, dtype, reg_ld, split, None, options)


def loss_opts_fwd(cls, reg, anc, annots, loss=None, box=None, matcher=None, levels=None, quality=None):
    """box_loss_fwd with the options of loss (None / the defaults: box_loss_fwd itself) -> (losses [2], ws).  matcher: an ATSSOptions
    assigns by ATSS over the pyramid levels (levels: the anchor count of every level) through the effdet_loss_atss_* calls, a
    TaskAlignedOptions by the task-aligned rule on the predictions through the effdet_loss_tal_* calls (no levels), either with
    the options struct of loss (None / the defaults: the default VALUES through the option kernels).  quality: a QualityLossOptions
    puts its IoU-aware class term in the place of the focal one through the effdet_loss_quality_* calls (the options struct likewise;
    one more launch, which leaves the targets in the workspace: loss_quality_targets)."""
    return _loss_forward(cls, reg, anc, annots, loss, box, None, matcher, levels, quality)


def loss_opts_fwd_grad(cls, reg, anc, annots, dtype, dld, split=False, loss=None, box=None, matcher=None, levels=None, quality=None):
    """box_loss_fwd_grad with the options of loss (and the matcher, and the quality loss) -> (losses [2], ws, dcls_pix [B, A/9, dld])."""
    return _loss_forward(cls, reg, anc, annots, loss, box, (dtype, dld, split), matcher, levels, quality)


def loss_opts_bwd_cls(cls, annots, gscale, ws, dtype, loss, dld=0, matcher=None, quality=None):
    """d(logits) of the class term with the (non-default) options of loss, from the workspace of a forward call with them:
    [B, A, nc], or with dld pixel-major and channel-padded [B, A/9, dld].  With a matcher or a quality loss the options path is taken
    whatever loss."""
    if matcher is None and quality is None and _loss_opts_struct(loss) is None:
        raise ValueError('loss_opts_bwd_cls is the non-default path: the defaults are focal_loss_bwd / focal_loss_bwd_pix')
    B, A, nc = cls.shape
    dcls = torch.empty((B, A // 9, dld) if dld else (B, A, nc), dtype=dtype, device=cls.device)
    fn, name, extra = _loss_entry('bwd_cls', loss, None, matcher, quality=quality)[:3]
    L.check(fn(L.ptr(cls), L.ptr(annots), L.ptr(gscale), L.ptr(ws), L.ptr(dcls), dld, L.dtype_code(dtype), B, A, nc, annots.shape[1],
               *extra, L.stream_ptr()), name)
    return dcls


def loss_opts_bwd_reg(reg, anc, annots, gscale, ws, dtype, reg_ld=0, split=False, loss=None, box=None, matcher=None, quality=None):
    """box_loss_bwd_reg with the options of loss: d(reg) in the same three layouts (matcher / quality: the options path whatever loss)."""
    return _loss_bwd_reg(reg, anc, annots, gscale, ws, dtype, reg_ld, split, loss, box, matcher, quality)


def _al256(n):
    return (n + 255) // 256 * 256


def _tal_tail_bytes(B, A, N):
    """The task-aligned matcher's own buffers behind q (include/effdet_tal.h): keys, (mmax, umax), claims."""
    return _al256(8 * L.TAL_MAX_TOPK * B * N) + _al256(8 * B * N) + _al256(8 * B * A)


def loss_quality_targets(ws, B, A, N, matcher=None):
    """-> q [B, A] fp32, a VIEW of the workspace ws that a forward call with a quality loss left (include/effdet_quality_loss.h): the
    IoU between a positive anchor's decoded prediction and its annotation, clamped to [0, 1]; 0 at every other anchor (so
    q.sum() / (codes >= 0).sum() is the mean IoU of the positives).  It is the last buffer of the workspace and lies at the same offset
    for the bands and ATSS; behind a TaskAlignedOptions call (matcher must then name it) the matcher's own buffers follow it, and with
    aligned_target q is the normalised alignment metric (include/effdet_tal.h).  N and matcher name the call that left ws."""
    if matcher is not None and not isinstance(matcher, MATCHERS):
        raise TypeError('matcher must be an ATSSOptions, a TaskAlignedOptions or None, not %r' % (matcher,))
    nq = _al256(4 * B * A)
    tail = _tal_tail_bytes(B, A, N) if isinstance(matcher, TaskAlignedOptions) else 0
    if ws.dtype != torch.uint8 or ws.dim() != 1 or N < 1 or ws.numel() < tail + nq + 4 * B * A:
        raise ValueError('ws is not the workspace of a forward call with a quality loss on [%d, %d] anchors' % (B, A))
    off = ws.numel() - tail - nq
    return ws[off:off + 4 * B * A].view(torch.float32).reshape(B, A)


def loss_tal_candidates(ws, B, A, N):
    """-> (keys [B, N, 16] int64, mm [B, N, 2] fp32), VIEWS of the workspace ws that a forward call with a TaskAlignedOptions left
    (include/effdet_tal.h).  keys: every annotation's selected anchors in rank order, (~bits(m) << 32) | anchor as the 64-bit pattern,
    padded with -1 (all ones); mm: (mmax, umax) of the rows an aligned target was formed for, else 0."""
    tail = _tal_tail_bytes(B, A, N)
    if ws.dtype != torch.uint8 or ws.dim() != 1 or N < 1 or ws.numel() < tail:
        raise ValueError('ws is not the workspace of a forward call with a TaskAlignedOptions on [%d, %d] anchors, %d rows' % (B, A, N))
    off = ws.numel() - tail
    nk = 8 * L.TAL_MAX_TOPK * B * N
    keys = ws[off:off + nk].view(torch.int64).reshape(B, N, L.TAL_MAX_TOPK)
    off += _al256(nk)
    return keys, ws[off:off + 8 * B * N].view(torch.float32).reshape(B, N, 2)


def loss_tal_metrics(cls, reg, anc, annots, options):
    """-> (m, u), each [B, N, A] fp32: the alignment metric and the IoU of every (annotation, anchor) pair as the task-aligned matcher
    of options evaluates them (the same device function); 0 where the anchor's centre is not inside the annotation, for a pad row and
    for a label outside the classes.  For inspection and tests: B N A values are written."""
    if not isinstance(options, TaskAlignedOptions):
        raise TypeError('options must be a TaskAlignedOptions, not %r' % (options,))
    B, A, nc = cls.shape
    N = annots.shape[1]
    out = torch.empty((2, B, N, A), dtype=torch.float32, device=cls.device)
    t = _tal_struct(options)
    lib = L.require('effdet_loss_tal_metrics')
    L.check(lib.effdet_loss_tal_metrics(L.ptr(cls), L.ptr(reg), L.ptr(anc), L.ptr(annots), L.ptr(out), B, A, nc, N, C.byref(t),
                                        L.stream_ptr()), 'effdet_loss_tal_metrics')
    return out[0], out[1]


def pad_rows(src_map, cpad):
    """Level map with unaligned channel count -> fresh contiguous [B,H,W,cpad] map, zero padded."""
    m = src_map
    dst = Map.new(m.B, m.H, m.W, cpad, m.dtype, m.t.device)
    L.check(L.lib().effdet_pad_rows(L.ptr(m.t), L.ptr(dst.t), L.dtype_code(m.dtype), m.off, m.bstride,
                                    m.ld, m.B, m.H * m.W, m.C, cpad, L.stream_ptr()), 'effdet_pad_rows')
    return dst


# ----------------------------------------------------------------------------- boundary kernels (csrc/pipeline.hip)
def drop_connect_scales(keep_dev, B, seed, step, step_dev=None):
    """-> [nslot, B] fp32 rows of floor(keep + u)/keep (models/utils.py:79-90), one launch for every skip block of a step.
    step_dev (int64 device tensor [1]): the step counter lives on the device and is advanced by the kernel (hipGraph replay)."""
    n = keep_dev.numel()
    out = torch.empty((n, B), dtype=torch.float32, device=keep_dev.device)
    L.check(L.lib().effdet_drop_connect_scales(L.ptr(out), L.ptr(keep_dev), n, B, seed & (2 ** 64 - 1), int(step), L.ptr(step_dev),
                                               L.stream_ptr()), 'effdet_drop_connect_scales')
    return out


def philox_host(ctr, key):
    """Host twin of the device generator (Philox4x32-10): -> 4 uint32 words."""
    c = (C.c_uint * 4)(*ctr); k = (C.c_uint * 2)(*key); o = (C.c_uint * 4)()
    L.lib().effdet_philox4x32_10(c, k, o)
    return [int(x) for x in o]


def preprocess_batch(src_u8, src_off, src_hw, S, dtype, cpad, mean, std, flip=None, annots=None):
    """uint8 HWC images (concatenated, device) -> (Map [B,S,S,cpad] normalised / resized / padded, scale [B] fp32).
    annots [B,M,5] fp32 (device) is transformed in place (datasets/augmentation.py:69-150)."""
    B = src_hw.shape[0]
    out = Map.new(B, S, S, cpad, dtype, src_u8.device)
    scale = torch.empty(B, dtype=torch.float32, device=src_u8.device)
    m = (C.c_float * 3)(*mean); s = (C.c_float * 3)(*std)
    L.check(L.lib().effdet_preprocess_batch(L.ptr(src_u8), L.ptr(src_off), L.ptr(src_hw), L.ptr(flip), L.ptr(out.t), L.ptr(scale),
                                            L.ptr(annots), annots.shape[1] if annots is not None else 0, L.dtype_code(dtype), B, S,
                                            cpad, m, s, L.stream_ptr()), 'effdet_preprocess_batch')
    return out, scale


def finalize_dets(score, label, boxes, count, scale, score_threshold, max_det, xywh=False):
    """Batched eval consumer: -> (out [B,max_det,6] = x1,y1,x2,y2,score,label with boxes / scale, out_count [B] int32)."""
    B, A = score.shape
    out = torch.empty((B, max_det, 6), dtype=torch.float32, device=score.device)
    oc = torch.empty(B, dtype=torch.int32, device=score.device)
    L.check(L.lib().effdet_finalize_dets(L.ptr(score), L.ptr(label), L.ptr(boxes), L.ptr(count), L.ptr(scale),
                                         float(score_threshold), max_det, int(xywh), L.ptr(out), L.ptr(oc), B, A,
                                         L.stream_ptr()), 'effdet_finalize_dets')
    return out, oc


VOC_MAX_GT = 2048                  # GT rows per image effdet_voc_match stages in LDS


def voc_match(dets, counts, gt_boxes, gt_labels, num_classes, iou_threshold, rec_key, rec_tp, gt_count):
    """VOC matching of one batch: dets [B,max_det,6] fp32 + counts [B] int32 (finalize_dets), gt_boxes [B,G,4] fp64, gt_labels [B,G]
    int32 (-1 = pad) -> writes rec_key / rec_tp [B*max_det] (int64 viewed as uint64 / uint8) and adds to gt_count [num_classes] int32."""
    B, max_det = int(dets.shape[0]), int(dets.shape[1])
    G = int(gt_boxes.shape[1])
    assert dets.dtype == torch.float32 and dets.is_contiguous() and dets.shape[2] == 6
    assert counts.dtype == torch.int32 and counts.is_contiguous() and counts.numel() == B
    assert gt_boxes.dtype == torch.float64 and gt_boxes.is_contiguous() and tuple(gt_boxes.shape) == (B, G, 4)
    assert gt_labels.dtype == torch.int32 and gt_labels.is_contiguous() and tuple(gt_labels.shape) == (B, G)
    assert rec_key.dtype == torch.int64 and rec_tp.dtype == torch.uint8 and rec_key.numel() >= B * max_det and rec_tp.numel() >= B * max_det
    assert gt_count.dtype == torch.int32 and gt_count.numel() == num_classes
    L.check(L.lib().effdet_voc_match(L.ptr(dets), L.ptr(counts), L.ptr(gt_boxes), L.ptr(gt_labels), B, max_det, G, int(num_classes),
                                     float(iou_threshold), L.ptr(rec_key), L.ptr(rec_tp), L.ptr(gt_count), L.stream_ptr()),
            'effdet_voc_match')


def voc_ap(rec_key, rec_tp, num_records, gt_count, num_classes):
    """Per-class AP over the first num_records records -> (out [2, C] fp64 = (ap, num_annotations), recall [N] fp64, precision [N]
    fp64 in sorted order, seg [C, 2] int32 = each class's [start, end) in that order)."""
    dev = gt_count.device
    N = int(num_records)
    ws = torch.empty(int(L.lib().effdet_voc_ap_workspace_bytes(N)), dtype=torch.uint8, device=dev)
    out = torch.empty((2, num_classes), dtype=torch.float64, device=dev)
    recall = torch.empty(max(N, 1), dtype=torch.float64, device=dev)
    precision = torch.empty(max(N, 1), dtype=torch.float64, device=dev)
    seg = torch.empty((num_classes, 2), dtype=torch.int32, device=dev)
    L.check(L.lib().effdet_voc_ap(L.ptr(rec_key), L.ptr(rec_tp), N, L.ptr(gt_count), int(num_classes), L.ptr(ws),
                                  ws.numel(), L.ptr(out[0]), L.ptr(out[1]), L.ptr(recall), L.ptr(precision), L.ptr(seg),
                                  L.stream_ptr()), 'effdet_voc_ap')
    return out, recall[:N], precision[:N], seg


OP_MAX_THRESHOLDS = L.OP_MAX_THRESHOLDS                # thresholds per effdet_op_curves call
_OP_POINT = ('effdet_op_curves_workspace_bytes', 'effdet_op_curves', 'effdet_confusion_match')


def op_thresholds(thresholds=None):
    """The confidence grid of op_curves as a checked fp32 array: None gives i / 1000 for i = 0..1000; anything else must be 1 to
    OP_MAX_THRESHOLDS finite, strictly ascending values; -0.0 becomes +0.0 (the one threshold whose key differs from `score > t`)."""
    if thresholds is None:
        return (np.arange(1001) / 1000).astype(np.float32)
    t = np.array(thresholds, dtype=np.float32).reshape(-1)
    if not 1 <= t.size <= OP_MAX_THRESHOLDS:
        raise ValueError('thresholds: 1 to %d values, got %d' % (OP_MAX_THRESHOLDS, t.size))
    if not np.all(np.isfinite(t)):
        raise ValueError('thresholds must be finite')
    if not np.all(t[1:] > t[:-1]):
        raise ValueError('thresholds must be strictly ascending')
    t[t == 0] = 0.0
    return t


def op_curves(rec_key, rec_tp, num_records, gt_count, num_classes, thresholds=None, out=None):
    """Precision / recall / F1 against a confidence grid over the first num_records records of voc_match (include/effdet_op_point.h)
    -> dict of device tensors: thresholds [M] fp32, tp / npred [C, M] int32, precision / recall / f1 [C, M] fp64, mean [3, M] fp64,
    best [C + 1, 4] fp64 (j*, P, R, F1; row C: the mean curves').  out: such a dict of the caller's (every element is overwritten)."""
    Lb = L.require(*_OP_POINT)
    dev = gt_count.device
    N, Cn = int(num_records), int(num_classes)
    th = op_thresholds(thresholds)
    M = int(th.size)
    assert gt_count.dtype == torch.int32 and gt_count.is_contiguous() and gt_count.numel() == Cn
    assert N == 0 or (rec_key.dtype == torch.int64 and rec_tp.dtype == torch.uint8 and rec_key.numel() >= N and rec_tp.numel() >= N)
    td = torch.from_numpy(th).to(dev)
    ws = torch.empty(max(int(Lb.effdet_op_curves_workspace_bytes(N)), 1), dtype=torch.uint8, device=dev)
    shapes = {'tp': ((Cn, M), torch.int32), 'npred': ((Cn, M), torch.int32), 'precision': ((Cn, M), torch.float64),
              'recall': ((Cn, M), torch.float64), 'f1': ((Cn, M), torch.float64), 'mean': ((3, M), torch.float64),
              'best': ((Cn + 1, 4), torch.float64)}
    if out is None:
        out = {k: torch.empty(s, dtype=dt, device=dev) for k, (s, dt) in shapes.items()}
    else:
        out = dict(out)
        for k, (s, dt) in shapes.items():
            assert tuple(out[k].shape) == s and out[k].dtype == dt and out[k].is_contiguous() and out[k].device == dev, k
    out['thresholds'] = td
    L.check(Lb.effdet_op_curves(L.ptr(rec_key) if N else None, L.ptr(rec_tp) if N else None, N, L.ptr(gt_count), Cn, L.ptr(td), M,
                                L.ptr(ws), ws.numel(), L.ptr(out['tp']), L.ptr(out['npred']), L.ptr(out['precision']),
                                L.ptr(out['recall']), L.ptr(out['f1']), L.ptr(out['mean']), L.ptr(out['best']), L.stream_ptr()),
            'effdet_op_curves')
    return out


def confusion_match(dets, counts, gt_boxes, gt_labels, num_classes, conf_threshold, iou_threshold, matrix):
    """Confusion counts of one batch (include/effdet_op_point.h): voc_match's dets / counts / gt_boxes / gt_labels; ADDS to matrix
    [num_classes + 1, num_classes + 1] int64 (row = predicted class, column = true class, index num_classes = background)."""
    B, max_det = int(dets.shape[0]), int(dets.shape[1])
    G = int(gt_boxes.shape[1])
    assert dets.dtype == torch.float32 and dets.is_contiguous() and dets.shape[2] == 6
    assert counts.dtype == torch.int32 and counts.is_contiguous() and counts.numel() == B
    assert gt_boxes.dtype == torch.float64 and gt_boxes.is_contiguous() and tuple(gt_boxes.shape) == (B, G, 4)
    assert gt_labels.dtype == torch.int32 and gt_labels.is_contiguous() and tuple(gt_labels.shape) == (B, G)
    assert matrix.dtype == torch.int64 and matrix.is_contiguous() and tuple(matrix.shape) == (num_classes + 1, num_classes + 1)
    L.check(L.require(*_OP_POINT).effdet_confusion_match(L.ptr(dets), L.ptr(counts), L.ptr(gt_boxes), L.ptr(gt_labels), B, max_det, G,
                                                         int(num_classes), float(conf_threshold), float(iou_threshold), L.ptr(matrix),
                                                         L.stream_ptr()), 'effdet_confusion_match')


TRACK_MAX_TRACKS, TRACK_MAX_DET, TRACK_ROW_WORDS = L.TRACK_MAX_TRACKS, L.TRACK_MAX_DET, L.TRACK_ROW_WORDS
_TRACK = ('effdet_track_state_bytes', 'effdet_track_reset', 'effdet_track_step', 'effdet_track_overflow')
ASSIGN_MAX_ROWS, ASSIGN_MAX_COLS = L.ASSIGN_MAX_ROWS, L.ASSIGN_MAX_COLS


class TrackOptions(_Options):
    """ByteTrack's settings for track_step (include/effdet_track.h): detections scoring >= track_thr are high, those in (low_thr,
    track_thr) low; the three associations allow a pair whose similarity is > match_sim (tracked + lost x high), > second_sim (the
    tracked left x low, plain IoU) and > unconfirmed_sim (unconfirmed x the high left); a high detection left over starts a track when
    its score is >= new_thr (None: track_thr + 0.1); a lost track is dropped after track_buffer frames without a match; fuse_score
    multiplies the IoU by the detection's score; class_aware also wants equal labels; max_tracks slots per stream.  assignment:
    'greedy' (the default: each association greedy by descending similarity) or 'optimal' (each association solved as the published
    tracker does, a maximum-weight matching over the allowed pairs; include/effdet_assign.h)."""

    def __init__(self, track_thr=0.5, low_thr=0.1, new_thr=None, match_sim=0.2, second_sim=0.5, unconfirmed_sim=0.3, track_buffer=30,
                 fuse_score=True, class_aware=False, max_tracks=128, assignment='greedy'):
        if assignment not in L.ASSIGNMENTS:
            raise ValueError('TrackOptions: assignment must be one of %s, got %r' % (', '.join(map(repr, L.ASSIGNMENTS)), assignment))
        self.assignment = assignment
        new_thr = float(np.float32(np.float32(track_thr) + np.float32(0.1))) if new_thr is None else new_thr
        for name, v in (('track_thr', track_thr), ('low_thr', low_thr), ('new_thr', new_thr)):
            if not abs(float(v)) < float('inf'):
                raise ValueError('TrackOptions: %s must be finite, got %r' % (name, v))
        if float(low_thr) > float(track_thr):
            raise ValueError('TrackOptions: low_thr must not exceed track_thr')
        for name, v in (('match_sim', match_sim), ('second_sim', second_sim), ('unconfirmed_sim', unconfirmed_sim)):
            if not 0.0 <= float(v) <= 1.0:
                raise ValueError('TrackOptions: %s must be in [0, 1], got %r' % (name, v))
        if not 0 <= float(track_buffer) < 2 ** 31 or int(track_buffer) != track_buffer:       # (the range first: int() of inf or NaN raises)
            raise ValueError('TrackOptions: track_buffer must be a whole number of frames >= 0')
        if not 1 <= float(max_tracks) <= TRACK_MAX_TRACKS or int(max_tracks) != max_tracks:
            raise ValueError('TrackOptions: max_tracks must be in 1..%d' % TRACK_MAX_TRACKS)
        self.track_thr, self.low_thr, self.new_thr = float(track_thr), float(low_thr), float(new_thr)
        self.match_sim, self.second_sim, self.unconfirmed_sim = float(match_sim), float(second_sim), float(unconfirmed_sim)
        self.track_buffer, self.fuse_score, self.class_aware, self.max_tracks = int(track_buffer), bool(fuse_score), bool(class_aware), int(max_tracks)

    def key(self):
        k = (self.track_thr, self.low_thr, self.new_thr, self.match_sim, self.second_sim, self.unconfirmed_sim, self.track_buffer,
             self.fuse_score, self.class_aware, self.max_tracks)
        return k if self.assignment == 'greedy' else k + (self.assignment,)            # (the default keeps the ten-tuple it always had)

    def __repr__(self):
        return ('TrackOptions(track_thr=%r, low_thr=%r, new_thr=%r, match_sim=%r, second_sim=%r, unconfirmed_sim=%r, track_buffer=%d, '
                'fuse_score=%r, class_aware=%r, max_tracks=%d' % self.key()[:10]
                + ('' if self.assignment == 'greedy' else ', assignment=%r' % self.assignment) + ')')


class TrackState:
    """The device state of B trackers of max_tracks slots (opaque bytes; include/effdet_track.h gives the layout)."""

    def __init__(self, buf, B, max_tracks):
        self.buf, self.B, self.max_tracks = buf, int(B), int(max_tracks)


def track_state(B, max_tracks, device, buf=None):
    """-> a TrackState of B streams, already reset.  buf: the caller's uint8 tensor of exactly the state's size (tests put guards
    around it)."""
    B, T = int(B), int(max_tracks)
    if B < 1 or not 1 <= T <= TRACK_MAX_TRACKS:
        raise ValueError('track_state: B >= 1 and max_tracks in 1..%d, got %d, %d' % (TRACK_MAX_TRACKS, B, T))
    n = int(L.require(*_TRACK).effdet_track_state_bytes(B, T))
    if buf is None:
        buf = torch.empty(n, dtype=torch.uint8, device=device)
    assert buf.dtype == torch.uint8 and buf.is_contiguous() and buf.numel() == n and buf.data_ptr() % 4 == 0
    state = TrackState(buf, B, T)
    track_reset(state)
    return state


def track_reset(state, mask=None):
    """Resets the streams whose entry of mask (a sequence or tensor of B flags) is set; every stream for None."""
    if mask is not None:
        mask = torch.as_tensor(mask, device=state.buf.device).reshape(-1).ne(0).to(torch.int32).contiguous()
        if mask.numel() != state.B:
            raise ValueError('track_reset: %d flags for %d streams' % (mask.numel(), state.B))
    L.check(L.require(*_TRACK).effdet_track_reset(L.ptr(state.buf), state.B, state.max_tracks, L.ptr(mask), L.stream_ptr()), 'effdet_track_reset')


def track_overflow(state):
    """-> [B] int32 on the device: the new tracks each stream has dropped for lack of a free slot since its last reset."""
    out = torch.empty(state.B, dtype=torch.int32, device=state.buf.device)
    L.check(L.require(*_TRACK).effdet_track_overflow(L.ptr(state.buf), state.B, state.max_tracks, L.ptr(out), L.stream_ptr()), 'effdet_track_overflow')
    return out


def track_step(dets, counts, state, options=None, out=None):
    """One frame of every stream (include/effdet_track.h): dets [B, max_det, 6] fp32 + counts [B] int32 as finalize_dets writes them ->
    (rows [B, max_tracks, 8] fp32: x1, y1, x2, y2, score, label, tracklet_len, frames_since_start; ids [B, max_tracks] int32; count [B]
    int32), the activated tracks of each stream in ascending id, rows past the count zero with id -1.  Everything stays on the device and
    nothing is read back, so the call can be captured in a graph.  out: such a triple of the caller's (every element is overwritten).
    options.assignment 'greedy' goes through effdet_track_step, 'optimal' through effdet_track_step_assign (include/effdet_assign.h)."""
    o = TrackOptions() if options is None else options
    if not isinstance(o, TrackOptions):
        raise TypeError('track_step: options must be a TrackOptions, not %r' % (o,))
    if not isinstance(state, TrackState):
        raise TypeError('track_step: state must come from track_state, not %r' % (state,))
    B, T = state.B, state.max_tracks
    if o.max_tracks != T:
        raise ValueError('track_step: the state has %d slots per stream, options.max_tracks is %d' % (T, o.max_tracks))
    if dets.dim() != 3 or dets.shape[0] != B or dets.shape[2] != 6:
        raise ValueError('track_step: dets must be [%d, max_det, 6], got %s' % (B, tuple(dets.shape)))
    max_det = int(dets.shape[1])
    if not 1 <= max_det <= TRACK_MAX_DET:
        raise ValueError('track_step: 1..%d detection rows per stream, got %d' % (TRACK_MAX_DET, max_det))
    assert dets.dtype == torch.float32 and dets.is_contiguous() and dets.device == state.buf.device
    assert counts.dtype == torch.int32 and counts.is_contiguous() and counts.numel() == B and counts.device == dets.device
    if out is None:
        out = (torch.empty((B, T, 8), dtype=torch.float32, device=dets.device), torch.empty((B, T), dtype=torch.int32, device=dets.device),
               torch.empty(B, dtype=torch.int32, device=dets.device))
    rows, ids, count = out
    assert rows.dtype == torch.float32 and rows.is_contiguous() and tuple(rows.shape) == (B, T, 8)
    assert ids.dtype == torch.int32 and ids.is_contiguous() and tuple(ids.shape) == (B, T)
    assert count.dtype == torch.int32 and count.is_contiguous() and count.numel() == B
    args = (L.ptr(dets), L.ptr(counts), B, max_det, L.ptr(state.buf), T, o.track_thr, o.low_thr, o.new_thr, o.match_sim, o.second_sim,
            o.unconfirmed_sim, o.track_buffer, int(o.fuse_score), int(o.class_aware), L.ptr(rows), L.ptr(ids), L.ptr(count))
    if o.assignment == 'greedy':
        L.check(L.require(*_TRACK).effdet_track_step(*args, L.stream_ptr()), 'effdet_track_step')
    else:
        L.check(L.require('effdet_track_step_assign').effdet_track_step_assign(*args, L.ASSIGNMENTS.index(o.assignment), L.stream_ptr()),
                'effdet_track_step_assign')
    return rows, ids, count


def linear_assignment(sim, gate=0.0, n_rows=None, n_cols=None, out=None):
    """Optimal assignment of B problems (include/effdet_assign.h): sim [B, R, C] fp32 (a 2-D sim is a batch of one), R <= 256 rows and
    C <= 128 columns.  A pair is allowed when sim > gate; the answer is the matching over allowed pairs with the largest sum of
    similarity above the gate (on a 2^-20 grid), nothing forced to be matched -- lap.lapjv(1 - sim, extend_cost=True, cost_limit=1 - gate).
    n_rows / n_cols: [B] int32 tensors, the rows / columns of each problem that take part (None: all).  -> (row_to_col [B, R] int32,
    col_to_row [B, C] int32, -1 = unmatched; total [B] int64, the sum of the integer weights); without the batch dimension for a 2-D
    sim.  Everything stays on the device and nothing is read back, so the call can be captured in a graph.  out: such a triple of
    the caller's (every element is overwritten)."""
    if sim.dim() not in (2, 3):
        raise ValueError('linear_assignment: sim must be [R, C] or [B, R, C], got %s' % (tuple(sim.shape),))
    batched = sim.dim() == 3
    B, R, C = (int(v) for v in (sim.shape if batched else (1,) + tuple(sim.shape)))
    if B < 1 or not 1 <= R <= ASSIGN_MAX_ROWS or not 1 <= C <= ASSIGN_MAX_COLS:
        raise ValueError('linear_assignment: B >= 1, 1..%d rows and 1..%d columns, got %d, %d, %d' % (ASSIGN_MAX_ROWS, ASSIGN_MAX_COLS, B, R, C))
    gate = float(gate)
    if not abs(gate) < float('inf'):
        raise ValueError('linear_assignment: gate must be finite, got %r' % (gate,))
    assert sim.dtype == torch.float32 and sim.is_contiguous()
    for name, n in (('n_rows', n_rows), ('n_cols', n_cols)):
        if n is not None:
            assert n.dtype == torch.int32 and n.is_contiguous() and n.numel() == B and n.device == sim.device, name
    if out is None:
        out = (torch.empty((B, R) if batched else (R,), dtype=torch.int32, device=sim.device),
               torch.empty((B, C) if batched else (C,), dtype=torch.int32, device=sim.device),
               torch.empty((B,) if batched else (), dtype=torch.int64, device=sim.device))
    r2c, c2r, total = out
    assert r2c.dtype == torch.int32 and r2c.is_contiguous() and r2c.numel() == B * R and r2c.device == sim.device
    assert c2r.dtype == torch.int32 and c2r.is_contiguous() and c2r.numel() == B * C and c2r.device == sim.device
    assert total.dtype == torch.int64 and total.is_contiguous() and total.numel() == B and total.device == sim.device
    L.check(L.require('effdet_assign').effdet_assign(L.ptr(sim), B, R, C, L.ptr(n_rows), L.ptr(n_cols), gate, L.ptr(r2c), L.ptr(c2r),
                                                     L.ptr(total), L.stream_ptr()), 'effdet_assign')
    return r2c, c2r, total


COCO_MAX_GT = 2048                 # GT rows per image effdet_coco_match stages in LDS
COCO_MAX_CATEGORIES = 1024
_COCO = ('effdet_coco_slots', 'effdet_coco_match', 'effdet_coco_accumulate', 'effdet_coco_accumulate_workspace_bytes')


def coco_slots(max_det, num_categories, max_dets_last=100):
    """Records effdet_coco_match writes per image: min(max_det, max_dets_last * num_categories)."""
    return int(L.require(*_COCO).effdet_coco_slots(int(max_det), int(num_categories), int(max_dets_last)))


def coco_match(dets, counts, image_ids, gt, num_categories, iou_thrs, area_rng, max_dets_last, rec, npig):
    """COCO matching of one batch: dets [B,max_det,6] fp32 (x, y, w, h, score, category index) + counts [B] int32, image_ids [B] int32,
    gt [B,G,7] fp64 (x, y, w, h, category index (-1 = pad), iscrowd, area); iou_thrs [T] / area_rng [A,2] fp64 numpy arrays.
    rec: (key int64, image int32, rank uint8, match int64, ignore int64) views of at least B * coco_slots(...) records each;
    adds to npig [num_categories, A] int32."""
    Lb = L.require(*_COCO)
    B, max_det = int(dets.shape[0]), int(dets.shape[1])
    G = int(gt.shape[1])
    it = np.ascontiguousarray(iou_thrs, dtype=np.float64)
    ar = np.ascontiguousarray(area_rng, dtype=np.float64).reshape(-1, 2)
    S = coco_slots(max_det, num_categories, max_dets_last)
    assert dets.dtype == torch.float32 and dets.is_contiguous() and dets.shape[2] == 6
    assert counts.dtype == torch.int32 and counts.is_contiguous() and counts.numel() == B
    assert image_ids.dtype == torch.int32 and image_ids.is_contiguous() and image_ids.numel() == B
    assert gt.dtype == torch.float64 and gt.is_contiguous() and tuple(gt.shape) == (B, G, 7)
    key, img, rank, match, ignore = rec
    assert key.dtype == torch.int64 and img.dtype == torch.int32 and rank.dtype == torch.uint8
    assert match.dtype == torch.int64 and ignore.dtype == torch.int64
    assert min(t.numel() for t in rec) >= B * S and all(t.is_contiguous() for t in rec)
    assert npig.dtype == torch.int32 and npig.is_contiguous() and npig.numel() == num_categories * len(ar)
    L.check(Lb.effdet_coco_match(L.ptr(dets), L.ptr(counts), L.ptr(image_ids), L.ptr(gt), B, max_det, G, int(num_categories),
                                 it.ctypes.data, len(it), ar.ctypes.data, len(ar),
                                 int(max_dets_last), L.ptr(key), L.ptr(img), L.ptr(rank), L.ptr(match), L.ptr(ignore), L.ptr(npig),
                                 L.stream_ptr()), 'effdet_coco_match')
    return B * S


def coco_accumulate(rec, num_records, max_image_id, npig, num_categories, iou_thrs, rec_thrs, num_areas, max_dets):
    """accumulate + summarize over the first num_records records -> (precision [T,R,K,A,M] fp64, recall [T,K,A,M] fp64, stats [12]
    fp64), all on the device."""
    Lb = L.require(*_COCO)
    dev = npig.device
    N, K = int(num_records), int(num_categories)
    it = np.ascontiguousarray(iou_thrs, dtype=np.float64)
    rt = np.ascontiguousarray(rec_thrs, dtype=np.float64)
    md = np.ascontiguousarray(max_dets, dtype=np.int32)
    T, R, A, M = len(it), len(rt), int(num_areas), len(md)
    ws = torch.empty(int(Lb.effdet_coco_accumulate_workspace_bytes(N, K)), dtype=torch.uint8, device=dev)
    precision = torch.empty((T, R, K, A, M), dtype=torch.float64, device=dev)
    recall = torch.empty((T, K, A, M), dtype=torch.float64, device=dev)
    stats = torch.empty(12, dtype=torch.float64, device=dev)
    key, img, rank, match, ignore = rec
    L.check(Lb.effdet_coco_accumulate(L.ptr(key), L.ptr(img), L.ptr(rank), L.ptr(match), L.ptr(ignore), N,
                                      int(max_image_id), L.ptr(npig), K, it.ctypes.data, T,
                                      rt.ctypes.data, R, A, md.ctypes.data, M,
                                      L.ptr(ws), ws.numel(), L.ptr(precision), L.ptr(recall), L.ptr(stats),
                                      L.stream_ptr()), 'effdet_coco_accumulate')
    return precision, recall, stats


def head_out_bwd(dprob, prob, dreg, dtype):
    """(d loss / d probability, probability, d loss / d regression) fp32 -> (dlogit, dreg) in the compute dtype."""
    dl = torch.empty(prob.shape, dtype=dtype, device=prob.device)
    dr = torch.empty(dreg.shape, dtype=dtype, device=prob.device)
    L.check(L.lib().effdet_head_out_bwd(L.ptr(dprob), L.ptr(prob), L.ptr(dreg), L.ptr(dl), L.ptr(dr), L.dtype_code(dtype),
                                        prob.numel(), dreg.numel(), L.stream_ptr()), 'effdet_head_out_bwd')
    return dl, dr


def tuning_set(key, value):
    """Kernel-selection knob of the library (speed only; see effdet_tuning_set in include/effdet_hip.h) -> previous value."""
    return int(L.lib().effdet_tuning_set(int(key), int(value)))


_AUG = ('effdet_augment_train', 'effdet_augment_resize', 'effdet_augment_boxes')
AUG_P = 23                         # EFFDET_AUG_P: columns of the per-image augmentation table


def _norm_consts(mean, std):
    """albumentations' Normalize constants: mean * 255 and 1 / (std * 255), each step in fp32."""
    m = np.asarray(mean, dtype=np.float32) * np.float32(255.0)
    inv = np.reciprocal(np.asarray(std, dtype=np.float32) * np.float32(255.0), dtype=np.float32)
    return (C.c_float * 3)(*[float(v) for v in m]), (C.c_float * 3)(*[float(v) for v in inv])


def augment_train(src_u8, src_off, src_hw, table, S, dtype, cpad, mean, std, stages=None):
    """'train' chain of get_augumentation: uint8 HWC images (concatenated, device) + table [B, AUG_P] fp32 (device) ->
    Map [B,S,S,cpad].  stages: optional dict that receives the uint8 intermediates 'a' (LongestMaxSize + pad) and 'b'
    (crop / flips / transpose / colour, 4th byte = CLAHE's L) as [B,S,S,4] tensors and the CLAHE LUTs 'lut' [B,64,256]."""
    B = int(src_hw.shape[0])
    dev = src_u8.device
    assert table.dtype == torch.float32 and table.is_contiguous() and tuple(table.shape) == (B, AUG_P)
    out = Map.new(B, S, S, cpad, dtype, dev)
    sa = torch.empty((B, S, S, 4), dtype=torch.uint8, device=dev)
    sb = torch.empty((B, S, S, 4), dtype=torch.uint8, device=dev)
    lut = torch.empty((B, 64, 256), dtype=torch.uint8, device=dev)
    m, inv = _norm_consts(mean, std)
    L.check(L.require(*_AUG).effdet_augment_train(L.ptr(src_u8), L.ptr(src_off), L.ptr(src_hw), L.ptr(table), B, int(S), L.ptr(sa),
                                                  L.ptr(sb), L.ptr(lut), L.ptr(out.t), L.dtype_code(dtype), cpad, m, inv,
                                                  L.stream_ptr()), 'effdet_augment_train')
    if stages is not None:
        stages.update(a=sa, b=sb, lut=lut)
    return out


def augment_resize(src_u8, src_off, src_hw, H, W, dtype, cpad, mean, std, stages=None):
    """'valid' / 'test' chain: Resize(H, W) + Normalize -> Map [B,H,W,cpad]; stages['a'] = the resized uint8 [B,H,W,4] if asked."""
    B = int(src_hw.shape[0])
    dev = src_u8.device
    out = Map.new(B, H, W, cpad, dtype, dev)
    sa = torch.empty((B, H, W, 4), dtype=torch.uint8, device=dev) if stages is not None else None
    m, inv = _norm_consts(mean, std)
    L.check(L.require(*_AUG).effdet_augment_resize(L.ptr(src_u8), L.ptr(src_off), L.ptr(src_hw), B, int(H), int(W), L.ptr(sa),
                                                   L.ptr(out.t), L.dtype_code(dtype), cpad, m, inv, L.stream_ptr()),
            'effdet_augment_resize')
    if stages is not None:
        stages.update(a=sa)
    return out


def augment_boxes(src_hw, table, H, W, annots, min_area=0.0, min_visibility=0.0):
    """Boxes [B,M,5] fp32 (label -1 = padding) through the chain's geometry (table None: the stretch resize to H x W), clipped and
    filtered -> (annots_out [B,M,5] with the kept rows first and -1 after, counts [B] int32)."""
    B, M = int(annots.shape[0]), int(annots.shape[1])
    assert annots.dtype == torch.float32 and annots.is_contiguous() and annots.shape[2] == 5
    out = torch.empty_like(annots)
    counts = torch.empty(B, dtype=torch.int32, device=annots.device)
    L.check(L.require(*_AUG).effdet_augment_boxes(L.ptr(src_hw), L.ptr(table), B, int(H), int(W), L.ptr(annots), M,
                                                  float(min_area), float(min_visibility), L.ptr(out), L.ptr(counts),
                                                  L.stream_ptr()), 'effdet_augment_boxes')
    return out, counts


# ----------------------------------------------------------------------------- Mosaic / MixUp (csrc/mosaic.hip)
_MOSAIC = ('effdet_mosaic_compose', 'effdet_mosaic_boxes')
MOSAIC_P = 14                      # EFFDET_MOSAIC_P: columns of the per-image mosaic table (include/effdet_mosaic.h)


def mosaic_compose(src_u8, src_off, src_hw, table, S, fill=114):
    """Mosaic / MixUp of a batch (include/effdet_mosaic.h): uint8 HWC images (concatenated, device) + table [B, MOSAIC_P] fp32
    (device) -> uint8 [B,S,S,3], the input of augment_train with src_off = b * S*S*3 and src_hw = (S, S)."""
    B = int(src_hw.shape[0])
    assert table.dtype == torch.float32 and table.is_contiguous() and tuple(table.shape) == (B, MOSAIC_P)
    out = torch.empty((B, int(S), int(S), 3), dtype=torch.uint8, device=src_u8.device)
    L.check(L.require(*_MOSAIC).effdet_mosaic_compose(L.ptr(src_u8), L.ptr(src_off), L.ptr(src_hw), L.ptr(table), B, int(S), int(fill),
                                                      L.ptr(out), L.stream_ptr()), 'effdet_mosaic_compose')
    return out


def mosaic_boxes(src_hw, table, S, annots, min_area=0.0, min_visibility=0.0):
    """Boxes [B,M,5] fp32 of the SOURCE images (label -1 = padding) through the mosaic geometry of `table`, clipped to their windows
    and filtered -> (out [B,5M,5]: per image the kept rows of TL, TR, BL, BR and the partner, -1 rows after; counts [B] int32)."""
    B, M = int(annots.shape[0]), int(annots.shape[1])
    assert annots.dtype == torch.float32 and annots.is_contiguous() and annots.shape[2] == 5
    assert table.dtype == torch.float32 and table.is_contiguous() and tuple(table.shape) == (B, MOSAIC_P)
    out = torch.empty((B, 5 * M, 5), dtype=torch.float32, device=annots.device)
    counts = torch.empty(B, dtype=torch.int32, device=annots.device)
    L.check(L.require(*_MOSAIC).effdet_mosaic_boxes(L.ptr(src_hw), L.ptr(table), B, int(S), L.ptr(annots), M, float(min_area),
                                                    float(min_visibility), L.ptr(out), 5 * M, L.ptr(counts), L.stream_ptr()),
            'effdet_mosaic_boxes')
    return out, counts


# ----------------------------------------------------------------------------- affine / perspective warp (csrc/affine.hip)
_AFFINE = ('effdet_affine_warp', 'effdet_affine_boxes')
AFFINE_P = 20                      # EFFDET_AFFINE_P: columns of the per-image warp table (include/effdet_affine.h)


def affine_warp(src_u8, src_off, src_hw, table, S, fill=114):
    """The warp of a batch (include/effdet_affine.h): uint8 HWC images (concatenated, device) + table [B, AFFINE_P] fp64 (device) ->
    uint8 [B,S,S,3], the input of augment_train with src_off = b * S*S*3 and src_hw = (S, S)."""
    B = int(src_hw.shape[0])
    assert table.dtype == torch.float64 and table.is_contiguous() and tuple(table.shape) == (B, AFFINE_P)
    out = torch.empty((B, int(S), int(S), 3), dtype=torch.uint8, device=src_u8.device)
    L.check(L.require(*_AFFINE).effdet_affine_warp(L.ptr(src_u8), L.ptr(src_off), L.ptr(src_hw), L.ptr(table), B, int(S), int(fill),
                                                   L.ptr(out), L.stream_ptr()), 'effdet_affine_warp')
    return out


def affine_boxes(src_hw, table, S, annots, wh_thr=2.0, ar_thr=100.0, area_thr=0.1):
    """Boxes [B,M,5] fp32 of the source images (label -1 = padding) through the forward matrices of `table`, clipped to the output
    and filtered by box_candidates' rule -> (out [B,M,5] with the kept rows first in input order and -1 after, counts [B] int32)."""
    B, M = int(annots.shape[0]), int(annots.shape[1])
    assert annots.dtype == torch.float32 and annots.is_contiguous() and annots.shape[2] == 5
    assert table.dtype == torch.float64 and table.is_contiguous() and tuple(table.shape) == (B, AFFINE_P)
    out = torch.empty_like(annots)
    counts = torch.empty(B, dtype=torch.int32, device=annots.device)
    L.check(L.require(*_AFFINE).effdet_affine_boxes(L.ptr(src_hw), L.ptr(table), B, int(S), L.ptr(annots), M, float(wh_thr),
                                                    float(ar_thr), float(area_thr), L.ptr(out), L.ptr(counts), L.stream_ptr()),
            'effdet_affine_boxes')
    return out, counts


# ----------------------------------------------------------------------------- JPEG decode (csrc/jpeg.hip)
_JPEG = ('effdet_jpeg_probe', 'effdet_jpeg_entropy_batch', 'effdet_jpeg_reconstruct')
JPEG_GREY, JPEG_444, JPEG_422, JPEG_420 = 0, 1, 2, 3
JPEG_REASONS = {1: 'progressive frame', 2: 'extended, lossless or arithmetic-coded frame', 3: 'sample precision other than 8 bits',
                4: '16-bit quantisation table', 5: 'component count other than 1 or 3', 6: 'sampling other than 4:4:4, 4:2:2 or 4:2:0',
                7: 'more than one scan', 8: 'three components that are not YCbCr'}
JPEG_DESC_BYTES = C.sizeof(L.JpegDesc)


def _as_u8(stream):
    return np.frombuffer(stream, dtype=np.uint8)


def jpeg_probe(stream):
    """Host only.  bytes -> (status, JpegInfo): 0, or _lib's EFFDET_EUNSUPPORTED (-3, info.reason says why) / EFFDET_EINVAL (-1)."""
    a = _as_u8(stream)
    info = L.JpegInfo()
    st = L.require(*_JPEG).effdet_jpeg_probe(a.ctypes.data, a.size, C.byref(info))
    return int(st), info


def jpeg_entropy_batch(streams, coef_out, coef_off, desc_out, threads=8):
    """Host only.  Huffman-decode the streams (list of bytes) into coef_out (uint8 numpy view of the caller's staging buffer; image
    b at byte coef_off[b], a multiple of 16) and desc_out (uint8 numpy view, len(streams) * JPEG_DESC_BYTES) on `threads` workers
    -> (status of the first image that failed or 0, (launch-1 workgroups, launch-2 workgroups)).  Per-image statuses are in the
    descriptors (jpeg_descs)."""
    B = len(streams)
    arrs = [_as_u8(s) for s in streams]
    ptrs = (C.c_void_p * B)(*[a.ctypes.data for a in arrs])
    lens = (C.c_longlong * B)(*[a.size for a in arrs])
    offs = (C.c_longlong * B)(*[int(o) for o in coef_off])
    assert coef_out.dtype == np.uint8 and coef_out.flags['C_CONTIGUOUS'] and coef_out.flags['WRITEABLE']
    assert desc_out.dtype == np.uint8 and desc_out.flags['C_CONTIGUOUS'] and desc_out.size >= B * JPEG_DESC_BYTES
    totals = (C.c_int * 2)()
    st = L.require(*_JPEG).effdet_jpeg_entropy_batch(ptrs, lens, B, coef_out.ctypes.data, coef_out.size, offs,
                                                     desc_out.ctypes.data, int(threads), totals)
    return int(st), (int(totals[0]), int(totals[1]))


def jpeg_descs(desc_out, B):
    """The B descriptor records of a jpeg_entropy_batch buffer as a ctypes array (a view, not a copy)."""
    return (L.JpegDesc * B).from_buffer(desc_out)


def jpeg_reconstruct(coef, desc, B, wgs, planes, planes_off, dst, dst_off):
    """Device: the two launches of effdet_jpeg_reconstruct on torch's current stream.  coef / desc: the staged coefficient bytes and
    descriptor records on the device (uint8 tensors, 16-byte aligned); wgs: the workgroup totals jpeg_entropy_batch returned;
    planes: uint8 workspace, image b's component planes at byte planes_off[b]; dst: uint8, image b's RGB HWC pixels at dst_off[b]
    (both int64 device tensors, multiples of 16)."""
    for t in (coef, desc, planes, dst):
        assert t.dtype == torch.uint8 and t.is_contiguous() and t.is_cuda
    assert planes_off.dtype == torch.int64 and dst_off.dtype == torch.int64 and planes_off.numel() >= B and dst_off.numel() >= B
    assert desc.numel() >= B * JPEG_DESC_BYTES
    L.check(L.require(*_JPEG).effdet_jpeg_reconstruct(L.ptr(coef), L.ptr(desc), int(B), int(wgs[0]), int(wgs[1]), L.ptr(planes),
                                                      L.ptr(planes_off), L.ptr(dst), L.ptr(dst_off), L.stream_ptr()),
            'effdet_jpeg_reconstruct')


# The device renderer lives in draw.py (it builds on _Options above); its names are reachable here as ops.draw_detections,
# ops.DrawOptions, ... but are not bound in this module: ops' own options classes stay the set that the wrapper tests enumerate.
_DRAW_NAMES = ('DrawOptions', 'DrawNames', 'draw_names', 'draw_palette', 'draw_palette_host', 'draw_detections', 'DRAW_MAX_ROWS',
               'DRAW_NAME_MAX', 'DRAW_MAX_THICKNESS', 'DRAW_MAX_TEXT_SCALE', 'DRAW_TILE_W', 'DRAW_TILE_H', 'DRAW_COLOR_BY')


def __getattr__(name):
    if name in _DRAW_NAMES:
        from . import draw
        return getattr(draw, name)
    raise AttributeError('module %r has no attribute %r' % (__name__, name))
