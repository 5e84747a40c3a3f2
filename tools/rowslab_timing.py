"""Per-launch timing of the row-slab activation staging (csrc/conv_igemm.hip, tuning knob TUNE_ROWSLAB) at the benchmark's shapes (D0,
B = 32 @512): the head's split-layout 3x3 launches -- the four paired tower layers, retina_cls and retina_reg (f16x3 forward), their data
gradients and the paired tower data gradients (bf16x3, ReLU mask) and the 256 -> 64 gradient back to the neck -- each dense and, where the
step passes flags, with the flags of the benchmark's batch (needed tiles forward, live tiles backward: the regression tower's half of a
paired launch), with the knob off (one tile per tap) and on (one slab per kernel row), alternating off / on / off / on.  15 warm-up + 50
timed launches per figure, device events.  One JSON document on stdout.

    python tools/rowslab_timing.py > profiles/rowslab_launch_timing.json"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from efficientdet.pytorch_amd import ops, functional as Fn, _lib as L          # noqa: E402
from efficientdet.pytorch_amd.synthetic import synthetic_batch                 # noqa: E402

B, S, WC = 32, 512, 64
SIZES = [(S >> (3 + i), S >> (3 + i)) for i in range(5)]
K3 = dict(KH=3, KW=3, pad_t=1, pad_l=1)


def timed(fn, warm=15, reps=50):
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return round(a.elapsed_time(b) * 1000.0 / reps, 1)


def ab(fn):
    """-> {'per_tap_us': [two windows], 'slab_us': [two windows]}, the knob alternating"""
    row = {'per_tap_us': [], 'slab_us': []}
    old = ops.tuning_set(L.TUNE_ROWSLAB, 0)
    try:
        for _ in range(2):
            for sw, key in ((0, 'per_tap_us'), (1, 'slab_us')):
                ops.tuning_set(L.TUNE_ROWSLAB, sw)
                row[key].append(timed(fn))
    finally:
        ops.tuning_set(L.TUNE_ROWSLAB, old)
    return row


def fill(maps, C, gen, h, relu=False, keep=None):
    """random values into the maps, in the H-split (h) or the split layout; keep (per level a [B, H, W] bool map): exact zeros outside it"""
    for l, m in enumerate(maps):
        src = torch.randn(m.B, m.H, m.W, C, generator=gen, device='cuda')
        if relu:
            src = torch.relu(src)
        if keep is not None:
            src = src * keep[l % len(SIZES)].unsqueeze(-1)
        ops.to_split2(src, None if h else m.addr(), m.addr() if h else None, src.numel(), None)
    return maps


def pair(C, gen, h, relu=False, keep_b=None):
    _, a, b = Fn.pyramid_alloc_pair(B, SIZES, C, torch.float32, 'cuda')
    fill(a, C, gen, h, relu); fill(b, C, gen, h, relu, keep_b)
    return a, b


def main():
    gen = torch.Generator(device='cuda').manual_seed(0)
    ann = synthetic_batch(B, S, seed=1, num_classes=80)[1].cuda().float().contiguous()      # the benchmark's batch (rank 0)
    anc = ops.anchors(S, S, 'cuda')
    A = anc.shape[1]
    need = ops.needed_tiles(anc, ann, B, SIZES)
    cls = torch.rand(B, A, 80, generator=gen, device='cuda').clamp(1e-3, 1 - 1e-3)
    reg = torch.randn(B, A, 4, generator=gen, device='cuda') * 0.3
    _, lws = ops.focal_loss_fwd(cls, reg, anc, ann)
    dreg = ops.focal_loss_bwd_reg(reg, anc, ann, torch.ones(B, device='cuda'), lws, torch.float32, reg_ld=64, split=True)
    _, live = ops.live_tiles(dreg, B, SIZES, 64, True)
    ntile = need.shape[1]
    out = {'needed128_fraction': [round(float(need[r].float().mean()), 4) for r in range(need.shape[0])],
           'live128_fraction': [round(float(live[r].float().mean()), 4) for r in range(live.shape[0])]}
    poff, nz = 0, []                 # d(reg) != 0 as [B, H, W] maps: the regression tower's gradients are zero outside their dilation
    for (h, w) in SIZES:
        rows = dreg.view(torch.int32)[:, poff:poff + h * w]
        nz.append(((rows & 0x7fff7fff) != 0).any(dim=2).view(B, h, w)); poff += h * w

    def dilated(r):
        return [torch.nn.functional.max_pool2d(m.float().unsqueeze(1), 2 * r + 1, 1, r).squeeze(1) > 0 for m in nz]

    def rnd_w(co, ci):
        return torch.randn(co, ci, 3, 3, generator=gen, device='cuda') / (9 * ci) ** 0.5

    # ---- f16x3 forward ----
    for t in range(4):
        cin = WC if t == 0 else 256
        xa, xb = pair(cin, gen, True, relu=True)
        ws = [ops.pack_weight(rnd_w(256, cin), torch.float32, h3=True) for _ in range(2)]
        bs = [torch.randn(256, generator=gen, device='cuda') * 0.1 for _ in range(2)]
        _, ya, yb = Fn.pyramid_alloc_pair(B, SIZES, 256, torch.float32, 'cuda')
        _, sa, sb = Fn.pyramid_alloc_pair(B, SIZES, 256, torch.float32, 'cuda')

        def launch(flags, tile0, xa=xa, xb=xb, ws=ws, bs=bs, ya=ya, yb=yb, sa=sa, sb=sb, cin=cin):
            ops.conv2d(xa + xb, ws[0], ya + yb, Cin=cin, Cout=256, **K3, shift=bs[0], act=ops.ACT_RELU, hsplit=True, ysplit=sa + sb,
                       seg_w=[ws[0]] * 5 + [ws[1]] * 5, seg_shift=[bs[0]] * 5 + [bs[1]] * 5, needed=flags, needed_tile0=tile0)
        r = 4 - t
        out['fwd paired tower layer %d (%d -> 256) r=%d' % (t, cin, r)] = {'dense': ab(lambda: launch(None, 0)),
                                                                            'flagged': ab(lambda: launch(need[r], ntile))}
        del xa, xb, ya, yb, sa, sb
    _, xa = Fn.pyramid_alloc(B, SIZES, 256, torch.float32, 'cuda')
    fill(xa, 256, gen, True, relu=True)
    for name, per, r in (('retina_cls (256 -> 720)', 80, None), ('retina_reg (256 -> 36)', 4, 0)):
        w = ops.pack_weight(rnd_w(9 * per, 256), torch.float32, h3=True)
        bias = torch.randn(9 * per, generator=gen, device='cuda') * 0.1
        buf = torch.empty(B, A, per, device='cuda')

        def final(flags, w=w, bias=bias, buf=buf, per=per):
            ops.conv2d(xa, w, Fn.head_out_maps(buf, B, SIZES, per), Cin=256, Cout=9 * per, **K3, shift=bias, out_f32=True, hsplit=True,
                       act=ops.ACT_SIGMOID if per == 80 else ops.ACT_NONE, needed=flags, needed_tile0=0)
        row = {'dense': ab(lambda: final(None))}
        if r is not None:
            row['flagged'] = ab(lambda: final(need[r]))
        out['fwd ' + name] = row
        del buf
    del xa
    # ---- bf16x3 data gradients (ReLU mask of the producing layer's activation) ----
    _, acts = Fn.pyramid_alloc(B, SIZES, 256, torch.float32, 'cuda')
    fill(acts, 256, gen, False, relu=True)
    rows = torch.rand(B, generator=gen, device='cuda') + 0.5
    for name, cfp, r in (('retina_cls (768 -> 256)', 768, None), ('retina_reg (64 -> 256)', 64, 1)):
        _, dz = Fn.pyramid_alloc(B, SIZES, cfp, torch.float32, 'cuda')
        fill(dz, cfp, gen, False, keep=dilated(0) if r is not None else None)
        w = ops.pack_weight(rnd_w(256, cfp), torch.float32, x3=True)
        _, g = Fn.pyramid_alloc(B, SIZES, 256, torch.float32, 'cuda')

        def dfinal(flags, dz=dz, w=w, g=g, cfp=cfp, r=r):
            ops.conv2d(dz, w, g, Cin=cfp, Cout=256, **K3, res=acts, res_mode=ops.RES_RELU_MASK, rowscale=rows if r is None else None,
                       split=True, live=flags)
        row = {'dense': ab(lambda: dfinal(None))}
        if r is not None:
            row['flagged'] = ab(lambda: dfinal(live[r].contiguous()))
        out['dgrad ' + name] = row
        del dz, g
    _, ra, rb = Fn.pyramid_alloc_pair(B, SIZES, 256, torch.float32, 'cuda')
    fill(ra + rb, 256, gen, False, relu=True)
    for t in range(3, 0, -1):
        r = 5 - t
        da, db = pair(256, gen, False, keep_b=dilated(r - 1))
        wd = [ops.pack_weight(rnd_w(256, 256), torch.float32, x3=True) for _ in range(2)]
        _, ga, gb = Fn.pyramid_alloc_pair(B, SIZES, 256, torch.float32, 'cuda')

        def dlayer(flags, da=da, db=db, wd=wd, ga=ga, gb=gb):
            ops.conv2d(da + db, wd[0], ga + gb, Cin=256, Cout=256, **K3, res=ra + rb, res_mode=ops.RES_RELU_MASK, split=True,
                       seg_w=[wd[0]] * 5 + [wd[1]] * 5, live=flags, live_tile0=ntile if flags is not None else 0)
        out['dgrad paired tower layer %d (256 -> 256) r=%d' % (t, r)] = {'dense': ab(lambda: dlayer(None)),
                                                                         'flagged': ab(lambda: dlayer(live[r].contiguous()))}
        del da, db, ga, gb
    _, d0 = Fn.pyramid_alloc(B, SIZES, 256, torch.float32, 'cuda')
    fill(d0, 256, gen, False)
    w0 = ops.pack_weight(rnd_w(WC, 256), torch.float32, x3=True)
    _, g0 = Fn.pyramid_alloc(B, SIZES, WC, torch.float32, 'cuda')
    out['dgrad tower layer 0 back to the neck (256 -> 64, 64-wide tile)'] = {
        'dense': ab(lambda: ops.conv2d(d0, w0, g0, Cin=256, Cout=WC, **K3, split=True, out_f32=True))}
    json.dump(out, sys.stdout, indent=1)
    print()


if __name__ == '__main__':
    main()
