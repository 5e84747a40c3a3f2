"""Per-launch timing of the regression tower's flagged launches in the gathered form (include/effdet_unit_lists.h) at the benchmark's
shapes (D0, B = 32 @512): the four paired forward tower launches, retina_reg, its data gradient, the three paired tower data gradients
and the 256 -> 64 gradient back to the neck, each
  dense / with the 128-pixel tile flags of the benchmark's batch / gathered (the device-side word decides, as in a step) /
  every unit set with the device's word (the worst case of a step: it falls back to the tile flags) / every unit set and gathered anyway
  (the overhead of the gathered addressing and of per-tap staging on the full tile count),
plus the unit and tile counts per radius and the time of ops.UnitLists.  The backward launches take the forward's flags (the positive
pixels; d(reg) is non-zero exactly there up to exact-zero gradients).  15 warm-up + 50 timed launches per figure, device events.  One
JSON document on stdout.

    python tools/sparse_units_timing.py > profiles/sparse_units_launch_timing.json"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from efficientdet.pytorch_amd import ops, functional as Fn                     # noqa: E402
from efficientdet.pytorch_amd.synthetic import synthetic_batch                 # noqa: E402

B, S, WC = 32, 512, 64
SIZES = [(S >> (3 + i), S >> (3 + i)) for i in range(5)]


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


def pair(C, gen, h, relu=True):
    """two random pyramids pairwise in one buffer, in the H-split (h) or the split layout"""
    _, xa, xb = Fn.pyramid_alloc_pair(B, SIZES, C, torch.float32, 'cuda')
    for m in xa + xb:
        src = torch.randn(m.B, m.H, m.W, C, generator=gen, device='cuda')
        src = torch.relu(src) if relu else src
        ops.to_split2(src, None if h else m.addr(), m.addr() if h else None, src.numel(), None)
    return xa, xb


def main():
    gen = torch.Generator(device='cuda').manual_seed(0)
    ann = synthetic_batch(B, S, seed=1, num_classes=80)[1].cuda().float().contiguous()      # the benchmark's batch (rank 0)
    anc = ops.anchors(S, S, 'cuda')
    l32, l128 = ops.live_tiles_from_map(ops.positive_pixel_map(anc, ann, SIZES), B, SIZES)
    ul = ops.UnitLists(l32, l128)
    full = ops.UnitLists(torch.ones_like(l32), torch.ones_like(l128))
    forced = ops.UnitLists(torch.ones_like(l32), torch.ones_like(l128))
    forced.counts[:, 2] = 1
    ntile = l128.shape[1]
    out = {'counts [units, tiles, gather, 0] per radius': ul.counts.cpu().tolist(), 'unit_lists_us': timed(lambda: ops.UnitLists(l32, l128))}

    def forms(name, launch, r, tile0, kind):
        def go(lists, units):
            kw = {kind: lists.live128[r], kind + '_tile0': tile0}
            if units:
                kw['units'] = lists.row(r)
            return timed(lambda: launch(**kw))
        out[name] = {'dense_us': timed(lambda: launch()), 'tile_flags_us': go(ul, False), 'gathered_us': go(ul, True),
                     'all_set_tile_flags_us': go(full, False), 'all_set_device_word_us': go(full, True), 'all_set_gathered_us': go(forced, True)}

    K3 = dict(KH=3, KW=3, pad_t=1, pad_l=1)
    for t in range(4):                       # forward tower layers, paired: classification dense in front
        cin = WC if t == 0 else 256
        xa, xb = pair(cin, gen, True)
        ws = [ops.pack_weight(torch.randn(256, cin, 3, 3, generator=gen, device='cuda') / (9 * cin) ** 0.5, torch.float32, h3=True) for _ in range(2)]
        bs = [torch.randn(256, generator=gen, device='cuda') * 0.1 for _ in range(2)]
        _, ya, yb = Fn.pyramid_alloc_pair(B, SIZES, 256, torch.float32, 'cuda')
        _, sa, sb = Fn.pyramid_alloc_pair(B, SIZES, 256, torch.float32, 'cuda')

        def launch(xa=xa, xb=xb, ws=ws, bs=bs, ya=ya, yb=yb, sa=sa, sb=sb, cin=cin, **kw):
            ops.conv2d(xa + xb, ws[0], ya + yb, Cin=cin, Cout=256, **K3, shift=bs[0], act=ops.ACT_RELU, hsplit=True, ysplit=sa + sb,
                       seg_w=[ws[0]] * 5 + [ws[1]] * 5, seg_shift=[bs[0]] * 5 + [bs[1]] * 5, **kw)
        forms('fwd paired tower layer %d (%d -> 256) r=%d' % (t, cin, 4 - t), launch, 4 - t, ntile, 'needed')
        del xa, xb, ya, yb, sa, sb
    xa, _ = pair(256, gen, True)
    w = ops.pack_weight(torch.randn(36, 256, 3, 3, generator=gen, device='cuda') / 48.0, torch.float32, h3=True)
    bias = torch.randn(36, generator=gen, device='cuda') * 0.1
    reg = torch.empty(B, sum(h * w_ for h, w_ in SIZES) * 9, 4, device='cuda')

    def final(**kw):
        ops.conv2d(xa, w, Fn.head_out_maps(reg, B, SIZES, 4), Cin=256, Cout=36, **K3, shift=bias, out_f32=True, hsplit=True, **kw)
    forms('fwd retina_reg (256 -> 36) r=0', final, 0, 0, 'needed')
    del xa

    da, _ = pair(64, gen, False, relu=False)             # d(reg) rows padded to 64 channels
    ra, rb = pair(256, gen, False)
    wd = ops.pack_weight(torch.randn(256, 64, 3, 3, generator=gen, device='cuda') / 24.0, torch.float32, x3=True)
    _, dz = Fn.pyramid_alloc(B, SIZES, 256, torch.float32, 'cuda')

    def reg_dgrad(**kw):
        ops.conv2d(da, wd, dz, Cin=64, Cout=256, **K3, res=ra, res_mode=ops.RES_RELU_MASK, split=True, **kw)
    forms('bwd retina_reg data gradient (64 -> 256) r=1', reg_dgrad, 1, 0, 'live')
    del da, dz
    xa, xb = pair(256, gen, False, relu=False)
    ws = [ops.pack_weight(torch.randn(256, 256, 3, 3, generator=gen, device='cuda') / 48.0, torch.float32, x3=True) for _ in range(2)]
    _, ya, yb = Fn.pyramid_alloc_pair(B, SIZES, 256, torch.float32, 'cuda')
    for t in (3, 2, 1):                      # tower data gradients, paired

        def launch(**kw):
            ops.conv2d(xa + xb, ws[0], ya + yb, Cin=256, Cout=256, **K3, res=ra + rb, res_mode=ops.RES_RELU_MASK, split=True,
                       seg_w=[ws[0]] * 5 + [ws[1]] * 5, **kw)
        forms('bwd paired tower data gradient layer %d (256 -> 256) r=%d' % (t, 5 - t), launch, 5 - t, ntile, 'live')
    del xb, ya, yb, ra, rb
    wn = ops.pack_weight(torch.randn(WC, 256, 3, 3, generator=gen, device='cuda') / 48.0, torch.float32, x3=True)
    flat, dp = Fn.pyramid_alloc(B, SIZES, WC, torch.float32, 'cuda')
    flat.zero_()

    def neck(**kw):
        ops.conv2d(xa, wn, dp, Cin=256, Cout=WC, **K3, res=dp, res_mode=ops.RES_ADD, split=True, out_f32=True, **kw)
    forms('bwd 256 -> 64 gradient back to the neck r=5', neck, 5, 0, 'live')
    keys = [k for k in out if isinstance(out[k], dict)]
    out['sum over the ten launches'] = {f: round(sum(out[k][f] for k in keys), 1) for f in out[keys[0]]}
    json.dump(out, sys.stdout, indent=1)
    print()


if __name__ == '__main__':
    main()
