"""Per-launch timing of the sparse regression-tower forward (include/effdet_needed_tiles.h) at the benchmark's shapes (D0, B = 32 @512):
the four paired tower launches and retina_reg, each dense / with every flag set (the overhead of the flag path) / with the flags of the
benchmark's batch, plus the needed-tile fractions per radius and the time of ops.needed_tiles (map + flag kernels with their host
side).  15 warm-up + 50 timed launches per figure, device events.  One JSON document on stdout.

    python tools/sparse_reg_fwd_timing.py > profiles/sparse_reg_fwd_launch_timing.json"""
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


def hsplit_pair(C, gen):
    _, xa, xb = Fn.pyramid_alloc_pair(B, SIZES, C, torch.float32, 'cuda')
    for m in xa + xb:
        src = torch.relu(torch.randn(m.B, m.H, m.W, C, generator=gen, device='cuda'))
        ops.to_split2(src, None, m.addr(), src.numel(), None)
    return xa, xb


def main():
    gen = torch.Generator(device='cuda').manual_seed(0)
    ann = synthetic_batch(B, S, seed=1, num_classes=80)[1].cuda().float().contiguous()      # the benchmark's batch (rank 0)
    anc = ops.anchors(S, S, 'cuda')
    need = ops.needed_tiles(anc, ann, B, SIZES)
    ones = torch.ones_like(need[0])
    ntile = need.shape[1]
    out = {'needed128_fraction': [round(float(need[r].float().mean()), 4) for r in range(need.shape[0])],
           'needed_tiles_us': timed(lambda: ops.needed_tiles(anc, ann, B, SIZES))}

    def three(name, launch, r, tile0):
        out[name] = {'dense_us': timed(lambda: launch(None, 0)), 'all_needed_us': timed(lambda: launch(ones, tile0)),
                     'flagged_us': timed(lambda: launch(need[r], tile0))}

    for t in range(4):
        cin = WC if t == 0 else 256
        xa, xb = hsplit_pair(cin, gen)
        ws = [ops.pack_weight(torch.randn(256, cin, 3, 3, generator=gen, device='cuda') / (9 * cin) ** 0.5, torch.float32, h3=True) for _ in range(2)]
        bs = [torch.randn(256, generator=gen, device='cuda') * 0.1 for _ in range(2)]
        _, ya, yb = Fn.pyramid_alloc_pair(B, SIZES, 256, torch.float32, 'cuda')
        _, sa, sb = Fn.pyramid_alloc_pair(B, SIZES, 256, torch.float32, 'cuda')

        def launch(flags, tile0, xa=xa, xb=xb, ws=ws, bs=bs, ya=ya, yb=yb, sa=sa, sb=sb, cin=cin):
            ops.conv2d(xa + xb, ws[0], ya + yb, Cin=cin, Cout=256, KH=3, KW=3, pad_t=1, pad_l=1, shift=bs[0], act=ops.ACT_RELU, hsplit=True,
                       ysplit=sa + sb, seg_w=[ws[0]] * 5 + [ws[1]] * 5, seg_shift=[bs[0]] * 5 + [bs[1]] * 5, needed=flags, needed_tile0=tile0)
        three('paired tower layer %d (%d -> 256) r=%d' % (t, cin, 4 - t), launch, 4 - t, ntile)
        del xa, xb, ya, yb, sa, sb
    xa, _ = hsplit_pair(256, gen)
    w = ops.pack_weight(torch.randn(36, 256, 3, 3, generator=gen, device='cuda') / 48.0, torch.float32, h3=True)
    bias = torch.randn(36, generator=gen, device='cuda') * 0.1
    reg = torch.empty(B, sum(h * w_ for h, w_ in SIZES) * 9, 4, device='cuda')

    def final(flags, tile0):
        ops.conv2d(xa, w, Fn.head_out_maps(reg, B, SIZES, 4), Cin=256, Cout=36, KH=3, KW=3, pad_t=1, pad_l=1, shift=bias, out_f32=True,
                   hsplit=True, needed=flags, needed_tile0=tile0)
    three('retina_reg (256 -> 36) r=0', final, 0, 0)
    json.dump(out, sys.stdout, indent=1)
    print()


if __name__ == '__main__':
    main()
