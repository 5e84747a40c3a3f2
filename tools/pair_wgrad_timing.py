"""Per-launch timing of the paired tower weight gradients (include/effdet_wgrad_pair.h) at the benchmark's shapes (D0, B = 32 @512): for
each of the four tower layers the two separate launches (the classification tower's dense one, the regression tower's flagged one) against
ops.conv2d_wgrad_pair in both block orders (the flagged problem's blocks first / the dense problem's first), with the flags of the
benchmark's batch at the layer's radius.  15 warm-up + 50 timed launches per figure, device events.  One JSON document on stdout.

    python tools/pair_wgrad_timing.py > profiles/pair_wgrad_launch_timing.json"""
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


def split_pyramid(C, gen, keep=None):
    """level-major split-layout maps of random values; keep (per level a [B, H, W] bool map): exact zeros outside it"""
    _, maps = Fn.pyramid_alloc(B, SIZES, C, torch.float32, 'cuda')
    for l, m in enumerate(maps):
        src = torch.randn(m.B, m.H, m.W, C, generator=gen, device='cuda')
        if keep is not None:
            src = src * keep[l].unsqueeze(-1)
        Fn.level_tensor(m).copy_(ops.to_split(src))
    return maps


def main():
    gen = torch.Generator(device='cuda').manual_seed(0)
    ann = synthetic_batch(B, S, seed=1, num_classes=80)[1].cuda().float().contiguous()      # the benchmark's batch (rank 0)
    anc = ops.anchors(S, S, 'cuda')
    A = anc.shape[1]
    cls = torch.rand(B, A, 80, generator=gen, device='cuda').clamp(1e-3, 1 - 1e-3)
    reg = torch.randn(B, A, 4, generator=gen, device='cuda') * 0.3
    _, ws = ops.focal_loss_fwd(cls, reg, anc, ann)
    dreg = ops.focal_loss_bwd_reg(reg, anc, ann, torch.ones(B, device='cuda'), ws, torch.float32, reg_ld=64, split=True)
    l32, _ = ops.live_tiles(dreg, B, SIZES, 64, True)
    out = {'live32_fraction': [round(float(l32[r].float().mean()), 4) for r in range(l32.shape[0])]}
    # the pixels of radius r as [B, H, W] maps: dz of the regression problem is zero outside them (what the flags promise)
    poff, nz = 0, []
    for (h, w) in SIZES:
        rows = dreg.view(torch.int32)[:, poff:poff + h * w]
        nz.append(((rows & 0x7fff7fff) != 0).any(dim=2).view(B, h, w)); poff += h * w
    old = os.environ.pop('EFFDET_WGRAD_PAIR_ORDER', None)
    for t in range(3, -1, -1):
        r, cin = 4 - t, (WC if t == 0 else 256)
        keep = [torch.nn.functional.max_pool2d(m.float().unsqueeze(1), 2 * r + 1, 1, r).squeeze(1) > 0 for m in nz]
        xa = split_pyramid(cin, gen)
        xb = xa if t == 0 else split_pyramid(cin, gen)
        za, zb = split_pyramid(256, gen), split_pyramid(256, gen, keep)
        kw = dict(Cin=cin, Cout=256, KH=3, KW=3, pad_t=1, pad_l=1)
        flags = l32[r].contiguous()

        def separate():
            ops.conv2d_wgrad(xa, za, split=True, **kw)
            ops.conv2d_wgrad(xb, zb, split=True, live32=flags, **kw)

        def paired():
            ops.conv2d_wgrad_pair(xa, za, xb, zb, live32_b=flags, **kw)
        row = {'dense_us': timed(lambda: ops.conv2d_wgrad(xa, za, split=True, **kw)),
               'flagged_us': timed(lambda: ops.conv2d_wgrad(xb, zb, split=True, live32=flags, **kw)),
               'separate_us': timed(separate)}
        for name, order in (('paired_flagged_first_us', '1'), ('paired_dense_first_us', '0')):
            os.environ['EFFDET_WGRAD_PAIR_ORDER'] = order       # (the library reads the knob at every call)
            row[name] = timed(paired)
        del os.environ['EFFDET_WGRAD_PAIR_ORDER']
        row['paired_both_dense_us'] = timed(lambda: ops.conv2d_wgrad_pair(xa, za, xb, zb, **kw))
        out['tower layer %d (%d -> 256) r=%d' % (t, cin, r)] = row
        del xa, xb, za, zb
    if old is not None:
        os.environ['EFFDET_WGRAD_PAIR_ORDER'] = old
    json.dump(out, sys.stdout, indent=1)
    print()


if __name__ == '__main__':
    main()
