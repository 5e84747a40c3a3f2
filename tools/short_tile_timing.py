"""Per-launch timing of the short pixel tile (csrc/conv_igemm.hip, tuning knob TUNE_SHORT_TILE) at the benchmark's small-map shapes (D0,
B = 32 @512): the BiFPN 3x3 64 -> 64 convs and their data gradients on the 4x4, 8x8 and 16x16 levels, and the project / expand 1x1 convs
of backbone blocks 8-15 with their data gradients, each in exact fp32 (the forward's arithmetic) and bf16x3 (the gradient convs'), with
the knob off (the 128-pixel plans) and on, alternating off / on / off / on in one process.  15 warm-up + 50 timed launches per figure,
device events; every row also carries both plans (tile, stages, workgroups, LDS), so a shape class the rule leaves alone shows as such.
One JSON document on stdout.

    python tools/short_tile_timing.py > profiles/short_tile_launch_timing.json"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from efficientdet.pytorch_amd import ops, _lib as L          # noqa: E402
from efficientdet.pytorch_amd.ops import Map                  # noqa: E402

B = 32
# (name, H = W, Cin, Cout, k)
FORWARD = [
    ('bifpn 3x3 64 -> 64', 4, 64, 64, 3), ('bifpn 3x3 64 -> 64', 8, 64, 64, 3), ('bifpn 3x3 64 -> 64', 16, 64, 64, 3),
    ('project 480 -> 112', 16, 480, 112, 1), ('project 672 -> 112', 16, 672, 112, 1),
    ('project 672 -> 192', 8, 672, 192, 1), ('project 1152 -> 192', 8, 1152, 192, 1), ('project 1152 -> 320', 4, 1152, 320, 1),
    ('expand 112 -> 672', 16, 112, 672, 1), ('expand 192 -> 1152', 8, 192, 1152, 1),
]


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


def ab(fn, plan):
    """-> {'tile128_us': [two windows], 'short_us': [two windows], 'plan128': ..., 'plan_short': ...}, the knob alternating"""
    row = {'tile128_us': [], 'short_us': []}
    old = ops.tuning_set(L.TUNE_SHORT_TILE, 0)
    try:
        for _ in range(2):
            for sw, key in ((0, 'tile128_us'), (1, 'short_us')):
                ops.tuning_set(L.TUNE_SHORT_TILE, sw)
                row[key].append(timed(fn))
        for sw, key in ((0, 'plan128'), (1, 'plan_short')):
            ops.tuning_set(L.TUNE_SHORT_TILE, sw)
            i = plan()
            row[key] = '%d x %d, %d stages, %d workgroups, %d KiB' % (i['tile_m'], i['tile_n'], i['stages'], i['grid'], i['lds_bytes'] // 1024)
    finally:
        ops.tuning_set(L.TUNE_SHORT_TILE, old)
    return row


def main():
    gen = torch.Generator(device='cuda').manual_seed(0)
    out = {}
    for arith in ('f32', 'bf16x3'):
        old = ops.set_f32_arith(arith)
        try:
            for name, hw, cin, cout, k in FORWARD:
                for grad in (False, True):
                    # the data gradient of a stride-1 conv: the same kernel on the transposed, flipped weights, Cout -> Cin channels
                    ci, co = (cout, cin) if grad else (cin, cout)
                    x = Map.of(torch.randn(B, hw, hw, ci, generator=gen, device='cuda'))
                    y = Map.new(B, hw, hw, co, torch.float32, 'cuda')
                    w = torch.randn(cout, cin, k, k, generator=gen, device='cuda') / (k * k * cin) ** 0.5
                    wp = ops.pack_weight(w, torch.float32, mode=1 if grad else 0)
                    kw = dict(Cin=ci, Cout=co, KH=k, KW=k, pad_t=k // 2, pad_l=k // 2)
                    if not grad:
                        kw.update(scale=torch.rand(co, generator=gen, device='cuda') + 0.5, shift=torch.randn(co, generator=gen, device='cuda'))
                    key = '%s %s %s @%dx%d' % (arith, 'dgrad' if grad else 'fwd', name, hw, hw)
                    out[key] = ab(lambda: ops.conv2d(x, wp, y, **kw), lambda: ops.conv2d_plan_info(x, wp, y, **kw))
        finally:
            ops.set_f32_arith(old)
    json.dump(out, sys.stdout, indent=1)
    print()


if __name__ == '__main__':
    main()
