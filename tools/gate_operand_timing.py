"""Per-launch timing of the squeeze-excite gate in the project conv's operands (include/effdet_gate_operand.h) at the benchmark's shapes
(D0, B = 32 @512, arithmetic f32_hf16x3_bwd_bf16x3: exact-fp32 forward, bf16x3 weight gradient): for each of the 16 MBConv blocks (11 of them
take the form: the 8 x 8 and 4 x 4 maps of blocks 11 .. 15 are no whole 128-pixel tiles) the old path -- ops.channel_scale, the project conv on its output, the per-image weight gradient on its output -- against the two launches
that take the depthwise pre-activation and the gate themselves.  15 warm-up + 50 timed launches per figure, device events, every launch
also on its own.  One JSON document on stdout; `saved_us` = old sum - new sum per block (what functional.GATE_OPERAND_MIN_HW is set from).

    python tools/gate_operand_timing.py > profiles/gate_operand_launch_timing.json"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from efficientdet.pytorch_amd import ops                                       # noqa: E402
from efficientdet.pytorch_amd.config import backbone_plan                      # noqa: E402
from efficientdet.pytorch_amd.ops import ACT_SWISH, RES_ADD, RES_NONE, Map     # noqa: E402

B, S = 32, 512


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


def main():
    gen = torch.Generator(device='cuda').manual_seed(0)
    _, _, blocks, _, _ = backbone_plan('efficientnet-b0')
    side = S // 2
    out, tot = {}, {'old_us': 0.0, 'new_us': 0.0}
    for i, blk in enumerate(blocks):
        side = (side + blk.stride - 1) // blk.stride
        Ce, Co = blk.cexp, blk.cout
        r = lambda *s: torch.randn(*s, generator=gen, device='cuda')
        z, dy, y = Map.of(r(B, side, side, Ce)), Map.of(r(B, side, side, Co)), Map.new(B, side, side, Co, torch.float32, 'cuda')
        gate = torch.rand(B, Ce, generator=gen, device='cuda')
        wp = ops.pack_weight(r(Co, Ce, 1, 1) * 0.1, torch.float32)
        kw = dict(Cin=Ce, Cout=Co, KH=1, KW=1, scale=torch.rand(Co, generator=gen, device='cuda') + 0.5, shift=r(Co),
                  rowscale=torch.ones(B, device='cuda') if blk.skip else None, res=Map.of(r(B, side, side, Co)) if blk.skip else None,
                  res_mode=RES_ADD if blk.skip else RES_NONE)
        wk = dict(Cin=Ce, Cout=Co, KH=1, KW=1, image_splits=True)
        xs = ops.channel_scale(z, gate, ACT_SWISH)

        def fwd(gated):
            ops.set_f32_arith('f32')
            if gated:
                ops.conv2d(z, wp, y, a_gate=gate, a_act=ACT_SWISH, **kw)
            else:
                ops.conv2d(xs, wp, y, **kw)

        def wgrad(gated):
            ops.set_f32_arith('bf16x3')
            if gated:
                ops.conv2d_wgrad(z, dy, a_gate=gate, a_act=ACT_SWISH, **wk)
            else:
                ops.conv2d_wgrad(xs, dy, **wk)

        def old():
            ops.channel_scale(z, gate, ACT_SWISH); fwd(False); wgrad(False)

        def new():
            fwd(True); wgrad(True)
        ops.set_f32_arith('f32')
        if not ops.conv2d_gated_ok(z, wp, y, gate, ACT_SWISH, **kw):      # (8 x 8 and 4 x 4 maps: no whole 128-pixel tiles per image)
            out['block %d' % i] = {'map': side, 'Cexp': Ce, 'Cout': Co, 'accepted': False,
                                   'channel_scale_us': timed(lambda: ops.channel_scale(z, gate, ACT_SWISH))}
            continue
        ops.set_f32_arith('bf16x3')
        kid = ops.conv2d_wgrad_kernel_id(z, dy, image_splits=True, a_gate=gate, a_act=ACT_SWISH, Cin=Ce, Cout=Co, KH=1, KW=1)
        row = {'map': side, 'Cexp': Ce, 'Cout': Co, 'wgrad_kernel': {0: 'f32dma bf16x3', 1: 'thin'}.get(kid, kid),
               'channel_scale_us': timed(lambda: ops.channel_scale(z, gate, ACT_SWISH)),
               'fwd_us': timed(lambda: fwd(False)), 'fwd_gated_us': timed(lambda: fwd(True)),
               'wgrad_us': timed(lambda: wgrad(False)), 'wgrad_gated_us': timed(lambda: wgrad(True)),
               'old_us': timed(old), 'new_us': timed(new)}
        row['saved_us'] = round(row['old_us'] - row['new_us'], 1)
        tot['old_us'] += row['old_us']; tot['new_us'] += row['new_us']
        out['block %d' % i] = row
        del z, dy, y, xs, kw
        torch.cuda.empty_cache()
    ops.set_f32_arith('f32')
    tot = {k: round(v, 1) for k, v in tot.items()}
    tot['saved_us'] = round(tot['old_us'] - tot['new_us'], 1)
    out['all blocks'] = tot
    json.dump(out, sys.stdout, indent=1)
    print()


if __name__ == '__main__':
    main()
