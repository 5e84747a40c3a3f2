"""Shapes of the fused squeeze-excite backward tests and the split plan each one must get.

(B, H, W, Co, Ce) of a project conv Ce -> Co whose weight gradient is taken per image (conv2d_wgrad(image_splits=True)), with the
slabs per image q the library plans for it in each arithmetic ('f32' / 'bf16x3': fp32 storage, 'bf16': bf16 storage; None = the
launch refuses the shape) and the kernel id conv2d_wgrad_kernel_id reports (0 tiled, 1 thin pointwise).  The table is pinned here so
that a planning change cannot quietly make the tests shallow: tests/test_se_fused_ref_host.py checks it against the host-only
planning query on the CPU, tests/test_gpu_se_fused_bwd.py checks the slab count of every launch against it.
"""

#   (B, H,  W,  Co,  Ce):    {arith: q},                            kernel id (fp32 storage)
IMAGE_SPLIT_CASES = {
    (3, 4, 8, 40, 240):     ({'f32': 1, 'bf16x3': 1, 'bf16': None}, 0),     # hw = 32: the fp32 minimum (bf16 needs hw % 64 == 0)
    (2, 8, 8, 112, 672):    ({'f32': 1, 'bf16x3': 1, 'bf16': 1}, 0),        # hw = 64: the bf16 minimum
    (2, 16, 32, 80, 480):   ({'f32': 2, 'bf16x3': 2, 'bf16': 1}, 0),
    (1, 32, 32, 24, 144):   ({'f32': 4, 'bf16x3': 4, 'bf16': 2}, 0),
    (5, 8, 8, 192, 1152):   ({'f32': 1, 'bf16x3': 1, 'bf16': 1}, 0),        # two Cout tiles, odd B
    (2, 8, 16, 88, 528):    ({'f32': 1, 'bf16x3': 1, 'bf16': 1}, 0),        # a scaled-width pair
    (3, 8, 8, 54, 240):     ({'f32': 1, 'bf16x3': 1}, 0),                   # Co % 4 != 0, dense rows: meant for the register-transpose kernel (*)
    (8, 64, 64, 24, 144):   ({'f32': 16, 'bf16x3': 16, 'bf16': 8}, 1),      # 32 k pixels, 168 channels: the thin pointwise kernel
}
# (*) the DMA kernels need 16-byte aligned dz rows, so this level should fall to the register-transpose kernel; neither the kernel id
#     (0 = tiled) nor the profile's name tells the tiled kernels apart, so that choice is NOT verified by the tests
ARITHS = ('f32', 'bf16x3', 'bf16')

# the wide low-resolution data gradients (project conv backward, Co -> Ce) of the epilogue tests: the tiled shapes above + one whose
# reduction length (Co = 320) is long enough for the bf16x3 operand form (K % 32 == 0, K >= 256)
DGRAD_CASES = [(3, 4, 8, 40, 240), (2, 8, 8, 112, 672), (2, 16, 32, 80, 480), (1, 32, 32, 24, 144), (5, 8, 8, 192, 1152),
               (2, 8, 16, 88, 528), (2, 4, 8, 320, 1152)]

# the whole-branch tests: one shape with q = 1 everywhere, one with q = 4 (fp32 storage) / 2 (bf16)
BRANCH_CASES = {(3, 8, 8, 112, 672): {'f32': 1, 'bf16x3': 1, 'bf16': 1}, (3, 32, 32, 24, 144): {'f32': 4, 'bf16x3': 4, 'bf16': 2}}
