/* effdet_gate_operand.h -- the squeeze-excite gate of an MBConv block applied inside the project conv's OPERAND registers: entry points
 * added to ABI generation 11 after effdet_hip.h's own set (effdet_hip.h documents effdet_conv_t / effdet_wgrad_t; a library of the same
 * generation built before this header lacks the symbols, so a binding looks them up by name before the first call).  The descriptors
 * keep their layout: the gate travels as two call arguments, like the flags of effdet_live_tiles.h / effdet_needed_tiles.h.
 *
 * In training the project conv of a block reads   xs[b][pix][c] = act(z[b][pix][c]) * a_gate[b][c]
 * (models/efficientnet.py:86-95; act = Swish on the stored depthwise pre-activation, or none on its Swish output), which
 * effdet_channel_scale writes in a read + write pass over the expanded map.  xs has two readers, the conv's forward and its per-image
 * weight gradient.  Both hold the raw operand value in a register between the LDS read and the matrix-core instruction; the calls below
 * form  v = act(v); v *= a_gate[b][c]  there -- the two statements of effdet_channel_scale's kernel -- so every matrix-core instruction
 * receives bit for bit the operand it would have read from xs, in the same order, and xs never exists in memory.  Outputs are those of
 * effdet_channel_scale followed by effdet_conv2d / effdet_conv2d_wgrad, bit for bit (NaN payloads included).  This is NOT
 * effdet_conv_t.w_image_stride, which folds the gate into per-image weights W diag(gate_b): other products, another rounding.
 *
 *   a_gate   fp32 [B][Cin], 4-byte aligned, never read past B * Cin floats        a_act   EFFDET_ACT_NONE or EFFDET_ACT_SWISH
 *
 * effdet_conv2d_gated: p as for effdet_conv2d with x = the UNgated map.  Accepted for dtype EFFDET_F32 (exact products), 1x1, stride 1,
 * no padding, one segment with Ho*Wo a multiple of 128 (a 128-pixel tile lies in one image: the rule of w_image_stride), shared weights
 * (no w_image_stride / seg_w); every epilogue option of effdet_conv2d is available.  It runs the 128-pixel-tile kernel effdet_conv2d
 * gives the same descriptor when that is one (ids 0..3), else that kernel in place of the skinny pointwise form.
 * Anything else returns EFFDET_EUNSUPPORTED (EFFDET_EINVAL for a_gate == NULL or another a_act): there is no silent launch on ungated data.
 *
 * effdet_conv2d_gated_plan_info: effdet_conv2d_plan_info for that call (no device work).  info->reserved[0] reports the form the launch
 * takes: 1 = x * gate, 2 = swish(x) * gate (0 from effdet_conv2d_plan_info itself: no gate).  Same return codes as effdet_conv2d_gated.
 *
 * effdet_conv2d_wgrad_gated: p as for effdet_conv2d_wgrad with x = the UNgated map.  Accepted with image_splits (a split lies in one
 * image: its gate row is loaded once per workgroup) where effdet_conv2d_wgrad launches the thin pointwise kernel or the DMA-staged fp32
 * kernel (dtype EFFDET_F32 or EFFDET_F32_BF16X3; 1x1, stride 1, contiguous maps -- the stem's form and the split-layout / bf16 /
 * register-transpose kernels are not covered).  Slabs, bias partial rows, workspace size and split count are those of effdet_conv2d_wgrad
 * on xs; the bias rows use dz alone.  Anything else: EFFDET_EUNSUPPORTED.
 *
 * effdet_conv2d_wgrad_gated_kernel: which kernel that call launches (effdet_conv2d_wgrad_kernel's ids: 0 the DMA-staged tiled kernel,
 * 1 the thin pointwise kernel), or the negative code the call returns.  No device work. */
#ifndef EFFDET_GATE_OPERAND_H
#define EFFDET_GATE_OPERAND_H
#include "effdet_hip.h"
#include "effdet_conv_plan.h"
#ifdef __cplusplus
extern "C" {
#endif

int effdet_conv2d_gated(const effdet_conv_t* p, const float* a_gate, int a_act, effdet_stream_t stream);
int effdet_conv2d_gated_plan_info(const effdet_conv_t* p, const float* a_gate, int a_act, effdet_conv_plan_info_t* info);
int effdet_conv2d_wgrad_gated(const effdet_wgrad_t* p, const float* a_gate, int a_act, void* workspace, long long workspace_bytes,
                              effdet_stream_t stream);
int effdet_conv2d_wgrad_gated_kernel(const effdet_wgrad_t* p, const float* a_gate, int a_act);

#ifdef __cplusplus
}
#endif
#endif /* EFFDET_GATE_OPERAND_H */
