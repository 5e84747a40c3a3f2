/* effdet_live_tiles.h -- sparse regression-tower gradients of libeffdet_hip.so: entry points added to ABI generation 11 after
 * effdet_hip.h's own set (its conventions hold: device pointers, 0 or a negative EFFDET_E* code, kernels enqueued on `stream`, no
 * memset / copy / host sync, so every call may be captured in a graph).  A library of the same generation built before this header
 * lacks the symbols, so a binding looks them up by name before the first call.
 *
 * The smooth-L1 gradient d(reg) is an exact zero everywhere but at the positive anchors, and the whole backward pass of the
 * RetinaHead's regression tower (3x3, stride 1, pad 1 convs without bias or affine) starts from it: after k data-gradient layers a
 * gradient pixel can be non-zero only within Chebyshev distance k of a non-zero d(reg) pixel of the same image and level.
 * effdet_live_tiles turns d(reg) into byte flags per unit of work of the gradient kernels; the two _live launches skip the units
 * whose flag is 0.  A skipped unit would have produced (data gradient) or added (weight gradient) exact zeros, so results are bit
 * for bit those of the dense launches -- unless a weight or activation is non-finite where the gradient is zero (dense: 0 * Inf =
 * NaN; sparse: 0). */
#ifndef EFFDET_LIVE_TILES_H
#define EFFDET_LIVE_TILES_H
#include "effdet_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define EFFDET_LIVE_RADII 6          /* flags for dilation radius r = 0 .. 5 */

/* Units of pyramid level l (H[l] x W[l], M = B * H * W pixels in (b, h, w) order): steps of 32 pixels and tiles of 128 pixels of
 * that linear index, the last one of a level possibly partial -- the K-step of the split-layout weight-gradient kernel and the
 * pixel tile of the implicit-GEMM kernel.  Levels are concatenated in order.  -> steps / tiles / pixels over all levels. */
long long effdet_live_tiles_counts(int B, int nlev, const int* H, const int* W, long long* steps, long long* tiles);

/* dreg: the rows effdet_focal_loss_bwd_reg leaves with reg_ld != 0 -- [B][sum_l H*W][reg_ld], level l of image b starting at pixel
 * sum_{l' < l} H*W -- in fp32 (dtype EFFDET_F32, reg_ld % 4 == 0) or the split layout (EFFDET_F32_SPLIT, reg_ld % 32 == 0).
 * A pixel is non-zero when any of its reg_ld words has a bit set outside the sign bit(s) (fp32: w & 0x7fffffff, split:
 * w & 0x7fff7fff): NaN is non-zero, -0.0 is zero.
 * live32 [6][steps], live128 [6][tiles] (bytes, 1 / 0): unit u of radius r is 1 iff one of its pixels lies within Chebyshev distance
 * r of a non-zero pixel of the same image and level.  Every flag is written, by one plain store.
 * scratch: 2 * `pixels` bytes (the per-pixel non-zero map and row-distance map between the kernels of the call). */
int effdet_live_tiles(const void* dreg, int dtype, int reg_ld, int B, int nlev, const int* H, const int* W, unsigned char* scratch,
                      unsigned char* live32, unsigned char* live128, effdet_stream_t stream);

/* effdet_conv2d with tile flags: live[mt - live_tile0] == 0 marks the 128-pixel tile mt (segments in order, each rounded up to whole
 * tiles) as one whose every input tap is zero; tiles below live_tile0 have no flag and are live (a paired launch whose first
 * segments are another conv).  A dead tile is written as zeros (split or, with out_f32, fp32 output; res_mode NONE or RELU_MASK) or,
 * with EFFDET_RES_ADD onto y == res, left as it is.  Honoured only by the EFFDET_F32_SPLIT 128-pixel-tile kernels (ids 8, 9) with no
 * scale / shift / rowscale / bc_* / z / y_split / activation / per-image weights; everywhere else the flags are ignored (the dense
 * launch is always right: the flags are a hint). */
int effdet_conv2d_live(const effdet_conv_t* p, const unsigned char* live, int live_tile0, effdet_stream_t stream);

/* effdet_conv2d_wgrad with step flags: live32[s] == 0 marks the 32-pixel step s (levels in segment order, each rounded up to whole
 * steps) as one whose dz pixels are all zero; every split walks only its live steps (none: a zero slab and zero bias row).
 * EFFDET_F32_SPLIT descriptors only (EFFDET_EUNSUPPORTED otherwise). */
int effdet_conv2d_wgrad_live(const effdet_wgrad_t* p, void* workspace, long long workspace_bytes, const unsigned char* live32,
                             effdet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EFFDET_LIVE_TILES_H */
