/* effdet_conv_plan.h -- a host-only query of the dense-conv launch plan of libeffdet_hip.so: an entry point added to ABI generation 11
 * after effdet_hip.h's own set (effdet_hip.h documents effdet_conv_t; a library of the same generation built before this header lacks
 * the symbol, so a binding looks it up by name before the first call).
 *
 * effdet_conv2d_plan_info answers "what would effdet_conv2d launch for this descriptor": it runs the planner effdet_conv2d runs and
 * copies the decision out of the plan the launch itself reads -- the template parameters are recorded into that plan by the helper
 * that picks the instance, not derived a second time.  No device work and no HIP runtime call, like effdet_conv2d_kernel, whose kernel
 * id names several template instances at once (ids 0 / 1 / 4 / 5 cover two staging depths and the narrow 32-channel tile).  Tests use
 * it to prove which instance a shape reaches, how many tiles the launch has and how long its K loop is, instead of restating the planner.
 *
 * info (written only when the return value is >= 0):
 *   id          the kernel id, = the return value = effdet_conv2d_kernel(p)
 *   form        EFFDET_CONV_FORM_PLAIN   exact-fp32 or bf16 products of the operands as stored
 *               EFFDET_CONV_FORM_BF16X3  fp32 storage, operands split into bf16 hi + lo in registers, three bf16 products
 *               EFFDET_CONV_FORM_SPLIT   activations (and weights) pre-split: the [32 x bf16 hi | 32 x bf16 lo] layout
 *               EFFDET_CONV_FORM_HSPLIT  the f16x3 form: [32 x f16 hi | 32 x f16 lo * 2^11] activations, row-scaled f16 weights
 *               EFFDET_CONV_FORM_SKINNY  the pointwise fp32 kernel for Cin 16 / 24 (no matrix-core tile)
 *   persistent  1: the persistent kernel -- min(grid, compute units) workgroups, each walking tiles b, b + workgroups, ...
 *   tile_m, tile_n   workgroup tile: output pixels x output channels (skinny: the 64-pixel LDS tile x all Cout channels)
 *   stages      LDS stages of the K loop
 *   threads     threads per workgroup
 *   mtiles, ntiles   pixel tiles (all segments) and channel tiles of the launch (skinny: workgroups, 1)
 *   grid        workgroups; for a persistent kernel the tile count mtiles * ntiles BEFORE the cap at the device's compute units
 *   ksteps      trips of the K loop (one trip = 128 bytes per operand row)
 *   kord        K walk: 0 tap-major, 1 channel-group-major
 *   lds_bytes   dynamic LDS of the launch
 *   m32         1: the loop runs on 32x32x16 matrix-core tiles, 0: on 16x16 ones
 * Returns the kernel id (>= 0), or the negative code effdet_conv2d returns for the descriptor (EFFDET_EINVAL, EFFDET_EUNSUPPORTED);
 * EFFDET_EINVAL for info == NULL. */
#ifndef EFFDET_CONV_PLAN_H
#define EFFDET_CONV_PLAN_H
#include "effdet_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

enum { EFFDET_CONV_FORM_PLAIN = 0, EFFDET_CONV_FORM_BF16X3 = 1, EFFDET_CONV_FORM_SPLIT = 2, EFFDET_CONV_FORM_HSPLIT = 3,
       EFFDET_CONV_FORM_SKINNY = 4 };

typedef struct effdet_conv_plan_info_t {
  int id, form, persistent;
  int tile_m, tile_n, stages, threads;
  int mtiles, ntiles, grid;
  int ksteps, kord, lds_bytes, m32;
  int reserved[2];
} effdet_conv_plan_info_t;

int effdet_conv2d_plan_info(const effdet_conv_t* p, effdet_conv_plan_info_t* info);

#ifdef __cplusplus
}
#endif
#endif /* EFFDET_CONV_PLAN_H */
