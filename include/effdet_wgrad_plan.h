/* effdet_wgrad_plan.h -- a host-only query of the weight-gradient launch plan of libeffdet_hip.so: an entry point added to ABI
 * generation 11 after effdet_hip.h's own set (effdet_hip.h documents effdet_wgrad_t; a library of the same generation built before this
 * header lacks the symbol, so a binding looks it up by name before the first call).
 *
 * effdet_conv2d_wgrad_plan_info answers "what would effdet_conv2d_wgrad launch for this descriptor": it runs the planner the launch
 * runs and copies the decision out of the plan the launch itself reads.  No device work and no HIP runtime call, like
 * effdet_conv2d_wgrad_splits / _kernel / _seg_slabs, whose answers it repeats (splits, path, first / count) and completes with the
 * length of a split-K range and the shape of the grid.  Tests use it to prove how many ranges a level is cut into, how many pipeline
 * stages a range runs and how many workgroups the launch has, instead of restating the planner.
 *
 * info (written only when the return value is >= 0):
 *   path          EFFDET_WGRAD_PATH_TILED  the 128 x 128 tile kernels: the DMA-staged one (exact fp32, bf16x3 or bf16) for the first
 *                                          nfast slabs, the register-transpose one for the levels it cannot take
 *                 EFFDET_WGRAD_PATH_THIN   the thin pointwise kernel (few channels, many pixels)
 *                 EFFDET_WGRAD_PATH_SPLIT  the split-layout kernel (EFFDET_F32_SPLIT operands, three bf16 products)
 *                 EFFDET_WGRAD_PATH_STEM   the thin kernel's stem form (effdet_conv2d_wgrad_kernel reports it as 1)
 *   splits        slabs (split-K ranges) of the launch, all levels
 *   nfast         TILED: slabs of the DMA-staged launch (the register-transpose launch owns the other splits - nfast); else = splits
 *   mchunk        pixels per split-K range; range r of a level of M pixels covers [r * mchunk, min(M, (r + 1) * mchunk))
 *   ntiles, jtiles   output-channel tiles and (tap, channel) tiles of a slab: the main launch has ntiles * jtiles * nfast workgroups
 *                 (THIN / STEM: one workgroup per slab, both 1)
 *   stage_pixels  pixels per pipeline stage of the main launch: 32 (fp32 storage and the split layout) or 64 (bf16); THIN / STEM: P
 *   allr          SPLIT: 1 = all fragment reads of a K-step are issued ahead of its MFMAs (the other template instance)
 *   thin_ns       THIN / STEM: ring slots; else 0
 *   gate          the kernels' operand-gate form; 0 from this query (effdet_conv2d_wgrad_gated_kernel answers for gated launches)
 *   nseg          levels of the descriptor
 *   first, count  per level l < nseg: its slabs are first[l] .. first[l] + count[l] - 1 (effdet_conv2d_wgrad_seg_slabs)
 * Returns the path (>= 0), or the negative code effdet_conv2d_wgrad returns for the descriptor (EFFDET_EINVAL, EFFDET_EUNSUPPORTED);
 * EFFDET_EINVAL for info == NULL. */
#ifndef EFFDET_WGRAD_PLAN_H
#define EFFDET_WGRAD_PLAN_H
#include "effdet_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

enum { EFFDET_WGRAD_PATH_TILED = 0, EFFDET_WGRAD_PATH_THIN = 1, EFFDET_WGRAD_PATH_SPLIT = 2, EFFDET_WGRAD_PATH_STEM = 3 };

typedef struct effdet_wgrad_plan_info_t {
  int path, splits, nfast, mchunk;
  int ntiles, jtiles, stage_pixels;
  int allr, thin_ns, gate, nseg;
  int first[EFFDET_MAX_SEG], count[EFFDET_MAX_SEG];
  int reserved[3];
} effdet_wgrad_plan_info_t;

int effdet_conv2d_wgrad_plan_info(const effdet_wgrad_t* p, effdet_wgrad_plan_info_t* info);

#ifdef __cplusplus
}
#endif
#endif /* EFFDET_WGRAD_PLAN_H */
