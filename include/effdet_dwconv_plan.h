/* effdet_dwconv_plan.h -- a host-only query of the depthwise-conv launch plans of libeffdet_hip.so: an entry point added to ABI
 * generation 11 after effdet_hip.h's own set (effdet_hip.h documents the depthwise entry points and their geometry arguments; a
 * library of the same generation built before this header lacks the symbol, so a binding looks it up by name before the first call).
 *
 * effdet_dwconv_plan_info answers "what would the entry point of `kind` launch for this geometry": it runs the planner that entry
 * point runs and copies the decision out.  No device work and no HIP runtime call, like effdet_conv2d_kernel and
 * effdet_conv2d_wgrad_kernel.  Tests use it to prove which kernel path a shape reaches (tiles per workgroup, one or two tile buffers,
 * a ragged last run) instead of restating the planner.
 *
 * kind: EFFDET_DW_PLAN_FWD effdet_dwconv_fwd, _DGRAD effdet_dwconv_dgrad, _WGRAD effdet_dwconv_wgrad, _BWD effdet_dwconv_bwd,
 * _EXPAND_FWD effdet_mbconv_expand_dw_fwd (C = Cexp, dtype = EFFDET_F32, Cin = the block's input channels; Cin is ignored by the
 * other kinds).  dtype .. Wo: as the entry point takes them.
 * info: EFFDET_DW_INFO_COUNT ints, indexed by the EFFDET_DW_INFO_* names:
 *   CQ      16-byte channel chunks per slab (4 or 8)
 *   TPI     tiles per image of the kernel's tile walk
 *   PPT     tiles one workgroup walks (the direct weight-gradient kernel: pixels per thread)
 *   NBUF    LDS tile buffers: 2 = the next tile of a run is prefetched under the taps, 1 = restaged behind a barrier
 *   GROUPS  tile groups (workgroups per slab) per image = ceil(TPI / PPT): rows per image of the pool partial sums [B][GROUPS][C] and
 *           of the weight-gradient slabs
 *   NSLAB   channel slabs
 *   DIRECT  1 when the weight gradient takes the direct kernel (maps of <= 16 outputs): CQ = TPI = NBUF = 0 then
 * Returns EFFDET_OK, or the code the entry point itself returns for the geometry (EFFDET_EINVAL, EFFDET_EUNSUPPORTED; _BWD:
 * EFFDET_EUNSUPPORTED where the fused backward does not serve the geometry); info is written only on EFFDET_OK. */
#ifndef EFFDET_DWCONV_PLAN_H
#define EFFDET_DWCONV_PLAN_H
#include "effdet_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

enum { EFFDET_DW_PLAN_FWD = 0, EFFDET_DW_PLAN_DGRAD = 1, EFFDET_DW_PLAN_WGRAD = 2, EFFDET_DW_PLAN_BWD = 3, EFFDET_DW_PLAN_EXPAND_FWD = 4 };
enum { EFFDET_DW_INFO_CQ = 0, EFFDET_DW_INFO_TPI = 1, EFFDET_DW_INFO_PPT = 2, EFFDET_DW_INFO_NBUF = 3, EFFDET_DW_INFO_GROUPS = 4,
       EFFDET_DW_INFO_NSLAB = 5, EFFDET_DW_INFO_DIRECT = 6, EFFDET_DW_INFO_COUNT = 7 };

int effdet_dwconv_plan_info(int kind, int dtype, int B, int H, int W, int C, int k, int stride, int pad_t, int pad_l,
                            int Ho, int Wo, int Cin, int* info);

#ifdef __cplusplus
}
#endif
#endif /* EFFDET_DWCONV_PLAN_H */
