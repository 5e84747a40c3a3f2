/* effdet_wgrad_pair.h -- two weight gradients of one geometry as one launch: an entry point added to ABI generation 11 of
 * libeffdet_hip.so after effdet_hip.h's own set (its conventions hold: device pointers, 0 or a negative EFFDET_E* code, kernels enqueued
 * on `stream`, no allocation / memset / copy / host sync, so the call may be captured in a graph).  A library of the same generation
 * built before this header lacks the symbol, so a binding looks it up by name before the first call.
 *
 * Layer t of the RetinaHead's two towers has two weight gradients of the same shape.  The regression tower's walks only the live
 * 32-pixel steps of every split-K range (effdet_live_tiles.h), but the ranges of the coarse pyramid levels are almost entirely live and
 * are dispatched last, so the flagged launch lasts about as long as one dense range started after the sparse ones.  As ONE grid with
 * the classification tower's dense launch the long ranges start at once and the dense blocks fill every slot behind them. */
#ifndef EFFDET_WGRAD_PAIR_H
#define EFFDET_WGRAD_PAIR_H
#include "effdet_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* effdet_conv2d_wgrad(a) and effdet_conv2d_wgrad(b) -- or, with live32_b, effdet_conv2d_wgrad_live(b, live32_b) -- as one launch.
 * Both descriptors must be EFFDET_F32_SPLIT problems with equal B, Cin, Cout, taps, stride, pads, ldx and lddz whose own plans cut
 * split-K ranges of the same length (EFFDET_EUNSUPPORTED otherwise, nothing launched); their levels and tensors may differ.  Each is
 * planned exactly as on its own: same ranges, same slab order, slabs and bias rows bit for bit those of the separate launches.
 * workspace: a's slabs and bias partial rows in effdet_conv2d_wgrad's layout, b's behind them at byte offset
 * effdet_conv2d_wgrad_workspace_bytes(a); workspace_bytes >= the sum of both.  live32_b: NULL (both dense) or b's step flags as for
 * effdet_conv2d_wgrad_live; the dense problem never reads flags. */
int effdet_conv2d_wgrad_pair(const effdet_wgrad_t* a, const effdet_wgrad_t* b, void* workspace, long long workspace_bytes,
                             const unsigned char* live32_b, effdet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EFFDET_WGRAD_PAIR_H */
