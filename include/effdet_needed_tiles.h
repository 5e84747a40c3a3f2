/* effdet_needed_tiles.h -- sparse regression-tower FORWARD of libeffdet_hip.so: entry points added to ABI generation 11 after
 * effdet_live_tiles.h's set (effdet_hip.h's conventions hold: device pointers, 0 or a negative EFFDET_E* code, kernels enqueued on
 * `stream`, no memset / copy / host sync, so every call may be captured in a graph).  A library of the same generation built before
 * this header lacks the symbols, so a binding looks them up by name before the first call.
 *
 * In training the regression output of the RetinaHead is read at the positive anchors only (the box term of the loss and its
 * gradient), and which anchors are positive follows from the anchors and the annotations alone -- it is known before the head runs.
 * Let pos be the pixels (image, level, h, w) with at least one positive anchor.  retina_reg's output is needed on pos, the output of
 * reg_convs.3 on dilate(pos, 1) (a 3x3, stride 1, pad 1 conv reads its input within Chebyshev distance 1), reg_convs.2 on
 * dilate(pos, 2), ... reg_convs.0 on dilate(pos, 4) -- the geometry of effdet_live_tiles.h's flags, read forwards.  A layer that
 * computes every 128-pixel tile holding a needed pixel gives every needed pixel its dense value (induction over the layers, the pyramid
 * input being dense); every other tile is written as zeros.  Pixels of a computed tile outside the needed set may then differ from the
 * dense ones (they saw zeros where the dense pass saw values): finite, deterministic, and read by nobody whose result counts. */
#ifndef EFFDET_NEEDED_TILES_H
#define EFFDET_NEEDED_TILES_H
#include "effdet_live_tiles.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The positive-pixel map of the default matcher (effdet_focal_loss_fwd's assign pass: an image with at least one valid annotation,
 * IoU with the first arg-max annotation >= 0.5): map[pixel] = 1 iff one of the pixel's 9 anchors is positive, else 0, in the layout
 * of effdet_live_tiles' per-pixel scratch map -- level-major, level l holding its B * H[l] * W[l] pixels in (b, h, w) order.
 * anchors [A][4] with A = 9 * sum_l H*W (anchor 9 * pixel + k, pixels level-major within an image), annots [B][N][5] (label -1 = pad
 * row).  Every byte is written, by one plain store. */
int effdet_positive_pixel_map(const float* anchors, const float* annots, int B, long long A, int N, int nlev, const int* H,
                              const int* W, unsigned char* map, effdet_stream_t stream);

/* effdet_live_tiles' flags from a caller-supplied per-pixel byte map (non-zero byte = non-zero pixel; the layout above) instead of
 * from d(reg): the same live32 [6][steps] / live128 [6][tiles] arrays, radii and scratch (2 * `pixels` bytes; map may be its first
 * half). */
int effdet_live_tiles_from_map(const unsigned char* map, int B, int nlev, const int* H, const int* W, unsigned char* scratch,
                               unsigned char* live32, unsigned char* live128, effdet_stream_t stream);

/* effdet_conv2d with "needed" flags: needed[mt - needed_tile0] == 0 marks the 128-pixel tile mt (segments in order, each rounded up to
 * whole tiles) as one whose result nobody reads; tiles below needed_tile0 carry no flag and are computed (a paired launch whose first
 * segments are another conv).  A tile that is not needed is not computed: its rows of every output stream (y in the H-split layout or,
 * with out_f32, fp32; y_split) are written as zero bytes, whatever bias or activation the descriptor names.  Honoured only by the
 * EFFDET_F32_HSPLIT 128-pixel-tile kernels (ids 30, 31); everywhere else the flags are ignored and the launch is the dense one. */
int effdet_conv2d_needed(const effdet_conv_t* p, const unsigned char* needed, int needed_tile0, effdet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EFFDET_NEEDED_TILES_H */
