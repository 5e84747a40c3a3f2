/* effdet_affine.h -- the random affine / perspective warp of libeffdet_hip.so (YOLOv5's random_perspective): the stage between Mosaic
 * (effdet_mosaic.h) and the 'train' chain.  It turns each of B uint8 source images (the layout src / src_off / src_hw of
 * effdet_augment_train; a source is a dataset image of any (h, w) or a mosaic canvas) into one image of S x S uint8 RGB through a
 * 3 x 3 homography and carries the boxes along; the chain of effdet_augment_train / effdet_augment_boxes then runs on the outputs
 * exactly as if they were dataset images.  Entry points added to ABI generation 11 after effdet_hip.h's own set; its conventions
 * (device pointers, 0 or a negative EFFDET_E* code, work enqueued on `stream`) hold here.  A library of the same generation built
 * before this header lacks the two symbols, so a binding looks them up by name first.
 *
 * The reference has no such transform; the semantics are this project's, stated here and restated in tests/affine_restated.py.
 *
 * The parameter table is [B, EFFDET_AFFINE_P] fp64, one row per output image b (output b is made from source b), drawn on the host.
 * Columns:
 *     on, f0 .. f8, g0 .. g8, scale
 * F = (f0 .. f8) is the forward matrix, row-major, source pixel -> output pixel; G = (g0 .. g8) is its inverse, output -> source;
 * scale is the isotropic scale factor in F, which only the box filter uses.  The table is fp64 so that the pixels and the boxes of
 * one image see the same geometry to well inside the 1e-4 px bound of the box tests.
 *
 * on == 0, pass-through.  The output is source image b through LongestMaxSize(S), then padded centrally with ZEROS to S x S: byte for
 *   byte the stage 'a' that the chain makes itself and the pass-through of the mosaic stage (the same lms_dims, the same bilinear_u8).
 *   The boxes are scaled and shifted the same way, bx * (rw/w, rh/h, rw/w, rh/h) + (ox, oy, ox, oy) in fp64, and are NOT filtered:
 *   every row with a label is kept.  The rest of the row is ignored.
 *
 * on == 1, pixels.  Integer output coordinates are pixel centres: there is no half-pixel shift, as in cv2.warpPerspective.  For the
 *   output pixel (x, y), in fp64 and without contraction, every product rounded on its own and the sums taken left to right:
 *     d = (g6 * x + g7 * y) + g8,    u = ((g0 * x + g1 * y) + g2) / d,    v = ((g3 * x + g4 * y) + g5) / d.
 *   The pixel is `fill` (a byte, a launch argument) on all three channels if d is not finite or d <= 0, if u or v is not finite, or
 *   if u <= -1, u >= w, v <= -1 or v >= h.  Otherwise x0 = floor(u), y0 = floor(v), fx = (float)(u - x0), fy = (float)(v - y0), and
 *   the four taps are (y0, x0), (y0, x0 + 1), (y0 + 1, x0), (y0 + 1, x0 + 1).  A tap outside [0, h) x [0, w) has the value `fill`:
 *   the constant border, not an edge clamp.  The blend is the resize rule's (csrc/resize_u8.h, blend_u8): per channel
 *     top = p00 + fx * (p01 - p00),   bot = p10 + fx * (p11 - p10),   top + fy * (bot - top)   in fp32,
 *   then round half up and saturate.  So an identity G on an S x S source is an exact copy, and an integer translation is an exact
 *   shifted copy with a `fill` border.
 *
 * on == 1, boxes.  In fp64, the four corners (x1, y1), (x2, y1), (x1, y2), (x2, y2) of a pascal_voc box go through F with the
 *   perspective divide, in the pixels' order of operations:
 *     d = (f6 * x + f7 * y) + f8,    X = ((f0 * x + f1 * y) + f2) / d,    Y = ((f3 * x + f4 * y) + f5) / d.
 *   A box with a corner whose d is <= 0 or not finite is dropped.  The new box is the corners' min / max, clipped to [0, S].  With
 *   w2, h2 its sides and w1, h1 the source box's, it is kept iff
 *     w2 > wh_thr  and  h2 > wh_thr  and  max(w2 / (h2 + 1e-16), h2 / (w2 + 1e-16)) < ar_thr
 *     and  w2 * h2 / (w1 * h1 * scale * scale + 1e-16) > area_thr
 *   (YOLOv5's box_candidates; the three thresholds are launch arguments).
 *
 * Box output.  Kept rows come first in input order, -1 rows follow, and counts[b] is written.  The label column is copied through;
 *   input rows with label -1 are padding and are skipped.  The output holds M rows for M input rows: the stage never adds rows.
 *
 * Domain.  h, w >= 1 for every source; a pass-through side that rounds to 0 is outside the domain, as it already is for the chain.
 *   No address is formed from a tap that the rule above calls outside: the kernel reads only taps inside [0, h) x [0, w) of source
 *   b, for any table whatever. */
#ifndef EFFDET_AFFINE_H
#define EFFDET_AFFINE_H
#include "effdet_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

enum {
  EFFDET_AFFINE_ON = 0, EFFDET_AFFINE_F0, EFFDET_AFFINE_F1, EFFDET_AFFINE_F2, EFFDET_AFFINE_F3, EFFDET_AFFINE_F4, EFFDET_AFFINE_F5,
  EFFDET_AFFINE_F6, EFFDET_AFFINE_F7, EFFDET_AFFINE_F8, EFFDET_AFFINE_G0, EFFDET_AFFINE_G1, EFFDET_AFFINE_G2, EFFDET_AFFINE_G3,
  EFFDET_AFFINE_G4, EFFDET_AFFINE_G5, EFFDET_AFFINE_G6, EFFDET_AFFINE_G7, EFFDET_AFFINE_G8, EFFDET_AFFINE_SCALE
};
#define EFFDET_AFFINE_P 20                         /* columns of the table */

/* src: the concatenated uint8 HWC RGB images, image b at src + src_off[b] with (h, w) = src_hw[2b], src_hw[2b+1]; table: [B][P] fp64;
 * out: [B][S][S][3] uint8.  EFFDET_EINVAL: a NULL pointer, S < 8, S * S > 2^30, B < 1, B > 65535 or fill outside [0, 255]; nothing is
 * launched then. */
int effdet_affine_warp(const unsigned char* src, const long long* src_off, const int* src_hw, const double* table,
                       int B, int S, int fill, unsigned char* out, effdet_stream_t stream);
/* annots: [B][M][5] fp32 of the source images; out: [B][M][5] fp32, counts: [B].  EFFDET_EINVAL: a NULL pointer, M < 1, S < 8,
 * S * S > 2^30, B < 1 or B > 65535; nothing is launched then. */
int effdet_affine_boxes(const int* src_hw, const double* table, int B, int S, const float* annots, int M,
                        double wh_thr, double ar_thr, double area_thr, float* out, int* counts, effdet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EFFDET_AFFINE_H */
