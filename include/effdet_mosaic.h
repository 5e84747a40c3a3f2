/* effdet_mosaic.h -- Mosaic and MixUp of libeffdet_hip.so: the multi-image first stage of the 'train' augmentation.  It composes a
 * batch of B uint8 source images (the layout src / src_off / src_hw of effdet_augment_train) into B images of S x S uint8 RGB with
 * their boxes; the chain of effdet_augment_train / effdet_augment_boxes then runs on those exactly as if they were dataset images.
 * Entry points added to ABI generation 11 after effdet_hip.h's own set; its conventions (device pointers, 0 or a negative EFFDET_E*
 * code, work enqueued on `stream`) hold here.  A library of the same generation built before this header lacks the two symbols, so a
 * binding looks them up by name first.
 *
 * The reference has neither transform; the semantics are this project's, stated here and restated in tests/mosaic_restated.py.
 *
 * The parameter table is [B, EFFDET_MOSAIC_P] fp32, one row per OUTPUT image b, drawn on the host.  Columns:
 *     on, cx, cy, src0, src1, src2, src3, side0, side1, side2, side3, mix, mix_src, lam
 * Every column is integer-valued except lam.
 *
 * on == 0, pass-through.  The output is source image b through LongestMaxSize(S), then padded centrally with ZEROS to S x S: byte for
 *   byte the stage 'a' that the chain makes itself.  The boxes are scaled and shifted the same way.  The rest of the row is ignored.
 *
 * on == 1, mosaic.  The canvas is S x S and `fill` (a launch argument) is the background.  Windows, written x-range x y-range, with
 *   0 <= cx, cy <= S (a window may be empty):
 *     quadrant 0 = TL  [0,cx) x [0,cy)        quadrant 1 = TR  [cx,S) x [0,cy)
 *     quadrant 2 = BL  [0,cx) x [cy,S)        quadrant 3 = BR  [cx,S) x [cy,S)
 *   Quadrant q shows source src_q resized to (rh, rw) = lms_dims(h, w, side_q), 1 <= side_q <= S (LongestMaxSize's rule: scale =
 *   side / max(h, w), both sides rounded half to even).  The resized image is placed so that its corner nearest the centre lies on
 *   the centre; its origin (ox, oy) is
 *     TL (cx - rw, cy - rh)     TR (cx, cy - rh)     BL (cx - rw, cy)     BR (cx, cy).
 *   A window pixel (x, y) inside [ox, ox+rw) x [oy, oy+rh) is the bilinear sample at (y - oy, x - ox) of the (h, w) -> (rh, rw)
 *   resize, by the chain's rule: half-pixel centres, edge clamp, fp32 blend, round half up.  So rh == h and rw == w is an exact copy.
 *   Any other window pixel is `fill`.  What the window does not cover of the image is cropped.
 *
 * mix == 1, allowed only with on == 1.  The partner P is source mix_src through LongestMaxSize(S), padded centrally with `fill`.
 *   Every output channel is round_u8((float)m * lam + (float)p * (1.f - lam)), m the mosaic byte and p the partner byte; the two
 *   products are rounded separately, then added (the file is compiled without contraction); round_u8 rounds half up.  0 <= lam <= 1.
 *
 * Boxes.  Each pascal_voc box (x1, y1, x2, y2, label) is mapped in fp64 through its source's geometry,
 *     bx * (rw/w, rh/h, rw/w, rh/h) + (ox, oy, ox, oy),
 *   then clipped: a quadrant box to its QUADRANT WINDOW, not the canvas; a pass-through or partner box to the canvas.  The filter is
 *   the chain's (albumentations filter_bboxes): a box is dropped if its unclipped area is 0, or clipped / unclipped < min_visibility,
 *   or its clipped area <= min_area.  Output rows are the kept boxes of TL, TR, BL, BR and then the partner, each in input order;
 *   -1 rows follow, and counts[b] is written.  The label column is copied through; input rows with label -1 are padding and are
 *   skipped.  The output holds 5 * M rows for M input rows per image, so no case can overflow.
 *
 * Domain.  src_* are indices into THIS batch, [0, B); the kernels clamp them into it before any address is formed (and cx, cy into
 *   [0, S], side_q into [1, S]).  A resized side that rounds to 0 is outside the domain, as it already is for the chain. */
#ifndef EFFDET_MOSAIC_H
#define EFFDET_MOSAIC_H
#include "effdet_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

enum {
  EFFDET_MOSAIC_ON = 0, EFFDET_MOSAIC_CX, EFFDET_MOSAIC_CY, EFFDET_MOSAIC_SRC0, EFFDET_MOSAIC_SRC1, EFFDET_MOSAIC_SRC2,
  EFFDET_MOSAIC_SRC3, EFFDET_MOSAIC_SIDE0, EFFDET_MOSAIC_SIDE1, EFFDET_MOSAIC_SIDE2, EFFDET_MOSAIC_SIDE3, EFFDET_MOSAIC_MIX,
  EFFDET_MOSAIC_MIX_SRC, EFFDET_MOSAIC_LAM
};
#define EFFDET_MOSAIC_P 14                         /* columns of the table */

/* src: the concatenated uint8 HWC RGB images, image b at src + src_off[b] with (h, w) = src_hw[2b], src_hw[2b+1]; out: [B][S][S][3]
 * uint8.  EFFDET_EINVAL: a NULL pointer, S < 8, S * S > 2^30, B < 1, B > 65535 or fill outside [0, 255]; nothing is launched then. */
int effdet_mosaic_compose(const unsigned char* src, const long long* src_off, const int* src_hw, const float* table,
                          int B, int S, int fill, unsigned char* out, effdet_stream_t stream);
/* annots: [B][M][5] fp32 of the SOURCE images; out: [B][M_out][5] fp32, counts: [B].  EFFDET_EINVAL: a NULL pointer, M < 1,
 * M_out < 5 * M, S < 8 or B < 1; nothing is launched then. */
int effdet_mosaic_boxes(const int* src_hw, const float* table, int B, int S, const float* annots, int M,
                        float min_area, float min_visibility, float* out, int M_out, int* counts, effdet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EFFDET_MOSAIC_H */
