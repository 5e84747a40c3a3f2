/* effdet_draw.h -- the device renderer of libeffdet_hip.so: boxes, optional translucent fills and text labels painted into uint8 RGB
 * frames straight from finalize_dets' rows or the tracker's rows (csrc/draw.hip; ops.draw_detections, evaluate.Annotator).  Entry points
 * added to ABI generation 11 after effdet_hip.h's, effdet_track.h's and effdet_assign.h's sets; their conventions (device pointers, 0 or
 * a negative EFFDET_E* code, work enqueued on `stream`) hold here.  A library of the same generation built before this header lacks the
 * symbols, so a binding looks them up by name first.
 *
 * One launch per call, nothing read back, no atomics, every pixel read at most once and written at most once by one thread: two calls
 * on equal input give equal bytes, and painting in place is safe.  Parity with cv2 is no goal (its Hershey font cannot be pinned); the
 * rule below is the project's own and tests/draw_restated.py restates it as a sequential painter.
 *
 * ---- the rule
 * Frame b is H x W pixels of 3 bytes (R, G, B), rows tightly packed (W * 3 bytes, so a row start is only byte-aligned):
 *   (H, W) = pix_hw[b] or (Hmax, Wmax) without pix_hw; it starts at pixels + pix_off[b], or pixels + b * Hmax * Wmax * 3 without pix_off.
 *   pix_hw[b] must not exceed (Hmax, Wmax): the grid covers Hmax x Wmax, and a frame with H < 1 or W < 1 is left alone.
 * Its rows are k = 0 .. min(max(counts[b], 0), K) - 1 of rows[b][k][row_stride] (fp32: x1, y1, x2, y2, score, label, ...).
 *
 * Coordinates.  v = (x1 * sx, y1 * sy, x2 * sx, y2 * sy) in fp32, one rounding each; (sx, sy) = box_scale[b], or 1 without box_scale.
 *   The row is SKIPPED when one of the four is not finite, or when its label column is < 0 (the padding rows) or NaN.  Each value is
 *   clamped to [-2^20, 2^20] and converted toward zero: X1, Y1, X2, Y2 (the demo's int(bbox[i] * origin / size)).  The row is skipped
 *   when X2 < X1 or Y2 < Y1.  The integer label is L = (int)min(label, 2147483520.0f) (the largest fp32 below 2^31).
 * Colour.  c = palette[key mod P] with the remainder taken non-negative; key = L, or ids[b][k] with color_by_id.  palette: uint8 [P][3].
 * Fill (fill_alpha = a > 0).  Every pixel p of [X1, X2] x [Y1, Y2] (inclusive) becomes (c * a + p * (255 - a) + 127) / 255 per
 *   channel, in integer division.
 * Outline (thickness = t > 0, o = t / 2).  Every pixel inside [X1 - o, X2 + o] x [Y1 - o, Y2 + o] and outside the hole
 *   [X1 - o + t, X2 + o - t] x [Y1 - o + t, Y2 + o - t] becomes c; when the hole's bounds cross on either axis there is no hole and the
 *   whole outer rectangle is painted.
 * Label (label != 0).  Text = ['#' id ' '] name [' ' pct]: the id part with show_id, the pct part with show_score.
 *   id   = max(ids[b][k], 0) in decimal.
 *   name = the name_len[L] bytes of names[L] when L < n_names, else L in decimal.
 *   pct  = 0 when the score is not finite; else with f = score * 100 + 0.5 (fp32, each operation rounded once): 0 when f <= 0, 100 when
 *          f >= 100, else (int)f -- clamp((int)(score * 100 + 0.5), 0, 100).
 *   A byte outside 0x20..0x7E prints as '?'.  The text has n <= EFFDET_DRAW_TEXT_MAX = 1 + 10 + 1 + 16 + 1 + 3 characters.
 *   With text scale s: the label rectangle is 6 * s * n + s wide and 9 * s tall; glyph j occupies the cell of 6s x 8s starting at
 *   (Lx + s + 6 * s * j, Ly + s); glyph bit (row r, column c) is the s x s square at (+ c * s, + r * s) of its cell.
 *   Position: Lx = X1 - o, Ly = Y1 - o - 9s; when Ly < 0, Ly = Y1 - o + t (inside the box, where YOLOv5's Annotator puts it); then
 *   Lx = max(min(Lx, W - width), 0).  The rectangle is c; set glyph pixels are black (0, 0, 0) when
 *   299 * R + 587 * G + 114 * B >= 128000 of c, else white (255, 255, 255).
 * Order.  The result equals painting sequentially: for k ascending, the fill and then the outline of row k; after all of those, for k
 *   ascending, the label of row k.  Later paint covers earlier paint; a fill blends with whatever is below it.  Everything is clipped to
 *   the frame.  Bytes outside the B frames are never written, and a pixel no primitive touches is not written at all.
 *
 * ---- the font
 * 95 glyphs of 5 columns x 8 rows for the codes 0x20..0x7E (a 5 x 7 face; row 7 holds the descenders).  effdet_draw_glyph returns one
 * as 40 bits: row r (0 = top) is bits [5r, 5r + 5), and within a row bit 4 is the LEFTMOST column: bit (r, c) is 5r + 4 - c.
 *
 * ---- the kernel (csrc/draw.hip)
 * One workgroup of 256 threads per EFFDET_DRAW_TILE_W x EFFDET_DRAW_TILE_H pixel tile of one frame; grid = ceil(Wmax / TILE_W) x
 * ceil(Hmax / TILE_H) x B, tiles outside a smaller frame exit.  The sequential rule comes out of a gather: 256 rows at a time are
 * tested against the tile (their outline rectangle for the first layer, their label rectangle for the second), compacted in row order
 * into an LDS list with per-wave ballots, and every thread walks the list over its own pixels, which it keeps in registers. */
#ifndef EFFDET_DRAW_H
#define EFFDET_DRAW_H
#include "effdet_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define EFFDET_DRAW_MAX_ROWS 1024                      /* K */
#define EFFDET_DRAW_NAME_MAX 16                        /* bytes per class name */
#define EFFDET_DRAW_MAX_THICKNESS 16
#define EFFDET_DRAW_MAX_TEXT_SCALE 8
#define EFFDET_DRAW_TEXT_MAX 32                        /* characters of a label at most */
#define EFFDET_DRAW_TILE_W 64                          /* the workgroup's pixel tile */
#define EFFDET_DRAW_TILE_H 16
#define EFFDET_DRAW_MAX_SIDE 1048576                   /* Hmax, Wmax (2^20, the clamp of the coordinates) */
#define EFFDET_DRAW_MAX_BATCH 65535                    /* B (the grid's z extent) */

/* Paints in place (above).  names: uint8 [n_names][16], name_len: uint8 [n_names] (each <= 16); n_names = 0 (both may be NULL) prints
 * every label as its number.  pix_off, pix_hw, ids and box_scale may be NULL as stated above.
 * EFFDET_EINVAL: a NULL pixels, rows, counts or palette; B, K, Hmax or Wmax < 1; row_stride < 6; P < 1; n_names < 0, or n_names > 0
 * with a NULL names or name_len; color_by_id or show_id without ids; thickness < 0; fill_alpha outside 0..255; text_scale < 1.
 * EFFDET_EUNSUPPORTED: K > 1024, thickness > 16, text_scale > 8, Hmax or Wmax > 2^20, B > 65535.  EFFDET_EINVAL wins where both apply.
 * Nothing is enqueued in either case. */
int effdet_draw_detections(unsigned char* pixels, const long long* pix_off, const int* pix_hw, int B, int Hmax, int Wmax,
                           const float* rows, int row_stride, int K, const int* counts, const int* ids, const float* box_scale,
                           const unsigned char* names, const unsigned char* name_len, int n_names, const unsigned char* palette, int P,
                           int thickness, int fill_alpha, int label, int show_score, int show_id, int text_scale, int color_by_id,
                           effdet_stream_t stream);
/* Host only: the glyph of `code` (the font above); a code outside 0x20..0x7E returns the glyph of '?'. */
unsigned long long effdet_draw_glyph(int code);

#ifdef __cplusplus
}
#endif
#endif /* EFFDET_DRAW_H */
