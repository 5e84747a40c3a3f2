/* effdet_slices.h -- sliced inference of libeffdet_hip.so: an image larger than the network's input is cut into overlapping
 * network-sized tiles on the device (effdet_slice_images), every tile goes through the detector, and the tiles' detection lists are
 * moved back into the image frame and merged (effdet_slice_merge) -- greedy suppression (NMS) or greedy merging (NMM) under IoU or
 * intersection-over-smaller, the scheme of SAHI (Akyon et al.).  Entry points added to ABI generation 11 after effdet_hip.h's own
 * set; its conventions (device pointers, 0 or a negative EFFDET_E* code, work enqueued on `stream`) hold here.  A library of the same
 * generation built before this header lacks the three symbols, so a binding looks them up by name first.
 *
 * The reference has no such path; the semantics are this project's, stated here and restated in tests/slices_restated.py.
 *
 * Tile table.  A device array of T records effdet_slice_tile_t {int x0, y0; float mx, my;}, 16-byte aligned, the same for every image
 *   of the batch: tile j shows the image from column x0 and row y0 on; a detection at (x, y) of the tile is at (x * mx + x0,
 *   y * my + y0) of the image.  A slice tile has mx = my = 1; a down-scaled view of the whole image has x0 = y0 = 0 and mx = W / w,
 *   my = H / h.  effdet_slice_images reads x0 and y0 only.
 *
 * ---- effdet_slice_images: the tile extractor
 * Source.  As effdet_resample_t's: EFFDET_RESAMPLE_NCHW: dense fp32 [B][3][H][W].  EFFDET_RESAMPLE_NHWC: element (b, y, x, c) of
 *   dtype `dtype` at src + b * src_bstride + (y * W + x) * src_ld + c (in elements), c = 0..C-1 with C >= 3; channels past the third
 *   are never used (the fourth may be loaded where the map has one), and no address outside a pixel's C elements is formed.  H and W
 *   are arbitrary: multiples of nothing.
 * Tiles.  The flat tile index is image-major, t = b * T + j; the call extracts the tiles t0 <= t < t1, each h x w.
 * Output.  Dense [t1 - t0][h][w][CE] of dtype `dtype`, CE = one 16-byte chunk (4 fp32 / 8 bf16).  Pixel (oy, ox) of flat tile t is
 *       src(b, clamp(y0 + oy, 0, H - 1), clamp(x0 + ox, 0, W - 1))          (y0 + oy and x0 + ox as exact integers, then clamped)
 *   channels 0..2 copied BIT FOR BIT (NaN payloads, Inf and -0 included), channels 3..CE-1 written as +0.  Every output element is
 *   written; nothing else is.  The clamp is part of the contract: no content of the table can form an address outside the source.
 *
 * ---- effdet_slice_merge: the cross-tile merge
 * Input.  One set of lists in the layout the NMS stage emits, narrowed to R columns: score [B][TPI][R] fp32, label [B][TPI][R]
 *   int64, boxes [B][TPI][R][4] fp32 (x1, y1, x2, y2 in the tile's frame), count [B][TPI] int32, and the tile table of TPI records.
 *   Rows of a list are score-descending; of list (b, j) the first min(max(count[b][j], 0), R) rows take part.
 * Semantics, per image, all in fp32, in this order of operations, nothing contracted into an FMA:
 *
 *  1. transform   x' = x * mx + (float)x0 for x1 and x2, y' = y * my + (float)y0 for y1 and y2 (multiply, then add: two roundings);
 *                 then x' = fmaxf(fminf(x', W), 0) and y' = fmaxf(fminf(y', H), 0).  A row takes part when score >= skip_thr, the
 *                 score is finite, its label is in [0, 65536), and the clipped box's area (x2' - x1') * (y2' - y1') is positive
 *                 and finite (so NaN scores and boxes that clip to nothing drop out).  The host cannot see the labels: a row whose
 *                 label is outside [0, 65536) drops out here, silently.
 *  2. order       the survivors by score descending (+0 before -0), then tile j ascending, then row ascending: a stable sort of the
 *                 tile-major rows on csrc/radix_sort.h's rs_score_key.
 *  3. metric      iw = fminf(ax2, bx2) - fmaxf(ax1, bx1), ih likewise; inter = iw * ih, and 0 when iw <= 0 || ih <= 0 -- effdet_nms's
 *                 rule.  EFFDET_SLICE_IOU: inter / (area_a + area_b - inter).  EFFDET_SLICE_IOS: inter / fminf(area_a, area_b).  Two
 *                 boxes match when metric > thr (a NaN never matches) and, with class_aware, their labels are equal.
 *  4. greedy pass candidates are taken in that order.  The next candidate that is still alive becomes a keeper; every later alive
 *                 candidate that matches the keeper's OWN transformed box dies.  Matching is never against a grown hull.
 *                 EFFDET_SLICE_NMS: the keeper is emitted as it is.  EFFDET_SLICE_NMM: the keeper's output box is the hull of itself
 *                 and everything it absorbed (fminf of x1 / y1, fmaxf of x2 / y2 -- order-independent, so exact however the work is
 *                 dealt); score and label are the keeper's.  The pass stops after max_det keepers.
 *  5. output      out_score [B][max_det], out_label [B][max_det] int64, out_boxes [B][max_det][4], out_count [B]: keepers in the
 *                 order they were emitted, which is score-descending; rows past the count are zero.  effdet_finalize_dets takes
 *                 them as they are.
 *
 * A key kernel and the shared radix sort order the rows; then one 1024-thread workgroup per image holds the sorted boxes (16 bytes)
 * and labels (2 bytes) in LDS, which is where the limit on TPI * R and on the labels comes from: 8192 * 18 bytes = 144 KiB of a
 * compute unit's 160 KiB, beside 1 KiB of reduction slots; which candidates are alive is a bit per candidate in its owner's
 * registers. */
#ifndef EFFDET_SLICES_H
#define EFFDET_SLICES_H
#include "effdet_hip.h"
#include "effdet_resample.h"
#ifdef __cplusplus
extern "C" {
#endif

enum { EFFDET_SLICE_NMS = 0, EFFDET_SLICE_NMM = 1 };   /* method */
enum { EFFDET_SLICE_IOU = 0, EFFDET_SLICE_IOS = 1 };   /* metric */
#define EFFDET_SLICE_MAX_TILES 1024                    /* TPI */
#define EFFDET_SLICE_MAX_IN 8192                       /* TPI * R: the candidates of an image live in one workgroup's LDS */

typedef struct {
  int x0, y0;                       /* the tile's origin in the image */
  float mx, my;                     /* tile frame -> image frame multipliers (1 for a slice) */
} effdet_slice_tile_t;

typedef struct {
  const void* src;                  /* NCHW: the [B][3][H][W] fp32 tensor; NHWC: element (0, 0, 0, 0) of the map */
  void* dst;                        /* [t1 - t0][h][w][CE], 16-byte aligned */
  const effdet_slice_tile_t* tiles; /* [T], 16-byte aligned */
  int src_layout;                   /* EFFDET_RESAMPLE_NCHW | EFFDET_RESAMPLE_NHWC */
  int dtype;                        /* EFFDET_F32 | EFFDET_BF16: of dst and of an NHWC src (an NCHW src is fp32 and takes EFFDET_F32) */
  int B, H, W;
  int C;                            /* NHWC only: channels of a source pixel, >= 3 */
  int T;                            /* tiles per image */
  int t0, t1;                       /* flat tile range, 0 <= t0 < t1 <= B * T */
  int h, w;                         /* tile size */
  long long src_ld, src_bstride;    /* NHWC only, in elements: pixel and image strides (src_ld >= C) */
} effdet_slice_images_t;

typedef struct {
  const float* score;               /* [B][TPI][R] */
  const long long* label;           /* [B][TPI][R] */
  const float* boxes;               /* [B][TPI][R][4], 16-byte aligned */
  const int* count;                 /* [B][TPI] */
  const effdet_slice_tile_t* tiles; /* [TPI], 16-byte aligned */
  int B, TPI, R;
  int method;                       /* EFFDET_SLICE_NMS | EFFDET_SLICE_NMM */
  int metric;                       /* EFFDET_SLICE_IOU | EFFDET_SLICE_IOS */
  int class_aware;                  /* 0 | 1 */
  int max_det;
  float W, H;                       /* the image's size: the clip */
  float thr, skip_thr;
  float* out_score;                 /* [B][max_det] */
  long long* out_label;             /* [B][max_det] */
  float* out_boxes;                 /* [B][max_det][4], 16-byte aligned */
  int* out_count;                   /* [B] */
} effdet_slice_merge_t;

/* p in HOST memory.  EFFDET_EINVAL: p, src, dst or tiles NULL, or dst or tiles not 16-byte aligned.  EFFDET_EUNSUPPORTED: a layout
 * or dtype other than the above (bf16 with NCHW included), B outside 1..65535, a side outside 1..32768 (H, W, h, w), T < 1, B * T
 * beyond an int, a range that is not 0 <= t0 < t1 <= B * T or longer than 65535 tiles, or an NHWC source with C < 3, src_ld < C or
 * src_bstride < 0.  Nothing is launched in either case. */
int effdet_slice_images(const effdet_slice_images_t* p, effdet_stream_t stream);

/* bytes of workspace for B images of TPI lists of R rows (the sort's buffers); 0 for arguments effdet_slice_merge refuses */
long long effdet_slice_merge_workspace_bytes(int B, int TPI, int R);
/* p in HOST memory.  TPI in 1..1024, R >= 1, TPI * R <= 8192, max_det in 1..TPI * R, method and metric 0..1, 0 <= thr <= 1, skip_thr
 * not NaN, W and H positive and finite: anything else is EFFDET_EUNSUPPORTED; a NULL or misaligned pointer, B < 1 or a workspace
 * smaller than effdet_slice_merge_workspace_bytes is EFFDET_EINVAL.  Nothing is launched in either case. */
int effdet_slice_merge(const effdet_slice_merge_t* p, void* workspace, long long workspace_bytes, effdet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EFFDET_SLICES_H */
