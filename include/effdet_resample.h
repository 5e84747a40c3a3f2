/* effdet_resample.h -- the model-input resampler of libeffdet_hip.so: a batch that is already normalised (an NCHW fp32 tensor, or the
 * stem conv's NHWC layout in fp32 or bf16) is resized bilinearly to another resolution on the device, optionally mirrored left-right,
 * and comes out in the stem conv's input layout.  It makes the scaled views of test-time augmentation and the per-member input of a
 * mixed-size ensemble; the boxes of such a view go back through effdet_wbf's multiplier.  Entry point added to ABI generation 11
 * after effdet_hip.h's own set; its conventions (device pointers, 0 or a negative EFFDET_E* code, work enqueued on `stream`) hold
 * here.  A library of the same generation built before this header lacks the symbol, so a binding looks it up by name first.
 *
 * The reference has no such transform; the semantics are this project's, stated here and restated in tests/resample_restated.py.
 *
 * Source.  EFFDET_RESAMPLE_NCHW: dense fp32 [B][3][H][W].  EFFDET_RESAMPLE_NHWC: element (b, y, x, c) of dtype `dtype` at
 *   src + b * src_bstride + (y * W + x) * src_ld + c (in elements), c = 0..C-1 with C >= 3; channels past the third are never used
 *   (the fourth may be loaded where the map has one), and no address outside a pixel's C elements is formed.
 * Output.  Dense [B][Ho][Wo][CE] of dtype `dtype`, CE = one 16-byte chunk (4 fp32 / 8 bf16): channels 0..2 are the result, channels
 *   3..CE-1 are written as +0.  Every output element is written; nothing else is.
 *
 * Geometry, per axis (n_src source samples, n_dst output samples, output index o), the rule of lin_axis_ratio in csrc/resize_u8.h:
 *     s  = (float)(((double)o + 0.5) * ((double)n_src / (double)n_dst) - 0.5)        the fp64 expression as written, rounded ONCE to fp32
 *     i0 = floor(s),  f = s - (float)i0                                               (fp32)
 *     i0 < 0            ->  i0 = 0,          f = 0
 *     i0 >= n_src - 1   ->  i0 = n_src - 1,  f = 0
 *     i1 = min(i0 + 1, n_src - 1)
 *   giving (y0, y1, fy) from (oy, H, Ho) and (x0, x1, fx) from (ox, W, Wo).  There is NO antialiasing: a downscale samples the same
 *   four taps as an upscale and skips the pixels between them (torch's interpolate(..., antialias=False), not a box or area filter).
 *
 * Blend, per channel, in fp32, in this order, nothing contracted into an FMA (p00 = src(y0, x0), p01 = src(y0, x1), p10 = src(y1, x0),
 * p11 = src(y1, x1)):
 *     top = p00 + fx * (p01 - p00)
 *     bot = p10 + fx * (p11 - p10)
 *     R   = top + fy * (bot - top)
 *   bf16 taps are widened exactly to fp32 first and R is rounded to bf16 round-to-nearest-even.  So H == Ho leaves the rows as they
 *   are (fy = 0 and finite taps give top + 0 * (bot - top) = top).
 *
 * Non-finite taps propagate by that arithmetic and nothing is special-cased; a tap with f = 0 still takes part.  For an Inf tap that
 *   gives: p00 = Inf -> top = Inf + fx * (p01 - Inf) is NaN for every fx (0 * -Inf and Inf - Inf are both NaN), so R is NaN; p01 =
 *   Inf alone -> top is Inf (fx > 0) or NaN (fx = 0), and R = top + fy * (bot - top) is NaN either way; p10 = Inf -> bot is NaN, R
 *   is NaN; only p11 = Inf alone with fx > 0 and fy > 0 gives bot = Inf and R = that Inf.  At a clamped edge two taps are the same
 *   element, so an Inf there is NaN.  A NaN tap gives NaN.  Sign and payload of a NaN result are not part of the contract.
 *
 * flip != 0.  The output is the resampled image mirrored left-right: out(b, oy, ox) = R(b, oy, Wo - 1 - ox) -- resample first, then
 *   mirror, so the bits are those of the unmirrored result in another place.
 *
 * Limits.  Isotropy is not required here (H -> Ho and W -> Wo are independent); the callers in ops.py keep both ratios equal. */
#ifndef EFFDET_RESAMPLE_H
#define EFFDET_RESAMPLE_H
#include "effdet_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

enum { EFFDET_RESAMPLE_NCHW = 0, EFFDET_RESAMPLE_NHWC = 1 };   /* src_layout */

typedef struct {
  const void* src;                  /* NCHW: the [B][3][H][W] fp32 tensor; NHWC: element (0, 0, 0, 0) of the map */
  void* dst;                        /* [B][Ho][Wo][CE], 16-byte aligned */
  int src_layout;                   /* EFFDET_RESAMPLE_NCHW | EFFDET_RESAMPLE_NHWC */
  int dtype;                        /* EFFDET_F32 | EFFDET_BF16: of dst and of an NHWC src (an NCHW src is fp32 and takes EFFDET_F32) */
  int B, H, W, Ho, Wo;
  int C;                            /* NHWC only: channels of a source pixel, >= 3 */
  int flip;                         /* 0 | 1 */
  long long src_ld, src_bstride;    /* NHWC only, in elements: pixel and image strides (src_ld >= C) */
} effdet_resample_t;

/* p in HOST memory.  EFFDET_EINVAL: p, src or dst NULL, or dst not 16-byte aligned.  EFFDET_EUNSUPPORTED: a layout or dtype other
 * than the above (bf16 with NCHW included), flip outside {0, 1}, B outside 1..65535, a side outside 1..32768 (H, W, Ho, Wo), or an
 * NHWC source with C < 3, src_ld < C or src_bstride < 0.  Nothing is launched in either case. */
int effdet_resample_images(const effdet_resample_t* p, effdet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EFFDET_RESAMPLE_H */
