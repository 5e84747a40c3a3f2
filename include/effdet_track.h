/* effdet_track.h -- multi-object tracking of libeffdet_hip.so: ByteTrack (Zhang et al., ECCV 2022) over the rows effdet_finalize_dets
 * writes, one independent tracker per image of the batch (B camera streams), state and outputs on the device, nothing read back.
 * Entry points added to ABI generation 11 after effdet_hip.h's own set; its conventions (device pointers, 0 or a negative EFFDET_E*
 * code, work enqueued on `stream`) hold here.  A library of the same generation built before this header lacks the four symbols, so a
 * binding looks them up by name first.
 *
 * The reference has no tracker (its camera mode draws every frame's boxes on their own); the semantics are this project's, stated here
 * and restated in tests/track_restated.py.  All arithmetic is fp32, every operation rounded once (nothing contracted); where an
 * expression below is written with parentheses, that is its order.
 *
 * ---- state
 * Per stream: frame_id, next_id, overflow (int32) and max_tracks slots.  A slot is FREE (0), UNCONFIRMED (1), TRACKED (2) or LOST (3)
 * and holds: id, tracklet_len, start_frame, last_frame (int32), score, label (fp32, the detection's label value as it came) and a
 * Kalman state of 8 means (cx, cy, a = w / h, h, and their velocities) and 12 covariance numbers (below).  After a reset a stream has
 * every slot FREE, frame_id = 0, next_id = 1, overflow = 0.  The state is opaque to a caller; its layout, for tests and tools: B
 * headers of 4 int32 (frame_id, next_id, overflow, 0), then [B][max_tracks] rows of EFFDET_TRACK_ROW_WORDS 32-bit words: mean[8],
 * (p, c, v)[4], score, label, state, id, tracklet_len, start_frame, last_frame, 0.  A FREE slot's row is all zero.
 *
 * ---- boxes
 * A detection (x1, y1, x2, y2) is measured as  w = x2 - x1, h = y2 - y1, z = (x1 + 0.5 * w, y1 + 0.5 * h, w / h, h).
 * A mean gives the box  w = a * h, x1 = cx - 0.5 * w, y1 = cy - 0.5 * h, x2 = x1 + w, y2 = y1 + h.
 * iou(A, B):  iw = min(A.x2, B.x2) - max(A.x1, B.x1), ih likewise; 0 when iw <= 0 or ih <= 0 (or either is a NaN); else
 *   inter = iw * ih, iou = inter / ((area(A) + area(B)) - inter), area = (x2 - x1) * (y2 - y1)   (postprocess.hip's expression).
 *
 * ---- Kalman filter (ByteTrack's: constant velocity on (cx, cy, a, h), position std h / 20, velocity std h / 160, the fixed terms of
 * the aspect ratio 1e-2, 1e-5 and 1e-1)
 * F couples coordinate i only with its own velocity and Q, R and the initial P are diagonal, so the 8 x 8 covariance never grows a
 * term between different coordinates: the filter is four independent two-state filters.  Coordinate i keeps (x, u) = (mean[i],
 * mean[4 + i]) and p = var(x), c = cov(x, u), v = var(u).  With h the mean's height BEFORE the step, sp = h / 20, su = h / 160:
 *   start    x = z_i, u = 0, c = 0; p = (2 * sp)^2, v = (10 * su)^2 with h = z_3; for i = 2 (a): p = 1e-4, v = 1e-10.
 *   predict  x = x + u;  p = ((p + c) + (c + v)) + sp^2;  c = c + v;  v = v + su^2;  for i = 2: sp = 1e-2, su = 1e-5.
 *   update   r = sp^2 (i = 2: 1e-2, the square of 1e-1), S = p + r, y = z_i - x;
 *            x = x + (p / S) * y;  u = u + (c / S) * y;  then with the OLD p and c:
 *            p = p - (p * p) / S;  c = c - (p * c) / S;  v = v - (c * c) / S.
 *   Squares are products s * s of the rounded fp32 s; the literals are the fp32 nearest to the decimal.
 *
 * ---- effdet_track_step, per stream b (one workgroup; streams do not interact)
 * Detections: rows r < min(max(counts[b], 0), max_det) of dets[b], x1, y1, x2, y2, score s, label.  A row is SKIPPED when a coordinate
 *   or the score is not finite, x2 <= x1 or y2 <= y1.  The others are HIGH (s >= track_thr), LOW (low_thr < s < track_thr) or ignored.
 * 0. frame_id += 1.
 * 1. Predict every UNCONFIRMED, TRACKED and LOST slot; a LOST slot's height velocity mean[7] is set to 0 first.  "Predicted box" below
 *    is the box of the mean after this step.
 * 2. (the split above)
 * 3. First association.  Rows: the TRACKED and LOST slots.  Columns: the HIGH detections.  sim = iou(predicted box, detection),
 *    times s when fuse_score; a pair is allowed when sim > match_sim and, with class_aware, the slot's label == the detection's
 *    (fp32 equality).
 * 4. Second association.  Rows: the TRACKED slots (as they were at step 3) that step 3 left unmatched.  Columns: the LOW detections.
 *    sim = the plain iou, allowed when sim > second_sim (and the labels, with class_aware).  A row left unmatched becomes LOST.
 * 5. Third association.  Rows: the UNCONFIRMED slots.  Columns: the HIGH detections step 3 left unmatched.  sim as in step 3, allowed
 *    when sim > unconfirmed_sim.  A matched slot becomes TRACKED; an unmatched one becomes FREE (its row zeroed).
 * Assignment in each association is GREEDY BY DESCENDING SIMILARITY: repeatedly the allowed pair with the largest sim among the rows
 *    and columns not yet matched is matched; among equal sims the lower detection row wins, then the lower slot.  (The published
 *    ByteTrack solves each association optimally by LAPJV; this is the stated deviation and the default.  csrc/track.hip keeps the
 *    similarity and the assignment as separate device functions so that another solver can replace the second: effdet_assign.h's
 *    effdet_track_step_assign(..., assignment = 1) is this step with the optimal assignment in its place.)
 * 6. Every match is a Kalman update of the slot with the detection's z; score and label become the detection's; last_frame =
 *    frame_id; tracklet_len += 1 -- except for a LOST slot matched in step 3, which becomes TRACKED with tracklet_len = 0 and keeps
 *    its id.
 * 7. New tracks.  The HIGH detections unmatched after step 5 with s >= new_thr, in row order, take the FREE slots (those free at this
 *    point, the ones step 5 freed included) in ascending slot order: the k-th such detection gets the k-th free slot, id = next_id + k,
 *    the started filter, its score and label, tracklet_len = 0, start_frame = last_frame = frame_id, and is TRACKED when frame_id == 1,
 *    UNCONFIRMED otherwise.  next_id advances by the number of tracks started; the detections beyond the free slots are dropped and
 *    overflow grows by their number (no id is spent on them).
 * 8. Removal.  A LOST slot with frame_id - last_frame > track_buffer becomes FREE.
 * 9. Duplicates (ByteTrack's remove_duplicate_stracks).  For every pair (T a TRACKED slot, L a LOST slot) after step 8 with
 *    iou(box of T's mean, box of L's mean) > 0.85: when frame_id - T.start_frame > frame_id - L.start_frame, L is marked, otherwise T
 *    (the younger one; on equal age the tracked one, as published).  All pairs are judged on the state after step 8; then every marked
 *    slot becomes FREE.  UNCONFIRMED slots take no part (the published code lets a track started this frame take part).
 * 10. Output.  The TRACKED slots in ascending id: out_rows[b][k] = x1, y1, x2, y2 of the mean's box, score, label,
 *    (float)tracklet_len, (float)(frame_id - start_frame); out_ids[b][k] = id; out_count[b] = their number.  Rows past the count are
 *    zero with id -1.  Every element of the three outputs is written on every call.
 * Ids are int32 and start at 1 per stream; 2^31 tracks of one stream are not expected.
 *
 * ---- the similarity matrix
 * max_tracks <= 256, max_det <= 128, one workgroup of 256 threads per stream.  Thread t OWNS slot t: the slot's Kalman state lives in
 * its registers for the whole step.  The detections sit in LDS (24 bytes a row, 3 KiB) and a pair's similarity is RECOMPUTED from the
 * two boxes when it is needed, not stored: a [256][128] fp32 matrix is 128 KiB, which fits a gfx950 CU's 160 KiB but would have to be
 * carved from dynamic LDS, filled (32 768 IoUs, most of them 0) and scanned row by row every frame, while the greedy rule needs, per
 * pick, only each row's current best column.  A thread therefore caches its row's best allowed column and rescans the columns still
 * free only when that column has just been taken by another row; rows whose best is untouched cost nothing per pick.  A pick is one
 * 64-bit key (sim bits, ~detection row, ~slot) per thread and one integer max over the workgroup.  No floating-point atomics, no
 * atomics at all: two calls on equal state and input give equal bits.  One launch per call; geometry follows from B alone. */
#ifndef EFFDET_TRACK_H
#define EFFDET_TRACK_H
#include "effdet_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define EFFDET_TRACK_MAX_TRACKS 256                    /* slots per stream */
#define EFFDET_TRACK_MAX_DET 128                       /* detection rows per stream */
#define EFFDET_TRACK_ROW_WORDS 28                      /* 32-bit words of a slot */

/* bytes of the device state of B streams of max_tracks slots (host only); 0 for B < 1 or max_tracks outside 1..256 */
long long effdet_track_state_bytes(int B, int max_tracks);
/* Resets the streams b with reset_mask[b] != 0 (int32 [B] on the device), every stream when reset_mask is NULL.
 * EFFDET_EUNSUPPORTED: max_tracks > 256.  EFFDET_EINVAL: a NULL state, B < 1 or max_tracks < 1.  Nothing is enqueued in either case. */
int effdet_track_reset(void* state, int B, int max_tracks, const int* reset_mask, effdet_stream_t stream);
/* One frame of every stream (above).  dets [B][max_det][6] fp32 + counts [B] int32 as effdet_finalize_dets writes them; out_rows
 * [B][max_tracks][8] fp32, out_ids [B][max_tracks] int32, out_count [B] int32.
 * EFFDET_EUNSUPPORTED: max_tracks > 256 or max_det > 128.  EFFDET_EINVAL: a NULL pointer; B, max_det or max_tracks < 1; a threshold
 * or similarity limit that is not finite; a similarity limit outside [0, 1]; low_thr > track_thr; track_buffer < 0.  Nothing is
 * enqueued in either case. */
int effdet_track_step(const float* dets, const int* counts, int B, int max_det, void* state, int max_tracks, float track_thr,
                      float low_thr, float new_thr, float match_sim, float second_sim, float unconfirmed_sim, int track_buffer,
                      int fuse_score, int class_aware, float* out_rows, int* out_ids, int* out_count, effdet_stream_t stream);
/* overflow[b] (int32 [B] on the device) = the number of new tracks stream b has dropped for lack of a free slot since its last reset.
 * Errors as effdet_track_reset (a NULL overflow is EFFDET_EINVAL). */
int effdet_track_overflow(const void* state, int B, int max_tracks, int* overflow, effdet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EFFDET_TRACK_H */
