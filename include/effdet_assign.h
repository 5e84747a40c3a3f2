/* effdet_assign.h -- optimal assignment of libeffdet_hip.so: the linear assignment problem ByteTrack solves in each of its associations
 * (lap.lapjv with a cost limit), as a batched stand-alone op (effdet_assign) and as the tracker's assignment stage
 * (effdet_track_step_assign).  Entry points added to ABI generation 11 after effdet_hip.h's and effdet_track.h's sets; their conventions
 * (device pointers, 0 or a negative EFFDET_E* code, work enqueued on `stream`) hold here.  A library of the same generation built before
 * this header lacks the two symbols, so a binding looks them up by name first.
 *
 * ---- the rule (restated in plain integers in tests/assign_restated.py)
 * An instance is a set of rows, a set of columns, a similarity sim(r, c) (fp32) and a gate (fp32).
 *   A pair is ADMISSIBLE exactly when  sim > gate  -- an fp32 compare, the rule the greedy assignment of effdet_track.h uses; a NaN is
 *   never admissible, -inf never, +inf always.  In the tracker with class_aware the labels must also agree (fp32 equality).
 *   The WEIGHT of an admissible pair is the int32
 *       w = max(1, (int)rintf(min(sim - gate, 1.0f) * 1048576.0f))                     (1048576 = 2^EFFDET_ASSIGN_SCALE_BITS)
 *   every operation in fp32 and rounded once (nothing contracted), rintf to nearest with ties to even.  1 <= w <= 2^20.
 *   The ANSWER is a matching over admissible pairs -- every row and every column used at most once, nothing forced to be matched --
 *   that MAXIMISES the sum of w.  At the caps the sum is at most 128 * 2^20 < 2^31.
 * Up to ties and the 2^-20 grid this is ByteTrack's  lap.lapjv(1 - sim, extend_cost=True, cost_limit=1 - gate) : that call pads the
 * cost matrix with cost_limit / 2 for "row unmatched" and for "column unmatched", so matching a pair instead of leaving both ends
 * unmatched changes the cost by (1 - sim) - (1 - gate) = -(sim - gate): it pays exactly when sim - gate > 0, and the objective is the
 * sum of (sim - gate) over the matched pairs.  What stays different from that call: the gate is strict (a pair at exactly the limit is
 * refused; lapjv is indifferent to it), the weights live on the 2^-20 grid (matchings whose sums differ by less than about n * 2^-21
 * may be ordered differently), and the choice among equal optima (below).
 *
 * ---- the choice among equal optima
 * The device algorithm is deterministic and uses no atomics and no floating-point reductions: two calls on equal input give equal bits.
 * Columns are inserted in ascending index.  An insertion searches the shortest augmenting path from the new column (a Dijkstra over
 * the rows in reduced integer costs) and takes, at every step, the smallest candidate in the order
 *   (distance, kind, row index),  kind: 0 = the column matched to an already visited row gives that row up and stays unmatched,
 *                                       1 = a row that is not matched yet, 2 = a matched row (the search goes on through its column);
 * the new column's own "stay unmatched" exit has distance 0 and wins every tie: the search ends as soon as no candidate is below 0.
 * A row keeps the first column that reached it at its final distance.  So among equal optima: the earlier columns keep what they have
 * unless a change gains at least 1.
 *
 * ---- effdet_assign, per problem b (one workgroup of 256 threads; thread t owns row t)
 * sim [B][R][C] fp32; rows r < nr = clamp(n_rows[b], 0, R) and columns c < nc = clamp(n_cols[b], 0, C) take part (NULL counts: R and
 * C).  row_to_col [B][R] int32 = the row's column or -1, col_to_row [B][C] int32 = the column's row or -1 (-1 also at and past the
 * counts); total [B] int64 = the sum of w over the matching.  Every element of the three outputs is written on every call.
 * Caps: R <= EFFDET_ASSIGN_MAX_ROWS, C <= EFFDET_ASSIGN_MAX_COLS.
 *
 * ---- effdet_track_step_assign
 * effdet_track_step (effdet_track.h) with the assignment of its steps 3, 4 and 5 chosen by `assignment`:
 *   EFFDET_ASSIGN_GREEDY  (0)  greedy by descending similarity: the very kernel effdet_track_step launches, bit for bit;
 *   EFFDET_ASSIGN_OPTIMAL (1)  the rule above in each of the three associations, with that association's rows, columns, sim and gate
 *                              (match_sim, second_sim, unconfirmed_sim); steps 0-2 and 6-10 are unchanged.
 * The similarity matrix is not stored in the tracker (effdet_track.h, "the similarity matrix"): a weight is recomputed from the slot's
 * predicted box in registers and the detection in LDS whenever the search relaxes a pair. */
#ifndef EFFDET_ASSIGN_H
#define EFFDET_ASSIGN_H
#include "effdet_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define EFFDET_ASSIGN_SCALE_BITS 20                    /* weights are multiples of 2^-20 of similarity */
#define EFFDET_ASSIGN_MAX_ROWS 256                     /* R of effdet_assign (EFFDET_TRACK_MAX_TRACKS) */
#define EFFDET_ASSIGN_MAX_COLS 128                     /* C of effdet_assign (EFFDET_TRACK_MAX_DET) */
#define EFFDET_ASSIGN_GREEDY 0
#define EFFDET_ASSIGN_OPTIMAL 1

/* B problems (above).  EFFDET_EINVAL: a NULL sim, row_to_col, col_to_row or total; B, R or C < 1; a gate that is not finite.
 * EFFDET_EUNSUPPORTED: R > 256 or C > 128.  Nothing is enqueued in either case. */
int effdet_assign(const float* sim, int B, int R, int C, const int* n_rows, const int* n_cols, float gate, int* row_to_col,
                  int* col_to_row, long long* total, effdet_stream_t stream);
/* effdet_track_step with its arguments and refusals, plus: EFFDET_EINVAL for an `assignment` other than 0 or 1. */
int effdet_track_step_assign(const float* dets, const int* counts, int B, int max_det, void* state, int max_tracks, float track_thr,
                             float low_thr, float new_thr, float match_sim, float second_sim, float unconfirmed_sim, int track_buffer,
                             int fuse_score, int class_aware, float* out_rows, int* out_ids, int* out_count, int assignment,
                             effdet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EFFDET_ASSIGN_H */
