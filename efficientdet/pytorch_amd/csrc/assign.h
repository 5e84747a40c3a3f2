// Optimal assignment inside one 256-thread workgroup (include/effdet_assign.h holds the rule; tests/assign_restated.py restates it in
// plain integers).  Device functions shared by assign.hip (the stand-alone op: weights from the caller's matrix) and track.hip (the
// tracker's associations: weights recomputed from the boxes).  Include from a source built with -ffp-contract=off.
//
// The problem as a min-cost assignment: every column c gets, besides the real rows, a private dummy row d_c it can take at cost 0 ("c
// stays unmatched"); an admissible pair costs -w, everything else is forbidden.  Every column is then assigned and the cheapest such
// assignment is the maximum-weight matching.  It is solved by successive shortest augmenting paths (Jonker-Volgenant / Hungarian):
// columns are inserted one at a time, an insertion is a Dijkstra from the new column over the ROWS in reduced costs
//   rc(r, c) = -w(r, c) - u[c] - v[r] >= 0  for the columns inserted so far,  = 0 on matched pairs,
// thread t owns row t: its dual v, its column, its tentative distance, visited flag and predecessor column live in registers; the
// column duals u[] and the two match arrays are in LDS.  A Dijkstra step is one packed 64-bit key per thread and one min over the
// workgroup (wave shuffle butterfly + ping-ponged LDS slots, ONE barrier): the key is (distance, kind, row, column) as the header
// orders them.  Dummies never need a node of their own: d_c is reachable from c alone and c, once it holds d_c, is reachable from
// nowhere, so v[d_c] stays 0, a column that went unmatched stays so, and "column c gives up its row and takes d_c" is just one more
// candidate of the thread whose visited row c holds, at distance dist(row) - u[c].  The new column's own dummy is at distance -u = 0:
// the search ends as soon as no candidate is below 0.  The path is walked back by thread 0 through the predecessors and the match
// arrays in LDS.  No atomics, no floating-point reductions: equal input gives equal bits.
//
// Ranges (why int32 is enough).  Invariants after every insertion, for the inserted columns c and all rows r:
//   (a) v[r] <= 0: it starts at 0 and an update only subtracts  minval - dist(r) >= 0  (r was visited at dist(r) <= minval);
//   (b) u[c] <= 0: the dummy edge's reduced cost 0 - u[c] - 0 stays >= 0 like every other;
//   (c) on a matched pair u[c] + v[r] = -w, so with (a) and (b) both lie in [-w, 0], within [-2^20, 0]; an unmatched row has v = 0 and a
//       column on its dummy has u = 0.
// During a search from a new column (u = 0): the first relaxations give -w - v[r] >= -w >= -2^20; distances of visited rows are
// non-decreasing from there (reduced costs out of visited columns are >= 0) and end at minval <= 0 (the own exit); a tentative distance
// is at most minval + (-w - u - v) < 0 + 2^21.  So every finite distance lies in [-2^20, 2^21), far inside the bias of 2^30 used for the
// packed key, and the total is at most 128 * 2^20 = 2^27.
#pragma once
#include "common.h"
#include "../../../include/effdet_assign.h"

namespace effdet_lap {

constexpr int AS_R = EFFDET_ASSIGN_MAX_ROWS, AS_C = EFFDET_ASSIGN_MAX_COLS, AS_WAVES = AS_R / 64;
constexpr int AS_INF = 0x3fffffff, AS_BIAS = 1 << 30;
static_assert(AS_R == 256 && AS_C == 128, "thread-per-row layout, 7-bit columns in the key");

struct AssignCols { unsigned long long w[2]; };                        // a set of columns, uniform over the workgroup

struct AssignLds {
  unsigned long long red[2][AS_WAVES];
  int ucol[AS_C];                                                      // column duals
  int col_row[AS_C];                                                   // a column's row, -1 unmatched
  int row_col[AS_R];                                                   // a row's column, -1 unmatched
  int pred[AS_R];                                                      // a row's predecessor column in the current search
};

// the weight of a pair, 0 when it is not admissible
__device__ __forceinline__ int assign_weight(float sim, float gate) {
  if (!(sim > gate)) return 0;
  const float d = fminf(sim - gate, 1.0f);
  const int q = (int)rintf(d * 1048576.0f);
  return q < 1 ? 1 : q;
}

// the workgroup's min of one 64-bit key per thread (one barrier; `par` ping-pongs the slots between calls)
__device__ __forceinline__ unsigned long long block_min_key(unsigned long long k, unsigned long long (*red)[AS_WAVES], int& par, int tid) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(k, o, 64);
    k = other < k ? other : k;
  }
  if ((tid & 63) == 0) red[par][tid >> 6] = k;
  __syncthreads();
  unsigned long long best = red[par][0];
#pragma unroll
  for (int w = 1; w < AS_WAVES; ++w) best = red[par][w] < best ? red[par][w] : best;
  par ^= 1;
  return best;
}

__device__ __forceinline__ unsigned long long assign_key(int dist, int kind, int row, int col) {
  return ((unsigned long long)(unsigned)(dist + AS_BIAS) << 32) | ((unsigned)kind << 16) | ((unsigned)row << 8) | (unsigned)col;
}

// Rows: the threads with in_pool (thread tid is row tid).  Columns: cols.  wt(c) -> this row's weight with column c (0: not
// admissible); it is called only by in_pool threads and only for members of cols.  Every thread of the workgroup calls this with the
// same cols.  Returns this row's column or -1; matched gains the columns that got a row and total the sum of the weights (both uniform).
template <class Weight>
__device__ __forceinline__ int assign_solve(bool in_pool, const AssignCols& cols, const Weight& wt, AssignLds& L, int& par, int tid,
                                            AssignCols& matched, int& total) {
  __syncthreads();                                                     // (a previous solve's readers of L)
  if (tid < AS_C) { L.ucol[tid] = 0; L.col_row[tid] = -1; }
  L.row_col[tid] = -1;
  __syncthreads();
  int v = 0, mine = -1, sum = 0;
#pragma unroll 1
  for (int h = 0; h < 2; ++h)
#pragma unroll 1
    for (unsigned long long m = cols.w[h]; m; m &= m - 1ull) {
      const int c = h * 64 + __ffsll((long long)m) - 1;
      int dist = AS_INF, pred = -1, dvis = 0, dexit = 0;
      bool vis = false;
      int cur = c, base = 0, ucur = 0, kind = -1, row = 0, col = 0, minval = 0;
#pragma unroll 1
      for (int step = 0; step <= AS_R; ++step) {                       // (every step but the last visits another row)
        if (in_pool && !vis) {                                         // relax this row from column cur
          const int w = wt(cur);
          if (w > 0) {
            const int nd = base - w - ucur - v;
            if (nd < dist) { dist = nd; pred = cur; }
          }
        }
        unsigned long long key = ~0ull;
        if (in_pool) {
          if (vis) key = assign_key(dexit, 0, tid, mine);
          else if (dist < AS_INF) key = mine >= 0 ? assign_key(dist, 2, tid, mine) : assign_key(dist, 1, tid, 0);
        }
        key = block_min_key(key, L.red, par, tid);
        const int bd = (int)(unsigned)(key >> 32) - AS_BIAS;
        if (key == ~0ull || bd >= 0) { minval = 0; break; }            // the new column's own exit (distance 0) is the cheapest
        kind = (int)((key >> 16) & 3ull); row = (int)((key >> 8) & 0xffull); col = (int)(key & 0x7full);
        minval = bd;
        if (kind != 2) break;                                          // a sink: an unmatched row, or column col gives up row `row`
        ucur = L.ucol[col];
        if (row == tid) { vis = true; dvis = dist; dexit = dist - ucur; }
        cur = col; base = bd;
        kind = -1;
      }
      // duals: visited rows and their columns move by minval - dist(row); the new column's dual becomes minval
      if (vis) {
        const int delta = minval - dvis;
        L.ucol[mine] += delta;
        v -= delta;
      }
      if (tid == 0) L.ucol[c] = minval;
      if (kind >= 0 && in_pool && (vis || tid == row)) L.pred[tid] = pred;
      sum -= minval;
      __syncthreads();
      if (kind >= 0) {                                                 // (uniform) augment along the predecessors
        if (tid == 0) {
          if (kind == 0) L.col_row[col] = -1;
          int j = row;
          for (int hop = 0; hop < AS_C && j >= 0; ++hop) {                      // (a path holds every column at most once)
            const int i = L.pred[j];
            if (i < 0) break;                                          // (never: every row on the path was reached from a column)
            L.row_col[j] = i;
            const int jp = L.col_row[i];
            L.col_row[i] = j;
            if (i == c) break;
            j = jp;
          }
        }
        __syncthreads();
        if (in_pool) mine = L.row_col[tid];
      }
    }
  matched.w[0] = 0ull; matched.w[1] = 0ull;
#pragma unroll 1
  for (int h = 0; h < 2; ++h)
    for (unsigned long long m = cols.w[h]; m; m &= m - 1ull) {
      const int c = h * 64 + __ffsll((long long)m) - 1;
      if (L.col_row[c] >= 0) matched.w[h] |= 1ull << (c & 63);
    }
  total = sum;
  return mine;
}

}  // namespace effdet_lap
