// effdet_assign: B independent optimal assignments (include/effdet_assign.h holds the rule, assign.h the solver).  ONE 256-thread
// workgroup per problem, thread t owns row t.  The caller's matrix is NOT staged: a Dijkstra step relaxes one column, i.e. reads one
// fp32 per row, and the search touches only the columns of the rows it visits -- usually a handful.  Staging [256][128] fp32 would
// need 128 KiB of dynamic LDS (one workgroup per CU) and a full pass over the matrix before the first step; read from memory, the
// 128 KiB of a problem at the caps stay in the L2 after their first touch.  Built with -ffp-contract=off: sim - gate rounds once.
#include "assign.h"

namespace {

using namespace effdet_lap;

struct MatrixWeight {                                                  // this row of the caller's matrix
  const float* row; float gate;
  __device__ __forceinline__ int operator()(int c) const { return assign_weight(row[c], gate); }
};

__global__ __launch_bounds__(AS_R) void assign_kernel(const float* sim, int R, int C, const int* n_rows, const int* n_cols, float gate,
                                                      int* row_to_col, int* col_to_row, long long* total) {
  __shared__ AssignLds L;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int nr = n_rows ? min(max(n_rows[b], 0), R) : R, nc = n_cols ? min(max(n_cols[b], 0), C) : C;
  AssignCols cols;
  cols.w[0] = nc >= 64 ? ~0ull : (1ull << nc) - 1ull;
  cols.w[1] = nc >= 128 ? ~0ull : (nc > 64 ? (1ull << (nc - 64)) - 1ull : 0ull);
  const bool in_pool = tid < nr;
  const MatrixWeight wt{sim + ((long long)b * R + (in_pool ? tid : 0)) * C, gate};
  AssignCols matched;
  int par = 0, sum = 0;
  const int mine = assign_solve(in_pool, cols, wt, L, par, tid, matched, sum);
  if (tid < R) row_to_col[(long long)b * R + tid] = mine;
  if (tid < C) col_to_row[(long long)b * C + tid] = L.col_row[tid];    // (-1 since the solver's start for the columns outside cols)
  if (tid == 0) total[b] = (long long)sum;
}

}  // namespace

extern "C" int effdet_assign(const float* sim, int B, int R, int C, const int* n_rows, const int* n_cols, float gate, int* row_to_col,
                             int* col_to_row, long long* total, effdet_stream_t stream) {
  if (!sim || !row_to_col || !col_to_row || !total || B < 1 || R < 1 || C < 1 || !(gate - gate == 0.f)) return EFFDET_EINVAL;
  if (R > AS_R || C > AS_C) return EFFDET_EUNSUPPORTED;
  hipLaunchKernelGGL(assign_kernel, dim3(B), dim3(AS_R), 0, (hipStream_t)stream, sim, R, C, n_rows, n_cols, gate, row_to_col, col_to_row, total);
  EFFDET_CHECK_LAUNCH();
  return EFFDET_OK;
}
