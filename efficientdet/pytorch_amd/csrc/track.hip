// ByteTrack over finalize_dets' rows, one tracker per image of the batch (include/effdet_track.h holds the semantics;
// tests/track_restated.py restates them in NumPy).  Built with -ffp-contract=off like postprocess.hip: every operation rounds once.
//
// ONE 256-thread workgroup per stream, the structure of postprocess.hip's soft_nms_kernel and wbf.hip:
//   * thread t OWNS slot t of the stream: the slot's 28 words are loaded into its registers, stepped there and stored once;
//   * the detections (box, score, label: 24 B a row) sit in LDS, and which of them are high / low / taken are 128-bit masks that are
//     UNIFORM over the workgroup (every thread builds the same ones from the same LDS words), so no flag array and no barrier for them;
//   * an association is track_greedy(): each thread caches its row's best allowed column (track_similarity() over the free columns) and
//     rescans only when that column has just gone to another row; a pick is one 64-bit key per thread and one max over the workgroup
//     (wave shuffle butterfly + four ping-ponged LDS slots, ONE barrier per pick);
//   * new tracks: the k-th free slot (ballot ranks) takes the k-th remaining detection (popcount ranks of the uniform mask);
//   * duplicates: the LOST slots are listed in LDS, every TRACKED thread walks that list; marks are plain stores of 1;
//   * output order: rank of a TRACKED slot's id among the ids in LDS;
//   * effdet_track_step_assign's optimal assignment is the second instance of the kernel: track_optimal() in place of track_greedy(),
//     the same rows, columns, track_similarity() and gate through assign.h's shortest-augmenting-path solver (its arrays in LDS, the
//     row's dual, distance and predecessor in the slot's thread), a pair's integer weight recomputed whenever the search relaxes it.
// No atomics of any kind.
#include "box_geom.h"
#include "../../../include/effdet_track.h"
#include "assign.h"

namespace {

constexpr int TR_T = EFFDET_TRACK_MAX_TRACKS, TR_D = EFFDET_TRACK_MAX_DET, TR_W = EFFDET_TRACK_ROW_WORDS, TR_WAVES = TR_T / 64;
enum { TR_FREE = 0, TR_UNCONFIRMED = 1, TR_TRACKED = 2, TR_LOST = 3 };
static_assert(TR_T == 256 && TR_D <= 128 && TR_W == 28, "thread-per-slot layout");

struct TrackArgs {
  const float* dets; const int* counts; int* hdr; unsigned* rows; int B, max_det, T;
  float track_thr, low_thr, new_thr, match_sim, second_sim, unconfirmed_sim; int track_buffer, fuse_score, class_aware;
  float* out_rows; int* out_ids; int* out_count;
};

// a set of detection rows (uniform over the workgroup)
struct Mask { unsigned long long w[2]; };
__device__ __forceinline__ Mask mask_none() { return Mask{{0ull, 0ull}}; }
__device__ __forceinline__ bool mask_has(const Mask& m, int d) { return (m.w[d >> 6] >> (d & 63)) & 1ull; }
__device__ __forceinline__ void mask_set(Mask& m, int d) { m.w[d >> 6] |= 1ull << (d & 63); }
__device__ __forceinline__ Mask mask_andnot(const Mask& a, const Mask& b) { return Mask{{a.w[0] & ~b.w[0], a.w[1] & ~b.w[1]}}; }
__device__ __forceinline__ int mask_count(const Mask& m) { return __popcll(m.w[0]) + __popcll(m.w[1]); }
// members of m below row d
__device__ __forceinline__ int mask_rank(const Mask& m, int d) {
  return d < 64 ? __popcll(m.w[0] & ((1ull << d) - 1ull)) : __popcll(m.w[0]) + __popcll(m.w[1] & ((1ull << (d - 64)) - 1ull));
}

struct Slot {                                                          // the 28 words of a slot
  float m[8], cov[12], score, label; int state, id, len, start, last;
};

__device__ __forceinline__ bool tr_finite(float a) { return fabsf(a) < __builtin_huge_valf(); }
__device__ __forceinline__ float4 mean_box(const float* m) {
  const float w = m[2] * m[3];
  const float x1 = m[0] - 0.5f * w, y1 = m[1] - 0.5f * m[3];
  return make_float4(x1, y1, x1 + w, y1 + m[3]);
}
__device__ __forceinline__ void det_z(const float4& b, float* z) {
  const float w = b.z - b.x, h = b.w - b.y;
  z[0] = b.x + 0.5f * w; z[1] = b.y + 0.5f * h; z[2] = w / h; z[3] = h;
}
// box_geom.h's IoU arithmetic with this file's own refusal: !(iw > 0.f) sends a NaN extent to 0, where box_iou lets the NaN through
__device__ __forceinline__ float tr_iou(const float4& a, const float4& b) {
  const float iw = fminf(a.z, b.z) - fmaxf(a.x, b.x);
  const float ih = fminf(a.w, b.w) - fmaxf(a.y, b.y);
  if (!(iw > 0.f) || !(ih > 0.f)) return 0.f;
  const float inter = iw * ih;
  return inter / ((box_area(a) + box_area(b)) - inter);
}

// ---- the Kalman filter in block form
__device__ __forceinline__ void kf_start(Slot& s, const float* z) {
  const float sp = 2.f * (z[3] / 20.f), su = 10.f * (z[3] / 160.f);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    s.m[i] = z[i]; s.m[4 + i] = 0.f;
    s.cov[3 * i] = i == 2 ? 1e-4f : sp * sp; s.cov[3 * i + 1] = 0.f; s.cov[3 * i + 2] = i == 2 ? 1e-10f : su * su;
  }
}
__device__ __forceinline__ void kf_predict(Slot& s) {
  const float h = s.m[3];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float sp = i == 2 ? 1e-2f : h / 20.f, su = i == 2 ? 1e-5f : h / 160.f;
    float& p = s.cov[3 * i]; float& c = s.cov[3 * i + 1]; float& v = s.cov[3 * i + 2];
    s.m[i] = s.m[i] + s.m[4 + i];
    p = ((p + c) + (c + v)) + sp * sp;
    c = c + v;
    v = v + su * su;
  }
}
__device__ __forceinline__ void kf_update(Slot& s, const float* z) {
  const float h = s.m[3];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float sp = h / 20.f;
    const float r = i == 2 ? 1e-2f : sp * sp;
    const float p = s.cov[3 * i], c = s.cov[3 * i + 1], v = s.cov[3 * i + 2];
    const float S = p + r, y = z[i] - s.m[i];
    s.m[i] = s.m[i] + (p / S) * y;
    s.m[4 + i] = s.m[4 + i] + (c / S) * y;
    s.cov[3 * i] = p - (p * p) / S;
    s.cov[3 * i + 1] = c - (p * c) / S;
    s.cov[3 * i + 2] = v - (c * c) / S;
  }
}

// ---- the workgroup's max of one 64-bit key per thread (one barrier; `par` ping-pongs the slots between calls)
__device__ __forceinline__ unsigned long long block_max_key(unsigned long long k, unsigned long long (*red)[TR_WAVES], int& par, int tid) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(k, o, 64);
    k = other > k ? other : k;
  }
  if ((tid & 63) == 0) red[par][tid >> 6] = k;
  __syncthreads();
  unsigned long long best = red[par][0];
#pragma unroll
  for (int w = 1; w < TR_WAVES; ++w) best = red[par][w] > best ? red[par][w] : best;
  par ^= 1;
  return best;
}

// ---- similarity stage: the value of one (row, column) pair; < 0 for a pair the labels forbid
__device__ __forceinline__ float track_similarity(const float4& tb, float tlabel, const float4& db, float dscore, float dlabel, bool fuse,
                                                  bool class_aware) {
  if (class_aware && !(tlabel == dlabel)) return -1.f;
  const float iou = tr_iou(tb, db);
  return fuse ? iou * dscore : iou;
}

// ---- assignment stage: greedy by descending similarity over rows (threads with in_pool) x columns (cols, minus taken).
// Returns this thread's column or -1; taken gains the matched columns (uniformly).
__device__ __forceinline__ int track_greedy(bool in_pool, const float4& tb, float tlabel, const Mask& cols, Mask& taken, float gate, bool fuse,
                                            bool class_aware, const float4* dbox, const float* dscore, const float* dlabel,
                                            unsigned long long (*red)[TR_WAVES], int& par, int tid) {
  Mask avail = mask_andnot(cols, taken);
  int mine = -1, bd = -1;
  float bs = 0.f;
  bool stale = true;
  for (;;) {
    if (in_pool && stale) {
      bs = gate; bd = -1;                                              // (strictly above the gate; ascending rows: the first maximum stays)
#pragma unroll
      for (int h = 0; h < 2; ++h)
        for (unsigned long long w = avail.w[h]; w; w &= w - 1ull) {
          const int d = h * 64 + __ffsll((long long)w) - 1;
          const float s = track_similarity(tb, tlabel, dbox[d], dscore[d], dlabel[d], fuse, class_aware);
          if (s > bs) { bs = s; bd = d; }
        }
      stale = false;
    }
    unsigned long long key = 0ull;                                     // (bs > gate >= 0: a positive float, whose bits order like it)
    if (in_pool && bd >= 0) key = ((unsigned long long)__float_as_uint(bs) << 32) | ((unsigned)(0xffff - bd) << 16) | (unsigned)(0xffff - tid);
    key = block_max_key(key, red, par, tid);
    if (key == 0ull) break;
    const int d = 0xffff - (int)((key >> 16) & 0xffffull), t = 0xffff - (int)(key & 0xffffull);
    mask_set(taken, d);
    avail = mask_andnot(cols, taken);
    if (t == tid) { mine = d; in_pool = false; }
    else if (bd == d) stale = true;
  }
  return mine;
}

// ---- assignment stage, optimal (include/effdet_assign.h): the same pool, columns (cols minus taken), similarity and gate; the weight of
// a pair is recomputed from the two boxes at every relaxation.  Returns this thread's column or -1; taken gains the matched columns.
struct TrackWeight {
  float4 tb; float tlabel, gate; bool fuse, class_aware; const float4* dbox; const float* dscore; const float* dlabel;
  __device__ __forceinline__ int operator()(int d) const {
    return effdet_lap::assign_weight(track_similarity(tb, tlabel, dbox[d], dscore[d], dlabel[d], fuse, class_aware), gate);
  }
};
__device__ __forceinline__ int track_optimal(bool in_pool, const float4& tb, float tlabel, const Mask& cols, Mask& taken, float gate, bool fuse,
                                             bool class_aware, const float4* dbox, const float* dscore, const float* dlabel,
                                             effdet_lap::AssignLds& lap, int& par, int tid) {
  const Mask avail = mask_andnot(cols, taken);
  const effdet_lap::AssignCols c{{avail.w[0], avail.w[1]}};
  effdet_lap::AssignCols got;
  int total;
  const TrackWeight wt{tb, tlabel, gate, fuse, class_aware, dbox, dscore, dlabel};
  const int mine = effdet_lap::assign_solve(in_pool, c, wt, lap, par, tid, got, total);
  taken.w[0] |= got.w[0]; taken.w[1] |= got.w[1];
  return mine;
}

// the solver's LDS, present only in the kernel instance that uses it
template <bool OPTIMAL> struct LapStore { effdet_lap::AssignLds lds; };
template <> struct LapStore<false> {};

template <bool OPTIMAL>
__device__ __forceinline__ int track_associate(bool in_pool, const float4& tb, float tlabel, const Mask& cols, Mask& taken, float gate, bool fuse,
                                               bool class_aware, const float4* dbox, const float* dscore, const float* dlabel,
                                               unsigned long long (*red)[TR_WAVES], LapStore<OPTIMAL>& lap, int& par, int tid) {
  if constexpr (OPTIMAL) return track_optimal(in_pool, tb, tlabel, cols, taken, gate, fuse, class_aware, dbox, dscore, dlabel, lap.lds, par, tid);
  else return track_greedy(in_pool, tb, tlabel, cols, taken, gate, fuse, class_aware, dbox, dscore, dlabel, red, par, tid);
}

__device__ __forceinline__ void slot_match(Slot& s, int d, const float4* dbox, const float* dscore, const float* dlabel, int frame) {
  float z[4];
  det_z(dbox[d], z);
  kf_update(s, z);
  s.score = dscore[d]; s.label = dlabel[d]; s.last = frame;
}

template <bool OPTIMAL>
__global__ __launch_bounds__(TR_T) void track_step_kernel(const TrackArgs a) {
  __shared__ LapStore<OPTIMAL> lap;
  __shared__ float4 dbox[TR_D];
  __shared__ float dscore[TR_D], dlabel[TR_D];
  __shared__ int dkind[TR_D];                                          // 0 skipped / ignored, 1 low, 2 high
  __shared__ unsigned long long red[2][TR_WAVES];
  __shared__ int wave_free[TR_WAVES], new_rows[TR_D], lost_list[TR_T], n_lost[TR_WAVES], dup_mark[TR_T], ids[TR_T];
  __shared__ float4 tbox[TR_T];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, T = a.T;
  const bool have = tid < T;
  int par = 0;

  // the detections, their kinds, the uniform masks
  const int rows = min(max(a.counts[b], 0), a.max_det);
  if (tid < TR_D) {
    int kind = 0;
    float4 bx = make_float4(0.f, 0.f, 0.f, 0.f); float sc = 0.f, lb = 0.f;
    if (tid < rows) {
      const float* r = a.dets + ((long long)b * a.max_det + tid) * 6;
      bx = make_float4(r[0], r[1], r[2], r[3]); sc = r[4]; lb = r[5];
      const bool ok = tr_finite(bx.x) && tr_finite(bx.y) && tr_finite(bx.z) && tr_finite(bx.w) && tr_finite(sc) && bx.z > bx.x && bx.w > bx.y;
      if (ok) kind = sc >= a.track_thr ? 2 : (sc > a.low_thr ? 1 : 0);
    }
    dbox[tid] = bx; dscore[tid] = sc; dlabel[tid] = lb; dkind[tid] = kind;
  }
  // this thread's slot
  Slot s;
  unsigned* row = a.rows + ((long long)b * T + (have ? tid : 0)) * TR_W;
  if (have) {
#pragma unroll
    for (int i = 0; i < 8; ++i) s.m[i] = __uint_as_float(row[i]);
#pragma unroll
    for (int i = 0; i < 12; ++i) s.cov[i] = __uint_as_float(row[8 + i]);
    s.score = __uint_as_float(row[20]); s.label = __uint_as_float(row[21]);
    s.state = (int)row[22]; s.id = (int)row[23]; s.len = (int)row[24]; s.start = (int)row[25]; s.last = (int)row[26];
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) s.m[i] = 0.f;
#pragma unroll
    for (int i = 0; i < 12; ++i) s.cov[i] = 0.f;
    s.score = 0.f; s.label = 0.f; s.state = TR_FREE; s.id = 0; s.len = 0; s.start = 0; s.last = 0;
  }
  const int frame = a.hdr[b * 4 + 0] + 1;                              // step 0
  int next_id = a.hdr[b * 4 + 1], overflow = a.hdr[b * 4 + 2];
  __syncthreads();
  Mask high = mask_none(), low = mask_none(), fresh = mask_none();
  for (int d = 0; d < rows; ++d) {                                     // (LDS broadcasts; uniform)
    const int k = dkind[d];
    if (k == 2) { mask_set(high, d); if (dscore[d] >= a.new_thr) mask_set(fresh, d); }
    else if (k == 1) mask_set(low, d);
  }

  // 1. predict
  if (s.state == TR_LOST) s.m[7] = 0.f;
  if (s.state != TR_FREE) kf_predict(s);
  const float4 pb = mean_box(s.m);
  const bool fuse = a.fuse_score != 0, ca = a.class_aware != 0;
  const int state0 = s.state;

  // 3. first association: TRACKED + LOST x HIGH
  Mask taken = mask_none();
  int d = track_associate<OPTIMAL>(state0 == TR_TRACKED || state0 == TR_LOST, pb, s.label, high, taken, a.match_sim, fuse, ca, dbox, dscore, dlabel,
                                   red, lap, par, tid);
  bool matched = d >= 0;
  if (matched) {                                                       // 6.
    slot_match(s, d, dbox, dscore, dlabel, frame);
    if (state0 == TR_LOST) { s.state = TR_TRACKED; s.len = 0; } else s.len += 1;
  }
  // 4. second association: the TRACKED left x LOW, plain IoU
  Mask taken_low = mask_none();
  d = track_associate<OPTIMAL>(state0 == TR_TRACKED && !matched, pb, s.label, low, taken_low, a.second_sim, false, ca, dbox, dscore, dlabel, red,
                               lap, par, tid);
  if (d >= 0) { slot_match(s, d, dbox, dscore, dlabel, frame); s.len += 1; matched = true; }
  if (state0 == TR_TRACKED && !matched) s.state = TR_LOST;
  // 5. third association: UNCONFIRMED x the HIGH left
  d = track_associate<OPTIMAL>(state0 == TR_UNCONFIRMED, pb, s.label, high, taken, a.unconfirmed_sim, fuse, ca, dbox, dscore, dlabel, red, lap, par,
                               tid);
  if (state0 == TR_UNCONFIRMED) {
    if (d >= 0) { slot_match(s, d, dbox, dscore, dlabel, frame); s.len += 1; s.state = TR_TRACKED; }
    else s.state = TR_FREE;
  }

  // 7. new tracks: the k-th free slot takes the k-th remaining detection
  const Mask born = mask_andnot(fresh, taken);
  const int n_born = mask_count(born);
  const bool is_free = have && s.state == TR_FREE;
  const unsigned long long fb = __ballot(is_free);
  if (lane == 0) wave_free[wave] = __popcll(fb);
  if (tid < TR_D && mask_has(born, tid)) new_rows[mask_rank(born, tid)] = tid;
  __syncthreads();
  int k = __popcll(fb & ((1ull << lane) - 1ull)), n_free = 0;
#pragma unroll
  for (int w = 0; w < TR_WAVES; ++w) { if (w < wave) k += wave_free[w]; n_free += wave_free[w]; }
  if (is_free && k < n_born) {
    const int r = new_rows[k];
    float z[4];
    det_z(dbox[r], z);
    kf_start(s, z);
    s.score = dscore[r]; s.label = dlabel[r]; s.id = next_id + k; s.len = 0; s.start = frame; s.last = frame;
    s.state = frame == 1 ? TR_TRACKED : TR_UNCONFIRMED;
  }
  next_id += min(n_born, n_free);
  overflow += max(n_born - n_free, 0);

  // 8. removal
  if (s.state == TR_LOST && frame - s.last > a.track_buffer) s.state = TR_FREE;

  // 9. duplicates: the LOST slots listed in slot order, every TRACKED thread walks the list
  const float4 fbx = mean_box(s.m);
  const bool is_lost = s.state == TR_LOST;
  const unsigned long long lb = __ballot(is_lost);
  if (lane == 0) n_lost[wave] = __popcll(lb);
  if (have) { tbox[tid] = fbx; dup_mark[tid] = 0; ids[tid] = s.start; }   // (ids doubles as the start frames until step 10)
  __syncthreads();
  int lk = __popcll(lb & ((1ull << lane) - 1ull)), nl = 0;
#pragma unroll
  for (int w = 0; w < TR_WAVES; ++w) { if (w < wave) lk += n_lost[w]; nl += n_lost[w]; }
  if (is_lost) lost_list[lk] = tid;
  __syncthreads();
  if (s.state == TR_TRACKED)
    for (int i = 0; i < nl; ++i) {
      const int l = lost_list[i];
      if (tr_iou(fbx, tbox[l]) > 0.85f) {
        if (frame - s.start > frame - ids[l]) dup_mark[l] = 1; else dup_mark[tid] = 1;
      }
    }
  __syncthreads();
  if (have && dup_mark[tid]) s.state = TR_FREE;
  __syncthreads();                                                     // (ids is rewritten below)

  // 10. output in ascending id; the state back
  const bool shown = s.state == TR_TRACKED;
  if (have) ids[tid] = shown ? s.id : 0x7fffffff;
  const unsigned long long sb = __ballot(shown);
  if (lane == 0) wave_free[wave] = __popcll(sb);                       // (its step-7 readers are behind three barriers)
  __syncthreads();
  int n_out = 0;
#pragma unroll
  for (int w = 0; w < TR_WAVES; ++w) n_out += wave_free[w];
  float* orow = a.out_rows + (long long)b * T * 8;
  int* oid = a.out_ids + (long long)b * T;
  if (shown) {
    int rank = 0;
    for (int t = 0; t < T; ++t) rank += ids[t] < s.id ? 1 : 0;
    float* o = orow + rank * 8;
    o[0] = fbx.x; o[1] = fbx.y; o[2] = fbx.z; o[3] = fbx.w; o[4] = s.score; o[5] = s.label; o[6] = (float)s.len; o[7] = (float)(frame - s.start);
    oid[rank] = s.id;
  }
  if (have && tid >= n_out) {
#pragma unroll
    for (int i = 0; i < 8; ++i) orow[tid * 8 + i] = 0.f;
    oid[tid] = -1;
  }
  if (have) {
    if (s.state == TR_FREE) {
#pragma unroll
      for (int i = 0; i < TR_W; ++i) row[i] = 0u;
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) row[i] = __float_as_uint(s.m[i]);
#pragma unroll
      for (int i = 0; i < 12; ++i) row[8 + i] = __float_as_uint(s.cov[i]);
      row[20] = __float_as_uint(s.score); row[21] = __float_as_uint(s.label);
      row[22] = (unsigned)s.state; row[23] = (unsigned)s.id; row[24] = (unsigned)s.len; row[25] = (unsigned)s.start; row[26] = (unsigned)s.last;
      row[27] = 0u;
    }
  }
  if (tid == 0) {
    a.hdr[b * 4 + 0] = frame; a.hdr[b * 4 + 1] = next_id; a.hdr[b * 4 + 2] = overflow; a.hdr[b * 4 + 3] = 0;
    a.out_count[b] = n_out;
  }
}

__global__ __launch_bounds__(TR_T) void track_reset_kernel(int* hdr, unsigned* rows, int T, const int* mask) {
  const int b = blockIdx.x;
  if (mask && mask[b] == 0) return;
  for (int i = threadIdx.x; i < T * TR_W; i += TR_T) rows[(long long)b * T * TR_W + i] = 0u;
  if (threadIdx.x < 4) hdr[b * 4 + threadIdx.x] = threadIdx.x == 1 ? 1 : 0;
}

__global__ void track_overflow_kernel(const int* hdr, int B, int* out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) out[b] = hdr[b * 4 + 2];
}

inline int track_shape(int B, int T) {
  if (B < 1 || T < 1) return EFFDET_EINVAL;
  if (T > TR_T) return EFFDET_EUNSUPPORTED;
  return EFFDET_OK;
}
inline bool lim_ok(float v) { return v >= 0.f && v <= 1.f; }
inline bool fin_ok(float v) { return v - v == 0.f; }

}  // namespace

extern "C" long long effdet_track_state_bytes(int B, int max_tracks) {
  if (track_shape(B, max_tracks) != EFFDET_OK) return 0;
  return (long long)B * 16 + (long long)B * max_tracks * TR_W * 4;
}

extern "C" int effdet_track_reset(void* state, int B, int max_tracks, const int* reset_mask, effdet_stream_t stream) {
  if (!state) return EFFDET_EINVAL;
  const int e = track_shape(B, max_tracks);
  if (e != EFFDET_OK) return e;
  hipLaunchKernelGGL(track_reset_kernel, dim3(B), dim3(TR_T), 0, (hipStream_t)stream, (int*)state, (unsigned*)state + (size_t)B * 4, max_tracks,
                     reset_mask);
  EFFDET_CHECK_LAUNCH();
  return EFFDET_OK;
}

extern "C" int effdet_track_overflow(const void* state, int B, int max_tracks, int* overflow, effdet_stream_t stream) {
  if (!state || !overflow) return EFFDET_EINVAL;
  const int e = track_shape(B, max_tracks);
  if (e != EFFDET_OK) return e;
  hipLaunchKernelGGL(track_overflow_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const int*)state, B, overflow);
  EFFDET_CHECK_LAUNCH();
  return EFFDET_OK;
}

// effdet_track_step and effdet_track_step_assign: the refusals, then one launch of the instance `assignment` names
static int track_step_launch(const float* dets, const int* counts, int B, int max_det, void* state, int max_tracks, float track_thr, float low_thr,
                             float new_thr, float match_sim, float second_sim, float unconfirmed_sim, int track_buffer, int fuse_score,
                             int class_aware, float* out_rows, int* out_ids, int* out_count, int assignment, effdet_stream_t stream) {
  if (!dets || !counts || !state || !out_rows || !out_ids || !out_count || max_det < 1) return EFFDET_EINVAL;
  const int e = track_shape(B, max_tracks);
  if (e == EFFDET_EINVAL) return e;
  if (!fin_ok(track_thr) || !fin_ok(low_thr) || !fin_ok(new_thr) || !lim_ok(match_sim) || !lim_ok(second_sim) || !lim_ok(unconfirmed_sim) ||
      low_thr > track_thr || track_buffer < 0)
    return EFFDET_EINVAL;
  if (assignment != EFFDET_ASSIGN_GREEDY && assignment != EFFDET_ASSIGN_OPTIMAL) return EFFDET_EINVAL;
  if (e != EFFDET_OK || max_det > TR_D) return EFFDET_EUNSUPPORTED;
  TrackArgs a;
  a.dets = dets; a.counts = counts; a.hdr = (int*)state; a.rows = (unsigned*)state + (size_t)B * 4; a.B = B; a.max_det = max_det; a.T = max_tracks;
  a.track_thr = track_thr; a.low_thr = low_thr; a.new_thr = new_thr; a.match_sim = match_sim; a.second_sim = second_sim;
  a.unconfirmed_sim = unconfirmed_sim; a.track_buffer = track_buffer; a.fuse_score = fuse_score; a.class_aware = class_aware;
  a.out_rows = out_rows; a.out_ids = out_ids; a.out_count = out_count;
  if (assignment == EFFDET_ASSIGN_OPTIMAL) hipLaunchKernelGGL(track_step_kernel<true>, dim3(B), dim3(TR_T), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(track_step_kernel<false>, dim3(B), dim3(TR_T), 0, (hipStream_t)stream, a);
  EFFDET_CHECK_LAUNCH();
  return EFFDET_OK;
}

extern "C" int effdet_track_step(const float* dets, const int* counts, int B, int max_det, void* state, int max_tracks, float track_thr,
                                 float low_thr, float new_thr, float match_sim, float second_sim, float unconfirmed_sim, int track_buffer,
                                 int fuse_score, int class_aware, float* out_rows, int* out_ids, int* out_count, effdet_stream_t stream) {
  return track_step_launch(dets, counts, B, max_det, state, max_tracks, track_thr, low_thr, new_thr, match_sim, second_sim, unconfirmed_sim,
                           track_buffer, fuse_score, class_aware, out_rows, out_ids, out_count, EFFDET_ASSIGN_GREEDY, stream);
}

extern "C" int effdet_track_step_assign(const float* dets, const int* counts, int B, int max_det, void* state, int max_tracks, float track_thr,
                                        float low_thr, float new_thr, float match_sim, float second_sim, float unconfirmed_sim,
                                        int track_buffer, int fuse_score, int class_aware, float* out_rows, int* out_ids, int* out_count,
                                        int assignment, effdet_stream_t stream) {
  return track_step_launch(dets, counts, B, max_det, state, max_tracks, track_thr, low_thr, new_thr, match_sim, second_sim, unconfirmed_sim,
                           track_buffer, fuse_score, class_aware, out_rows, out_ids, out_count, assignment, stream);
}
