// Device-side post-processing: anchors (float64, bit-exact with the reference's NumPy path), box
// decode + clip + per-anchor class max, and class-agnostic greedy NMS with no host round trip.
// Compiled with -ffp-contract=off so the fp32 box / IoU arithmetic rounds exactly like the
// reference's unfused torch / torchvision CPU ops.
//
// NMS design (worst case of the synthetic benchmark: every one of the 49 104 / 196 416 anchors is a
// candidate, ~11 % survive):
//   1. key = ~orderable(score) (invalid -> 0xffffffff), value = anchor index; an in-tree stable LSD
//      radix sort of the B per-image segments gives "descending score, ties by index".
//   2. candidates are walked in rounds of 2048 (4096 above 64 k anchors).  The cross phase (whole GPU, one wave
//      per candidate) marks candidates suppressed by boxes kept in EARLIER rounds through the spatial
//      hash of the kept boxes (brute force over the kept list for iou_threshold < 0.5).
//   3. nms_matrix_kernel (several workgroups per image) compacts the round's survivors and builds their
//      suppression bit-matrix; nms_resolve_kernel (one wave per image) walks the rows in blocks of 64 --
//      exactly the sequential greedy result -- appends the kept boxes in order and files them into the grid.
//   All loops are bounded by device-side counts; the host launches ceil(A / round) rounds blindly; every
//   launch geometry depends on shapes only and the call consists of kernel nodes only: capture-safe.
#include "box_geom.h"
#include "block_best.h"
#include "../../../include/effdet_soft_nms.h"
#include "radix_sort.h"
#include <stdlib.h>

namespace {

// ------------------------------------------------------------------ anchors
struct AnchorK { double base[5][9][4]; int fh[5], fw[5]; long long start[5]; float* out; long long total; };

__global__ void anchors_kernel(const AnchorK p) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < p.total; i += (long long)gridDim.x * blockDim.x) {
    int l = 0;
#pragma unroll
    for (int q = 1; q < 5; ++q) if (i >= p.start[q]) l = q;
    const long long r = i - p.start[l];
    const int a = (int)(r % 9); const long long cell = r / 9;
    const int x = (int)(cell % p.fw[l]), y = (int)(cell / p.fw[l]);
    const double stride = (double)(1 << (l + 3));
    const double sx = ((double)x + 0.5) * stride, sy = ((double)y + 0.5) * stride;
    float4 o;
    o.x = (float)(p.base[l][a][0] + sx); o.y = (float)(p.base[l][a][1] + sy);
    o.z = (float)(p.base[l][a][2] + sx); o.w = (float)(p.base[l][a][3] + sy);
    ((float4*)p.out)[i] = o;
  }
}

// ------------------------------------------------------------------ decode + clip + class max
// 64 anchors per 256-thread block: the 64 x nc probability tile is read with fully coalesced loads into LDS
// (row stride nc+1 -> conflict-free), 4 lanes scan each anchor's row and combine with shuffles keeping the
// FIRST maximum (torch.max tie order); lane 0 of each quad also decodes + clips the box.
__global__ __launch_bounds__(256) void decode_score_kernel(const float* __restrict__ anchors, const float* __restrict__ reg,
                                                           const float* __restrict__ cls, float* __restrict__ boxes,
                                                           float* __restrict__ score, int* __restrict__ label, long long A,
                                                           int nc, float img_w, float img_h, long long total) {
  extern __shared__ float tile[];                 // [64][nc + 1]
  const long long i0 = (long long)blockIdx.x * 64;
  const int na = (int)min(64LL, total - i0);
  const int ld = nc + 1;
  const float* src = cls + i0 * nc;
  for (int e = threadIdx.x; e < na * nc; e += 256) { const int r = e / nc, k = e - r * nc; tile[r * ld + k] = src[e]; }
  __syncthreads();
  const int r = threadIdx.x >> 2, q = threadIdx.x & 3;
  float m = -1.0f; int arg = 0x7fffffff;
  if (r < na) {
    // (torch.max: a NaN is the maximum -- the first NaN; the anchor's score is then NaN and the NMS threshold drops it)
    for (int k = q; k < nc; k += 4) { const float v = tile[r * ld + k]; if (v > m || (v != v && m == m)) { m = v; arg = k; } }
  }
#pragma unroll
  for (int o = 1; o <= 2; o <<= 1) {
    const float om = __shfl_xor(m, o, 64); const int oa = __shfl_xor(arg, o, 64);
    const bool on = om != om, mn = m != m;
    if (on ? (!mn || oa < arg) : (!mn && (om > m || (om == m && oa < arg)))) { m = om; arg = oa; }
  }
  if (r < na && q == 0) {
    const long long i = i0 + r;
    const long long a = i % A;
    const float4 an = ((const float4*)anchors)[a];
    const float4 d = ((const float4*)reg)[i];
    const float w = an.z - an.x, h = an.w - an.y;
    const float cx = an.x + 0.5f * w, cy = an.y + 0.5f * h;
    const float dx = d.x * 0.1f, dy = d.y * 0.1f, dw = d.z * 0.2f, dh = d.w * 0.2f;
    const float pcx = cx + dx * w, pcy = cy + dy * h;
    const float pw = expf(dw) * w, ph = expf(dh) * h;
    float4 b;
    // (torch.clamp of ClipBoxes keeps a NaN coordinate; the NMS below files no NaN box and cell_of stays in range for one)
    b.x = nan_max(pcx - 0.5f * pw, 0.f); b.y = nan_max(pcy - 0.5f * ph, 0.f);
    b.z = nan_min(pcx + 0.5f * pw, img_w); b.w = nan_min(pcy + 0.5f * ph, img_h);
    ((float4*)boxes)[i] = b;
    score[i] = m; label[i] = arg;
  }
}

// ------------------------------------------------------------------ NMS
constexpr int NT = 1024;          // threads per NMS workgroup = candidates per tile

struct KeptGrid { int* kcount; float4* kcell; int* kover_n; float4* kover; int HT; };      // see "spatial hash of the KEPT boxes" below
constexpr int KG_CAP = 8;                 // boxes per cell (NMS keeps same-size boxes in one cell sparse); more go to the overflow list

struct NmsWs {
  int* nvalid; int* kept; unsigned* dead; float4* sbox; float4* kbox;
  KeptGrid kg;                                      // spatial hash of the kept boxes (cross phase, iou_threshold >= 0.5)
  // round 4: in-tree radix sort (32-bit keys per image, ping-pong; rs.va is the first buffer of the workspace) + the multi-workgroup round
  RsBufs<unsigned> rs;
  unsigned long long* rowbits; float4* surv_box; unsigned* surv_idx; int* surv_n; int RND, NW;
};

// greedy NMS: box_geom.h's IoU from the stored fp32 areas above thr; false for boxes that do not overlap, whatever thr is
__device__ __forceinline__ bool suppresses(const float4& a, float aa, const float4& b, float ab, float thr) {
  float inter;
  return box_inter(a, b, inter) && inter / (aa + ab - inter) > thr;
}

// `me` against n kept boxes staged in LDS (tb / ta, padded to a multiple of 8 with boxes that suppress nothing).
// The obvious loop -- one box per iteration, break on the first hit -- is a chain of dependent LDS round trips (the
// break forbids hoisting the next read): measured 640 cycles per box, 71 % of the per-image round kernel.  Here 8
// boxes are fetched and tested per iteration with no exit in between, and the loop ends when the whole WAVE is
// dead; the extra comparisons cannot change the outcome (the answer is the OR over all n).
__device__ __forceinline__ bool scan_kept(const float4& me, float ma, const float4* tb, const float* ta, int n, bool alive, float thr) {
  for (int j0 = 0; j0 < n; j0 += 8) {
    float4 q[8]; float qa[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) { q[u] = tb[j0 + u]; qa[u] = ta[j0 + u]; }
    bool hit = false;
#pragma unroll
    for (int u = 0; u < 8; ++u) hit |= suppresses(me, ma, q[u], qa[u], thr);
    alive = alive && !hit;
    if (__ballot(alive) == 0ull) break;
  }
  return alive;
}
// sentinel for the padding slots: empty box far away -> negative overlap width -> never suppresses
__device__ __forceinline__ float4 no_box() { return make_float4(-3.0e30f, -3.0e30f, -3.0e30f, -3.0e30f); }

__global__ void nms_gather_kernel(const float* __restrict__ boxes, const unsigned* __restrict__ idx, const int* __restrict__ nvalid,
                                  float4* __restrict__ sbox, long long A, int B) {
  const long long total = A * B;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long b = i / A, r = i - b * A;
    if (r < nvalid[b]) sbox[i] = ((const float4*)boxes)[b * A + idx[i]];
  }
}

// ------------------------------------------------------------------ NMS: spatial hash of the KEPT boxes (iou_threshold >= 0.5)
// The cross phase (candidates of a round against every box kept in earlier rounds) was the largest part of the NMS: N x K / 2
// IoU tests per image (1.2e8 for D0's worst case, 1.7e9 for D4 @1024).  For thr >= 0.5 a suppressor must (a) have an area
// within a factor 2 and (b) contain the candidate's centre and have its own centre inside the candidate (the intersection
// covers more than half of either box along both axes).  So kept boxes are filed by (area octave, centre cell) in a hashed
// grid -- cell = half a box side, fixed capacity, one cache line per cell, overflow into a per-image list that everyone scans --
// and a candidate only visits the cells of <= 3 octaves that its own box covers: tens of tests instead of thousands.
// (Tried first and dropped: filing ALL candidates and resolving the greedy order by a whole-batch monotone fixed point --
//  exact, no rounds, but the dependency DAG of the dense-anchor worst case is ~40 layers deep and every sweep re-walks
//  ~400 divergent, uncoalesced entries per open candidate: 109 ms vs 5 ms for D0 B = 32.)
// The IoU arithmetic is `suppresses()`, bit for bit; boxes with non-positive / non-finite area suppress nothing and are never
// suppressed (exactly as there) and are not filed.  Rounding slack: the octave window is taken from a * (0.5, 2) widened by
// 2^-20 and the query rectangle is grown by 1e-4 of the box size, so a pair whose COMPUTED IoU exceeds thr is never missed;
// hash collisions only add tests.
constexpr int SB_MIN = 4, SB_MAX = 40;

__device__ __forceinline__ bool box_live(const float4& b, float a) {       // can take part in suppression at all
  return a > 0.f && a < 3.0e38f && fabsf(b.x) < 1.0e18f && fabsf(b.y) < 1.0e18f && fabsf(b.z) < 1.0e18f && fabsf(b.w) < 1.0e18f;
}
__device__ __forceinline__ int octave(float a) { const int e = ilogbf(a); return e < SB_MIN ? SB_MIN : (e > SB_MAX ? SB_MAX : e); }
__device__ __forceinline__ float inv_cell(int lvl) { return ldexpf(1.0f, 1 - (lvl >> 1)); }     // 1 / 2^(lvl/2 - 1): cell = half a side
__device__ __forceinline__ unsigned cell_hash(int lvl, int cx, int cy, unsigned mask) {
  return (((unsigned)lvl * 0x9E3779B1u) ^ ((unsigned)cx * 73856093u) ^ ((unsigned)cy * 83492791u)) & mask;
}
__device__ __forceinline__ int cell_of(float v, float inv) { return (int)fminf(fmaxf(floorf(v * inv), -1.0e9f), 1.0e9f); }

// file one kept box of image b (called by the per-image round kernel: the only writer of that image's grid)
__device__ __forceinline__ void kg_insert(const KeptGrid& kg, long long b, long long A, const float4& bx) {
  const float a = box_area(bx);
  if (!box_live(bx, a)) return;
  const int lvl = octave(a);
  const float inv = inv_cell(lvl);
  const long long hs = b * kg.HT + cell_hash(lvl, cell_of(0.5f * (bx.x + bx.z), inv), cell_of(0.5f * (bx.y + bx.w), inv), (unsigned)kg.HT - 1u);
  const int pos = atomicAdd(kg.kcount + hs, 1);
  if (pos < KG_CAP) kg.kcell[hs * KG_CAP + pos] = bx;
  else kg.kover[b * A + atomicAdd(kg.kover_n + b, 1)] = bx;
}

// Kernel A': candidates of round `round` vs the hashed grid of boxes kept in earlier rounds.  ONE WAVE per candidate: a thread
// per candidate walks ~20 cells as a chain of dependent global loads (measured 110 us per round, no better than brute force);
// here the 64 lanes take (cell, entry) pairs -- 8 cells x 8 entries per pass, count and box loads independent of each other --
// so a candidate costs a handful of round trips and a round of 2048 candidates fills the chip (B x 2048 waves).
__global__ __launch_bounds__(256) void nms_cross_grid_kernel(const float4* __restrict__ sbox, const KeptGrid kg, const int* nvalid,
                                                             unsigned* dead, long long A, int round, float thr, int RND) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const long long i = (long long)round * RND + blockIdx.x * 4LL + (threadIdx.x >> 6);
  if (i >= A) return;                                                // wave-uniform (structural bound: sbox has A slots per image)
  // three independent loads in flight (round 4: the count used to gate the box load -- two dependent L2 round trips per wave)
  const int nv = nvalid[b];
  const float4 me = sbox[b * A + i];
  const int no = kg.kover_n[b];
  if (i >= nv) return;                                               // wave-uniform
  const float ma = box_area(me);
  if (!box_live(me, ma)) return;
  const float ex = 1.0e-4f * (me.z - me.x) + 1.0e-6f, ey = 1.0e-4f * (me.w - me.y) + 1.0e-6f;
  const float qx0 = me.x - ex, qx1 = me.z + ex, qy0 = me.y - ey, qy1 = me.w + ey;
  const int l0 = octave(ma * 0.4999995f), l1 = octave(ma * 2.000002f);          // <= 4 octaves
  const unsigned mask = (unsigned)kg.HT - 1u;
  int cxa[4], cya[4], nxa[4], base[5];
  base[0] = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int lvl = l0 + k;
    int nx = 0, ny = 0; cxa[k] = 0; cya[k] = 0;
    if (lvl <= l1) {
      const float inv = inv_cell(lvl);
      cxa[k] = cell_of(qx0, inv); cya[k] = cell_of(qy0, inv);
      nx = cell_of(qx1, inv) - cxa[k] + 1; ny = cell_of(qy1, inv) - cya[k] + 1;
    }
    nxa[k] = nx;
    const long long cells = (long long)nx * ny;
    base[k + 1] = base[k] + (int)(cells > 100000000LL ? 100000000LL : cells);   // (absurd extents: clamp; such boxes are scanned exhaustively below)
  }
  const int T = base[4];
  bool hit = false;
  if (T >= 100000000) {
    // a box spanning > 1e8 cells (coordinates ~1e9 px): walk the image's cells linearly instead -- every filed box is visited
    for (long long hs0 = lane; hs0 < (long long)kg.HT * KG_CAP && !__ballot(hit); hs0 += 64) {
      const long long hs = (long long)b * kg.HT + hs0 / KG_CAP; const int e = (int)(hs0 % KG_CAP);
      if (e < min(kg.kcount[hs], KG_CAP)) { const float4 q = kg.kcell[hs * KG_CAP + e]; hit = suppresses(me, ma, q, box_area(q), thr); }
    }
  } else {
    // Two dependent steps instead of streaming every probed cell: (1) one lane per CELL reads its 4-byte occupancy count -- the count
    // table is 4 MB for 32 images and lives in L2, and ~85 % of the probed cells are empty; (2) the lanes then take (non-empty cell,
    // entry) pairs, 8 cells x 8 entries per pass.  Reading the 128-byte line of EVERY probed cell (round 3: ~50 cells per candidate out
    // of a 134 MB table) moved ~400 MB per round: the kernel ran at the bandwidth of random 128-byte lines, 73-80 us per round.
    const int e = lane & 7, slot = lane >> 3;
    for (int c0 = 0; c0 < T && !hit; c0 += 64) {
      const int c = c0 + lane;
      const bool in = c < T;
      const int cc = in ? c : 0;
      const int k = (cc >= base[1]) + (cc >= base[2]) + (cc >= base[3]);
      const int r = cc - base[k], nx = nxa[k] > 0 ? nxa[k] : 1;
      const int cy = r / nx, cx = r - cy * nx;
      const long long hs = (long long)b * kg.HT + cell_hash(l0 + k, cxa[k] + cx, cya[k] + cy, mask);
      const int cnt = kg.kcount[hs];                                   // (lanes past T read cell 0 of their first octave: masked)
      const int n = in ? min(cnt, KG_CAP) : 0;
      unsigned long long ne = __ballot(n > 0);                         // non-empty cells of this pass (uniform)
      const int hs_lo = (int)(hs & 0xffffffffll), hs_hi = (int)(hs >> 32);
      while (ne) {                                                     // uniform: up to 8 non-empty cells per step
        int src = 0, found = 0;
        unsigned long long m = ne;
#pragma unroll
        for (int q8 = 0; q8 < 8; ++q8) {
          const int pos = m ? __builtin_ctzll(m) : 0;
          if (q8 == slot) { src = pos; found = m != 0ull; }
          m &= m - 1ull;                                               // (0 & anything stays 0)
        }
        ne = m;
        const int n_s = __shfl(n, src, 64);
        const long long hs_s = ((long long)__shfl(hs_hi, src, 64) << 32) | (unsigned)__shfl(hs_lo, src, 64);
        const float4 q = kg.kcell[hs_s * KG_CAP + e];                  // (src = 0 for unused slots: a valid line, masked by found)
        const bool h = found && e < n_s && suppresses(me, ma, q, box_area(q), thr);
        if (__ballot(h)) { hit = true; break; }
      }
    }
  }
  if (!__ballot(hit)) {
    for (int e0 = 0; e0 < no; e0 += 64) {
      bool h = false;
      if (e0 + lane < no) { const float4 q = kg.kover[b * A + e0 + lane]; h = suppresses(me, ma, q, box_area(q), thr); }
      if (__ballot(h)) { hit = true; break; }
    }
  }
  if (__ballot(hit) && lane == 0) dead[b * A + i] = 1u;
}

// Kernel A: candidates of round `round` vs boxes kept in earlier rounds (split over blockIdx.z).
__global__ __launch_bounds__(NT) void nms_cross_kernel(const float4* __restrict__ sbox, const float4* kbox, const int* nvalid,
                                                       const int* kept, unsigned* dead, long long A, int round, int splits, float thr, int RND) {
  __shared__ float4 kb[NT + 8];
  __shared__ float ka[NT + 8];
  const int b = blockIdx.x, sub = blockIdx.y, sp = blockIdx.z;
  const int nv = nvalid[b], kc = kept[b];
  const long long i = (long long)round * RND + sub * NT + threadIdx.x;
  if ((long long)round * RND + (long long)sub * NT >= nv) return;
  const int k0 = (int)((long long)kc * sp / splits), k1 = (int)((long long)kc * (sp + 1) / splits);
  if (k0 >= k1) return;
  const bool valid = i < nv;
  float4 me = make_float4(0, 0, 0, 0); float ma = 0.f;
  if (valid) { me = sbox[b * A + i]; ma = (me.z - me.x) * (me.w - me.y); }
  bool alive = valid;
  for (int c0 = k0; c0 < k1; c0 += NT) {
    const int n = min(NT, k1 - c0);
    __syncthreads();
    if ((int)threadIdx.x < n) { const float4 q = kbox[b * A + c0 + threadIdx.x]; kb[threadIdx.x] = q; ka[threadIdx.x] = (q.z - q.x) * (q.w - q.y); }
    else if ((int)threadIdx.x < n + 8) { kb[threadIdx.x] = no_box(); ka[threadIdx.x] = 0.f; }
    if (threadIdx.x < 8) { kb[NT + threadIdx.x] = no_box(); ka[NT + threadIdx.x] = 0.f; }
    __syncthreads();
    alive = scan_kept(me, ma, kb, ka, n, alive, thr);
  }
  if (valid && !alive) dead[b * A + i] = 1u;
}

// ------------------------------------------------------------------ NMS, round 4: in-tree sort + a round spread over the GPU
// (1) Stable LSD radix sort of the B equal-length segments (one per image) of 32-bit keys with their anchor indices: 4 passes of
//     8 bits, each pass = histogram per 4096-key tile -> per-image exclusive scan over (digit, tile) -> stable scatter (inside a
//     workgroup the keys are ranked 256 at a time: wave-level match by 8 ballots, per-wave digit counts, running digit cursors).
//     Replaces rocprim::radix_sort_pairs (the one third-party device routine on the path; its captured replay faulted, which kept
//     NMS out of the detection graph).  Nothing here depends on run-time data for its launch geometry: capture-safe.
// (2) A round (RND = 2048 candidates; 4096 for > 64 k anchors) is three launches: the cross phase above (whole GPU) marks
//     candidates suppressed by boxes kept in EARLIER rounds; nms_matrix_kernel (G workgroups per image) compacts the round's
//     survivors and computes their suppression bit-matrix -- one wave per (64-row block, 64-column word), every lane its own row
//     against the same 64 staged boxes, one coalesced 512-byte store of the word column -- into global memory (word-major); and
//     nms_resolve_kernel (one WAVE per image) walks the rows in blocks of 64 exactly like the single-workgroup kernel did (earlier
//     kept words AND-ed against the row, one ballot per kept box inside the block), appends the kept boxes in order and files them
//     into the kept-box grid.  The old per-image round kernel did all of this on ONE CU per image (32 of 256 CUs at B = 32) and was
//     2/3 of the decode + NMS time.

// The per-call resets as ONE kernel (three integer regions) instead of hipMemsetAsync nodes, and the final count written by the
// resolve kernel instead of a hipMemcpyAsync: the captured NMS is then made of kernel nodes only.
__global__ __launch_bounds__(256) void nms_reset_kernel(int* a, long long na, int* b, long long nb, int* c, long long nc) {
  const long long n = na + nb + nc;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    if (i < na) a[i] = 0; else if (i < na + nb) b[i - na] = 0; else c[i - na - nb] = 0;
  }
}

__global__ __launch_bounds__(256) void nms_keys32_kernel(const float* __restrict__ score, float thr, unsigned* keys, unsigned* vals,
                                                         int* nvalid, int* kept, unsigned* dead, long long A) {
  const int b = blockIdx.y;
  __shared__ int cnt[4];
  int mine = 0;
  for (long long a = blockIdx.x * 256LL + threadIdx.x; a < A; a += (long long)gridDim.x * 256) {
    const long long i = (long long)b * A + a;
    const float s = score[i];
    unsigned k = 0xffffffffu;
    if (s > thr) {
      k = rs_score_key(s);
      if (k == 0xffffffffu) k = 0xfffffffeu;          // (0xffffffff is the key of the invalid ones)
      ++mine;
    }
    keys[i] = k; vals[i] = (unsigned)a; dead[i] = 0u;
  }
  mine = (int)wave_sum((float)mine);
  if ((threadIdx.x & 63) == 0) cnt[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int t = cnt[0] + cnt[1] + cnt[2] + cnt[3];
    if (t) atomicAdd(nvalid + b, t);
    if (blockIdx.x == 0) kept[b] = 0;
  }
}

struct NmsRound { unsigned long long* rowbits; float4* surv_box; unsigned* surv_idx; int* surv_n; int RND, NW; };

// grid (G, B): the survivors of round `round` of image b and the word columns (rb, w), w <= rb, of their suppression bit-matrix.
// rowbits[b][w][r] bit j: survivor 64 w + j (an EARLIER survivor) suppresses survivor r.
__global__ __launch_bounds__(256) void nms_matrix_kernel(const float4* __restrict__ sbox, const unsigned* __restrict__ sidx,
                                                         const int* __restrict__ nvalid, const unsigned* __restrict__ dead,
                                                         const NmsRound q, long long A, int round, float thr) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  float4* tb = (float4*)smem_raw;                                      // [RND + 64] survivor boxes
  float* ta = (float*)(tb + q.RND + 64);                               // [RND + 64] areas
  __shared__ int wcnt[8][4];
  const int g = blockIdx.x, G = gridDim.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nv = nvalid[b];
  const long long r0 = (long long)round * q.RND;
  if (r0 >= nv) return;
  const unsigned long long lt = (1ull << lane) - 1ull;
  int S = 0;
  for (int h0 = 0; h0 < q.RND; h0 += 2048) {                           // 8 chunks of 256 candidates at a time: their loads share a round trip
    if (r0 + h0 >= nv) break;                                          // uniform
    unsigned dd[8]; float4 bx[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const long long i = r0 + h0 + u * 256 + tid;
      const long long ii = i < A ? i : A - 1;                          // (always a valid slot; masked below)
      dd[u] = dead[b * A + ii]; bx[u] = sbox[b * A + ii];
    }
    // order-preserving compaction of the 8 chunks with TWO barriers (all ballots, then all offsets) instead of two per chunk
    unsigned long long bal[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int c0 = h0 + u * 256;
      const long long i = r0 + c0 + tid;
      const bool alive = c0 < q.RND && i < nv && dd[u] == 0u;
      bal[u] = __ballot(alive);
      if (lane == 0) wcnt[u][wave] = __popcll(bal[u]);
    }
    __syncthreads();
    int run = S;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      int off = run, tot = 0;
#pragma unroll
      for (int w = 0; w < 4; ++w) { const int c = wcnt[u][w]; if (w < wave) off += c; tot += c; }
      if ((bal[u] >> lane) & 1ull) {
        const int sl = off + __popcll(bal[u] & lt);
        const float4 me = bx[u];
        tb[sl] = me; ta[sl] = (me.z - me.x) * (me.w - me.y);
        if (g == 0) { q.surv_box[(long long)b * q.RND + sl] = me; q.surv_idx[(long long)b * q.RND + sl] = sidx[b * A + r0 + h0 + u * 256 + tid]; }
      }
      run += tot;
    }
    S = run;
    __syncthreads();
  }
  if (tid < 64) { tb[S + tid] = no_box(); ta[S + tid] = 0.f; }         // columns past S suppress nothing
  if (g == 0 && tid == 0) q.surv_n[b] = S;
  __syncthreads();
  const int nb = (S + 63) >> 6, items = nb * (nb + 1) / 2;
  for (int item = g * 4 + wave; item < items; item += G * 4) {         // (rb, w) pairs in row-block-major order
    int rb = (int)((sqrtf(8.f * (float)item + 1.f) - 1.f) * 0.5f);
    while ((rb + 1) * (rb + 2) / 2 <= item) ++rb;
    while (rb * (rb + 1) / 2 > item) --rb;
    const int w = item - rb * (rb + 1) / 2;
    const int r = rb * 64 + lane;
    const float4 me = tb[r]; const float ma = ta[r];                   // (rows past S read the sentinels: all-zero words)
    unsigned long long bits = 0ull;
#pragma unroll 1
    for (int j0 = 0; j0 < 64; j0 += 8) {
      float4 c[8]; float ca[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) { c[u] = tb[w * 64 + j0 + u]; ca[u] = ta[w * 64 + j0 + u]; }
#pragma unroll
      for (int u = 0; u < 8; ++u) if (suppresses(me, ma, c[u], ca[u], thr)) bits |= 1ull << (j0 + u);
    }
    if (w == rb) bits &= lt;                                           // only EARLIER survivors count
    if (r < S) q.rowbits[((long long)b * q.NW + w) * q.RND + r] = bits;
  }
}

// grid B, ONE wave per image: the greedy order of the round's survivors from the bit-matrix, == sequential greedy NMS.
// Column form: once block blk's kept set K is known, every LATER row r' is dead iff rowbits[blk][r'] & K -- the loads of word column
// blk (rows blk*64 ..) do not depend on K, so they are issued (8 blocks = 8 independent 512-byte loads at a time, the first carrying
// the block's own diagonal word) before the block's ballot loop and consumed after it: one L2 round trip per block instead of
// ceil(blk / 4) + 1.  The kept boxes' grid insertion (an atomic whose result addresses a store) is software-pipelined one block
// behind for the same reason.
__global__ __launch_bounds__(64) void nms_resolve_kernel(const NmsRound q, const int* __restrict__ nvalid, int* kept, float4* kbox, int* out_idx,
                                                         int* out_count, long long A, int round, const KeptGrid kg) {
  __shared__ unsigned long long gonew[64];                              // per row block: rows already suppressed by earlier kept boxes
  const int b = blockIdx.x, lane = threadIdx.x;
  if ((long long)round * q.RND >= nvalid[b]) return;
  const int S = q.surv_n[b];
  int kc = kept[b];
  const int nw = (S + 63) >> 6;
  const unsigned long long lt = (1ull << lane) - 1ull;
  const unsigned long long* rows = q.rowbits + (long long)b * q.NW * q.RND;
  gonew[lane] = 0ull;
  __syncthreads();
  // pending grid insertion of the previous block's kept boxes
  bool pend = false; long long pend_hs = 0; int pend_pos = 0; float4 pend_box = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int blk = 0; blk < nw; ++blk) {
    const int r = blk * 64 + lane;
    // ---- loads of this block: word column blk for row blocks blk .. blk+7 (first = the diagonal word), the block's boxes ----
    unsigned long long col[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int rr = min((blk + j) * 64 + lane, q.RND - 1);           // (in range; blocks past nw are ignored below)
      col[j] = rows[(long long)blk * q.RND + rr];
    }
    const float4 bx = q.surv_box[(long long)b * q.RND + min(r, q.RND - 1)];
    const unsigned sidx_r = q.surv_idx[(long long)b * q.RND + min(r, q.RND - 1)];
    // ---- the previous block's pending grid insertion (its atomic has long returned) ----
    if (pend) {
      if (pend_pos < KG_CAP) kg.kcell[pend_hs * KG_CAP + pend_pos] = pend_box;
      else kg.kover[b * A + atomicAdd(kg.kover_n + b, 1)] = pend_box;
      pend = false;
    }
    const bool gone = r >= S || ((gonew[blk] >> lane) & 1ull);
    const unsigned long long diag = r < S ? col[0] : 0ull;
    unsigned long long cand = __ballot(!gone), keep = 0ull;
    while (cand) {                                                     // uniform
      const int i = __builtin_ctzll(cand);
      keep |= 1ull << i;
      cand &= ~(__ballot((diag >> i) & 1ull) | (1ull << i));           // a row's bits only name earlier rows: lanes > i
    }
    // ---- later rows suppressed by this block's kept boxes ----
#pragma unroll
    for (int j = 1; j < 8; ++j) {
      const unsigned long long bal = __ballot((col[j] & keep) != 0ull);
      if (blk + j < nw && lane == 0) gonew[blk + j] |= bal;
    }
    for (int b2 = blk + 8; b2 < nw; b2 += 8) {                         // (more than 8 later blocks: S > 512 past this block)
      unsigned long long c2[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) c2[j] = rows[(long long)blk * q.RND + min((b2 + j) * 64 + lane, q.RND - 1)];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const unsigned long long bal = __ballot((c2[j] & keep) != 0ull);
        if (b2 + j < nw && lane == 0) gonew[b2 + j] |= bal;
      }
    }
    __syncthreads();                                                   // (one wave: orders lane 0's LDS writes before the next block's reads)
    // ---- append the kept boxes in order; start their grid insertion ----
    if ((keep >> lane) & 1ull) {
      const int pos = kc + __popcll(keep & lt);
      kbox[b * A + pos] = bx;
      out_idx[b * A + pos] = (int)sidx_r;
      if (kg.kcount) {
        const float a = box_area(bx);
        if (box_live(bx, a)) {
          const int lvl = octave(a);
          const float inv = inv_cell(lvl);
          pend_hs = (long long)b * kg.HT + cell_hash(lvl, cell_of(0.5f * (bx.x + bx.z), inv), cell_of(0.5f * (bx.y + bx.w), inv), (unsigned)kg.HT - 1u);
          pend_pos = atomicAdd(kg.kcount + pend_hs, 1);
          pend_box = bx; pend = true;
        }
      }
    }
    kc += __popcll(keep);
  }
  if (pend) {
    if (pend_pos < KG_CAP) kg.kcell[pend_hs * KG_CAP + pend_pos] = pend_box;
    else kg.kover[b * A + atomicAdd(kg.kover_n + b, 1)] = pend_box;
  }
  if (lane == 0) { kept[b] = kc; out_count[b] = kc; }
}

__global__ void gather_dets_kernel(const float* __restrict__ boxes, const float* __restrict__ score, const int* __restrict__ label,
                                   const int* __restrict__ idx, const int* __restrict__ count, float* __restrict__ os,
                                   long long* __restrict__ ol, float* __restrict__ ob, long long A, int B) {
  const long long total = A * B;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long b = i / A, r = i - b * A;
    if (r < count[b]) {
      const long long src = b * A + idx[i];
      os[i] = score[src]; ol[i] = (long long)label[src]; ((float4*)ob)[i] = ((const float4*)boxes)[src];
    }
  }
}

// ------------------------------------------------------------------ rescoring NMS (Soft-NMS; hard / per-class suppression as special cases)
// Same keys and sort as the greedy path; then ONE workgroup per image keeps the first n = min(candidates, top_n) sorted candidates in
// LDS (box 16 B, area, running score, label: 28 B each, 112 KB at the 4096 cap) and runs the sequential pick loop: pick the live
// candidate with the largest running score (ties: smallest sorted position), emit it, rescore the live candidates (of its class).
// A thread owns the candidates q = tid, tid + 1024, ..: it alone reads and writes their running scores, and while it rescores them for
// pick k it already keeps its best for pick k + 1 -- so a pick is one sweep, one wave + cross-wave arg-max and ONE barrier (the
// reduction slots ping-pong; boxes, areas and labels are never written after the load).  A dead candidate's score is -inf, so
// "live" is `s > threshold` everywhere.  Degenerate boxes (area not positive and finite) neither rescore nor are rescored.
constexpr int SN_T = 1024, SN_MAX = 4096;
constexpr float SN_DEAD = -__builtin_huge_valf();

struct SoftNms {
  const float* boxes; const float* score; const int* label; const unsigned* sidx; const int* nvalid;
  int* out_idx; float* out_score; int* out_count; long long A;
  float thr, iou_thr, sigma; int method, top_n, max_det;
};

// the (score, sorted position) arg-max of a pick goes by block_best.h's order; dead entries are (-inf, INT_MAX)

__global__ __launch_bounds__(SN_T) void soft_nms_kernel(const SoftNms p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  float4* tb = (float4*)smem_raw;                                      // [top_n] boxes in sorted order
  float* ta = (float*)(tb + p.top_n);                                  // [top_n] areas
  float* ts = ta + p.top_n;                                            // [top_n] running scores (owner thread only)
  int* tl = (int*)(ts + p.top_n);                                      // [top_n] labels (0 when class-agnostic)
  __shared__ float red_s[2][SN_T / 64];
  __shared__ int red_q[2][SN_T / 64];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long base = (long long)b * p.A;
  const int n = min(p.nvalid[b], p.top_n);
  float bs = SN_DEAD; int bq = 0x7fffffff;
  for (int q = tid; q < n; q += SN_T) {
    const long long src = base + p.sidx[base + q];
    const float4 bx = ((const float4*)p.boxes)[src];
    const float s = p.score[src];                                      // (> thr: it is a candidate)
    tb[q] = bx; ta[q] = box_area(bx); ts[q] = s; tl[q] = p.label ? p.label[src] : 0;
    best_take(bs, bq, s, q);
  }
  int k = 0;
  for (; k < p.max_det; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best_take(bs, bq, __shfl_xor(bs, o, 64), __shfl_xor(bq, o, 64));
    if (lane == 0) { red_s[k & 1][wave] = bs; red_q[k & 1][wave] = bq; }
    __syncthreads();                                                   // (also publishes the loads above before pick 0 reads a box)
    float ws = red_s[k & 1][lane & 15]; int wq = red_q[k & 1][lane & 15];
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) best_take(ws, wq, __shfl_xor(ws, o, 64), __shfl_xor(wq, o, 64));
    if (!(ws > p.thr)) break;                                          // nothing live (block-uniform: every thread reduced the same 16 slots)
    if (tid == 0) { p.out_idx[base + k] = (int)p.sidx[base + wq]; p.out_score[base + k] = ws; }
    const float4 pb = tb[wq]; const float pa = ta[wq]; const int pl = tl[wq];
    const bool pick_ok = pos_finite(pa);
    bs = SN_DEAD; bq = 0x7fffffff;
    for (int q = tid; q < n; q += SN_T) {
      float s = ts[q];
      if (q == wq) { s = SN_DEAD; ts[q] = s; }
      else if (s > p.thr && pick_ok && tl[q] == pl) {
        const float a = ta[q];
        if (pos_finite(a)) {
          const float iou = box_iou(pb, pa, tb[q], a);
          if (p.method == 0) { if (iou > p.iou_thr) s = SN_DEAD; }
          else if (p.method == 1) { if (iou > p.iou_thr) s = s * (1.f - iou); }
          else s = s * expf(-(iou * iou) / p.sigma);
          if (!(s > p.thr)) s = SN_DEAD;
          ts[q] = s;
        }
      }
      best_take(bs, bq, s, q);
    }
  }
  if (tid == 0) p.out_count[b] = k;
}

// candidates per round of the multi-workgroup form: 2048 (D0 @512: 24 rounds), 4096 above 64 k anchors (D4 @1024: 48 rounds);
// EFFDET_NMS_ROUND overrides (A/B)
inline int nms_round_size(long long A) {
  static const int env = getenv("EFFDET_NMS_ROUND") ? atoi(getenv("EFFDET_NMS_ROUND")) : 0;
  if (env >= 256 && env <= 4096 && (env & 63) == 0) return env;
  return A > 65536 ? 4096 : 2048;
}

size_t carve(NmsWs& w, void* base, int B, long long A) {
  const size_t n = (size_t)B * A;
  Carver c(base);
  w.rs.va = c.take<unsigned>(n);
  w.dead = c.take<unsigned>(n);
  w.sbox = c.take<float4>(n); w.kbox = c.take<float4>(n);
  w.nvalid = c.take<int>(B); w.kept = c.take<int>(B);
  int ht = 1024; while (ht < A / 2) ht <<= 1;      // hash slots per image (kept boxes are a fraction of the candidates), a power of two
  w.kg.HT = ht;
  w.kg.kcount = c.take<int>((size_t)B * ht); w.kg.kover_n = c.take<int>(B);
  w.kg.kcell = c.take<float4>((size_t)B * ht * KG_CAP); w.kg.kover = c.take<float4>(n);
  // in-tree radix sort (32-bit keys per image, ping-pong) + the multi-workgroup round
  rs_carve(w.rs, c, B, A, false);
  w.RND = nms_round_size(A); w.NW = w.RND / 64;
  w.rowbits = c.take<unsigned long long>((size_t)B * w.NW * w.RND);
  w.surv_box = c.take<float4>((size_t)B * w.RND); w.surv_idx = c.take<unsigned>((size_t)B * w.RND); w.surv_n = c.take<int>(B);
  return c.off;
}

// workspace of the rescoring NMS: the sort's ping-pong pairs and histograms, and what nms_keys32_kernel writes besides the keys
struct SoftNmsWs { RsBufs<unsigned> rs; unsigned* dead; int* nvalid; int* kept; };

size_t carve(SoftNmsWs& w, void* base, int B, long long A) {
  Carver c(base);
  rs_carve(w.rs, c, B, A);
  w.dead = c.take<unsigned>((size_t)B * A);
  w.nvalid = c.take<int>(B); w.kept = c.take<int>(B);
  return c.off;
}

}  // namespace

extern "C" long long effdet_num_anchors(int H, int W) {
  long long n = 0;
  for (int l = 3; l <= 7; ++l) { const int s = 1 << l; n += (long long)((H + s - 1) / s) * ((W + s - 1) / s) * 9; }
  return n;
}

extern "C" int effdet_anchors(float* out, int H, int W, effdet_stream_t stream) {
  if (!out || H <= 0 || W <= 0) return EFFDET_EINVAL;
  AnchorK k;
  // models/module.py:183-214 in float64, same operation order as NumPy (IEEE sqrt / div are exact)
  const double scales[3] = {1.0, 0x1.428a2f98d728bp+0 /* 2**(1/3) */, 0x1.965fea53d6e3cp+0 /* 2**(2/3) */};
  const double ratios[3] = {0.5, 1.0, 2.0};
  long long start = 0;
  for (int l = 0; l < 5; ++l) {
    const double base = (double)(1 << (l + 5));       // 2 ** (level + 2), level = l + 3
    for (int a = 0; a < 9; ++a) {
      const double s = base * scales[a % 3];
      const double area = s * s;
      const double r = ratios[a / 3];
      const double w = sqrt(area / r);
      const double h = w * r;
      k.base[l][a][0] = 0.0 - w * 0.5; k.base[l][a][1] = 0.0 - h * 0.5;
      k.base[l][a][2] = w - w * 0.5;   k.base[l][a][3] = h - h * 0.5;
    }
    const int st = 1 << (l + 3);
    k.fh[l] = (H + st - 1) / st; k.fw[l] = (W + st - 1) / st;
    k.start[l] = start; start += (long long)k.fh[l] * k.fw[l] * 9;
  }
  k.out = out; k.total = start;
  hipLaunchKernelGGL(anchors_kernel, dim3(grid_for(start)), dim3(256), 0, (hipStream_t)stream, k);
  EFFDET_CHECK_LAUNCH();
  return EFFDET_OK;
}

extern "C" int effdet_decode_score(const float* anchors, const float* reg, const float* cls, float* boxes, float* score,
                                   int* label, int B, long long A, int num_classes, float img_w, float img_h,
                                   effdet_stream_t stream) {
  if (!anchors || !reg || !cls || !boxes || !score || !label || num_classes < 1) return EFFDET_EINVAL;
  const long long n = (long long)B * A;
  const size_t lds = (size_t)64 * (num_classes + 1) * sizeof(float);
  if (lds > 150 * 1024) return EFFDET_EUNSUPPORTED;
  if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)decode_score_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(decode_score_kernel, dim3((unsigned)((n + 63) / 64)), dim3(256), lds, (hipStream_t)stream, anchors, reg, cls, boxes, score, label, A, num_classes, img_w, img_h, n);
  EFFDET_CHECK_LAUNCH();
  return EFFDET_OK;
}

extern "C" long long effdet_nms_workspace_bytes(int B, long long A) {
  NmsWs w;
  return (long long)carve(w, nullptr, B, A);
}

extern "C" int effdet_nms(const float* boxes, const float* score, float threshold, float iou_threshold, int* out_idx,
                          int* out_count, void* workspace, long long workspace_bytes, int B, long long A,
                          effdet_stream_t stream) {
  if (!boxes || !score || !out_idx || !out_count || !workspace || B < 1 || A < 1) return EFFDET_EINVAL;
  NmsWs w;
  const size_t need = carve(w, workspace, B, A);
  if ((long long)need > workspace_bytes) return EFFDET_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const long long n = (long long)B * A;
  static const int grid_env = getenv("EFFDET_NMS_GRID") ? atoi(getenv("EFFDET_NMS_GRID")) : 1;       // A/B switch (0 = brute-force cross phase)
  const bool use_grid = grid_env && iou_threshold >= 0.5f;
  KeptGrid kg = w.kg;
  // resets: nvalid [B], out_count [B] (stays 0 for an image without candidates) and, with the kept-box grid, its cell counters
  hipLaunchKernelGGL(nms_reset_kernel, dim3(use_grid ? 512 : 1), dim3(256), 0, st, w.nvalid, (long long)B, out_count, (long long)B,
                     use_grid ? kg.kcount : kg.kover_n, use_grid ? (long long)B * kg.HT + 0 : (long long)B);
  EFFDET_CHECK_LAUNCH();
  if (use_grid) {
    hipLaunchKernelGGL(nms_reset_kernel, dim3(1), dim3(256), 0, st, kg.kover_n, (long long)B, (int*)nullptr, 0LL, (int*)nullptr, 0LL);
    EFFDET_CHECK_LAUNCH();
  } else {
    kg.kcount = nullptr;
  }
  // ---- keys, in-tree stable radix sort per image (4 x 8 bits), boxes in sorted order ----
  {
    { long long gx = (A + 2047) / 2048; if (gx > 64) gx = 64;      // (one atomic per workgroup onto nvalid[b]: 32 counters in ONE cache line serialise at ~8 ns each)
      hipLaunchKernelGGL(nms_keys32_kernel, dim3((unsigned)gx, B), dim3(256), 0, st, score, threshold, w.rs.ka, w.rs.va, w.nvalid, w.kept, w.dead, A); }
    EFFDET_CHECK_LAUNCH();
    unsigned *ki = w.rs.ka, *vi = w.rs.va, *ko = w.rs.kb, *vo = w.rs.vb;
    if (const int rc = rs_sort(ki, vi, ko, vo, w.rs.hist, B, A, w.rs.T, 0, 4, st)) return rc;
    hipLaunchKernelGGL(nms_gather_kernel, dim3(grid_for(n)), dim3(256), 0, st, boxes, (const unsigned*)vi, w.nvalid, w.sbox, A, B);
    EFFDET_CHECK_LAUNCH();
    // ---- rounds: cross phase (whole GPU) -> survivors + bit-matrix (G workgroups per image) -> greedy resolve (one wave per image) ----
    NmsRound q; q.rowbits = w.rowbits; q.surv_box = w.surv_box; q.surv_idx = w.surv_idx; q.surv_n = w.surv_n; q.RND = w.RND; q.NW = w.NW;
    const int RND = w.RND, rounds = (int)((A + RND - 1) / RND);
    int G = 2048 / B; if (G < 2) G = 2; if (G > 16) G = 16;                          // ~2048 workgroups of 4 waves per launch
    const size_t lds2 = (size_t)(RND + 64) * (16 + 4);
    EFFDET_SET_MAX_LDS((nms_matrix_kernel), (size_t)(4096 + 64) * (16 + 4));      // (the largest round size: the attribute is set once per device)
    for (int r = 0; r < rounds; ++r) {
      if (r > 0 && use_grid) {
        hipLaunchKernelGGL(nms_cross_grid_kernel, dim3(RND / 4, B), dim3(256), 0, st, w.sbox, kg, w.nvalid, w.dead, A, r, iou_threshold, RND);
        EFFDET_CHECK_LAUNCH();
      } else if (r > 0) {
        hipLaunchKernelGGL(nms_cross_kernel, dim3(B, RND / NT, 16), dim3(NT), 0, st, w.sbox, w.kbox, w.nvalid, w.kept, w.dead, A, r, 16, iou_threshold, RND);
        EFFDET_CHECK_LAUNCH();
      }
      hipLaunchKernelGGL(nms_matrix_kernel, dim3(G, B), dim3(256), lds2, st, w.sbox, (const unsigned*)vi, w.nvalid, w.dead, q, A, r, iou_threshold);
      hipLaunchKernelGGL(nms_resolve_kernel, dim3(B), dim3(64), 0, st, q, w.nvalid, w.kept, w.kbox, out_idx, out_count, A, r, kg);
      EFFDET_CHECK_LAUNCH();
    }
    return EFFDET_OK;
  }
}

extern "C" long long effdet_soft_nms_workspace_bytes(int B, long long A, int pre_nms_top_n) {
  (void)pre_nms_top_n;                                 // (the top-N candidates live in LDS; the workspace is the sort's)
  if (B < 1 || A < 1) return 0;
  SoftNmsWs w;
  return (long long)carve(w, nullptr, B, A);
}

extern "C" int effdet_soft_nms(const float* boxes, const float* score, const int* label, float threshold, float iou_threshold,
                               int method, float sigma, int class_aware, int pre_nms_top_n, int max_det, int* out_idx,
                               float* out_score, int* out_count, void* workspace, long long workspace_bytes, int B, long long A,
                               effdet_stream_t stream) {
  if (!boxes || !score || !out_idx || !out_score || !out_count || !workspace || B < 1 || A < 1) return EFFDET_EINVAL;
  if ((label != nullptr) != (class_aware != 0)) return EFFDET_EINVAL;
  if (method < 0 || method > 2 || pre_nms_top_n < 1 || pre_nms_top_n > SN_MAX || max_det < 1 || max_det > pre_nms_top_n || !(sigma > 0.f))
    return EFFDET_EUNSUPPORTED;
  SoftNmsWs w;
  const size_t need = carve(w, workspace, B, A);
  if ((long long)need > workspace_bytes) return EFFDET_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  // resets as a kernel (no memset nodes): nvalid [B], and the output rows -- rows past the count stay index 0, score 0 (+0.f is all-zero bits)
  hipLaunchKernelGGL(nms_reset_kernel, dim3(512), dim3(256), 0, st, w.nvalid, (long long)B, out_idx, (long long)B * A, (int*)out_score, (long long)B * A);
  EFFDET_CHECK_LAUNCH();
  { long long gx = (A + 2047) / 2048; if (gx > 64) gx = 64;
    hipLaunchKernelGGL(nms_keys32_kernel, dim3((unsigned)gx, B), dim3(256), 0, st, score, threshold, w.rs.ka, w.rs.va, w.nvalid, w.kept, w.dead, A); }
  EFFDET_CHECK_LAUNCH();
  unsigned *ki = w.rs.ka, *vi = w.rs.va, *ko = w.rs.kb, *vo = w.rs.vb;
  if (const int rc = rs_sort(ki, vi, ko, vo, w.rs.hist, B, A, w.rs.T, 0, 4, st)) return rc;
  SoftNms p;
  p.boxes = boxes; p.score = score; p.label = label; p.sidx = vi; p.nvalid = w.nvalid;
  p.out_idx = out_idx; p.out_score = out_score; p.out_count = out_count; p.A = A;
  p.thr = threshold; p.iou_thr = iou_threshold; p.sigma = sigma; p.method = method; p.top_n = pre_nms_top_n; p.max_det = max_det;
  EFFDET_SET_MAX_LDS(soft_nms_kernel, (size_t)SN_MAX * 28);          // (the cap: the attribute is set once per device)
  hipLaunchKernelGGL(soft_nms_kernel, dim3(B), dim3(SN_T), (size_t)pre_nms_top_n * 28, st, p);
  EFFDET_CHECK_LAUNCH();
  return EFFDET_OK;
}

extern "C" int effdet_gather_dets(const float* boxes, const float* score, const int* label, const int* idx, const int* count,
                                  float* out_scores, long long* out_labels, float* out_boxes, int B, long long A,
                                  effdet_stream_t stream) {
  if (!boxes || !score || !label || !idx || !count || !out_scores || !out_labels || !out_boxes) return EFFDET_EINVAL;
  hipLaunchKernelGGL(gather_dets_kernel, dim3(grid_for((long long)B * A)), dim3(256), 0, (hipStream_t)stream, boxes, score, label, idx, count, out_scores, out_labels, out_boxes, A, B);
  EFFDET_CHECK_LAUNCH();
  return EFFDET_OK;
}
