// Stable LSD radix sort of (key, uint32 value) pairs in B independent segments of A elements, 8 bits per pass; used by the NMS
// (32-bit score keys per image, postprocess.hip), the VOC metric (64-bit (class, score) keys, one segment, voc_map.hip) and the
// COCO metric (32-bit image ids, then 64-bit (category, score) keys, one segment, coco_map.hip).
// A pass is three launches: rs_hist_kernel (per-tile digit counts), rs_scan_kernel (per-segment exclusive scan over (digit, tile)
// in digit-major order) and rs_scatter_kernel (tile-ordered, rank-within-wave ordered stores: stable).  The grid depends on B and
// A only.  rs_sort drives the passes over the buffers of an RsBufs; rs_score_key makes the score part of a key; the two metrics
// also share the sort input (rs_init_kernel) and the segment bounds of their sorted 64-bit keys (rs_segment_bounds); the VOC and the
// operating-point metrics (op_point.hip) share their whole class sort (rs_class_sort, which ends on rs_segments_kernel).
#pragma once
#include "common.h"

namespace {

constexpr int RS_TILE = 2048;                    // keys per workgroup and pass

// descending-score key of an fp32 score: ascending radix order of the keys = descending order of the scores
__device__ __forceinline__ unsigned rs_score_key(float s) {
  unsigned u = __float_as_uint(s);
  u ^= (u >> 31) ? 0xffffffffu : 0x80000000u;     // ascending-orderable
  return ~u;                                      // descending
}

// hist[b][digit][tile]
template <typename K>
__global__ __launch_bounds__(256) void rs_hist_kernel(const K* __restrict__ keys, unsigned* __restrict__ hist, long long A, int T, int shift) {
  __shared__ unsigned digit_counter[256];            // (integer LDS atomics: order-independent)
  const int tile = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  digit_counter[tid] = 0u;
  __syncthreads();
  const K* k = keys + (long long)b * A;
  const long long i0 = (long long)tile * RS_TILE, i1 = min(A, i0 + RS_TILE);
  for (long long i = i0 + tid; i < i1; i += 256) atomicAdd(&digit_counter[(unsigned)(k[i] >> shift) & 255u], 1u);
  __syncthreads();
  hist[((long long)b * 256 + tid) * T + tile] = digit_counter[tid];
}

// per image: exclusive scan over (digit, tile) in digit-major order, in place
__global__ __launch_bounds__(256) void rs_scan_kernel(unsigned* __restrict__ hist, int T) {
  __shared__ unsigned tot[256];
  const int b = blockIdx.x, d = threadIdx.x;
  unsigned* row = hist + ((long long)b * 256 + d) * T;
  unsigned s = 0u;
  for (int t = 0; t < T; ++t) s += row[t];
  tot[d] = s;
  __syncthreads();
  if (d == 0) { unsigned run = 0u; for (int q = 0; q < 256; ++q) { const unsigned c = tot[q]; tot[q] = run; run += c; } }
  __syncthreads();
  unsigned run = tot[d];
  for (int t = 0; t < T; ++t) { const unsigned c = row[t]; row[t] = run; run += c; }
}

template <typename K>
__global__ __launch_bounds__(256) void rs_scatter_kernel(const K* __restrict__ kin, const unsigned* __restrict__ vin,
                                                         K* __restrict__ kout, unsigned* __restrict__ vout,
                                                         const unsigned* __restrict__ hist, long long A, int T, int shift) {
  __shared__ unsigned cur[256];                  // next output slot of each digit for this tile
  __shared__ unsigned wcnt[4][256];              // per-wave digit counts of the current 256-key chunk
  const int tile = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  cur[tid] = hist[((long long)b * 256 + tid) * T + tile];
  const long long base = (long long)b * A, i0 = (long long)tile * RS_TILE;
  const unsigned long long lt = (1ull << lane) - 1ull;
  for (int c = 0; c < RS_TILE / 256; ++c) {
    const long long i = i0 + c * 256 + tid;
    if (i0 + c * 256 >= A) break;                                      // uniform
    const bool valid = i < A;
    const K key = valid ? kin[base + i] : (K)0;
    const unsigned val = valid ? vin[base + i] : 0u;
    const unsigned d = (unsigned)(key >> shift) & 255u;
#pragma unroll
    for (int w = 0; w < 4; ++w) wcnt[w][tid] = 0u;
    __syncthreads();
    unsigned long long peers = __ballot(valid);                        // lanes of this wave holding the same digit
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const bool on = (d >> bit) & 1u;
      const unsigned long long bb = __ballot(on);
      peers &= on ? bb : ~bb;
    }
    const int rank = __popcll(peers & lt);
    if (valid && rank == 0) wcnt[wave][d] = (unsigned)__popcll(peers);
    __syncthreads();
    if (valid) {
      unsigned pos = cur[d] + (unsigned)rank;
      for (int w = 0; w < wave; ++w) pos += wcnt[w][d];
      kout[base + pos] = key; vout[base + pos] = val;
    }
    __syncthreads();
    cur[tid] += wcnt[0][tid] + wcnt[1][tid] + wcnt[2][tid] + wcnt[3][tid];
    __syncthreads();                                                   // (the next chunk zeroes wcnt)
  }
}

// ping-pong (key, value) buffers, hist [B][256][T] and the tiles per segment
template <typename K> struct RsBufs { K *ka, *kb; unsigned *va, *vb, *hist; int T; };

// takes ka, kb, (va,) vb, hist in this order; with own_va = false the caller has taken va elsewhere in its workspace
template <typename K> void rs_carve(RsBufs<K>& s, Carver& c, size_t B, size_t A, bool own_va = true) {
  s.T = (int)((A + RS_TILE - 1) / RS_TILE);
  s.ka = c.take<K>(B * A); s.kb = c.take<K>(B * A);
  if (own_va) s.va = c.take<unsigned>(B * A);
  s.vb = c.take<unsigned>(B * A);
  s.hist = c.take<unsigned>(B * 256 * s.T);
}

// `passes` passes over bits [shift, shift + 8 * passes) of the B segments of A keys; (ki, vi) ends on the sorted pairs and
// (ko, vo) on the other half of the ping-pong.  -> EFFDET_OK or EFFDET_ELAUNCH
template <typename K> int rs_sort(K*& ki, unsigned*& vi, K*& ko, unsigned*& vo, unsigned* hist, int B, long long A, int T, int shift,
                                  int passes, hipStream_t st) {
  for (int pass = 0; pass < passes; ++pass, shift += 8) {
    hipLaunchKernelGGL((rs_hist_kernel<K>), dim3(T, B), dim3(256), 0, st, (const K*)ki, hist, A, T, shift);
    hipLaunchKernelGGL(rs_scan_kernel, dim3(B), dim3(256), 0, st, hist, T);
    hipLaunchKernelGGL((rs_scatter_kernel<K>), dim3(T, B), dim3(256), 0, st, (const K*)ki, (const unsigned*)vi, ko, vo,
                       (const unsigned*)hist, A, T, shift);
    EFFDET_CHECK_LAUNCH();
    K* t = ki; ki = ko; ko = t;
    unsigned* u = vi; vi = vo; vo = u;
  }
  return EFFDET_OK;
}

// sort input of the metrics: keys = src, values = record index; and the reset of the per-class segment bounds seg[2 * C]
template <typename K>
__global__ __launch_bounds__(256) void rs_init_kernel(const K* __restrict__ src, K* __restrict__ ka, unsigned* __restrict__ va, long long N,
                                                      int* __restrict__ seg, int C) {
  const long long n = N > 2LL * C ? N : 2LL * C;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    if (i < N) { ka[i] = src[i]; va[i] = (unsigned)i; }
    if (i < 2LL * C) seg[i] = 0;
  }
}

// sorted position i of N 64-bit keys whose high word is the class: seg[2c], seg[2c + 1] = [first, last + 1) position of class c < C
// (left at 0, 0 when the class has no records)
__device__ __forceinline__ void rs_segment_bounds(const unsigned long long* __restrict__ skey, long long i, long long N, int C,
                                                  int* __restrict__ seg) {
  const unsigned c = (unsigned)(skey[i] >> 32);
  if (c >= (unsigned)C) return;
  if (i == 0 || (unsigned)(skey[i - 1] >> 32) != c) seg[2 * c] = (int)i;
  if (i == N - 1 || (unsigned)(skey[i + 1] >> 32) != c) seg[2 * c + 1] = (int)(i + 1);
}

// the bounds alone (voc_map.hip, op_point.hip; coco_segments_kernel also gathers its payload and stays in coco_map.hip).  K is
// unsigned long long; this kernel and rs_class_sort are templates so that only the files that call them get the 64-bit instances.
template <typename K>
__global__ __launch_bounds__(256) void rs_segments_kernel(const K* __restrict__ skey, long long N, int C, int* __restrict__ seg) {
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < N; i += (long long)gridDim.x * 256) rs_segment_bounds(skey, i, N, C, seg);
}

// The class sort of the VOC and operating-point metrics: N records (class << 32 | score key), class values 0..C (C = empty slot).
// Sort input and reset of seg[2 * C]; then, for N > 0, 4 score passes + 1 class pass (2 above 255 classes) and the segment bounds.
// (ki, vi) are the sorted keys and record indices (w.ka, w.va when N == 0).  -> EFFDET_OK or EFFDET_ELAUNCH
template <typename K> int rs_class_sort(const K* rec_key, long long N, int C, const RsBufs<K>& w, int* seg, K*& ki, unsigned*& vi, hipStream_t st) {
  hipLaunchKernelGGL(rs_init_kernel<K>, dim3(grid_for(N > 2LL * C ? N : 2LL * C)), dim3(256), 0, st, rec_key, w.ka, w.va, N, seg, C);
  EFFDET_CHECK_LAUNCH();
  ki = w.ka; vi = w.va;
  if (N > 0) {
    K* ko = w.kb;
    unsigned* vo = w.vb;
    if (const int rc = rs_sort(ki, vi, ko, vo, w.hist, 1, N, w.T, 0, 4 + (C <= 255 ? 1 : 2), st)) return rc;
    hipLaunchKernelGGL(rs_segments_kernel<K>, dim3(grid_for(N)), dim3(256), 0, st, (const K*)ki, N, C, seg);
    EFFDET_CHECK_LAUNCH();
  }
  return EFFDET_OK;
}

}  // namespace
