// Stable LSD radix sort of (key, uint32 value) pairs in B independent segments of A elements, 8 bits per pass; used by the NMS
// (32-bit score keys per image, postprocess.hip) and by the VOC metric (64-bit (class, score) keys, one segment, voc_map.hip).
// A pass is three launches: rs_hist_kernel (per-tile digit counts), rs_scan_kernel (per-segment exclusive scan over (digit, tile)
// in digit-major order) and rs_scatter_kernel (tile-ordered, rank-within-wave ordered stores: stable).  The grid depends on B and
// A only.
#pragma once
#include "common.h"

namespace {

constexpr int RS_TILE = 2048;                    // keys per workgroup and pass

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

}  // namespace
