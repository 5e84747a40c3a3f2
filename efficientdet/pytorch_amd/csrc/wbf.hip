// Weighted Boxes Fusion of several views' detection lists (include/effdet_wbf.h holds the semantics; tests/wbf_restated.py restates
// them in NumPy fp32 and the kernel must equal it BIT FOR BIT, so this file is built with -ffp-contract=off like postprocess.hip).
//
// ONE 1024-thread workgroup per image, the structure of postprocess.hip's soft_nms_kernel:
//   1. every (view, row) slot j = v * top_n + r makes a 64-bit key (~conf bits << 32 | j; all ones for a row that does not take part):
//      ascending key order IS conf descending, then view, then row.  The keys are sorted in LDS (bitonic, P = pow2 >= V * top_n).
//   2. the survivors are loaded into LDS in sorted order: transformed box 16 B, conf 4 B, label 4 B -- 24 B each, 96 KB at the 4096 cap,
//      beside the 32 KB of keys (128 KB of the CU's 160 KB: one workgroup per CU, which is what a 1024-thread workgroup gets anyway).
//   3. the clustering is SEQUENTIAL in the candidates (a candidate's match depends on every fused box the earlier ones left behind).
//      A cluster table in LDS does not fit beside the candidates; a thread OWNS the clusters tid, tid + 1024, .. (at most four) and is
//      the only one that reads or writes them, so their state lives in its registers.  A step: every thread reads the candidate
//      (an LDS broadcast), scans its own clusters, then a wave + cross-wave arg-max on (IoU, lowest index) through ping-ponged
//      reduction slots with ONE barrier, then the owner joins or founds.  The number of clusters is block-uniform.
//   4. the clusters' scores make keys the same way (~score bits << 32 | cluster index), the same sort orders them, and every owner
//      writes its clusters to the rows the sort gave them; the remaining rows are zeroed.
#include "box_geom.h"
#include "block_best.h"
#include "../../../include/effdet_wbf.h"

namespace {

constexpr int WBF_T = 1024, WBF_MAX = EFFDET_WBF_MAX_IN, WBF_OWN = WBF_MAX / WBF_T, WBF_V = EFFDET_WBF_MAX_VIEWS;
constexpr unsigned long long WBF_NO_KEY = ~0ull;

struct Wbf {
  const float* score[WBF_V]; const long long* label[WBF_V]; const float* boxes[WBF_V]; const int* count[WBF_V];
  long long A[WBF_V]; float weight[WBF_V], width[WBF_V], mul[WBF_V]; int flip[WBF_V];
  int V, top_n, conf_type, P; float iou_thr, skip_thr, wsum, wmax;
  float* out_score; long long* out_label; float* out_boxes; int* out_count;
};

// The IoU is box_geom.h's box_iou from the two areas; the (IoU, cluster) arg-max goes by block_best.h's order and starts with its DPP
// wave step (all 64 lanes are active here).

// row r of view v of image b after the view's transform -> takes part?
__device__ __forceinline__ bool wbf_row(const Wbf& p, int b, int v, int r, float4& bx, float& conf) {
  const long long at = (long long)b * p.A[v] + r;
  const float s = p.score[v][at];
  bx = ((const float4*)p.boxes[v])[at];
  if (p.flip[v]) { const float x1 = p.width[v] - bx.z, x2 = p.width[v] - bx.x; bx.x = x1; bx.z = x2; }
  const float m = p.mul[v];
  bx.x *= m; bx.y *= m; bx.z *= m; bx.w *= m;
  conf = s * p.weight[v];
  return s >= p.skip_thr && pos_finite(conf) && pos_finite(box_area(bx));
}

// ascending bitonic sort of key[0 .. P) (P a power of two) by the whole workgroup; ends on a barrier
__device__ __forceinline__ void wbf_sort(unsigned long long* key, int P, int tid) {
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (P >> 1); t += WBF_T) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        const unsigned long long a = key[i], c = key[l];
        if ((a > c) == ((i & k) == 0)) { key[i] = c; key[l] = a; }
      }
      __syncthreads();
    }
}

__global__ __launch_bounds__(WBF_T) void wbf_kernel(const Wbf p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int N = p.V * p.top_n;
  float4* tb = (float4*)smem_raw;                                      // [N] transformed boxes in candidate order
  float* tc = (float*)(tb + N);                                        // [N] conf
  int* tl = (int*)(tc + N);                                            // [N] labels
  unsigned long long* key = (unsigned long long*)(smem_raw + (((size_t)N * 24 + 15) & ~(size_t)15));      // [P] sort keys
  int* rank = (int*)smem_raw;                                          // [N] cluster -> output row (over tb, once the clustering is done)
  __shared__ float red_s[2][WBF_T / 64];
  __shared__ int red_q[2][WBF_T / 64];
  __shared__ int s_m;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  // 1. keys of every slot, sorted
  if (tid == 0) s_m = 0;
  for (int j = tid; j < p.P; j += WBF_T) {
    unsigned long long k = WBF_NO_KEY;
    if (j < N) {
      const int v = j / p.top_n, r = j - v * p.top_n;
      const long long rows = min((long long)min(p.count[v][b], p.top_n), p.A[v]);
      float4 bx; float conf;
      if (r < rows && wbf_row(p, b, v, r, bx, conf)) k = ((unsigned long long)~__float_as_uint(conf) << 32) | (unsigned)j;
    }
    key[j] = k;
  }
  wbf_sort(key, p.P, tid);
  // 2. the survivors in order (a valid key's high word is ~(bits of a positive finite float): never all ones)
  for (int q = tid; q < N; q += WBF_T) {
    const unsigned long long k = key[q];
    if (k == WBF_NO_KEY) continue;
    if (q + 1 == p.P || key[q + 1] == WBF_NO_KEY) s_m = q + 1;
    const int j = (int)(unsigned)k, v = j / p.top_n, r = j - v * p.top_n;
    float4 bx; float conf;
    wbf_row(p, b, v, r, bx, conf);
    tb[q] = bx; tc[q] = conf; tl[q] = (int)p.label[v][(long long)b * p.A[v] + r];
  }
  __syncthreads();
  const int M = s_m;

  // 3. the clustering; cluster c = tid + u * 1024 is register set u of thread tid
  float4 fb[WBF_OWN], S[WBF_OWN]; float sc[WBF_OWN], cmax[WBF_OWN]; int cnt[WBF_OWN], lab[WBF_OWN];
  int ncl = 0;
  for (int i = 0; i < M; ++i) {
    const float4 cb = tb[i]; const float cc = tc[i]; const int cl = tl[i];
    const float ca = box_area(cb);
    float bs = -__builtin_huge_valf(); int bq = 0x7fffffff;
#pragma unroll
    for (int u = 0; u < WBF_OWN; ++u) {
      const int c = tid + u * WBF_T;
      if (c < ncl && lab[u] == cl) best_take(bs, bq, box_iou(fb[u], box_area(fb[u]), cb, ca), c);
    }
    wave_best_dpp(bs, bq);
    if (lane == 0) { red_s[i & 1][wave] = bs; red_q[i & 1][wave] = bq; }
    __syncthreads();
    float ws = red_s[i & 1][lane & 15]; int wq = red_q[i & 1][lane & 15];
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) best_take(ws, wq, __shfl_xor(ws, o, 64), __shfl_xor(wq, o, 64));
    const bool join = ws > p.iou_thr;                                  // (block-uniform: every thread reduced the same 16 slots)
    const int c = join ? wq : ncl;
    if ((c & (WBF_T - 1)) == tid) {
#pragma unroll
      for (int u = 0; u < WBF_OWN; ++u)
        if (u == (c >> 10)) {
          if (join) {
            S[u].x += cc * cb.x; S[u].y += cc * cb.y; S[u].z += cc * cb.z; S[u].w += cc * cb.w;
            sc[u] += cc; cmax[u] = fmaxf(cmax[u], cc); cnt[u] += 1;
            fb[u] = make_float4(S[u].x / sc[u], S[u].y / sc[u], S[u].z / sc[u], S[u].w / sc[u]);
          } else {
            S[u] = make_float4(cc * cb.x, cc * cb.y, cc * cb.z, cc * cb.w);
            sc[u] = cc; cmax[u] = cc; cnt[u] = 1; lab[u] = cl; fb[u] = cb;
          }
        }
    }
    if (!join) ++ncl;
  }

  // 4. scores, output order, rows
  float fs[WBF_OWN];
#pragma unroll
  for (int u = 0; u < WBF_OWN; ++u) {                                  // (slot c of the keys is its owner's too: P <= 4 * 1024)
    const int c = tid + u * WBF_T;
    if (c < ncl) {
      fs[u] = p.conf_type == EFFDET_WBF_MAX ? cmax[u] / p.wmax
                                            : ((sc[u] / (float)cnt[u]) * (float)min(cnt[u], p.V)) / p.wsum;
      key[c] = ((unsigned long long)~__float_as_uint(fs[u]) << 32) | (unsigned)c;
    } else if (c < p.P) {
      key[c] = WBF_NO_KEY;
    }
  }
  wbf_sort(key, p.P, tid);                                             // (its first barrier also ends the last step's reads of tb: rank overlays it)
  for (int k = tid; k < ncl; k += WBF_T) rank[(int)(unsigned)key[k]] = k;
  __syncthreads();
  const long long base = (long long)b * N;
#pragma unroll
  for (int u = 0; u < WBF_OWN; ++u) {
    const int c = tid + u * WBF_T;
    if (c < ncl) {
      const long long at = base + rank[c];
      p.out_score[at] = fs[u]; p.out_label[at] = lab[u]; ((float4*)p.out_boxes)[at] = fb[u];
    }
  }
  for (int k = ncl + tid; k < N; k += WBF_T) {
    p.out_score[base + k] = 0.f; p.out_label[base + k] = 0; ((float4*)p.out_boxes)[base + k] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if (tid == 0) p.out_count[b] = ncl;
}

}  // namespace

extern "C" long long effdet_wbf_workspace_bytes(int B, int V, int top_n) {
  (void)B; (void)V; (void)top_n;                       // (candidates and keys live in LDS, cluster state in registers)
  return 0;
}

extern "C" int effdet_wbf(const effdet_wbf_t* d, void* workspace, long long workspace_bytes, effdet_stream_t stream) {
  (void)workspace;
  if (!d || d->B < 1 || !d->out_score || !d->out_label || !d->out_boxes || !d->out_count || workspace_bytes < 0) return EFFDET_EINVAL;
  if (((unsigned long long)d->out_boxes & 15ull) != 0ull) return EFFDET_EINVAL;
  if (d->V < 1 || d->V > WBF_V || d->top_n < 1 || (long long)d->V * d->top_n > WBF_MAX || d->conf_type < 0 || d->conf_type > 1 ||
      !(d->iou_thr >= 0.f && d->iou_thr <= 1.f) || d->skip_thr != d->skip_thr)
    return EFFDET_EUNSUPPORTED;
  Wbf p;
  p.wsum = 0.f; p.wmax = 0.f;
  for (int v = 0; v < WBF_V; ++v) {
    const bool on = v < d->V;
    if (on) {
      if (!d->score[v] || !d->label[v] || !d->boxes[v] || !d->count[v] || d->A[v] < 1 || ((unsigned long long)d->boxes[v] & 15ull) != 0ull)
        return EFFDET_EINVAL;
      if (!pos_finite(d->weight[v]) || !pos_finite(d->mul[v]) || (d->flip[v] && !(fabsf(d->width[v]) < __builtin_huge_valf())))
        return EFFDET_EUNSUPPORTED;
      p.wsum += d->weight[v]; p.wmax = fmaxf(p.wmax, d->weight[v]);
    }
    p.score[v] = on ? d->score[v] : nullptr; p.label[v] = on ? d->label[v] : nullptr;
    p.boxes[v] = on ? d->boxes[v] : nullptr; p.count[v] = on ? d->count[v] : nullptr;
    p.A[v] = on ? d->A[v] : 0; p.weight[v] = on ? d->weight[v] : 0.f; p.width[v] = on ? d->width[v] : 0.f;
    p.mul[v] = on ? d->mul[v] : 0.f; p.flip[v] = on ? (d->flip[v] != 0) : 0;
  }
  if (!pos_finite(p.wsum)) return EFFDET_EUNSUPPORTED;  // (the weights' fp32 sum overflowed)
  const int N = d->V * d->top_n;
  p.V = d->V; p.top_n = d->top_n; p.conf_type = d->conf_type; p.iou_thr = d->iou_thr; p.skip_thr = d->skip_thr;
  p.P = 1; while (p.P < N) p.P <<= 1;
  p.out_score = d->out_score; p.out_label = d->out_label; p.out_boxes = d->out_boxes; p.out_count = d->out_count;
  const size_t lds = (((size_t)N * 24 + 15) & ~(size_t)15) + (size_t)p.P * 8;
  EFFDET_SET_MAX_LDS(wbf_kernel, (size_t)WBF_MAX * 32);                // (the cap: the attribute is set once per device)
  hipLaunchKernelGGL(wbf_kernel, dim3(d->B), dim3(WBF_T), lds, (hipStream_t)stream, p);
  EFFDET_CHECK_LAUNCH();
  return EFFDET_OK;
}
