// Train-step tail (reference train.py:115-118): global-norm gradient clipping + AdamW as TWO
// multi-tensor passes over a device-resident pointer table instead of ~17 torch foreach / fused launches:
//   pass 1  norm:   per 4096-element slice  sum g^2  -> partial[block]; a one-workgroup kernel finishes sqrt(sum)
//   pass 2  update: coef = min(1, max_norm / (norm + 1e-6))            (torch.nn.utils.clip_grad_norm_)
//                   g' = coef*g;  p -= lr*wd*p;  m = b1*m + (1-b1)*g';  v = b2*v + (1-b2)*g'^2
//                   p -= (lr/(1-b1^t)) * m / (sqrt(v)/sqrt(1-b2^t) + eps)                    (torch.optim.AdamW)
// HBM-bound: reads g twice, p/m/v once, writes p/m/v: 7 x 4 bytes per parameter (275 MB per D0 step).  The clipped
// gradient is not written back (p.grad keeps the unclipped values) unless write_grad is set.
//
// Training-loop control on the device (reference train.py:104-120: `if bool(loss == 0): continue`, gradient accumulation over
// grad_accumulation_steps micro-batches, total_loss.append(loss.item())): a 32-byte control block (effdet_train_ctl_t) written by
// one-thread launches and read by the multi-tensor passes, so a captured loop needs no host decision that depends on data:
//   train_gate_kernel       skip = (loss == 0); otherwise the fp64 loss meter advances
//   grad_accumulate_kernel  unless skip: acc = g (pending == 0) or acc += g over the optimizer's block table; then
//   train_pending_kernel    unless skip: pending += 1                    (single writer, ordered behind every reader)
//   the GATED instantiations of the three step kernels do nothing unless (!skip && pending != 0); they read acc as the gradient; then
//   train_release_kernel    if the step ran: pending = 0, applied += 1   (single writer, ordered behind every reader)
// No kernel both reads a control word from many workgroups and writes it.  Accumulate moves 12 bytes per parameter (8 on the first
// micro-batch of a window, which writes instead of adding: the arena never needs a zeroing pass).
//
// Parameter EMA (include/effdet_ema.h; the EMA instantiations): the update kernel has every new parameter value in registers, so the
// average is one more stream of it -- e += om * (p - e), 8 more bytes per parameter, no second read of p -- and a tensor without a
// gradient takes an EMA-only pass over its chunk.  om = 1 - min(decay, (1 + t) / (10 + t)) is computed ONCE per step by thread 0 of
// opt_norm_final_kernel (one workgroup) from the counter `updates` of effdet_ema_ctl_t, stored next to the norm (scratch[1]) and read
// from there by the update kernel's workgroups; the same thread then advances `updates`: it is the word's only reader and only writer,
// so no launch is added.  ema_swap_kernel exchanges p and e in place over the same block table (evaluation with the averaged weights).
//
// Parameter groups and a second update rule (include/effdet_opt_groups.h; the GROUPED instantiations of the update kernel): the step
// already works per tensor, so a group is tensor_group[ti], an index into a DEVICE table of 8-float rows, read once per workgroup in
// place of the one hyper buffer.  The norm pass reads no per-group value (one global norm, one EMA counter; max_norm and ema_decay are
// optimizer-wide and sit at the legacy offsets 0 and 6 of row 0), so opt_norm_kernel / opt_norm_final_kernel serve both forms as they
// are and only the update kernel has a grouped form.  RULE_SGD is torch.optim.SGD's update (sgd1) over the same tables with ONE moment
// arena; like ema1 it is separately rounded fp32 with contraction off, so a NumPy restatement is bit-exact.
#include "common.h"
#include "../../../include/effdet_ema.h"
#include "../../../include/effdet_opt_groups.h"

namespace {

constexpr int OPT_CHUNK = 4096;       // elements per workgroup (256 threads x 4 x float4)

struct OptK {
  const unsigned long long* p; const unsigned long long* g; const unsigned long long* m; const unsigned long long* v;
  const long long* n; const int* block_tensor; const int* block_first;
  float* partial; float* norm; int* steps;
  float max_norm, lr, beta1, beta2, eps, wd;
  int nblocks, ntensors, write_grad;
  const float* hyper;      // optional DEVICE copy of {max_norm, lr, beta1, beta2, eps, wd}: read at run time, so a captured
                           // step (hipGraph replay) follows a learning-rate schedule instead of the values frozen at capture
  // GATED instantiations only: g is the accumulation arena's table, `has` the micro-step's gradient table (has[i] == 0: tensor i has
  // no gradient) and ctl the control block that says whether the step runs at all
  const unsigned long long* has; const effdet_train_ctl_t* ctl;
  // EMA instantiations only: the average's table (the moments' offsets), its control block, the by-value decay (used when hyper is
  // null; hyper[6] otherwise) and the warm-up switch.  om lives in norm[1].
  const unsigned long long* e; effdet_ema_ctl_t* ectl; float ema_decay; int ema_warmup;
};

// GROUPED instantiations only (a struct of its own: OptK, the kernel argument of the one-group instantiations, stays as it is)
struct OptG : OptK {
  const int* tensor_group;   // int32[ntensors]: row of `table` for tensor ti
  const float* table;        // ngroups rows of EFFDET_OPT_ROW floats (effdet_opt_groups.h); k.hyper aliases it (row 0) for the norm pass
};
constexpr int RULE_ADAMW = EFFDET_OPT_RULE_ADAMW, RULE_SGD = EFFDET_OPT_RULE_SGD;

static_assert(sizeof(effdet_train_ctl_t) == 32, "effdet_train_ctl_t is read back as 32 bytes by the binding");
static_assert(sizeof(effdet_ema_ctl_t) == 16, "effdet_ema_ctl_t is read back as 16 bytes by the binding");

__device__ __forceinline__ bool gate_open(const effdet_train_ctl_t* c) { return c->skip == 0 && c->pending != 0; }

struct Hyper { float max_norm, lr, beta1, beta2, eps, wd; };
__device__ __forceinline__ Hyper hyper_of(const OptK& k) {
  if (k.hyper) return Hyper{k.hyper[0], k.hyper[1], k.hyper[2], k.hyper[3], k.hyper[4], k.hyper[5]};
  return Hyper{k.max_norm, k.lr, k.beta1, k.beta2, k.eps, k.wd};
}

__device__ __forceinline__ float block_sum(float s) {
  __shared__ float red[4];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// 4 consecutive elements starting at g + i: ONE 16-byte load when the address allows it, four scalar loads otherwise -- the
// VALUES and everything computed from them are the same either way.  (Round 3 summed aligned tensors float4-wise and unaligned
// ones element-strided: two summation orders, so the norm -- and through the clip coefficient every parameter -- differed in the
// last bit between a model whose gradients are separate allocations and the same model under DistributedDataParallel, whose
// gradients are views into flat buckets at arbitrary 4-byte offsets.  Found by the world_size-1 RCCL test.)
__device__ __forceinline__ f32x4 load4_any(const float* q, bool al) {
  if (al) return *(const f32x4*)q;
  return f32x4{q[0], q[1], q[2], q[3]};
}

// The EMA recurrence: subtract, multiply, add -- three fp32 operations, each rounded to nearest, never contracted into an FMA (a
// contracted e + om * d rounds once and differs from the restatement in the last bit).  This toolchain's __fsub_rn / __fmul_rn /
// __fadd_rn / __fdiv_rn are the plain operators and inherit the translation unit's contraction, so the functions below switch
// contraction off for their own statements instead; adamw1 keeps the file's default.
__device__ __forceinline__ float ema1(float e, float p, float om) {
#pragma clang fp contract(off)
  const float d = p - e;
  const float q = om * d;
  return e + q;
}

// 1 - d, d = decay or, during the warm-up, min(decay, (1 + t) / (10 + t)) with t the updates made so far (0 on the first)
__device__ __forceinline__ float ema_one_minus_decay(float decay, int warmup, int updates) {
#pragma clang fp contract(off)
  float d = decay;
  if (warmup) {
    const float t = (float)updates;
    const float num = 1.0f + t, den = 10.0f + t;
    d = fminf(d, num / den);                                 // (hipcc's fp32 division is correctly rounded by default)
  }
  return 1.0f - d;
}

template <bool GATED> __global__ __launch_bounds__(256) void opt_norm_kernel(const OptK k) {
  if (GATED && !gate_open(k.ctl)) return;                    // (the whole grid takes the same branch: partial[] stays untouched)
  const int ti = k.block_tensor[blockIdx.x];
  const float* g = (const float*)(GATED && !k.has[ti] ? 0ull : k.g[ti]);
  float s = 0.f;
  if (g) {
    const long long n = k.n[ti], off = (long long)(blockIdx.x - k.block_first[ti]) * OPT_CHUNK;
    const long long end = off + OPT_CHUNK < n ? off + OPT_CHUNK : n;
    const bool al = (((unsigned long long)(g + off)) & 15ull) == 0;
    // thread t owns elements off + 4t .. 4t + 3 (+ 1024 per round) whatever the alignment: ONE summation order
    for (long long i = off + threadIdx.x * 4; i < end; i += 1024) {
      if (i + 3 < end) { const f32x4 x = load4_any(g + i, al); s += x[0] * x[0] + x[1] * x[1] + x[2] * x[2] + x[3] * x[3]; }
      else for (long long j = i; j < end; ++j) s += g[j] * g[j];
    }
  }
  s = block_sum(s);
  if (threadIdx.x == 0) k.partial[blockIdx.x] = s;
}

// one workgroup: finishes the norm and advances the per-tensor AdamW step counters (torch keeps one per parameter: a
// parameter without gradient in some step is skipped and its bias correction lags behind)
struct EmaStep { effdet_ema_ctl_t* ectl; const float* hyper; float decay; int warmup; };

template <bool GATED, bool EMA>
__global__ __launch_bounds__(1024) void opt_norm_final_kernel(const float* __restrict__ partial, int nb, float* __restrict__ norm,
                                                              const unsigned long long* __restrict__ g, int* __restrict__ steps, int nt,
                                                              const effdet_train_ctl_t* __restrict__ ctl, const EmaStep es) {
  __shared__ float red[16];
  if (GATED && !gate_open(ctl)) return;
  if (EMA && threadIdx.x == 0) {                             // this step's om, then the counter: one thread reads and writes `updates`
    const int u = es.ectl->updates;
    norm[1] = ema_one_minus_decay(es.hyper ? es.hyper[6] : es.decay, es.warmup, u);
    es.ectl->updates = u + 1;
  }
  for (int i = threadIdx.x; i < nt; i += 1024) if (g[i]) steps[i] += 1;
  float s = 0.f;
  for (int i = threadIdx.x; i < nb; i += 1024) s += partial[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) { float t = 0.f; for (int i = 0; i < 16; ++i) t += red[i]; norm[0] = sqrtf(t); }
}

__device__ __forceinline__ void adamw1(float& p, float& m, float& v, float g, const Hyper& k, float step_size, float bc2_sqrt) {
  p -= k.lr * k.wd * p;
  m = k.beta1 * m + (1.f - k.beta1) * g;
  v = k.beta2 * v + (1.f - k.beta2) * g * g;
  p -= step_size * m / (sqrtf(v) / bc2_sqrt + k.eps);
}

// torch.optim.SGD, one element (effdet_opt_groups.h): every operation a separately rounded fp32 one, never an FMA (see ema1).  The row
// is read through Hyper's names: beta1 = momentum, beta2 = 1 - dampening, eps = the nesterov flag.  `first`: this is the tensor's first
// step, the buffer starts as a copy of d.  The branches are uniform over the workgroup.
__device__ __forceinline__ void sgd1(float& p, float& buf, float& g, float coef, const Hyper& k, bool first) {
#pragma clang fp contract(off)
  g = g * coef;                                              // (in here: the product may not fuse into d's sum either)
  float d = g;
  if (k.wd != 0.f) { const float w = k.wd * p; d = g + w; }
  float u = d;
  if (k.beta1 != 0.f) {
    if (first) buf = d;
    else { const float a = k.beta1 * buf; const float b = k.beta2 * d; buf = a + b; }
    if (k.eps != 0.f) { const float a = k.beta1 * buf; u = d + a; }
    else u = buf;
  }
  const float s = k.lr * u;
  p = p - s;
}

// a tensor without a gradient in this step: AdamW leaves it alone, its average still follows the unchanged p
__device__ __forceinline__ void ema_only_chunk(const OptK& kk, int ti, float om) {
  const float* p = (const float*)kk.p[ti]; float* e = (float*)kk.e[ti];
  const long long n = kk.n[ti], off = (long long)(blockIdx.x - kk.block_first[ti]) * OPT_CHUNK;
  const long long end = off + OPT_CHUNK < n ? off + OPT_CHUNK : n;
  const bool alp = (((unsigned long long)(p + off)) & 15ull) == 0, ale = (((unsigned long long)(e + off)) & 15ull) == 0;
  for (long long i = off + threadIdx.x * 4; i < end; i += 1024) {
    if (i + 3 < end) {
      const f32x4 pv = load4_any(p + i, alp);
      f32x4 ev = load4_any(e + i, ale);
#pragma unroll
      for (int c = 0; c < 4; ++c) ev[c] = ema1(ev[c], pv[c], om);
      if (ale) *(f32x4*)(e + i) = ev;
      else {
#pragma unroll
        for (int c = 0; c < 4; ++c) e[i + c] = ev[c];
      }
    } else {
      for (long long j = i; j < end; ++j) e[j] = ema1(e[j], p[j], om);
    }
  }
}

template <bool GROUPED> struct OptArg { using type = OptK; };
template <> struct OptArg<true> { using type = OptG; };

// the one set of hypers, read where the one-group kernel has always read it, or (GROUPED) the row of the workgroup's tensor
__device__ __forceinline__ Hyper hyper_one(const OptK& k) { return hyper_of(k); }
__device__ __forceinline__ Hyper hyper_one(const OptG&) { return Hyper{}; }
__device__ __forceinline__ Hyper hyper_row(const OptK&, int, const Hyper& one) { return one; }
__device__ __forceinline__ Hyper hyper_row(const OptG& k, int ti, const Hyper&) {
  const float* r = k.table + (long long)k.tensor_group[ti] * EFFDET_OPT_ROW;
  return Hyper{r[0], r[1], r[2], r[3], r[4], r[5]};
}

// clip_grad_norm_: min(1, max_norm / (norm + 1e-6)) with torch.clamp's NaN rule -- a NaN norm turns every gradient into NaN
__device__ __forceinline__ float clip_coef(const Hyper& k, float norm) {
  return k.max_norm > 0.f ? nan_min(1.0f, k.max_norm / (norm + 1e-6f)) : 1.0f;
}

// RULE_SGD over one chunk: g twice with clipping (norm pass + here), p and the momentum buffer read and written once; a group with
// momentum 0 never touches the buffer
template <bool EMA>
__device__ __forceinline__ void sgd_chunk(const OptK& kk, const Hyper& k, int ti, float* g, float coef, float om) {
  float* p = (float*)kk.p[ti]; float* b = (float*)kk.m[ti];
  float* ea = EMA ? (float*)kk.e[ti] : nullptr;
  const bool mom = k.beta1 != 0.f, first = kk.steps[ti] == 1;              // (already advanced by opt_norm_final_kernel)
  const long long n = kk.n[ti], off = (long long)(blockIdx.x - kk.block_first[ti]) * OPT_CHUNK;
  const long long end = off + OPT_CHUNK < n ? off + OPT_CHUNK : n;
  const bool alg = (((unsigned long long)(g + off)) & 15ull) == 0;
  const bool alp = ((((unsigned long long)(p + off)) | ((unsigned long long)(b + off))) & 15ull) == 0;
  const bool ale = EMA && (((unsigned long long)(ea + off)) & 15ull) == 0;
  for (long long i = off + threadIdx.x * 4; i < end; i += 1024) {
    if (i + 3 < end) {
      f32x4 gv = load4_any(g + i, alg), pv = load4_any(p + i, alp), bv{}, ev{};
      if (mom && !first) bv = load4_any(b + i, alp);
      if (EMA) ev = load4_any(ea + i, ale);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pe = pv[e], be = bv[e];
        float ge = gv[e];
        sgd1(pe, be, ge, coef, k, first);
        pv[e] = pe; bv[e] = be; gv[e] = ge;
        if (EMA) ev[e] = ema1(ev[e], pe, om);
      }
      if (alp) { *(f32x4*)(p + i) = pv; if (mom) *(f32x4*)(b + i) = bv; }
      else {
#pragma unroll
        for (int e = 0; e < 4; ++e) { p[i + e] = pv[e]; if (mom) b[i + e] = bv[e]; }
      }
      if (EMA) {
        if (ale) *(f32x4*)(ea + i) = ev;
        else {
#pragma unroll
          for (int e = 0; e < 4; ++e) ea[i + e] = ev[e];
        }
      }
      if (kk.write_grad) {
        if (alg) *(f32x4*)(g + i) = gv;
        else {
#pragma unroll
          for (int e = 0; e < 4; ++e) g[i + e] = gv[e];
        }
      }
    } else {
      for (long long j = i; j < end; ++j) {
        float pe = p[j], be = mom && !first ? b[j] : 0.f;
        float gj = g[j];
        sgd1(pe, be, gj, coef, k, first);
        p[j] = pe;
        if (mom) b[j] = be;
        if (EMA) ea[j] = ema1(ea[j], pe, om);
        if (kk.write_grad) g[j] = gj;
      }
    }
  }
}

template <bool GATED, bool EMA, bool GROUPED = false, int RULE = RULE_ADAMW>
__global__ __launch_bounds__(256) void opt_adamw_kernel(const typename OptArg<GROUPED>::type kk) {
  if (GATED && !gate_open(kk.ctl)) return;
  const Hyper one = hyper_one(kk);
  const int ti = kk.block_tensor[blockIdx.x];
  const Hyper k = hyper_row(kk, ti, one);
  float* g = (float*)(GATED && !kk.has[ti] ? 0ull : kk.g[ti]);
  const float om = EMA ? kk.norm[1] : 0.f;                   // written by opt_norm_final_kernel of this step
  if (!g) {
    if (EMA) ema_only_chunk(kk, ti, om);
    return;
  }
  if (RULE == RULE_SGD) { sgd_chunk<EMA>(kk, k, ti, g, clip_coef(k, kk.norm[0]), om); return; }     // (before kk.v is read: SGD has no second arena)
  float* p = (float*)kk.p[ti]; float* m = (float*)kk.m[ti]; float* v = (float*)kk.v[ti];
  float* ea = EMA ? (float*)kk.e[ti] : nullptr;
  const float coef = clip_coef(k, kk.norm[0]);
  const float t = (float)kk.steps[ti];                       // already advanced by opt_norm_final_kernel
  const float step_size = k.lr / (1.0f - powf(k.beta1, t)), bc2_sqrt = sqrtf(1.0f - powf(k.beta2, t));
  const long long n = kk.n[ti], off = (long long)(blockIdx.x - kk.block_first[ti]) * OPT_CHUNK;
  const long long end = off + OPT_CHUNK < n ? off + OPT_CHUNK : n;
  const bool alg = (((unsigned long long)(g + off)) & 15ull) == 0;
  const bool alp = ((((unsigned long long)(p + off)) | ((unsigned long long)(m + off)) | ((unsigned long long)(v + off))) & 15ull) == 0;
  const bool ale = EMA && (((unsigned long long)(ea + off)) & 15ull) == 0;
  // one code path for the arithmetic (see load4_any): vector or scalar memory operations, identical values
  for (long long i = off + threadIdx.x * 4; i < end; i += 1024) {
    if (i + 3 < end) {
      f32x4 gv = load4_any(g + i, alg), pv = load4_any(p + i, alp), mv = load4_any(m + i, alp), vv = load4_any(v + i, alp);
      f32x4 ev{};
      if (EMA) ev = load4_any(ea + i, ale);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pe = pv[e], me = mv[e], ve = vv[e];
        const float ge = gv[e] * coef;
        adamw1(pe, me, ve, ge, k, step_size, bc2_sqrt);
        pv[e] = pe; mv[e] = me; vv[e] = ve; gv[e] = ge;
        if (EMA) ev[e] = ema1(ev[e], pe, om);
      }
      if (alp) { *(f32x4*)(p + i) = pv; *(f32x4*)(m + i) = mv; *(f32x4*)(v + i) = vv; }
      else {
#pragma unroll
        for (int e = 0; e < 4; ++e) { p[i + e] = pv[e]; m[i + e] = mv[e]; v[i + e] = vv[e]; }
      }
      if (EMA) {
        if (ale) *(f32x4*)(ea + i) = ev;
        else {
#pragma unroll
          for (int e = 0; e < 4; ++e) ea[i + e] = ev[e];
        }
      }
      if (kk.write_grad) {
        if (alg) *(f32x4*)(g + i) = gv;
        else {
#pragma unroll
          for (int e = 0; e < 4; ++e) g[i + e] = gv[e];
        }
      }
    } else {
      for (long long j = i; j < end; ++j) { const float gj = g[j] * coef; adamw1(p[j], m[j], v[j], gj, k, step_size, bc2_sqrt); if (kk.write_grad) g[j] = gj; }
      if (EMA) for (long long j = i; j < end; ++j) ea[j] = ema1(ea[j], p[j], om);       // (a loop of its own: the one above stays the EMA-less kernel's, instruction for instruction)
    }
  }
}

// ---- the loop's control block: one-thread launches are its only writers ----
__global__ void train_gate_kernel(const float* __restrict__ loss, effdet_train_ctl_t* __restrict__ ctl) {
  const float l = loss[0];
  if (l == 0.0f) { ctl->skip = 1; ctl->skipped += 1; }       // train.py:110 `if bool(loss == 0): continue` (-0.0 skips; NaN / Inf do not)
  else { ctl->skip = 0; ctl->loss_sum += (double)l; ctl->loss_count += 1; }
}

__global__ void train_pending_kernel(effdet_train_ctl_t* __restrict__ ctl) {
  if (!ctl->skip) ctl->pending += 1;
}

__global__ void train_release_kernel(effdet_train_ctl_t* __restrict__ ctl) {
  if (gate_open(ctl)) { ctl->pending = 0; ctl->applied += 1; }
}

__global__ __launch_bounds__(256) void grad_accumulate_kernel(const unsigned long long* __restrict__ grads,
                                                              const unsigned long long* __restrict__ acc, const long long* __restrict__ numel,
                                                              const int* __restrict__ block_tensor, const int* __restrict__ block_first,
                                                              const effdet_train_ctl_t* __restrict__ ctl) {
  if (ctl->skip) return;                                     // a skipped micro-step: its gradients (NaN included) are never read
  const int ti = block_tensor[blockIdx.x];
  const float* g = (const float*)grads[ti];
  if (!g) return;
  float* a = (float*)acc[ti];
  const bool first = ctl->pending == 0;                      // the first micro-batch of a window WRITES: no zeroing pass
  const long long n = numel[ti], off = (long long)(blockIdx.x - block_first[ti]) * OPT_CHUNK;
  const long long end = off + OPT_CHUNK < n ? off + OPT_CHUNK : n;
  const bool alg = (((unsigned long long)(g + off)) & 15ull) == 0, ala = (((unsigned long long)(a + off)) & 15ull) == 0;
  for (long long i = off + threadIdx.x * 4; i < end; i += 1024) {
    if (i + 3 < end) {
      f32x4 gv = load4_any(g + i, alg);
      if (!first) {
        const f32x4 av = load4_any(a + i, ala);
#pragma unroll
        for (int e = 0; e < 4; ++e) gv[e] = av[e] + gv[e];
      }
      if (ala) *(f32x4*)(a + i) = gv;
      else {
#pragma unroll
        for (int e = 0; e < 4; ++e) a[i + e] = gv[e];
      }
    } else {
      for (long long j = i; j < end; ++j) a[j] = first ? g[j] : a[j] + g[j];
    }
  }
}

// in-place exchange of p and e over the optimizer's block table (one launch; no control word is read)
__global__ __launch_bounds__(256) void ema_swap_kernel(const unsigned long long* __restrict__ params, const unsigned long long* __restrict__ ema,
                                                       const long long* __restrict__ numel, const int* __restrict__ block_tensor,
                                                       const int* __restrict__ block_first) {
  const int ti = block_tensor[blockIdx.x];
  float* p = (float*)params[ti]; float* e = (float*)ema[ti];
  const long long n = numel[ti], off = (long long)(blockIdx.x - block_first[ti]) * OPT_CHUNK;
  const long long end = off + OPT_CHUNK < n ? off + OPT_CHUNK : n;
  const bool alp = (((unsigned long long)(p + off)) & 15ull) == 0, ale = (((unsigned long long)(e + off)) & 15ull) == 0;
  for (long long i = off + threadIdx.x * 4; i < end; i += 1024) {
    if (i + 3 < end) {
      const f32x4 pv = load4_any(p + i, alp), ev = load4_any(e + i, ale);
      if (alp) *(f32x4*)(p + i) = ev;
      else {
#pragma unroll
        for (int c = 0; c < 4; ++c) p[i + c] = ev[c];
      }
      if (ale) *(f32x4*)(e + i) = pv;
      else {
#pragma unroll
        for (int c = 0; c < 4; ++c) e[i + c] = pv[c];
      }
    } else {
      for (long long j = i; j < end; ++j) { const float x = p[j]; p[j] = e[j]; e[j] = x; }
    }
  }
}

template <bool GATED, bool EMA = false> int launch_step(const OptK& k, float max_norm, hipStream_t st) {
  if (max_norm > 0.f) {
    hipLaunchKernelGGL(opt_norm_kernel<GATED>, dim3(k.nblocks), dim3(256), 0, st, k);
    EFFDET_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL((opt_norm_final_kernel<GATED, EMA>), dim3(1), dim3(1024), 0, st, (const float*)k.partial, max_norm > 0.f ? k.nblocks : 0,
                     k.norm, GATED ? k.has : k.g, k.steps, k.ntensors, k.ctl, EmaStep{k.ectl, k.hyper, k.ema_decay, k.ema_warmup});
  EFFDET_CHECK_LAUNCH();
  hipLaunchKernelGGL((opt_adamw_kernel<GATED, EMA>), dim3(k.nblocks), dim3(256), 0, st, k);
  EFFDET_CHECK_LAUNCH();
  return EFFDET_OK;
}

}  // namespace

extern "C" int effdet_clip_adamw_step(const unsigned long long* params, const unsigned long long* grads, const unsigned long long* exp_avg,
                                      const unsigned long long* exp_avg_sq, const long long* numel, const int* block_tensor,
                                      const int* block_first, int ntensors, int nblocks, float* scratch, int* steps, float max_norm,
                                      float lr, float beta1, float beta2, float eps, float weight_decay, int write_grad,
                                      const float* hyper_dev, effdet_stream_t stream) {
  if (!params || !grads || !exp_avg || !exp_avg_sq || !numel || !block_tensor || !block_first || !scratch || !steps || nblocks < 1 ||
      ntensors < 1)
    return EFFDET_EINVAL;
  OptK k{};
  k.p = params; k.g = grads; k.m = exp_avg; k.v = exp_avg_sq; k.n = numel; k.block_tensor = block_tensor; k.block_first = block_first;
  k.norm = scratch; k.partial = scratch + 64;                       // scratch: 64 + nblocks floats
  k.max_norm = max_norm; k.lr = lr; k.beta1 = beta1; k.beta2 = beta2; k.eps = eps; k.wd = weight_decay;
  k.steps = steps; k.nblocks = nblocks; k.ntensors = ntensors; k.write_grad = write_grad; k.hyper = hyper_dev;
  return launch_step<false>(k, max_norm, (hipStream_t)stream);
}

extern "C" int effdet_train_gate(const float* loss, effdet_train_ctl_t* ctl, effdet_stream_t stream) {
  if (!loss || !ctl) return EFFDET_EINVAL;
  hipLaunchKernelGGL(train_gate_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, loss, ctl);
  EFFDET_CHECK_LAUNCH();
  return EFFDET_OK;
}

extern "C" int effdet_grad_accumulate(const unsigned long long* grads, const unsigned long long* acc, const long long* numel,
                                      const int* block_tensor, const int* block_first, int ntensors, int nblocks, effdet_train_ctl_t* ctl,
                                      effdet_stream_t stream) {
  if (!grads || !acc || !numel || !block_tensor || !block_first || !ctl || nblocks < 1 || ntensors < 1) return EFFDET_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(grad_accumulate_kernel, dim3(nblocks), dim3(256), 0, st, grads, acc, numel, block_tensor, block_first,
                     (const effdet_train_ctl_t*)ctl);
  EFFDET_CHECK_LAUNCH();
  hipLaunchKernelGGL(train_pending_kernel, dim3(1), dim3(1), 0, st, ctl);
  EFFDET_CHECK_LAUNCH();
  return EFFDET_OK;
}

extern "C" int effdet_clip_adamw_step_gated(const unsigned long long* params, const unsigned long long* grads, const unsigned long long* acc,
                                            const unsigned long long* exp_avg, const unsigned long long* exp_avg_sq, const long long* numel,
                                            const int* block_tensor, const int* block_first, int ntensors, int nblocks, float* scratch,
                                            int* steps, float max_norm, float lr, float beta1, float beta2, float eps, float weight_decay,
                                            const float* hyper_dev, effdet_train_ctl_t* ctl, effdet_stream_t stream) {
  if (!params || !grads || !acc || !exp_avg || !exp_avg_sq || !numel || !block_tensor || !block_first || !scratch || !steps || !ctl ||
      nblocks < 1 || ntensors < 1)
    return EFFDET_EINVAL;
  OptK k{};
  k.p = params; k.g = acc; k.has = grads; k.m = exp_avg; k.v = exp_avg_sq; k.n = numel; k.block_tensor = block_tensor; k.block_first = block_first;
  k.norm = scratch; k.partial = scratch + 64;
  k.max_norm = max_norm; k.lr = lr; k.beta1 = beta1; k.beta2 = beta2; k.eps = eps; k.wd = weight_decay;
  k.steps = steps; k.nblocks = nblocks; k.ntensors = ntensors; k.write_grad = 0; k.hyper = hyper_dev; k.ctl = ctl;
  hipStream_t st = (hipStream_t)stream;
  const int rc = launch_step<true>(k, max_norm, st);
  if (rc != EFFDET_OK) return rc;
  hipLaunchKernelGGL(train_release_kernel, dim3(1), dim3(1), 0, st, ctl);
  EFFDET_CHECK_LAUNCH();
  return EFFDET_OK;
}

// ---- include/effdet_ema.h: the two steps with the parameter average as one more stream, and the in-place weight swap ----
extern "C" int effdet_clip_adamw_step_ema(const unsigned long long* params, const unsigned long long* grads, const unsigned long long* exp_avg,
                                          const unsigned long long* exp_avg_sq, const unsigned long long* ema, const long long* numel,
                                          const int* block_tensor, const int* block_first, int ntensors, int nblocks, float* scratch,
                                          int* steps, float max_norm, float lr, float beta1, float beta2, float eps, float weight_decay,
                                          int write_grad, float ema_decay, int ema_warmup, const float* hyper_dev, effdet_ema_ctl_t* ema_ctl,
                                          effdet_stream_t stream) {
  if (!params || !grads || !exp_avg || !exp_avg_sq || !ema || !numel || !block_tensor || !block_first || !scratch || !steps || !ema_ctl ||
      nblocks < 1 || ntensors < 1)
    return EFFDET_EINVAL;
  if (!hyper_dev && !(ema_decay >= 0.f && ema_decay < 1.f)) return EFFDET_EINVAL;
  OptK k{};
  k.p = params; k.g = grads; k.m = exp_avg; k.v = exp_avg_sq; k.n = numel; k.block_tensor = block_tensor; k.block_first = block_first;
  k.norm = scratch; k.partial = scratch + 64;
  k.max_norm = max_norm; k.lr = lr; k.beta1 = beta1; k.beta2 = beta2; k.eps = eps; k.wd = weight_decay;
  k.steps = steps; k.nblocks = nblocks; k.ntensors = ntensors; k.write_grad = write_grad; k.hyper = hyper_dev;
  k.e = ema; k.ectl = ema_ctl; k.ema_decay = ema_decay; k.ema_warmup = ema_warmup;
  return launch_step<false, true>(k, max_norm, (hipStream_t)stream);
}

extern "C" int effdet_clip_adamw_step_gated_ema(const unsigned long long* params, const unsigned long long* grads,
                                                const unsigned long long* acc, const unsigned long long* exp_avg,
                                                const unsigned long long* exp_avg_sq, const unsigned long long* ema, const long long* numel,
                                                const int* block_tensor, const int* block_first, int ntensors, int nblocks, float* scratch,
                                                int* steps, float max_norm, float lr, float beta1, float beta2, float eps, float weight_decay,
                                                float ema_decay, int ema_warmup, const float* hyper_dev, effdet_train_ctl_t* ctl,
                                                effdet_ema_ctl_t* ema_ctl, effdet_stream_t stream) {
  if (!params || !grads || !acc || !exp_avg || !exp_avg_sq || !ema || !numel || !block_tensor || !block_first || !scratch || !steps || !ctl ||
      !ema_ctl || nblocks < 1 || ntensors < 1)
    return EFFDET_EINVAL;
  if (!hyper_dev && !(ema_decay >= 0.f && ema_decay < 1.f)) return EFFDET_EINVAL;
  OptK k{};
  k.p = params; k.g = acc; k.has = grads; k.m = exp_avg; k.v = exp_avg_sq; k.n = numel; k.block_tensor = block_tensor; k.block_first = block_first;
  k.norm = scratch; k.partial = scratch + 64;
  k.max_norm = max_norm; k.lr = lr; k.beta1 = beta1; k.beta2 = beta2; k.eps = eps; k.wd = weight_decay;
  k.steps = steps; k.nblocks = nblocks; k.ntensors = ntensors; k.write_grad = 0; k.hyper = hyper_dev; k.ctl = ctl;
  k.e = ema; k.ectl = ema_ctl; k.ema_decay = ema_decay; k.ema_warmup = ema_warmup;
  hipStream_t st = (hipStream_t)stream;
  const int rc = launch_step<true, true>(k, max_norm, st);
  if (rc != EFFDET_OK) return rc;
  hipLaunchKernelGGL(train_release_kernel, dim3(1), dim3(1), 0, st, ctl);
  EFFDET_CHECK_LAUNCH();
  return EFFDET_OK;
}

extern "C" int effdet_ema_swap(const unsigned long long* params, const unsigned long long* ema, const long long* numel,
                               const int* block_tensor, const int* block_first, int ntensors, int nblocks, effdet_stream_t stream) {
  if (!params || !ema || !numel || !block_tensor || !block_first || nblocks < 1 || ntensors < 1) return EFFDET_EINVAL;
  hipLaunchKernelGGL(ema_swap_kernel, dim3(nblocks), dim3(256), 0, (hipStream_t)stream, params, ema, numel, block_tensor, block_first);
  EFFDET_CHECK_LAUNCH();
  return EFFDET_OK;
}

// ---- include/effdet_opt_groups.h: parameter groups (a hyper table indexed per tensor) and the SGD rule, all four forms ----
namespace {

// the norm pass is the one-group form's (it reads the OptK part only: max_norm / ema_decay of row 0 through k.hyper); the update is the
// GROUPED instantiation of the rule
template <bool GATED, bool EMA, int RULE> int launch_step_groups(const OptG& k, float max_norm, hipStream_t st) {
  const OptK& k1 = k;
  if (max_norm > 0.f) {
    hipLaunchKernelGGL(opt_norm_kernel<GATED>, dim3(k.nblocks), dim3(256), 0, st, k1);
    EFFDET_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL((opt_norm_final_kernel<GATED, EMA>), dim3(1), dim3(1024), 0, st, (const float*)k.partial, max_norm > 0.f ? k.nblocks : 0,
                     k.norm, GATED ? k.has : k.g, k.steps, k.ntensors, k.ctl, EmaStep{k.ectl, k.hyper, k.ema_decay, k.ema_warmup});
  EFFDET_CHECK_LAUNCH();
  hipLaunchKernelGGL((opt_adamw_kernel<GATED, EMA, true, RULE>), dim3(k.nblocks), dim3(256), 0, st, k);
  EFFDET_CHECK_LAUNCH();
  if (GATED) {
    hipLaunchKernelGGL(train_release_kernel, dim3(1), dim3(1), 0, st, const_cast<effdet_train_ctl_t*>(k.ctl));
    EFFDET_CHECK_LAUNCH();
  }
  return EFFDET_OK;
}

template <int RULE> int launch_step_groups_form(const OptG& k, int flags, float max_norm, hipStream_t st) {
  switch (flags) {
    case 0: return launch_step_groups<false, false, RULE>(k, max_norm, st);
    case EFFDET_OPT_EMA: return launch_step_groups<false, true, RULE>(k, max_norm, st);
    case EFFDET_OPT_GATED: return launch_step_groups<true, false, RULE>(k, max_norm, st);
    default: return launch_step_groups<true, true, RULE>(k, max_norm, st);
  }
}

}  // namespace

extern "C" int effdet_opt_step_groups(int rule, int flags, const unsigned long long* params, const unsigned long long* grads,
                                      const unsigned long long* acc, const unsigned long long* moment1, const unsigned long long* moment2,
                                      const unsigned long long* ema, const long long* numel, const int* block_tensor,
                                      const int* block_first, const int* tensor_group, int ntensors, int nblocks, int ngroups,
                                      float* scratch, int* steps, const float* hyper_table, float max_norm, int write_grad,
                                      int ema_warmup, effdet_train_ctl_t* ctl, effdet_ema_ctl_t* ema_ctl, effdet_stream_t stream) {
  if (rule != EFFDET_OPT_RULE_ADAMW && rule != EFFDET_OPT_RULE_SGD) return EFFDET_EINVAL;
  if (flags & ~(EFFDET_OPT_GATED | EFFDET_OPT_EMA)) return EFFDET_EINVAL;
  const bool gated = flags & EFFDET_OPT_GATED, avg = flags & EFFDET_OPT_EMA;
  if (!params || !grads || !moment1 || !numel || !block_tensor || !block_first || !tensor_group || !scratch || !steps || !hyper_table ||
      nblocks < 1 || ntensors < 1 || ngroups < 1)
    return EFFDET_EINVAL;
  if ((rule == EFFDET_OPT_RULE_ADAMW) != (moment2 != nullptr)) return EFFDET_EINVAL;      // two arenas for AdamW, one for SGD
  if (gated != (acc != nullptr) || gated != (ctl != nullptr) || avg != (ema != nullptr) || avg != (ema_ctl != nullptr)) return EFFDET_EINVAL;
  if (gated && write_grad) return EFFDET_EINVAL;
  OptG k{};
  k.p = params; k.m = moment1; k.v = moment2; k.n = numel; k.block_tensor = block_tensor; k.block_first = block_first;
  if (gated) { k.g = acc; k.has = grads; k.ctl = ctl; } else k.g = grads;
  k.norm = scratch; k.partial = scratch + 64;                       // scratch: 64 + nblocks floats
  k.steps = steps; k.nblocks = nblocks; k.ntensors = ntensors; k.write_grad = write_grad;
  k.hyper = hyper_table; k.table = hyper_table; k.tensor_group = tensor_group;
  k.e = ema; k.ectl = ema_ctl; k.ema_warmup = ema_warmup;
  hipStream_t st = (hipStream_t)stream;
  if (rule == EFFDET_OPT_RULE_SGD) return launch_step_groups_form<RULE_SGD>(k, flags, max_norm, st);
  return launch_step_groups_form<RULE_ADAMW>(k, flags, max_norm, st);
}

extern "C" int effdet_opt_chunk(void) { return OPT_CHUNK; }
