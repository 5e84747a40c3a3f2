/* effdet_ema.h -- the exponential moving average of the parameters, kept by the clip + AdamW step of libeffdet_hip.so, and the in-place
 * exchange of parameters and average for evaluation: entry points added to ABI generation 11 after effdet_hip.h's own set.
 * effdet_hip.h documents effdet_clip_adamw_step / effdet_clip_adamw_step_gated, whose tables, scratch, hyper-parameters and gates
 * these share; its conventions (device pointers, 0 or a negative EFFDET_E* code, work enqueued on `stream`, no allocation and no
 * synchronisation: capture-safe) hold here.  A library of the same generation built before this header lacks the three symbols, so
 * a binding looks them up by name before the first call.
 *
 * ema is a table of ntensors device pointers like exp_avg.  For EVERY tensor of the table -- one without a gradient in this step is
 * not touched by AdamW, but its average still follows its unchanged p -- on every step that is applied, with p the value after the
 * AdamW update of that step:
 *     t  = (float)updates                               updates made so far; 0 on the first
 *     d  = decay                                        fp32: hyper_dev[6] when hyper_dev is given, ema_decay otherwise
 *     if (ema_warmup) d = fminf(d, (1.0f + t) / (10.0f + t))
 *     om = 1.0f - d
 *     e  = e + om * (p - e)                             subtract, multiply, add: three fp32 roundings, never an FMA
 *     updates += 1                                      once per step, not per tensor
 * p, both moments, the step counters and the norm are bit for bit what the entry point without the average computes.  16-byte
 * accesses where the addresses allow, the same values where not.  No launch is added: om is computed once per step by the
 * one-workgroup kernel that finishes the norm, which is also the only reader and the only writer of `updates`.
 * hyper_dev, when given, holds SEVEN floats: {max_norm, lr, beta1, beta2, eps, weight_decay, ema_decay}; with hyper_dev NULL an
 * ema_decay outside [0, 1) (NaN included) is EFFDET_EINVAL.
 * effdet_clip_adamw_step_gated_ema: when the gate is closed (skip set or pending == 0) the average and `updates` stay untouched
 * bit for bit, like everything else.
 * effdet_ema_swap: p[i] <-> ema[i] for every element of every tensor, in one launch over the same block table. */
#ifndef EFFDET_EMA_H
#define EFFDET_EMA_H
#include "effdet_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* DEVICE control block of the average (16 bytes, zero = nothing averaged yet), written by one thread of one launch per step */
typedef struct {
  int updates;          /* EMA updates applied so far */
  int reserved[3];
} effdet_ema_ctl_t;

int effdet_clip_adamw_step_ema(const unsigned long long* params, const unsigned long long* grads,
                               const unsigned long long* exp_avg, const unsigned long long* exp_avg_sq,
                               const unsigned long long* ema, const long long* numel, const int* block_tensor,
                               const int* block_first, int ntensors, int nblocks, float* scratch, int* steps, float max_norm,
                               float lr, float beta1, float beta2, float eps, float weight_decay, int write_grad,
                               float ema_decay, int ema_warmup, const float* hyper_dev, effdet_ema_ctl_t* ema_ctl,
                               effdet_stream_t stream);
int effdet_clip_adamw_step_gated_ema(const unsigned long long* params, const unsigned long long* grads,
                                     const unsigned long long* acc, const unsigned long long* exp_avg,
                                     const unsigned long long* exp_avg_sq, const unsigned long long* ema, const long long* numel,
                                     const int* block_tensor, const int* block_first, int ntensors, int nblocks, float* scratch,
                                     int* steps, float max_norm, float lr, float beta1, float beta2, float eps,
                                     float weight_decay, float ema_decay, int ema_warmup, const float* hyper_dev,
                                     effdet_train_ctl_t* ctl, effdet_ema_ctl_t* ema_ctl, effdet_stream_t stream);
int effdet_ema_swap(const unsigned long long* params, const unsigned long long* ema, const long long* numel,
                    const int* block_tensor, const int* block_first, int ntensors, int nblocks, effdet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EFFDET_EMA_H */
