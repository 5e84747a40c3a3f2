/* effdet_opt_groups.h -- parameter groups and a second update rule (SGD with momentum) for the fused optimizer step of
 * libeffdet_hip.so: one entry point added to ABI generation 11 after effdet_hip.h's own set.  effdet_hip.h documents
 * effdet_clip_adamw_step / effdet_clip_adamw_step_gated and effdet_ema.h their forms with the parameter average; the tables
 * (params, grads, acc, numel, block_tensor, block_first), scratch (64 + nblocks floats; [0] the norm), steps, the gates and the
 * average are THOSE, and so are the conventions (device pointers, 0 or a negative EFFDET_E* code, work enqueued on `stream`, no
 * allocation and no synchronisation: capture-safe).  A library of the same generation built before this header lacks the symbol, so a
 * binding looks it up by name before the first call.
 *
 * Groups.  tensor_group is a DEVICE int32[ntensors] (0 <= tensor_group[i] < ngroups; the caller guarantees it, nothing checks it on the
 * device) and hyper_table a DEVICE array of ngroups rows of EFFDET_OPT_ROW = 8 floats:
 *     rule AdamW   { max_norm, lr, beta1,    beta2,         eps,      weight_decay, ema_decay, reserved }
 *     rule SGD     { max_norm, lr, momentum, 1 - dampening, nesterov, weight_decay, ema_decay, reserved }
 * A workgroup of the update kernel reads the row of its tensor once; lr, the betas (and with them the bias corrections of the
 * tensor's own step count), eps and weight_decay -- momentum, dampening, nesterov for SGD -- are per group.  max_norm and ema_decay
 * are optimizer-wide: ONE global norm over every tensor of the table in table order (torch.nn.utils.clip_grad_norm_ over all
 * parameters; the partial sums and their order are those of the one-group step), ONE update counter of the average.  Every row must
 * carry the same two values; the norm pass reads row 0's, the update kernel its own row's.  The by-value max_norm only decides whether
 * the norm pass is launched (> 0), as in the one-group entry points: it must agree with the table in that.  With equal rows the result
 * is bit for bit the one-group entry point's.  The launch count is the one-group step's: norm (with clipping), finish, update (and the
 * release of the gate).  A group whose lr and weight_decay are 0 holds its tensors still: AdamW's p -= lr * wd * p and
 * p -= (lr / bc1) * m / (...) subtract a zero (finite moments; the one value that can change is a parameter of -0.0, which may become +0.0), the moments and
 * step counters advance and the average follows the unchanged p.
 *
 * Rule SGD is torch.optim.SGD (no maximize).  Per element, with coef the clip coefficient min(1, max_norm / (norm + 1e-6)) (1 without
 * clipping) and t the tensor's own step count after this step (a tensor without a gradient in a step is skipped: its buffer stays
 * and its count lags, as for AdamW; with the average on it takes the average-only pass):
 *     g' = coef * g
 *     d  = weight_decay != 0 ? g' + weight_decay * p : g'          coupled L2
 *     momentum != 0:  buf = t == 1 ? d : momentum * buf + (1 - dampening) * d        (the buffer starts as a copy of d, undamped)
 *                     u   = nesterov != 0 ? d + momentum * buf : buf
 *     momentum == 0:  u = d                                        (the buffer is neither read nor written)
 *     p  = p - lr * u
 * Every product, sum and difference above is one fp32 operation rounded to nearest, never contracted into an FMA, so a NumPy float32
 * restatement is bit-exact.  1 - dampening arrives as the fp32 rounding of the host's double 1.0 - dampening (torch passes that
 * value as the alpha of its add).  moment1 is the one momentum-buffer table and moment2 must be NULL; for rule AdamW they are
 * exp_avg and exp_avg_sq.  Deviation from torch: a group whose momentum is switched from 0 to non-zero after its tensors have stepped
 * continues from the zero-filled buffer (torch would start it as a copy of d).
 *
 * flags selects the form: EFFDET_OPT_GATED reads acc as the gradient, grads as the has-a-gradient table and does nothing unless the
 * gate of ctl is open, then releases it (effdet_clip_adamw_step_gated); EFFDET_OPT_EMA keeps the average (effdet_ema.h; the decay is
 * hyper_table[6]).  acc / ctl and ema / ema_ctl must be given exactly when their flag is set; write_grad is refused with the gate. */
#ifndef EFFDET_OPT_GROUPS_H
#define EFFDET_OPT_GROUPS_H
#include "effdet_ema.h"
#ifdef __cplusplus
extern "C" {
#endif

#define EFFDET_OPT_ROW 8            /* floats per row of hyper_table */
#define EFFDET_OPT_RULE_ADAMW 0
#define EFFDET_OPT_RULE_SGD 1
#define EFFDET_OPT_GATED 1          /* flags */
#define EFFDET_OPT_EMA 2

int effdet_opt_step_groups(int rule, int flags, const unsigned long long* params, const unsigned long long* grads,
                           const unsigned long long* acc, const unsigned long long* moment1,
                           const unsigned long long* moment2, const unsigned long long* ema, const long long* numel,
                           const int* block_tensor, const int* block_first, const int* tensor_group, int ntensors, int nblocks,
                           int ngroups, float* scratch, int* steps, const float* hyper_table, float max_norm, int write_grad,
                           int ema_warmup, effdet_train_ctl_t* ctl, effdet_ema_ctl_t* ema_ctl, effdet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EFFDET_OPT_GROUPS_H */
