"""Fused train-step tail: global-norm gradient clipping + AdamW in three HIP launches.

Replaces the pair of the reference's train step (train.py:115-118)

    torch.nn.utils.clip_grad_norm_(model.parameters(), 0.1)
    optimizer.step()                      # torch.optim.AdamW(lr=1e-4), train.py:268

with `ClipAdamW(params, lr=..., max_norm=0.1).step()`: same arithmetic (clip coefficient max_norm / (norm + 1e-6)
clamped to 1; decoupled weight decay; bias-corrected moments), one pass for the norm and one for the update over a
device-resident pointer table instead of ~17 foreach / multi-tensor launches.  Only the gradient pointers change from
step to step (fresh tensors after zero_grad(set_to_none=True)); they are refreshed through a pinned staging buffer.
fp32 parameters on one GPU; moments live in two flat arenas.  There is no CPU fallback.

`ClipAdamW(..., accumulate=True)` adds the rest of the reference's loop body (train.py:104-120) as device-side gates, so that a
captured loop (graph.GraphedTrainLoop) takes no host decision that depends on data:

    loss = cls.mean() + reg.mean(); loss.backward()
    opt.accumulate_grads(loss)          # `if bool(loss == 0): continue` + the sum over micro-batches + total_loss.append(loss.item())
    if (idx + 1) % grad_accumulation_steps == 0:
        opt.step()                      # clip + AdamW on the sum; a no-op when the micro-step just run was skipped or nothing is pending

A third arena holds the sum, a 32-byte device control block (effdet_train_ctl_t) the skip flag, the number of pending micro-batches,
the counters and the fp64 loss meter; loss_meter() reads it back (one device-to-host copy), reset_epoch() clears it.

`ClipAdamW(..., ema_decay=0.9998)` keeps an exponential moving average of the parameters (the EfficientDet paper trains and evaluates
with one) as one more stream of the update kernel: an fp32 arena with the moments' offsets and a device counter of the updates made.
On every step that is APPLIED (the gated form decides that on the device), for every tensor of the table, with p the value after AdamW:

    d = min(decay, (1 + updates) / (10 + updates)) if ema_warmup else decay;   e += (1 - d) * (p - e);   updates += 1

No second pass over the parameters, nothing extra to capture (GraphedTrainStep / GraphedTrainLoop call step()), and the decay travels
in the device hyper buffer like lr.  swap_ema() exchanges parameters and average in place; `with opt.ema_weights():` evaluates with the
averaged weights and swaps back; checkpoint.ema_state_dict(model, opt) is the file to publish."""
import contextlib
import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L
from . import ops as ops_mod


class ClipAdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=0.0, write_clipped_grads=False,
                 accumulate=False, ema_decay=None, ema_warmup=True):
        if accumulate and write_clipped_grads:
            raise ValueError('ClipAdamW: write_clipped_grads=True cannot be combined with accumulate=True (the step clips the sum held in '
                             'the accumulation arena; p.grad holds one micro-batch and is not what was clipped)')
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_norm=max_norm)
        self.ema = ema_decay is not None
        if self.ema:                         # (the key exists only with the average on: param_groups of a plain ClipAdamW stay as they were)
            defaults['ema_decay'] = self._checked_decay(ema_decay)
        self.ema_warmup = bool(ema_warmup)
        self._swapped = False                # swap_ema(): the parameters hold the average and the arena the trained weights
        super().__init__(params, defaults)
        if len(self.param_groups) != 1:
            raise ValueError('ClipAdamW supports a single parameter group (the reference uses one, train.py:268)')
        self.write_clipped_grads = bool(write_clipped_grads)
        self.accumulate = bool(accumulate)
        self._grad_mask = None               # accumulate: which tensors had a gradient in the epoch's first micro-step
        self._table = None
        self._step = 0
        self._captured = False               # a step() ran under stream capture (its launch sequence is frozen in a hipGraph)

    @staticmethod
    def _checked_decay(d):
        """0 <= decay < 1 as the fp32 value the kernel reads (a decay that rounds to 1.0f would freeze the average); NaN is refused."""
        try:
            d = float(d)
        except (TypeError, ValueError):
            raise ValueError('ClipAdamW: ema_decay must be a number in [0, 1), got %r' % (d,))
        if math.isnan(d) or not (0.0 <= d < 1.0) or not float(np.float32(d)) < 1.0:
            raise ValueError('ClipAdamW: ema_decay must satisfy 0 <= decay < 1 (as fp32), got %r' % (d,))
        return d

    # ---- the device tables (built once; parameter and moment storage is stable) ----
    def _build(self):
        ps = [p for p in self.param_groups[0]['params'] if p.requires_grad]
        if not ps:
            raise ValueError('no trainable parameters')
        dev = ps[0].device
        for p in ps:
            if p.dtype != torch.float32 or p.device != dev or not p.is_contiguous() or not p.is_cuda:
                raise ValueError('ClipAdamW needs contiguous fp32 parameters on one GPU')
        chunk = int(L.lib().effdet_opt_chunk())
        n = len(ps)
        numel = [p.numel() for p in ps]
        offs = np.concatenate([[0], np.cumsum([(k + 63) // 64 * 64 for k in numel])]).astype(np.int64)
        self.exp_avg = torch.zeros(int(offs[-1]), dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(int(offs[-1]), dtype=torch.float32, device=dev)
        block_tensor, block_first, nb = [], [], 0
        for i, k in enumerate(numel):
            b = (k + chunk - 1) // chunk
            block_first.append(nb); block_tensor += [i] * b; nb += b
        i64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int64)).to(dev)
        i32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int32)).to(dev)
        t = {
            'params': ps, 'n': n, 'nblocks': nb,
            'p_ptr': i64([p.data_ptr() for p in ps]),
            'm_ptr': i64([self.exp_avg.data_ptr() + 4 * int(o) for o in offs[:-1]]),
            'v_ptr': i64([self.exp_avg_sq.data_ptr() + 4 * int(o) for o in offs[:-1]]),
            'numel': i64(numel), 'block_tensor': i32(block_tensor), 'block_first': i32(block_first),
            'g_ptr': torch.zeros(n, dtype=torch.int64, device=dev),
            # pinned staging ring for the gradient-pointer upload: a slot is rewritten only after the event recorded behind
            # its previous H2D copy has completed (the host may run a step ahead of the stream)
            'g_host': [torch.zeros(n, dtype=torch.int64).pin_memory() for _ in range(2)], 'g_evt': [None, None], 'g_slot': 0,
            'g_graph_host': torch.zeros(n, dtype=torch.int64).pin_memory(),      # source of the memcpy node of a captured step

            'g_last': None,
            'scratch': torch.zeros(64 + nb, dtype=torch.float32, device=dev), 'offs': offs,
            'steps': torch.zeros(n, dtype=torch.int32, device=dev), 'p_sig': [p.data_ptr() for p in ps],
            # hyper-parameters live on the device (read by the update kernel at run time): a captured step follows the
            # schedule of param_groups[0] -- sync_hyper() refreshes them ahead of a graph replay
            # (a seventh float carries the EMA decay; the six the kernels without the average read stay where they are)
            'hyper': torch.zeros(7 if self.ema else 6, dtype=torch.float32, device=dev),
            'hyper_host': torch.zeros(7 if self.ema else 6, dtype=torch.float32).pin_memory(),
            'hyper_last': None, 'hyper_evt': None,
        }
        if self.ema:
            # the average (same offsets as the moments; e = p to begin with) and its control block (effdet_ema_ctl_t: the update counter)
            self.ema_avg = torch.zeros(int(offs[-1]), dtype=torch.float32, device=dev)
            t['e_ptr'] = i64([self.ema_avg.data_ptr() + 4 * int(o) for o in offs[:-1]])
            t['ectl'] = torch.zeros(C.sizeof(L.EmaCtl) // 4, dtype=torch.int32, device=dev)
            t['e_views'] = [self.ema_avg[int(offs[i]):int(offs[i]) + numel[i]].view_as(p) for i, p in enumerate(ps)]
            with torch.no_grad():
                for e, p in zip(t['e_views'], ps):
                    e.copy_(p)
            self._swapped = False
        if self.accumulate:
            # the sum over a window's micro-batches (same offsets as the moments; written, not added to, by the first micro-batch of a
            # window, so it is never zeroed) and the control block (effdet_train_ctl_t, 32 bytes; zero = start of an epoch)
            self.grad_acc = torch.zeros(int(offs[-1]), dtype=torch.float32, device=dev)
            t['a_ptr'] = i64([self.grad_acc.data_ptr() + 4 * int(o) for o in offs[:-1]])
            t['ctl'] = torch.zeros(C.sizeof(L.TrainCtl) // 8, dtype=torch.int64, device=dev)
            self._grad_mask = None
        for i, p in enumerate(ps):                                     # per-parameter views for state_dict()
            self.state[p] = {'step': torch.tensor(0.0),                # refreshed from the device counters in state_dict()
                             'exp_avg': self.exp_avg[int(offs[i]):int(offs[i]) + numel[i]].view_as(p),
                             'exp_avg_sq': self.exp_avg_sq[int(offs[i]):int(offs[i]) + numel[i]].view_as(p)}
            if self.ema:
                self.state[p]['ema'] = t['e_views'][i]
        self._table = t

    # ---- checkpointing (train.py:279-291 saves only the model; resuming needs the moments + per-tensor step counters) ----
    def state_dict(self):
        """torch.optim.AdamW-compatible: per-parameter {'step', 'exp_avg', 'exp_avg_sq'}; 'step' is read back from the
        device-resident counters (they advance on the GPU), the moments are views of the two arenas.  accumulate=True adds nothing:
        a checkpoint is an epoch boundary, where nothing is pending, so the accumulation arena and the control block are not saved."""
        if self._table is not None:
            steps = self._table['steps'].cpu()
            for i, p in enumerate(self._table['params']):
                self.state[p]['step'] = torch.tensor(float(steps[i]))
        sd = super().state_dict()
        if self.ema:
            # the average travels as 'ema' per parameter (views of the arena) and the counter as 'ema_updates', read from the device.
            # Save outside ema_weights(): while swapped in, 'ema' holds the trained weights and the model the average.
            sd['ema_updates'] = self.ema_updates()
        return sd

    def load_state_dict(self, state_dict):
        """Loads a state_dict of this class or of torch.optim.AdamW over the same parameter list: moments are copied INTO
        the arenas and the step counters into the device array (super() alone would leave self.state pointing at fresh
        tensors the kernels never see)."""
        if self._swapped:
            raise RuntimeError('ClipAdamW.load_state_dict while the averaged weights are swapped in; call swap_ema() (or leave ema_weights()) first')
        decay = self.param_groups[0].get('ema_decay')
        super().load_state_dict(state_dict)
        g = self.param_groups[0]                                       # (now the loaded group: the average is on or off by construction)
        if not self.ema:
            g.pop('ema_decay', None)
        else:
            g['ema_decay'] = self._checked_decay(decay if g.get('ema_decay') is None else g['ema_decay'])
        loaded = {p: dict(st) for p, st in self.state.items()}
        self.state.clear()
        self._build()                                                  # (with the average on: e = the current p, updates = 0)
        t = self._table
        if self.ema:
            have = [i for i, p in enumerate(t['params']) if (loaded.get(p) or {}).get('ema') is not None]
            for i in have:
                p = t['params'][i]
                t['e_views'][i].copy_(loaded[p]['ema'].to(p.device, torch.float32).view_as(p))
            # a state without the average (torch's AdamW, or this class with it off) starts one at the current parameters
            t['ectl'][0] = int(state_dict.get('ema_updates', 0)) if have else 0
        steps = torch.zeros(t['n'], dtype=torch.int32)
        for i, p in enumerate(t['params']):
            st = loaded.get(p)
            if not st:
                continue
            self.state[p]['exp_avg'].copy_(st['exp_avg'].to(p.device, torch.float32).view_as(p))
            self.state[p]['exp_avg_sq'].copy_(st['exp_avg_sq'].to(p.device, torch.float32).view_as(p))
            steps[i] = int(float(st['step']))
        t['steps'].copy_(steps)
        self._step = int(steps.max()) if t['n'] else 0

    def _hyper_values(self):
        g = self.param_groups[0]
        b1, b2 = g['betas']
        hv = (float(g['max_norm'] or 0.0), float(g['lr']), float(b1), float(b2), float(g['eps']), float(g['weight_decay']))
        return hv + (self._checked_decay(g['ema_decay']),) if self.ema else hv

    def sync_hyper(self):
        """Upload param_groups[0]'s {max_norm, lr, betas, eps, weight_decay} (and ema_decay) to the device buffer the update kernel reads, if
        they changed since the last upload.  step() calls it; graph.GraphedTrainStep calls it before every replay, so an lr
        scheduler (train.py:133,269: ReduceLROnPlateau) drives captured steps exactly like eager ones."""
        if self._table is None:
            return
        t, hv = self._table, self._hyper_values()
        if hv == t['hyper_last']:
            return
        if t['hyper_last'] is not None and (hv[0] > 0.0) != (t['hyper_last'][0] > 0.0) and self._captured:
            raise RuntimeError('ClipAdamW: max_norm switched between 0 and > 0 after the step was captured as a hipGraph '
                               '(the norm pass is part of the captured launch sequence); re-capture the step')
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('ClipAdamW: hyper-parameters changed under stream capture; call sync_hyper() before capturing')
        if t['hyper_evt'] is not None:
            t['hyper_evt'].synchronize()                               # the copy that last read the pinned buffer has finished
        t['hyper_host'].copy_(torch.tensor(hv, dtype=torch.float32))
        t['hyper'].copy_(t['hyper_host'], non_blocking=True)
        ev = torch.cuda.Event(); ev.record()
        t['hyper_evt'], t['hyper_last'] = ev, hv

    def _ensure_table(self):
        if self._table is None or self._table['p_sig'] != [p.data_ptr() for p in self._table['params']]:
            if self.accumulate and torch.cuda.is_current_stream_capturing():
                raise RuntimeError('ClipAdamW: the device tables are not built (or a parameter moved) and the stream is capturing: '
                                   'building them allocates and uploads; run one eager accumulate_grads() + step() before capturing')
            self._build()
        return self._table

    def _grad_ptrs(self):
        ptrs = []
        for p in self._table['params']:
            gr = p.grad
            if gr is None:
                ptrs.append(0)
                continue
            if gr.dtype != torch.float32 or not gr.is_contiguous():
                gr = gr.float().contiguous(); p.grad = gr
            ptrs.append(gr.data_ptr())
        return ptrs

    def _upload_grad_ptrs(self, ptrs):
        t = self._table
        if ptrs != t['g_last']:                                        # (DDP bucket views keep their addresses: no upload)
            if torch.cuda.is_current_stream_capturing():
                # hipGraph capture: the memcpy node keeps reading this pinned buffer on every replay, so it gets a buffer of
                # its own that is not rewritten by eager steps (gradient addresses are static inside the graph's memory pool)
                t['g_graph_host'].copy_(torch.tensor(ptrs, dtype=torch.int64))      # (allocated in _build: no pinned allocation under capture)
                t['g_ptr'].copy_(t['g_graph_host'], non_blocking=True)
                t['g_last'] = None                                     # eager steps after the capture upload again
            else:
                slot = t['g_slot']; t['g_slot'] = slot ^ 1
                if t['g_evt'][slot] is not None:
                    t['g_evt'][slot].synchronize()                     # the copy that last read this pinned slot has finished
                t['g_host'][slot].copy_(torch.tensor(ptrs, dtype=torch.int64))
                t['g_ptr'].copy_(t['g_host'][slot], non_blocking=True)
                ev = torch.cuda.Event(); ev.record()
                t['g_evt'][slot] = ev
                t['g_last'] = ptrs

    def _hyper_ready(self):
        t = self._table
        if torch.cuda.is_current_stream_capturing():
            self._captured = True
            if t['hyper_last'] is None:
                raise RuntimeError('ClipAdamW: run one eager step (or sync_hyper()) before capturing the step as a hipGraph')
            if self._hyper_values() != t['hyper_last']:
                raise RuntimeError('ClipAdamW: param_groups changed since the last upload of the device hyper-parameter buffer and '
                                   'the stream is capturing (no upload possible); call sync_hyper() before capturing')
        else:
            self.sync_hyper()

    def _one_group(self):
        if len(self.param_groups) != 1:         # (before anything is uploaded or counted: a refused step leaves no trace)
            raise RuntimeError('ClipAdamW honours ONE parameter group (the reference builds one, train.py:266); got %d -- other '
                               "groups' lr / weight_decay would be silently ignored" % len(self.param_groups))

    def _not_swapped(self, what):
        if self._swapped:
            raise RuntimeError('ClipAdamW.%s while the averaged weights are swapped in: the step would train the average; call swap_ema() '
                               '(or leave ema_weights()) first' % what)

    @torch.no_grad()
    def step(self, closure=None):
        self._one_group()
        self._not_swapped('step')
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        t, g = self._ensure_table(), self.param_groups[0]
        if not self.accumulate:
            self._upload_grad_ptrs(self._grad_ptrs())
        self._step += 1
        b1, b2 = g['betas']
        self._hyper_ready()
        ops_mod.bump_param_generation()      # parameters are rewritten through raw pointers: Tensor._version does not move
        if self.accumulate:
            # the gated form: the sum in the arena is the gradient; which tensors have one is what the last accumulate_grads() uploaded.
            # Nothing moves when the micro-step just run was skipped or nothing is pending (decided on the device).
            if self.ema:
                Lb = L.require('effdet_clip_adamw_step_gated_ema')
                L.check(Lb.effdet_clip_adamw_step_gated_ema(L.ptr(t['p_ptr']), L.ptr(t['g_ptr']), L.ptr(t['a_ptr']), L.ptr(t['m_ptr']),
                                                            L.ptr(t['v_ptr']), L.ptr(t['e_ptr']), L.ptr(t['numel']), L.ptr(t['block_tensor']),
                                                            L.ptr(t['block_first']), t['n'], t['nblocks'], L.ptr(t['scratch']),
                                                            L.ptr(t['steps']), float(g['max_norm'] or 0.0), float(g['lr']), float(b1),
                                                            float(b2), float(g['eps']), float(g['weight_decay']), float(g['ema_decay']),
                                                            int(self.ema_warmup), L.ptr(t['hyper']), L.ptr(t['ctl']), L.ptr(t['ectl']),
                                                            L.stream_ptr()),
                        'effdet_clip_adamw_step_gated_ema')
                return loss
            Lb = L.require('effdet_clip_adamw_step_gated')
            L.check(Lb.effdet_clip_adamw_step_gated(L.ptr(t['p_ptr']), L.ptr(t['g_ptr']), L.ptr(t['a_ptr']), L.ptr(t['m_ptr']), L.ptr(t['v_ptr']),
                                                    L.ptr(t['numel']), L.ptr(t['block_tensor']), L.ptr(t['block_first']), t['n'], t['nblocks'],
                                                    L.ptr(t['scratch']), L.ptr(t['steps']), float(g['max_norm'] or 0.0),
                                                    float(g['lr']), float(b1), float(b2), float(g['eps']),
                                                    float(g['weight_decay']), L.ptr(t['hyper']), L.ptr(t['ctl']), L.stream_ptr()),
                    'effdet_clip_adamw_step_gated')
            return loss
        if self.ema:
            Lb = L.require('effdet_clip_adamw_step_ema')
            L.check(Lb.effdet_clip_adamw_step_ema(L.ptr(t['p_ptr']), L.ptr(t['g_ptr']), L.ptr(t['m_ptr']), L.ptr(t['v_ptr']), L.ptr(t['e_ptr']),
                                                  L.ptr(t['numel']), L.ptr(t['block_tensor']), L.ptr(t['block_first']), t['n'], t['nblocks'],
                                                  L.ptr(t['scratch']), L.ptr(t['steps']), float(g['max_norm'] or 0.0), float(g['lr']),
                                                  float(b1), float(b2), float(g['eps']), float(g['weight_decay']),
                                                  int(self.write_clipped_grads), float(g['ema_decay']), int(self.ema_warmup),
                                                  L.ptr(t['hyper']), L.ptr(t['ectl']), L.stream_ptr()),
                    'effdet_clip_adamw_step_ema')
            return loss
        L.check(L.lib().effdet_clip_adamw_step(L.ptr(t['p_ptr']), L.ptr(t['g_ptr']), L.ptr(t['m_ptr']), L.ptr(t['v_ptr']), L.ptr(t['numel']),
                                               L.ptr(t['block_tensor']), L.ptr(t['block_first']), t['n'], t['nblocks'],
                                               L.ptr(t['scratch']), L.ptr(t['steps']), float(g['max_norm'] or 0.0),
                                               float(g['lr']), float(b1), float(b2), float(g['eps']),
                                               float(g['weight_decay']), int(self.write_clipped_grads), L.ptr(t['hyper']), L.stream_ptr()),
                'effdet_clip_adamw_step')
        return loss

    # ---- the reference's loop body around the step (train.py:104-120), accumulate=True only ----
    def _need_accumulate(self, what):
        if not self.accumulate:
            raise RuntimeError('ClipAdamW.%s needs ClipAdamW(accumulate=True)' % what)

    @torch.no_grad()
    def accumulate_grads(self, loss):
        """Call after loss.backward() with the micro-step's fp32 DEVICE scalar loss.  Device side, no host sync: loss == 0 (the
        reference's `if bool(loss == 0): continue`; -0.0 skips, NaN and Inf do not) marks the micro-step skipped and nothing else
        happens; otherwise the loss enters the meter and the current p.grad tensors are added into the accumulation arena (the first
        micro-batch of a window is copied, not added).
        The tensors that have a gradient must be the same ones in every micro-step from reset_epoch() to reset_epoch(): a window's first
        micro-batch overwrites the arena only where it has a gradient, and the host cannot see whether the device skipped a boundary
        step and let pending gradients ride into the next window (train.py's own behaviour), so a window never ends for certain
        before the epoch does."""
        self._need_accumulate('accumulate_grads')
        self._one_group()
        self._not_swapped('accumulate_grads')
        if not (isinstance(loss, torch.Tensor) and loss.is_cuda and loss.dtype == torch.float32 and loss.numel() == 1):
            raise ValueError('ClipAdamW.accumulate_grads needs the loss as a one-element fp32 GPU tensor (it is read on the device)')
        t = self._ensure_table()
        ptrs = self._grad_ptrs()
        mask = [x != 0 for x in ptrs]
        if self._grad_mask is not None and mask != self._grad_mask:
            changed = [i for i, (a, b) in enumerate(zip(mask, self._grad_mask)) if a != b]
            raise RuntimeError('ClipAdamW.accumulate_grads: the set of tensors that have a gradient changed between micro-steps '
                               '(%d tensors, first: parameter %d); the accumulation arena would mix windows' % (len(changed), changed[0]))
        self._grad_mask = mask
        self._upload_grad_ptrs(ptrs)
        if torch.cuda.is_current_stream_capturing():
            self._captured = True
        Lb = L.require('effdet_train_gate', 'effdet_grad_accumulate')
        L.check(Lb.effdet_train_gate(L.ptr(loss.detach()), L.ptr(t['ctl']), L.stream_ptr()), 'effdet_train_gate')
        L.check(Lb.effdet_grad_accumulate(L.ptr(t['g_ptr']), L.ptr(t['a_ptr']), L.ptr(t['numel']), L.ptr(t['block_tensor']),
                                          L.ptr(t['block_first']), t['n'], t['nblocks'], L.ptr(t['ctl']), L.stream_ptr()),
                'effdet_grad_accumulate')

    def _ctl(self):
        return L.TrainCtl.from_buffer_copy(self._table['ctl'].cpu().numpy().tobytes())       # the one device-to-host read

    def loss_meter(self):
        """-> (mean, count, skipped, applied): np.mean(total_loss) of train.py:133 over the micro-steps since reset_epoch() that were not
        skipped (a sequential fp64 sum of the fp32 losses; NaN for count 0, as np.mean([]) is), their number, the number of skipped
        micro-steps and the number of optimizer steps applied.  One device-to-host read."""
        self._need_accumulate('loss_meter')
        if self._table is None:
            return float('nan'), 0, 0, 0
        c = self._ctl()
        return (c.loss_sum / c.loss_count if c.loss_count else float('nan')), int(c.loss_count), int(c.skipped), int(c.applied)

    def pending(self):
        """Micro-batches summed in the arena and not yet applied (one device-to-host read)."""
        self._need_accumulate('pending')
        return 0 if self._table is None else int(self._ctl().pending)

    def reset_epoch(self):
        """optimizer.zero_grad() at the top of train() (train.py:97): pending gradients are dropped, the meter and the counters cleared."""
        self._need_accumulate('reset_epoch')
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('ClipAdamW.reset_epoch under stream capture: an epoch boundary is a host event, not part of a captured step')
        if self._table is not None:
            self._table['ctl'].zero_()
        self._grad_mask = None

    def grad_norm(self):
        """Total gradient norm measured by the last step() (device scalar; clipping enabled only)."""
        return self._table['scratch'][0] if self._table is not None else None

    # ---- the parameter average (ema_decay=...) ----
    def _need_ema(self, what):
        if not self.ema:
            raise RuntimeError('ClipAdamW.%s needs ClipAdamW(ema_decay=...)' % what)

    def ema_params(self):
        """The average, one view of the arena per trainable parameter, in the optimizer's order (while swapped in by swap_ema() these
        hold the trained weights and the parameters the average)."""
        self._need_ema('ema_params')
        return list(self._ensure_table()['e_views'])

    def ema_updates(self):
        """EMA updates applied so far: the device counter (one device-to-host read)."""
        self._need_ema('ema_updates')
        return 0 if self._table is None else int(self._table['ectl'][:1].cpu()[0])

    @torch.no_grad()
    def swap_ema(self):
        """Exchange parameters and average in place (one launch over the optimizer's block table).  After an odd number of calls the
        model computes with the averaged weights, and step() / accumulate_grads() are refused; a second call restores both bit for bit."""
        self._need_ema('swap_ema')
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('ClipAdamW.swap_ema under stream capture: every replay would exchange the weights again; swap outside the graph')
        t = self._ensure_table()
        Lb = L.require('effdet_ema_swap')
        L.check(Lb.effdet_ema_swap(L.ptr(t['p_ptr']), L.ptr(t['e_ptr']), L.ptr(t['numel']), L.ptr(t['block_tensor']), L.ptr(t['block_first']),
                                   t['n'], t['nblocks'], L.stream_ptr()), 'effdet_ema_swap')
        self._swapped = not self._swapped
        ops_mod.bump_param_generation()      # parameters were rewritten through raw pointers: packed-weight caches must refresh

    @contextlib.contextmanager
    def ema_weights(self):
        """`with opt.ema_weights(): evaluate(model)`: the averaged weights are swapped in for the block and the trained ones are back
        after it, also when the block raises."""
        self._need_ema('ema_weights')
        self._not_swapped('ema_weights')
        self.swap_ema()
        try:
            yield self
        finally:
            self.swap_ema()
