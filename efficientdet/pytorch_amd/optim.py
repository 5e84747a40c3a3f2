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
averaged weights and swaps back; checkpoint.ema_state_dict(model, opt) is the file to publish.

Parameter groups (include/effdet_opt_groups.h): `ClipAdamW([{'params': ..., 'weight_decay': 0.0}, {'params': ..., 'lr': 1e-5}], ...)`.
The tensor table is the flattened param_groups in order; a per-tensor group index selects a row of a device hyper table, so lr, betas,
eps and weight_decay are per group and follow any torch lr scheduler into a captured step through sync_hyper().  max_norm and
ema_decay are optimizer-wide (one global norm, one EMA counter): groups that disagree are refused.  split_param_groups(model, wd)
builds the usual no-decay / backbone split.  One group keeps making the one-group calls.

`ClipSGD(params, lr, momentum=0.9, weight_decay=4e-5, max_norm=...)` is torch.optim.SGD's rule (momentum, dampening, nesterov, coupled
weight decay) as a second rule of the same pass, with one moment arena and everything else of ClipAdamW: groups, clipping, gates,
average, captured steps, a torch.optim.SGD-compatible state_dict."""
import contextlib
import ctypes as C
import math
import re

import numpy as np
import torch

from . import _lib as L
from . import ops as ops_mod


def layout_tables(group_numels, chunk):
    """The host side of the device tables, from the element counts of each group's trainable tensors (a plain function: no GPU).
    The tensor table is the groups' tensors in order; arena offsets (in elements, each tensor padded to a multiple of 64) and the
    block table (one workgroup per `chunk` elements of a tensor) follow that order and do not know about group boundaries; a group
    without tensors contributes nothing.  -> {'numel', 'tensor_group', 'offs' (n + 1 entries), 'block_tensor', 'block_first', 'nblocks'}"""
    numel = [int(k) for ks in group_numels for k in ks]
    tensor_group = [gi for gi, ks in enumerate(group_numels) for _ in ks]
    if any(k < 1 for k in numel):
        raise ValueError('a parameter without elements cannot be laid out')
    offs = np.concatenate([[0], np.cumsum([(k + 63) // 64 * 64 for k in numel])]).astype(np.int64)
    block_tensor, block_first, nb = [], [], 0
    for i, k in enumerate(numel):
        b = (k + chunk - 1) // chunk
        block_first.append(nb); block_tensor += [i] * b; nb += b
    return {'numel': numel, 'tensor_group': tensor_group, 'offs': offs, 'block_tensor': block_tensor, 'block_first': block_first,
            'nblocks': nb}


def shared_hyper(name, key, values):
    """max_norm and ema_decay are optimizer-wide (one global norm, one EMA counter): the value all groups agree on, or ValueError
    naming the groups that do not."""
    if any(v != values[0] for v in values):
        bad = [i for i, v in enumerate(values) if v != values[0]]
        raise ValueError('%s: %s is optimizer-wide (one global norm, one EMA counter) but param_groups[0] has %r and group%s %s %s'
                         % (name, key, values[0], 's' if len(bad) > 1 else '', ', '.join(map(str, bad)),
                            ', '.join(repr(values[i]) for i in bad)))
    return values[0]


def check_unique_params(name, param_groups):
    seen = {}
    for gi, g in enumerate(param_groups):
        for pi, p in enumerate(g['params']):
            if id(p) in seen:
                raise ValueError('%s: a parameter appears twice (param_groups[%d][%d] and param_groups[%d][%d]); it would be updated '
                                 'twice per step' % ((name,) + seen[id(p)] + (gi, pi)))
            seen[id(p)] = (gi, pi)


_FUSION_WEIGHT = re.compile(r'(^|\.)stack_bifpn_convs\.\d+\.w[12]$')


def split_param_groups(model, weight_decay, backbone_lr_scale=1.0, decay_norm_and_bias=False):
    """The parameter groups most detection recipes want, from model.named_parameters() (trainable ones only):
      * no weight decay for the BiFPN fusion weights (...stack_bifpn_convs.N.w1 / w2) and, unless decay_norm_and_bias, for every tensor
        with ndim <= 1 (BatchNorm scales and shifts, conv and linear biases); `weight_decay` for everything else;
      * names under 'backbone.' get 'lr_scale': backbone_lr_scale, the others 'lr_scale': 1.0.  The CALLER multiplies it into lr once the
        optimizer exists and before a scheduler reads the groups (`for g in opt.param_groups: g['lr'] *= g['lr_scale']`).
    Every trainable parameter lands in exactly one group; empty groups are omitted; each group carries a 'name'."""
    groups = {}
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        name = name[len('module.'):] if name.startswith('module.') else name
        backbone = name.startswith('backbone.')
        no_decay = bool(_FUSION_WEIGHT.search(name)) or (p.ndim <= 1 and not decay_norm_and_bias)
        key = (backbone and backbone_lr_scale != 1.0, no_decay)
        if key not in groups:
            groups[key] = {'params': [], 'weight_decay': 0.0 if no_decay else float(weight_decay),
                           'lr_scale': float(backbone_lr_scale) if backbone else 1.0,
                           'name': ('backbone_' if key[0] else '') + ('no_decay' if no_decay else 'decay')}
        groups[key]['params'].append(p)
    return [groups[k] for k in sorted(groups)]


class _FusedStep(torch.optim.Optimizer):
    """What ClipAdamW and ClipSGD share: the device tables, the hyper table and its upload, the norm pass, the gates, the average, the
    checkpoint format.  A subclass names its rule (RULE), its moment arenas (MOMENTS: (attribute, state_dict key) pairs) and the row of
    the hyper table a group makes (_row)."""
    RULE = None
    MOMENTS = ()

    def __init__(self, params, defaults, write_clipped_grads=False, accumulate=False, ema_decay=None, ema_warmup=True):
        self._name = type(self).__name__
        if accumulate and write_clipped_grads:
            raise ValueError('%s: write_clipped_grads=True cannot be combined with accumulate=True (the step clips the sum held in '
                             'the accumulation arena; p.grad holds one micro-batch and is not what was clipped)' % self._name)
        self.ema = ema_decay is not None
        if self.ema:                         # (the key exists only with the average on: param_groups of a plain ClipAdamW stay as they were)
            defaults['ema_decay'] = self._checked_decay(ema_decay)
        self.ema_warmup = bool(ema_warmup)
        self._swapped = False                # swap_ema(): the parameters hold the average and the arena the trained weights
        self._table = None
        super().__init__(params, defaults)
        check_unique_params(self._name, self.param_groups)
        self._rows()                         # (refuses groups that disagree on max_norm / ema_decay, and what _row refuses)
        self.write_clipped_grads = bool(write_clipped_grads)
        self.accumulate = bool(accumulate)
        self._grad_mask = None               # accumulate: which tensors had a gradient in the epoch's first micro-step
        self._step = 0
        self._captured = False               # a step() ran under stream capture (its launch sequence is frozen in a hipGraph)

    @classmethod
    def _checked_decay(cls, d):
        """0 <= decay < 1 as the fp32 value the kernel reads (a decay that rounds to 1.0f would freeze the average); NaN is refused."""
        try:
            d = float(d)
        except (TypeError, ValueError):
            raise ValueError('%s: ema_decay must be a number in [0, 1), got %r' % (cls.__name__, d))
        if math.isnan(d) or not (0.0 <= d < 1.0) or not float(np.float32(d)) < 1.0:
            raise ValueError('%s: ema_decay must satisfy 0 <= decay < 1 (as fp32), got %r' % (cls.__name__, d))
        return d

    def add_param_group(self, param_group):
        if getattr(self, '_table', None) is not None:
            raise RuntimeError('%s.add_param_group after the device tables were built: the arenas are laid out over the tensor table; '
                               'add every group before the first step()' % self._name)
        super().add_param_group(param_group)

    def _grouped(self):
        """The hyper TABLE and the grouped entry point, or (one-group ClipAdamW only) the one hyper buffer and the one-group calls."""
        return True

    # ---- the device tables (built once; parameter and moment storage is stable) ----
    def _build(self):
        check_unique_params(self._name, self.param_groups)
        per_group = [[p for p in g['params'] if p.requires_grad] for g in self.param_groups]
        ps = [p for gp in per_group for p in gp]                      # the tensor table: the flattened groups, frozen tensors dropped
        if not ps:
            raise ValueError('no trainable parameters')
        dev = ps[0].device
        for p in ps:
            if p.dtype != torch.float32 or p.device != dev or not p.is_contiguous() or not p.is_cuda:
                raise ValueError('%s needs contiguous fp32 parameters on one GPU' % self._name)
        lay = layout_tables([[p.numel() for p in gp] for gp in per_group], int(L.lib().effdet_opt_chunk()))
        n, numel, offs, nb = len(ps), lay['numel'], lay['offs'], lay['nblocks']
        i64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int64)).to(dev)
        i32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int32)).to(dev)
        for attr, _ in self.MOMENTS:
            setattr(self, attr, torch.zeros(int(offs[-1]), dtype=torch.float32, device=dev))
        arena_ptrs = lambda a: i64([a.data_ptr() + 4 * int(o) for o in offs[:-1]])
        views = lambda a: [a[int(offs[i]):int(offs[i]) + numel[i]].view_as(p) for i, p in enumerate(ps)]
        grouped = self._grouped()
        nh = L.OPT_ROW * len(self.param_groups) if grouped else (7 if self.ema else 6)
        t = {
            'params': ps, 'n': n, 'nblocks': nb, 'grouped': grouped, 'ngroups': len(self.param_groups),
            'p_ptr': i64([p.data_ptr() for p in ps]),
            'm_ptr': arena_ptrs(getattr(self, self.MOMENTS[0][0])),
            'v_ptr': arena_ptrs(getattr(self, self.MOMENTS[1][0])) if len(self.MOMENTS) > 1 else None,
            'numel': i64(numel), 'block_tensor': i32(lay['block_tensor']), 'block_first': i32(lay['block_first']),
            'tensor_group': i32(lay['tensor_group']),
            'g_ptr': torch.zeros(n, dtype=torch.int64, device=dev),
            # pinned staging ring for the gradient-pointer upload: a slot is rewritten only after the event recorded behind
            # its previous H2D copy has completed (the host may run a step ahead of the stream)
            'g_host': [torch.zeros(n, dtype=torch.int64).pin_memory() for _ in range(2)], 'g_evt': [None, None], 'g_slot': 0,
            'g_graph_host': torch.zeros(n, dtype=torch.int64).pin_memory(),      # source of the memcpy node of a captured step

            'g_last': None,
            'scratch': torch.zeros(64 + nb, dtype=torch.float32, device=dev), 'offs': offs,
            'steps': torch.zeros(n, dtype=torch.int32, device=dev), 'p_sig': [p.data_ptr() for p in ps],
            # hyper-parameters live on the device (read by the update kernel at run time): a captured step follows the
            # schedule of param_groups -- sync_hyper() refreshes them ahead of a graph replay.  One group of ClipAdamW: six floats
            # (a seventh carries the EMA decay; the six the kernels without the average read stay where they are); otherwise the
            # table of include/effdet_opt_groups.h, one row of eight per group
            'hyper': torch.zeros(nh, dtype=torch.float32, device=dev),
            'hyper_host': torch.zeros(nh, dtype=torch.float32).pin_memory(),
            'hyper_last': None, 'hyper_evt': None,
        }
        if self.ema:
            # the average (same offsets as the moments; e = p to begin with) and its control block (effdet_ema_ctl_t: the update counter)
            self.ema_avg = torch.zeros(int(offs[-1]), dtype=torch.float32, device=dev)
            t['e_ptr'] = arena_ptrs(self.ema_avg)
            t['ectl'] = torch.zeros(C.sizeof(L.EmaCtl) // 4, dtype=torch.int32, device=dev)
            t['e_views'] = views(self.ema_avg)
            with torch.no_grad():
                for e, p in zip(t['e_views'], ps):
                    e.copy_(p)
            self._swapped = False
        if self.accumulate:
            # the sum over a window's micro-batches (same offsets as the moments; written, not added to, by the first micro-batch of a
            # window, so it is never zeroed) and the control block (effdet_train_ctl_t, 32 bytes; zero = start of an epoch)
            self.grad_acc = torch.zeros(int(offs[-1]), dtype=torch.float32, device=dev)
            t['a_ptr'] = arena_ptrs(self.grad_acc)
            t['ctl'] = torch.zeros(C.sizeof(L.TrainCtl) // 8, dtype=torch.int64, device=dev)
            self._grad_mask = None
        moment_views = [(key, views(getattr(self, attr))) for attr, key in self.MOMENTS]
        for i, p in enumerate(ps):                                     # per-parameter views for state_dict()
            self.state[p] = {'step': torch.tensor(0.0)}                # refreshed from the device counters in state_dict()
            for key, vs in moment_views:
                self.state[p][key] = vs[i]
            if self.ema:
                self.state[p]['ema'] = t['e_views'][i]
        self._table = t

    def moment_arenas(self):
        """The optimizer's flat moment arenas in MOMENTS' order (graph.replay_vs_eager saves and restores whichever there are)."""
        return [getattr(self, attr) for attr, _ in self.MOMENTS]

    # ---- checkpointing (train.py:279-291 saves only the model; resuming needs the moments + per-tensor step counters) ----
    def state_dict(self):
        """torch.optim.AdamW- / torch.optim.SGD-compatible: per-parameter {'step', <the moments>} in torch's grouped param_groups layout;
        'step' is read back from the device-resident counters (they advance on the GPU), the moments are views of the arenas.
        accumulate=True adds nothing: a checkpoint is an epoch boundary, where nothing is pending, so the accumulation arena and the
        control block are not saved."""
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

    def _loaded_step(self, st):
        return int(float(st['step']))

    def load_state_dict(self, state_dict):
        """Loads a state_dict of this class or of its torch.optim twin over the same parameter lists (the same groups): moments are
        copied INTO the arenas and the step counters into the device array (super() alone would leave self.state pointing at fresh
        tensors the kernels never see).  Keys a loaded group lacks (torch's groups have no max_norm) keep this optimizer's values."""
        if self._swapped:
            raise RuntimeError('%s.load_state_dict while the averaged weights are swapped in; call swap_ema() (or leave ema_weights()) first'
                               % self._name)
        before = [{k: v for k, v in g.items() if k != 'params'} for g in self.param_groups]
        super().load_state_dict(state_dict)
        for g, old in zip(self.param_groups, before):                  # (now the loaded groups: the average is on or off by construction)
            for k, v in old.items():
                if k != 'ema_decay':
                    g.setdefault(k, v)
            if not self.ema:
                g.pop('ema_decay', None)
            else:
                g['ema_decay'] = self._checked_decay(old.get('ema_decay') if g.get('ema_decay') is None else g['ema_decay'])
        loaded = {p: dict(st) for p, st in self.state.items()}
        self.state.clear()
        self._build()                                                  # (with the average on: e = the current p, updates = 0)
        t = self._table
        if self.ema:
            have = [i for i, p in enumerate(t['params']) if (loaded.get(p) or {}).get('ema') is not None]
            for i in have:
                p = t['params'][i]
                t['e_views'][i].copy_(loaded[p]['ema'].to(p.device, torch.float32).view_as(p))
            # a state without the average (torch's optimizer, or this class with it off) starts one at the current parameters
            t['ectl'][0] = int(state_dict.get('ema_updates', 0)) if have else 0
        steps = torch.zeros(t['n'], dtype=torch.int32)
        for i, p in enumerate(t['params']):
            st = loaded.get(p)
            if not st:
                continue
            for _, key in self.MOMENTS:
                if st.get(key) is not None:
                    self.state[p][key].copy_(st[key].to(p.device, torch.float32).view_as(p))
            steps[i] = self._loaded_step(st)
        t['steps'].copy_(steps)
        self._step = int(steps.max()) if t['n'] else 0

    def _row(self, g):
        """The group's row of the hyper table without the two shared values: (lr, slot 2, slot 3, slot 4, weight_decay)."""
        raise NotImplementedError

    def _rows(self):
        """One row of eight per group (include/effdet_opt_groups.h); refuses groups that disagree on max_norm or ema_decay."""
        gs = self.param_groups
        max_norm = shared_hyper(self._name, 'max_norm', [float(g['max_norm'] or 0.0) for g in gs])
        decay = shared_hyper(self._name, 'ema_decay', [self._checked_decay(g['ema_decay']) for g in gs]) if self.ema else 0.0
        rows = []
        for g in gs:
            lr, a, b, c, wd = self._row(g)
            rows.append((max_norm, float(lr), float(a), float(b), float(c), float(wd), decay, 0.0))
        return tuple(rows)

    def _hyper_values(self):
        """What sync_hyper uploads: the rows of the hyper table, flattened by sync_hyper (ClipAdamW with one group: the 6- / 7-tuple)."""
        return self._rows()

    @staticmethod
    def _clips(hv):
        return (hv[0][0] if isinstance(hv[0], tuple) else hv[0]) > 0.0

    def sync_hyper(self):
        """Upload every group's {max_norm, lr, betas, eps, weight_decay} (and ema_decay) -- the whole table -- to the device buffer the
        update kernel reads, if anything changed since the last upload.  step() calls it; graph.GraphedTrainStep calls it before every
        replay, so an lr scheduler (train.py:133,269: ReduceLROnPlateau) drives captured steps exactly like eager ones, group by group."""
        if self._table is None:
            return
        t, hv = self._table, self._hyper_values()
        if hv == t['hyper_last']:
            return
        if t['hyper_last'] is not None and self._clips(hv) != self._clips(t['hyper_last']) and self._captured:
            raise RuntimeError('%s: max_norm switched between 0 and > 0 after the step was captured as a hipGraph '
                               '(the norm pass is part of the captured launch sequence); re-capture the step' % self._name)
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('%s: hyper-parameters changed under stream capture; call sync_hyper() before capturing' % self._name)
        if t['hyper_evt'] is not None:
            t['hyper_evt'].synchronize()                               # the copy that last read the pinned buffer has finished
        t['hyper_host'].copy_(torch.tensor(hv, dtype=torch.float32).reshape(-1))
        t['hyper'].copy_(t['hyper_host'], non_blocking=True)
        ev = torch.cuda.Event(); ev.record()
        t['hyper_evt'], t['hyper_last'] = ev, hv

    def _ensure_table(self):
        if self._table is None or self._table['p_sig'] != [p.data_ptr() for p in self._table['params']]:
            if self.accumulate and torch.cuda.is_current_stream_capturing():
                raise RuntimeError(self._name + ': the device tables are not built (or a parameter moved) and the stream is capturing: '
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
                raise RuntimeError(self._name + ': run one eager step (or sync_hyper()) before capturing the step as a hipGraph')
            if self._hyper_values() != t['hyper_last']:
                raise RuntimeError(self._name + ': param_groups changed since the last upload of the device hyper-parameter buffer and '
                                   'the stream is capturing (no upload possible); call sync_hyper() before capturing')
        else:
            self.sync_hyper()

    def _groups_as_built(self):
        if self._table is not None and len(self.param_groups) != self._table['ngroups']:     # (someone edited the list itself)
            raise RuntimeError('%s: %d parameter groups, the device tables were built for %d'
                               % (self._name, len(self.param_groups), self._table['ngroups']))

    def _not_swapped(self, what):
        if self._swapped:
            raise RuntimeError('%s.%s while the averaged weights are swapped in: the step would train the average; call swap_ema() '
                               '(or leave ema_weights()) first' % (self._name, what))

    @torch.no_grad()
    def step(self, closure=None):
        self._groups_as_built()
        self._not_swapped('step')
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        t = self._ensure_table()
        if not self.accumulate:
            self._upload_grad_ptrs(self._grad_ptrs())
        self._step += 1
        self._hyper_ready()
        ops_mod.bump_param_generation()      # parameters are rewritten through raw pointers: Tensor._version does not move
        self._launch(t)
        return loss

    def _launch(self, t):
        """The grouped entry point (include/effdet_opt_groups.h): the rule, the form flags, the tables, the per-tensor group index and
        the hyper table.  With accumulate the gated form: the sum in the arena is the gradient; which tensors have one is what the last
        accumulate_grads() uploaded; nothing moves when the micro-step just run was skipped or nothing is pending (decided on the device)."""
        flags = (L.OPT_GATED if self.accumulate else 0) | (L.OPT_EMA if self.ema else 0)
        Lb = L.require('effdet_opt_step_groups')
        L.check(Lb.effdet_opt_step_groups(self.RULE, flags, L.ptr(t['p_ptr']), L.ptr(t['g_ptr']), L.ptr(t.get('a_ptr')), L.ptr(t['m_ptr']),
                                          L.ptr(t['v_ptr']), L.ptr(t.get('e_ptr')), L.ptr(t['numel']), L.ptr(t['block_tensor']),
                                          L.ptr(t['block_first']), L.ptr(t['tensor_group']), t['n'], t['nblocks'], t['ngroups'],
                                          L.ptr(t['scratch']), L.ptr(t['steps']), L.ptr(t['hyper']), float(t['hyper_last'][0][0]),
                                          int(self.write_clipped_grads), int(self.ema_warmup), L.ptr(t.get('ctl')), L.ptr(t.get('ectl')),
                                          L.stream_ptr()),
                'effdet_opt_step_groups')

    # ---- the reference's loop body around the step (train.py:104-120), accumulate=True only ----
    def _need_accumulate(self, what):
        if not self.accumulate:
            raise RuntimeError('%s.%s needs %s(accumulate=True)' % (self._name, what, self._name))

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
        self._groups_as_built()
        self._not_swapped('accumulate_grads')
        if not (isinstance(loss, torch.Tensor) and loss.is_cuda and loss.dtype == torch.float32 and loss.numel() == 1):
            raise ValueError(self._name + '.accumulate_grads needs the loss as a one-element fp32 GPU tensor (it is read on the device)')
        t = self._ensure_table()
        ptrs = self._grad_ptrs()
        mask = [x != 0 for x in ptrs]
        if self._grad_mask is not None and mask != self._grad_mask:
            changed = [i for i, (a, b) in enumerate(zip(mask, self._grad_mask)) if a != b]
            raise RuntimeError(self._name + '.accumulate_grads: the set of tensors that have a gradient changed between micro-steps '
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
            raise RuntimeError(self._name + '.reset_epoch under stream capture: an epoch boundary is a host event, not part of a captured step')
        if self._table is not None:
            self._table['ctl'].zero_()
        self._grad_mask = None

    def grad_norm(self):
        """Total gradient norm measured by the last step() (device scalar; clipping enabled only)."""
        return self._table['scratch'][0] if self._table is not None else None

    # ---- the parameter average (ema_decay=...) ----
    def _need_ema(self, what):
        if not self.ema:
            raise RuntimeError('%s.%s needs %s(ema_decay=...)' % (self._name, what, self._name))

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
            raise RuntimeError(self._name + '.swap_ema under stream capture: every replay would exchange the weights again; swap outside the graph')
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


class ClipAdamW(_FusedStep):
    """clip_grad_norm_ + torch.optim.AdamW (the module docstring).  One parameter group makes the one-group calls of effdet_hip.h /
    effdet_ema.h with the 6- / 7-float hyper buffer; more groups make the grouped call with the hyper table."""
    RULE = L.OPT_RULE_ADAMW
    MOMENTS = (('exp_avg', 'exp_avg'), ('exp_avg_sq', 'exp_avg_sq'))

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=0.0, write_clipped_grads=False,
                 accumulate=False, ema_decay=None, ema_warmup=True):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_norm=max_norm)
        super().__init__(params, defaults, write_clipped_grads, accumulate, ema_decay, ema_warmup)

    def _grouped(self):
        return self._table['grouped'] if self._table is not None else len(self.param_groups) != 1

    def _row(self, g):
        b1, b2 = g['betas']
        return g['lr'], b1, b2, g['eps'], g['weight_decay']

    def _hyper_values(self):
        if self._grouped():
            return self._rows()
        g = self.param_groups[0]
        b1, b2 = g['betas']
        hv = (float(g['max_norm'] or 0.0), float(g['lr']), float(b1), float(b2), float(g['eps']), float(g['weight_decay']))
        return hv + (self._checked_decay(g['ema_decay']),) if self.ema else hv

    def _launch(self, t):
        if t['grouped']:
            return super()._launch(t)
        g = self.param_groups[0]
        b1, b2 = g['betas']
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
                return
            Lb = L.require('effdet_clip_adamw_step_gated')
            L.check(Lb.effdet_clip_adamw_step_gated(L.ptr(t['p_ptr']), L.ptr(t['g_ptr']), L.ptr(t['a_ptr']), L.ptr(t['m_ptr']), L.ptr(t['v_ptr']),
                                                    L.ptr(t['numel']), L.ptr(t['block_tensor']), L.ptr(t['block_first']), t['n'], t['nblocks'],
                                                    L.ptr(t['scratch']), L.ptr(t['steps']), float(g['max_norm'] or 0.0),
                                                    float(g['lr']), float(b1), float(b2), float(g['eps']),
                                                    float(g['weight_decay']), L.ptr(t['hyper']), L.ptr(t['ctl']), L.stream_ptr()),
                    'effdet_clip_adamw_step_gated')
            return
        if self.ema:
            Lb = L.require('effdet_clip_adamw_step_ema')
            L.check(Lb.effdet_clip_adamw_step_ema(L.ptr(t['p_ptr']), L.ptr(t['g_ptr']), L.ptr(t['m_ptr']), L.ptr(t['v_ptr']), L.ptr(t['e_ptr']),
                                                  L.ptr(t['numel']), L.ptr(t['block_tensor']), L.ptr(t['block_first']), t['n'], t['nblocks'],
                                                  L.ptr(t['scratch']), L.ptr(t['steps']), float(g['max_norm'] or 0.0), float(g['lr']),
                                                  float(b1), float(b2), float(g['eps']), float(g['weight_decay']),
                                                  int(self.write_clipped_grads), float(g['ema_decay']), int(self.ema_warmup),
                                                  L.ptr(t['hyper']), L.ptr(t['ectl']), L.stream_ptr()),
                    'effdet_clip_adamw_step_ema')
            return
        L.check(L.lib().effdet_clip_adamw_step(L.ptr(t['p_ptr']), L.ptr(t['g_ptr']), L.ptr(t['m_ptr']), L.ptr(t['v_ptr']), L.ptr(t['numel']),
                                               L.ptr(t['block_tensor']), L.ptr(t['block_first']), t['n'], t['nblocks'],
                                               L.ptr(t['scratch']), L.ptr(t['steps']), float(g['max_norm'] or 0.0),
                                               float(g['lr']), float(b1), float(b2), float(g['eps']),
                                               float(g['weight_decay']), int(self.write_clipped_grads), L.ptr(t['hyper']), L.stream_ptr()),
                'effdet_clip_adamw_step')


class ClipSGD(_FusedStep):
    """clip_grad_norm_ + torch.optim.SGD (momentum, dampening, nesterov, coupled weight decay; no maximize) as the second rule of the
    fused step: include/effdet_opt_groups.h states the arithmetic.  One moment arena (`momentum_buf`); state_dict() speaks
    torch.optim.SGD's format ('momentum_buffer' per parameter; None for a tensor that has not stepped or whose group has momentum 0)
    plus the per-tensor 'step' the rule's first-step branch needs.  A torch.optim.SGD state has no 'step': a tensor that comes with
    a buffer continues at step 1, one without starts at 0."""
    RULE = L.OPT_RULE_SGD
    MOMENTS = (('momentum_buf', 'momentum_buffer'),)

    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, nesterov=False, weight_decay=0.0, max_norm=0.0, accumulate=False,
                 ema_decay=None, ema_warmup=True):
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, nesterov=nesterov, weight_decay=weight_decay, max_norm=max_norm)
        self._row(defaults)
        super().__init__(params, defaults, False, accumulate, ema_decay, ema_warmup)

    def _row(self, g):
        momentum, dampening, nesterov = float(g['momentum']), float(g['dampening']), bool(g['nesterov'])
        if nesterov and (momentum <= 0.0 or dampening != 0.0):
            raise ValueError('ClipSGD: Nesterov momentum requires a momentum and zero dampening')
        if momentum < 0.0:
            raise ValueError('ClipSGD: invalid momentum value: %r' % momentum)
        # slot 3 is 1 - dampening: the double difference rounded to fp32, the alpha torch hands to its add
        return g['lr'], momentum, float(np.float32(1.0 - dampening)), 1.0 if nesterov else 0.0, g['weight_decay']

    def state_dict(self):
        sd = super().state_dict()
        if self._table is None:
            return sd
        momentum = {id(p): float(g['momentum']) for g in self.param_groups for p in g['params']}
        index, k = {}, 0
        for g in self.param_groups:                                    # super()'s numbering: every parameter of every group, in order
            for p in g['params']:
                index[k] = p; k += 1
        state = {}
        for k, st in sd['state'].items():
            st = dict(st)                                              # (super() hands out self.state's own dicts)
            if float(st['step']) == 0.0 or momentum[id(index[k])] == 0.0:
                st['momentum_buffer'] = None
            state[k] = st
        sd['state'] = state
        return sd

    def _loaded_step(self, st):
        if st.get('step') is not None:
            return int(float(st['step']))
        return 1 if st.get('momentum_buffer') is not None else 0
