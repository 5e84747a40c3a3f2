#!/usr/bin/env python
"""bench.py -- EfficientDet-D0 512px train step (fwd + focal/smooth-L1 loss + bwd + clip + AdamW) on MI355X.

    python bench.py --gpus N --steps K --warmup W [--full]

A plain run sets up, warms up, times the K steps of the headline leg, writes --dump-outputs if asked and prints the result line: nothing
else.  --full adds, after the headline leg, everything else the benchmark measures: the instrumented roofline step and the extra objects
listed below.  The captured step's replay-vs-eager self-check stays in a plain run: it decides whether the timed steps replay the graph,
and it leaves the model one step further on, so the dumped outputs depend on it.

Works by itself for every N: with N > 1 and no WORLD_SIZE in the environment it re-launches itself under
`python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1` (the reference self-spawns too,
train.py:311-326); started by a launcher that already set RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* it uses those.

Prints ONE JSON line on rank 0.  metric = BASELINE.json's "images/sec EfficientDet-D0 512px fwd+bwd";
workload = configs[2] (batch 32 per GPU @ 512x512, synthetic COCO-shape targets, random-init weights,
80 classes, W_bifpn 64 / D_bifpn 2).  Weak scaling: per-GPU batch fixed, value = total images / s.

The HEADLINE (top-level value / dtype / roofline) is `--dtype f32_hf16x3_bwd_bf16x3`: the trunk (EfficientNet + BiFPN) forward, the losses
and every max-pool / IoU decision in exact-fp32 MFMA products; the RetinaHead's forward convs (95 % of the forward FLOPs) in the
fp32-EQUIVALENT f16x3 form -- operands as fp16 hi + scaled fp16 lo (22 significand bits), three fp16 MFMAs per product, fp32 accumulate: per
product ~2^-22, inside the rounding noise of the fp32 accumulation (against a float64 head the outputs sit 0.4-1.1x as far as the exact-fp32
head's, tests/test_gpu_model.py::test_f16x3_head_is_fp32_equivalent_at_model_level; every complete-detection-list golden of the real
reference incl. D4 @1024 holds); only the GRADIENT convolutions run on bf16 hi + lo operand splits (3 bf16 MFMAs per product, ~1e-5 per
product).  Losses / outputs / all parameter-gradient norms are gated at 1e-3 (+ the reference's own measured instability s_k) against the
real reference's goldens on EVERY model family D0..D6 (profiles/r06_parity_errors.txt).  Extra objects in the same line (--full only):
  exact_forward_mode_f32fwd_bf16x3bwd   round 5's headline: the whole forward bit for bit the f32 mode's, bf16x3 gradient convs;
  strict_mode_f32        the SAME step with exact-fp32 products in the backward too;
  fast_mode_bf16x3       bf16x3 products in the forward as well: faster, but NOT parity-qualified -- its box deltas / neck taps measure
                         1.3-1.9e-3 element-relative against the real reference (gated at 2.5e-3) and its deep-family gradient norms 3-5e-3;
  throughput_mode_bf16   bf16 storage + bf16 products: 2.5e-2 gates, NOT a parity mode;
  roofline               dominant MFMA kernel, timed live with HIP events on the launch stream, against the dense peak of ITS arithmetic;
  inference / inference_d4   configs[1] (batch-32 eval forward + decode + on-device NMS, ms/img) and configs[4] (D4 batch 8 @ 1024) in the
                         headline's forward arithmetic (exact fp32), the other modes as named extras;
  cpu_baseline           the oracle = torch-CPU restatement of the reference, bounded sample, thread sweep + configs[0].
The headline leg times exactly --steps steps; every extra-mode leg --extra-steps (default 20).

--dump-outputs DIR writes what the headline's timed step computed in its LAST timed step (before --full's instrumented roofline step):
DIR/cls_loss.npy and DIR/reg_loss.npy (what the step returns) and DIR/parameters.npy (every trainable parameter after the optimizer
update, flattened in named_parameters() order), float32, at most 64 MB in all (a larger output is cut to a fixed, seeded sample of its
elements).  Weights (torch.manual_seed(0)), the synthetic batch and the drop_connect stream are seeded, so the same arguments give the
same inputs on every run: two builds can be compared output for output.

N > 1 (one process per GPU, RCCL): the ranks the launcher started only SUPERVISE -- each runs its share of a leg in a child process, so
a leg that crashes or hangs (a failed hipGraph capture of the DDP step is not recoverable in-process) costs that attempt, not the run:
  attempt 1  the DDP step captured as ONE hipGraph with its bucketed RCCL all-reduces inside, validated before it is timed: one replay
             and one eager DDP step from the same restored state must produce the same parameters, on every rank, and all ranks must
             hold the same parameters afterwards;
  attempt 2  (only if attempt 1 failed anywhere) eager launches under DDP, in fresh processes and a fresh process group.
`config.ddp_graph` records which path produced the number and why.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

ARITH = {'bf16': 'f32', 'f32': 'f32', 'f32_bf16x3': 'bf16x3', 'f32_bwd_bf16x3': 'f32_bwd_bf16x3', 'f32_hf16x3_bwd_bf16x3': 'f32_hf16x3_bwd_bf16x3'}     # --dtype -> EfficientDet(f32_arith=)
BF16_MFMA_PEAK_TFLOPS = 2500.0      # MI355X dense bf16 (MI355X_MICROARCH.md); fp32-input MFMA: 157.3
F32_MFMA_PEAK_TFLOPS = 157.3
TRAIN_GFLOP_PER_IMG = 192.15        # 3*64.089 - 0.113 (conv FLOPs, 2*MAC)
LEG_MARK = 'EFFDET_LEG_RESULT '     # a DDP leg's child (rank 0) hands its result to its supervisor on a stdout line with this prefix

MODE_NOTE = {
    'f32_hf16x3_bwd_bf16x3': 'fp32 storage; forward in exact-fp32 MFMA products except the RetinaHead\'s convs (95 % of the forward FLOPs), which run the '
                             'fp32-EQUIVALENT f16x3 form: operands as fp16 hi + scaled fp16 lo (22 significand bits), hi*hi + lo*hi + hi*lo on '
                             'v_mfma_f32_16x16x32_f16, fp32 accumulate -- per product ~2^-22, inside the rounding noise of the fp32 accumulation (against a '
                             'float64 head the outputs are 1.0-1.2x as far as the exact-fp32 head\'s; gated at 2x in tests/test_gpu_model.py, and every '
                             'complete-detection-list golden of the real reference incl. D4 @1024 holds); BACKWARD as in f32_bwd_bf16x3 -- the parity-qualified headline mode',
    'f32_bwd_bf16x3': 'fp32 storage; FORWARD in exact-fp32 MFMA products (v_mfma_f32_16x16x4_f32): classification / regression / anchors / losses are '
                      'bit for bit the f32 mode\'s, 1e-3 element-relative vs the real reference with the exact mode\'s margin; BACKWARD (data + weight '
                      'gradient convs) in bf16x3 products (hi*hi + hi*lo + lo*hi, fp32 accumulate) on exactly decided masks: all gradient norms within '
                      '1e-3 (+ s_k) of the real reference on every family D0..D6, within 1e-4 of the f32 mode per tensor (tests/test_gpu_model.py) '
                      '-- the parity-qualified headline mode',
    'f32': 'fp32 storage, exact-fp32 MFMA products (v_mfma_f32_16x16x4_f32) in forward AND backward: the strict parity mode (1e-3 element-relative)',
    'f32_bf16x3': 'fp32 storage, bf16x3 MFMA products in forward and backward: class probabilities within 1e-3 element-relative, but box deltas / neck '
                  'taps measure 1.3-1.9e-3 (gated 2.5e-3) and the deep families\' gradient norms 3-5e-3 (gated 1e-2, D3..D6) -- faster, NOT parity-qualified',
    'bf16': 'bf16 storage + bf16 MFMA products: throughput mode, gated at 2.5e-2 of tensor scale (10 % D4) -- NOT a parity mode',
}
EXTRA_KEY = {'f32_hf16x3_bwd_bf16x3': 'parity_mode_f16x3head', 'f32_bwd_bf16x3': 'exact_forward_mode_f32fwd_bf16x3bwd', 'f32_bf16x3': 'fast_mode_bf16x3', 'f32': 'strict_mode_f32', 'bf16': 'throughput_mode_bf16'}
FWD_MODE = {'f32_hf16x3_bwd_bf16x3': 'f32_hf16x3_bwd_bf16x3', 'f32_bwd_bf16x3': 'f32', 'f32': 'f32', 'f32_bf16x3': 'f32_bf16x3', 'bf16': 'bf16'}      # arithmetic of a mode's FORWARD (inference legs)
PATH_NAME = {'graph': 'captured DDP step (one hipGraph with the RCCL all-reduces inside)', 'eager': 'eager launches under DDP'}


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=32, help='images per GPU')
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--network', default='efficientdet-d0')
    ap.add_argument('--dtype', default='f32_hf16x3_bwd_bf16x3', choices=['bf16', 'f32', 'f32_bf16x3', 'f32_bwd_bf16x3', 'f32_hf16x3_bwd_bf16x3'],
                    help='arithmetic mode of the headline leg (default: exact-fp32 trunk + fp32-equivalent f16x3 RetinaHead forward, bf16x3 gradient '
                         'convs -- the fastest mode that meets the 1e-3 parity gates and reproduces every complete-detection-list golden)')
    ap.add_argument('--full', action='store_true',
                    help='after the headline leg, also run the instrumented roofline step, the other arithmetic modes, the inference legs '
                         '(configs[1], configs[4]) and the CPU baseline; the --no-* switches below leave single parts out of a --full run')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--no-inference', action='store_true')
    ap.add_argument('--no-roofline', action='store_true')
    ap.add_argument('--no-graph', action='store_true', help='eager launches instead of replaying the captured hipGraph of the step')
    ap.add_argument('--no-extra-modes', '--no-parity-mode', dest='no_extra_modes', action='store_true',
                    help='skip the legs of the other arithmetic modes')
    ap.add_argument('--no-d4', action='store_true', help='skip configs[4] (D4 batch 8 @ 1024 inference)')
    ap.add_argument('--extra-steps', type=int, default=20, help='timed steps of each extra-mode train leg')
    ap.add_argument('--extra-warmup', type=int, default=3)
    ap.add_argument('--no-ddp-graph', action='store_true',
                    help='N > 1: eager launches under DDP only (skip the attempt that captures the DDP step, RCCL all-reduces included, as ONE hipGraph)')
    ap.add_argument('--ddp-graph', action='store_true', help='(kept for older command lines: the captured DDP step is attempted first by default)')
    ap.add_argument('--ddp-single', action='store_true',
                    help='N = 1 through the N > 1 code path: supervisor + child leg, world_size-1 RCCL process group, ddp.wrap, bucketed all-reduce, '
                         'captured DDP step with its self-check (what a box with one GPU can validate of the multi-GPU path)')
    ap.add_argument('--leg-timeout', type=float, default=240.0, help='N > 1: seconds the child processes of one attempt get before it is abandoned')
    ap.add_argument('--infer-reps', type=int, default=20, help='timed repetitions of every inference leg')
    ap.add_argument('--torch-optim', action='store_true', help='stock clip_grad_norm_ + torch.optim.AdamW(fused) instead of the HIP ClipAdamW')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='write the outputs of the headline leg\'s last timed step to DIR/<name>.npy (float32, <= 64 MB in all)')
    ap.add_argument('--_leg', dest='leg', default=None, choices=['graph', 'eager', 'dry'], help=argparse.SUPPRESS)   # internal: this process IS one rank of a DDP leg
    a = ap.parse_args(argv)
    if a.steps < 1 or a.extra_steps < 1:
        ap.error('--steps and --extra-steps must be >= 1')
    if not a.full:      # a plain run does what the headline line needs and nothing after it
        a.no_roofline = a.no_extra_modes = a.no_inference = a.no_d4 = a.no_cpu_baseline = True
    if a.dump_outputs:
        a.dump_outputs = os.path.abspath(a.dump_outputs)       # (DDP legs run in child processes started with cwd=ROOT)
    return a


DUMP_BUDGET_BYTES = 64 * 1000 * 1000       # files included (an .npy header is < 4 KiB)


def dump_outputs(dirname, outputs, budget=DUMP_BUDGET_BYTES, seed=0):
    """{name: tensor | array} -> dirname/<name>.npy, float32 (float64 stays float64), at most `budget` bytes in all.  Arrays that fit
    their share are written whole; a larger one is cut to a fixed, seeded sample of its flattened elements (sorted indices, the same on
    every run for the same size), each of the cut arrays getting an equal share of what the whole ones leave.  A directory this creates
    gets a '*' .gitignore, like pytest's cache."""
    import numpy as np
    import torch
    arrs = {}
    for k, v in outputs.items():
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu()
            v = (v.double() if v.dtype == torch.float64 else v.float()).numpy()        # (numpy has no bf16)
        v = np.asarray(v)
        arrs[k] = np.ascontiguousarray(v, dtype=np.float64 if v.dtype == np.float64 else np.float32)
    left, todo = budget - 4096 * len(arrs), sorted(arrs, key=lambda k: arrs[k].nbytes)
    if not os.path.isdir(dirname):
        os.makedirs(dirname)
        with open(os.path.join(dirname, '.gitignore'), 'w') as f:     # a dump made inside a checkout stays out of `git status`
            f.write('*\n')
    for i, k in enumerate(todo):
        v, share = arrs[k], left // (len(todo) - i)
        if v.nbytes > share:
            n = share // v.itemsize
            idx = np.sort(np.random.default_rng(seed).choice(v.size, size=n, replace=False))
            v = v.reshape(-1)[idx]
        np.save(os.path.join(dirname, k + '.npy'), v)
        left -= v.nbytes
    return sorted(arrs)


def free_port():
    s = socket.socket(); s.bind(('127.0.0.1', 0)); p = s.getsockname()[1]; s.close()
    return p


# ------------------------------------------------------------------------------------------------ CPU baseline (the oracle: checker code, never shipped)
def cpu_baseline(network, size, seconds_budget=25.0):
    """The oracle (kind 'port': torch-CPU restatement of the reference, pinned on its golden vectors) timed on this host:
    forward + FocalLoss + backward at 512x512, B = 4, over a sweep of intra-op thread counts (an over-subscribed pool is
    SLOWER than a moderate one for these small-batch convs), best reported with its thread count; plus BASELINE configs[0]
    (B=1 forward to (cls, reg, anchors))."""
    import torch
    from oracle import effdet_oracle as O
    nc, B = 80, 4
    ncpu = os.cpu_count() or 1
    sd = O.make_state_dict(network, nc, seed=0)
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items() if v.is_floating_point() and 'running_' not in k
              and not k.startswith(('backbone._conv_head', 'backbone._bn1', 'backbone._fc'))}
    live = dict(sd); live.update(params)
    img, ann = O.synthetic_batch(B, size, seed=1, num_classes=nc)

    def one():
        t0 = time.perf_counter()
        cl, rl = O.train_losses(live, network, nc, img, ann)
        (cl.mean() + rl.mean()).backward()
        dt = time.perf_counter() - t0
        for p in params.values():
            p.grad = None
        return dt
    t_start = time.perf_counter()
    sweep, first = {}, True
    for nt in [t for t in (16, 8, 32, 64) if t <= ncpu] or [ncpu]:
        torch.set_num_threads(nt)
        if first:
            one(); first = False                       # warm-up (allocator, oneDNN primitive cache)
        ts = [one()]
        if time.perf_counter() - t_start < seconds_budget * 0.7:
            ts.append(one())
        sweep[nt] = round(B / min(ts), 3)
        if time.perf_counter() - t_start > seconds_budget:
            break
    best_nt = max(sweep, key=sweep.get)
    torch.set_num_threads(best_nt)
    with torch.no_grad():                               # configs[0]: D0, 1x3x512x512, forward only
        O.forward_raw(sd, network, nc, img[:1])
        f = []
        for _ in range(3):
            t0 = time.perf_counter(); O.forward_raw(sd, network, nc, img[:1]); f.append(time.perf_counter() - t0)
    return {'value': sweep[best_nt], 'unit': 'images/sec', 'cores': best_nt, 'kind': 'port', 'host_cpus': ncpu,
            'threads_sweep_img_per_s': {str(k): v for k, v in sorted(sweep.items())},
            'config0_forward_ms': round(min(f) * 1e3, 1), 'config0_threads': best_nt,
            'sample': 'oracle (torch-CPU fp32 restatement of the reference; /root/reference does not exist on the GPU box, hence kind "port") %s '
                      'B=%d (the batch SURVEY 8d names) %dx%d fwd+loss+bwd on %d intra-op threads of %d host CPUs = the best of the sweep %s '
                      '(best of <=2 reps per count after one warm-up, %.0f-s budget); config0 = B=1 forward, best of 3'
                      % (network, B, size, size, best_nt, ncpu, sorted(sweep), seconds_budget)}


# ------------------------------------------------------------------------------------------------ GPU legs
def build_model(network, dtype, dev, training, f32_arith='f32'):
    import torch
    from efficientdet.pytorch_amd import EfficientDet, EFFICIENTDET
    cfg = EFFICIENTDET[network]
    torch.manual_seed(0)
    m = EfficientDet(num_classes=80, network=network, W_bifpn=cfg['W_bifpn'], D_bifpn=cfg['D_bifpn'], D_class=cfg['D_class'],
                     is_training=training, compute_dtype=dtype, f32_arith=f32_arith).to(dev)
    if training:
        m.train(); m.is_training = True; m.freeze_bn()
    else:
        m.eval(); m.is_training = False
    return m


def kernel_peak(name, dtype_name):
    """Dense MFMA peak of the arithmetic ONE kernel symbol computes in (a mode may mix two: f32_bwd_bf16x3 runs exact-fp32 forward kernels
    and bf16x3 gradient kernels).  bf16x3: every algorithmic MAC costs three bf16 MFMA MACs -> the dense bf16 peak / 3 in algorithmic FLOP/s."""
    if dtype_name == 'bf16':
        return BF16_MFMA_PEAK_TFLOPS
    if 'bf16x3' in name or 'split' in name or 'f16x3' in name:
        return round(BF16_MFMA_PEAK_TFLOPS / 3.0, 1)
    return F32_MFMA_PEAK_TFLOPS


def _kernel_rows(mf, dtype_name):
    rows = {}
    for k, v in mf.items():
        tf, pk = v['flops'] / (v['ms'] * 1e-3) / 1e12, kernel_peak(k, dtype_name)
        rows[k] = {'launches': v['launches'], 'ms': round(v['ms'], 3), 'tflops': round(tf, 2), 'peak': pk, 'frac': round(tf / pk, 4)}
    return rows


def roofline_of(summ, dtype_name, batch, size):
    """Dominant MFMA kernel of one instrumented step (per-launch HIP events on the launch stream) against the dense peak of its arithmetic."""
    hbm = {k: v for k, v in summ.items() if not k.startswith('conv_')}       # byte-counted (HBM-bound) kernels
    mf = {k: v for k, v in summ.items() if k.startswith('conv_')}            # flop-counted MFMA kernels
    name, d = max(mf.items(), key=lambda kv: kv[1]['ms'])
    peak = kernel_peak(name, dtype_name)
    ach = d['flops'] / (d['ms'] * 1e-3) / 1e12
    # HBM bytes per launch and MFMA-pipe utilisation of the dominant kernel: PMC counters cannot be read from inside this
    # process; the values are those measured by separate `rocprofv3 --pmc` passes on this same command and committed
    # under profiles/ (null when no such file / another dtype or shape)
    traffic = util = src = None
    import glob
    for fn in sorted((os.path.basename(f) for f in glob.glob(os.path.join(ROOT, 'profiles', 'r*_pmc*.json'))), reverse=True) + ['r01_hbm_traffic.json']:
        try:
            tj = json.load(open(os.path.join(ROOT, 'profiles', fn)))
            if tj.get('dtype', 'bf16') == dtype_name and batch == 32 and size == 512 and 'infer' not in fn:
                kk = tj['kernels'].get(name, {})
                traffic, util, src = kk.get('hbm_bytes_per_launch'), kk.get('mfma_busy_frac'), 'profiles/' + fn
                break
        except Exception:
            pass
    return {'bound': 'mfma', 'kernel': name, 'achieved': round(ach, 2), 'peak': peak, 'unit': 'TFLOP/s', 'frac': round(ach / peak, 4),
            'traffic': traffic, 'mfma_busy_frac': util,
            # traffic / mfma_busy_frac: NOT observed in this run (PMC counters cannot be read from inside the process) -- copied from the
            # committed rocprofv3 --pmc passes of this same command
            'traffic_source': ('committed profile ' + src + ' (rocprofv3 PMC, per launch)') if src else None,
            # every MFMA launch of the step at the dense peak of ITS arithmetic: the time the step's matrix work alone would take
            'step_floor_ms': round(sum(v['flops'] / (kernel_peak(k, dtype_name) * 1e12) for k, v in mf.items()) * 1e3, 3),
            'launches_per_step': d['launches'], 'avg_launch_ms': round(d['ms'] / d['launches'], 4),
            'flops_per_launch': round(d['flops'] / d['launches'] / 1e9, 3),
            # operands read once + outputs written once, averaged over the symbol's launches: what `traffic` (PMC) is to be compared with
            'algorithmic_bytes_per_launch': round(d.get('bytes', 0.0) / d['launches']),
            'all_kernels': _kernel_rows(mf, dtype_name),
            'hbm_kernels': {k: {'launches': v['launches'], 'ms': round(v['ms'], 3), 'GBps': round(v['flops'] / (v['ms'] * 1e-3) / 1e9, 1)}
                            for k, v in hbm.items()}}


class DdpSelfCheckFailed(RuntimeError):
    pass


def graph_self_check(graphed, dev, world, use_dist=True):
    """A captured step must BE the eager step (N = 1: the plain step; N > 1: the DDP step with its all-reduces): graph.replay_vs_eager
    runs one eager step and one replay from the same restored state (same batch, same Bernoulli masks) and compares the parameters they
    produce.  Gate: the difference within 1e-3 of the step's own update on every rank (a gradient that does not reach the optimizer --
    buckets read half-written, a workspace not reset inside the graph -- moves it by 10-20 % of the update), finite, and after the replay
    every rank holds the same parameters (checksum MIN == MAX over ranks).  Raises DdpSelfCheckFailed; under DDP the supervisor then
    re-runs the leg eagerly, at N = 1 the leg times eager launches."""
    import torch
    import torch.distributed as dist
    from efficientdet.pytorch_amd.graph import replay_vs_eager
    r = replay_vs_eager(graphed)
    ps = graphed.optimizer._table['params']
    cs = torch.cat([p.detach().reshape(-1) for p in ps]).double().sum().reshape(1)
    stat = torch.tensor([r['replay_vs_eager'], 0.0 if r['finite'] else 1.0, r['eager_vs_eager'], r['replay_vs_replay']], device=dev, dtype=torch.float64)
    lo, hi = cs.clone(), cs.clone()
    if use_dist:
        dist.all_reduce(stat, op=dist.ReduceOp.MAX)
        dist.all_reduce(lo, op=dist.ReduceOp.MIN); dist.all_reduce(hi, op=dist.ReduceOp.MAX)
    note = {'replay_vs_eager_rel_to_update': float(stat[0].item()), 'eager_vs_eager': float(stat[2].item()), 'replay_vs_replay': float(stat[3].item()),
            'update_norm_rank0': r['update_norm'], 'losses_replay_rank0': r['losses_replay'], 'losses_eager_rank0': r['losses_eager'],
            'ranks_hold_equal_parameters': bool((lo == hi).item()), 'finite': float(stat[1].item()) == 0.0, 'world': world}
    if not (note['finite'] and note['ranks_hold_equal_parameters'] and note['replay_vs_eager_rel_to_update'] <= 1e-3 and r['update_norm'] > 0.0):
        raise DdpSelfCheckFailed('captured step != eager step: %s' % json.dumps(note))
    return note


def train_leg(a, dtype_name, steps, warmup, rank, world, local, dev, want_roofline, use_ddp=False, ddp_graph=False, dump_dir=None):
    """EXACTLY `steps` timed train steps (after `warmup` untimed ones) in one compute dtype
    -> dict(value img/s, ms_per_step, final_loss, roofline, graphed, host_ms, self_check[, img]).
    dump_dir: rank 0 writes the outputs of the last timed step there (dump_outputs) before the instrumented roofline step."""
    import contextlib
    import torch
    import torch.distributed as dist
    from efficientdet.pytorch_amd import ops, ddp
    from efficientdet.pytorch_amd.optim import ClipAdamW
    from efficientdet.pytorch_amd.synthetic import synthetic_batch      # the package's own generator: the GPU legs are oracle-free
    dtype = torch.bfloat16 if dtype_name == 'bf16' else torch.float32
    model = build_model(a.network, dtype, dev, True, ARITH[dtype_name])
    ddp.freeze_dead_parameters(model)
    # (captured DDP step: the module lives on the stream GraphedTrainStep warms up and captures on; eager DDP: the ambient stream)
    want_graph = (ddp_graph if use_ddp else True) and not a.no_graph and not a.torch_optim
    net = (ddp.wrap_for_capture(model, device_ids=[local]) if want_graph else ddp.wrap(model, device_ids=[local])) if use_ddp else model
    params = [p for p in model.parameters() if p.requires_grad]
    if a.torch_optim:
        opt = torch.optim.AdamW(params, lr=1e-4, fused=True)
    else:   # the same arithmetic (clip_grad_norm_(0.1) + AdamW(lr 1e-4, wd 1e-2)) as three HIP launches
        opt = ClipAdamW(params, lr=1e-4, max_norm=0.1)
    # synthetic data resident in HBM before the timed region (randn images, COCO-shape targets)
    img, ann = synthetic_batch(a.batch, a.size, seed=1 + rank, num_classes=80)
    img, ann = img.to(dev), ann.to(dev)

    def step():
        # -> (loss, (cls_loss, reg_loss)).  Whoever keeps them keeps this step's autograd graph alive, its AccumulateGrad nodes
        # included; warm-up outputs kept across the hipGraph capture below made the captured run segfault -- only the timed loop keeps them.
        opt.zero_grad(set_to_none=True)
        cl, rl = net([img, ann])
        loss = cl.mean() + rl.mean()
        loss.backward()
        if a.torch_optim:
            torch.nn.utils.clip_grad_norm_(params, 0.1)
        opt.step()
        return loss, (cl, rl)

    def sync_all():
        if use_ddp:
            dist.barrier()
        torch.cuda.synchronize()

    cap_stream = getattr(net, '_effdet_capture_stream', None)      # eager steps of a capture-bound DDP module run on ITS stream too

    def on_stream():
        return torch.cuda.stream(cap_stream) if cap_stream is not None else contextlib.nullcontext()
    with on_stream():
        for _ in range(warmup):
            step()
    sync_all()
    graphed, self_check = None, None
    if want_graph:
        # the SAME step (zero_grad, forward, loss, backward, clip + AdamW) captured once as a hipGraph and replayed: one
        # hipGraphLaunch per step instead of ~400 launches through Python; every replay does the full work on the resident
        # batch (fresh drop_connect masks from the device-side step counter, parameters updated in place).  Under DDP the bucketed
        # RCCL all-reduces are captured with the step (11 eager iterations first: DDP rebuilds its buckets after the first one).
        # A capture that fails with collectives in flight is not recoverable in this process: the exception ends this CHILD and the
        # supervisor re-runs the leg eagerly in fresh processes (N = 1, no DDP: fall back to eager launches right here).
        from efficientdet.pytorch_amd.graph import GraphedTrainStep
        try:
            graphed = GraphedTrainStep(net, opt, img, ann, warmup=11 if use_ddp else 2)
            for _ in range(2):
                graphed()
            sync_all()
        except Exception as e:
            if use_ddp:
                raise
            sys.stderr.write('hipGraph capture failed (%s: %s); timing eager launches\n' % (type(e).__name__, e))
            graphed = None
        if graphed is not None and not a.torch_optim:
            # the number below is only worth reporting if a replay IS a step: checked against an eager step from the same state, every leg
            try:
                self_check = graph_self_check(graphed, dev, world, use_dist=use_ddp)
            except DdpSelfCheckFailed as e:
                if use_ddp:
                    raise
                sys.stderr.write('%s; timing eager launches\n' % e)
                graphed, self_check = None, {'failed': str(e)}
    sync_all()
    t0 = time.perf_counter()
    if graphed is not None:
        for _ in range(steps):
            cl_rl = graphed()
        loss = cl_rl[0].mean() + cl_rl[1].mean()
    else:
        with on_stream():
            for _ in range(steps):
                loss, cl_rl = step()
    host_dt = time.perf_counter() - t0          # time the HOST needed to issue the steps (a host-bound regime shows as host ~= wall)
    sync_all()
    dt = time.perf_counter() - t0
    host_ms = [round(host_dt / steps * 1e3, 3)]
    if use_ddp:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
        hm = [torch.zeros(1, device=dev, dtype=torch.float64) for _ in range(world)]
        dist.all_gather(hm, torch.tensor([host_ms[0]], device=dev, dtype=torch.float64))
        host_ms = [round(float(x.item()), 3) for x in hm]
    if dump_dir and rank == 0:
        cl, rl = cl_rl
        dump_outputs(dump_dir, {'cls_loss': cl, 'reg_loss': rl,
                                'parameters': torch.cat([p.detach().reshape(-1).float() for p in params])})
    roof = None
    if want_roofline:
        # live per-launch timing with HIP events on the launch stream (one instrumented step).  EVERY rank runs the step
        # (under DDP its gradient all-reduce is collective); only rank 0 instruments it.
        if rank == 0:
            ops.PROFILE = ops.LaunchProfile()
        with on_stream():
            step()
        torch.cuda.synchronize()
        if rank == 0:
            summ = ops.PROFILE.summary()
            roof = roofline_of(summ, dtype_name, a.batch, a.size)
            # the dominant symbol's launches by shape: its MFMA-bound head shapes apart from the HBM-bound backbone ones
            # step-level roofline: the blended MFMA floor (each kernel's algorithmic FLOPs at the dense peak of its arithmetic) / the timed step
            roof['step_frac'] = round(roof['step_floor_ms'] / (dt / steps * 1e3), 4)
            roof['dominant_by_shape'] = ops.PROFILE.by_shape(roof['kernel'])
            roof['other_mfma_by_shape'] = {k: ops.PROFILE.by_shape(k, top=3) for k, v in summ.items()
                                           if k.startswith('conv_') and k != roof['kernel'] and v['ms'] >= 1.0}
            ops.PROFILE = None
        if use_ddp:
            dist.barrier()
    final = float(loss.item())
    del opt, net, model
    torch.cuda.empty_cache()
    return {'value': a.batch * world * steps / dt, 'ms_per_step': dt / steps * 1e3, 'final_loss': final, 'roofline': roof, 'img': img,
            'graphed': graphed is not None, 'host_ms': host_ms, 'self_check': self_check}


INFER_GFLOP_PER_IMG = {('efficientdet-d0', 512): 64.089, ('efficientdet-d4', 1024): 455.596}     # SURVEY 8(d) forward conv FLOPs (2*MAC)


def inference_roofline(model, img, dtype_name):
    """The dominant MFMA kernel of ONE instrumented eager forward (per-launch HIP events on the launch stream) against the dense
    peak of its arithmetic, like the train legs' roofline; traffic = the committed PMC pass of the inference command when there is one
    (profiles/r*_pmc_infer_<d0|d4>_<dtype>.json)."""
    import torch
    from efficientdet.pytorch_amd import ops
    ops.PROFILE = ops.LaunchProfile()
    try:
        with torch.no_grad():
            model.detect(img)              # forward + decode + NMS + gather, eager, every launch timed
        torch.cuda.synchronize()
        summ = ops.PROFILE.summary()
        mf = {k: v for k, v in summ.items() if k.startswith('conv_')}
        name, d = max(mf.items(), key=lambda kv: kv[1]['ms'])
        peak = kernel_peak(name, dtype_name)
        ach = d['flops'] / (d['ms'] * 1e-3) / 1e12
        traffic = util = src = None
        tag = '_pmc_infer_%s_%s.json' % ('d4' if img.shape[-1] == 1024 else 'd0', dtype_name)
        for fn in sorted(os.listdir(os.path.join(ROOT, 'profiles')), reverse=True):
            if fn.endswith(tag):
                try:
                    kk = json.load(open(os.path.join(ROOT, 'profiles', fn)))['kernels'].get(name, {})
                    traffic, util, src = kk.get('hbm_bytes_per_launch'), kk.get('mfma_busy_frac'), 'profiles/' + fn + ' (rocprofv3 PMC, per launch)'
                    break
                except Exception:
                    pass
        roof = {'bound': 'mfma', 'kernel': name, 'achieved': round(ach, 2), 'peak': peak, 'unit': 'TFLOP/s', 'frac': round(ach / peak, 4),
                'traffic': traffic, 'mfma_busy_frac': util, 'traffic_source': ('committed profile ' + src) if src else None,
                'launches_per_forward': d['launches'], 'avg_launch_ms': round(d['ms'] / d['launches'], 4),
                'flops_per_launch': round(d['flops'] / d['launches'] / 1e9, 3),
                'algorithmic_bytes_per_launch': round(d.get('bytes', 0.0) / d['launches']),
                'dominant_by_shape': ops.PROFILE.by_shape(name, top=3),
                'all_kernels': _kernel_rows(mf, dtype_name),
                'hbm_kernels': {k: {'launches': v['launches'], 'ms': round(v['ms'], 3), 'GBps': round(v['flops'] / (v['ms'] * 1e-3) / 1e9, 1)}
                                for k, v in summ.items() if not k.startswith('conv_')}}
    finally:
        ops.PROFILE = None
    return roof


def inference_leg(network, mode, dev, img, reps=20, graph=True, want_roofline=False):
    """eval forward + decode + per-image NMS (thr 0.01, IoU 0.5) on RANDOM-INIT weights: every anchor passes the threshold = the
    NMS worst case.  mode: a forward arithmetic (f32 | f32_bf16x3 | bf16).
    -> (ms/img end to end, ms/img forward only, kept boxes of image 0, roofline of the forward or None)."""
    import torch
    dtype = torch.bfloat16 if mode == 'bf16' else torch.float32
    model = build_model(network, dtype, dev, False, ARITH[mode])
    B = img.shape[0]
    with torch.no_grad():
        for _ in range(2):
            model.detect(img)
        detect = lambda: model.detect(img)
        if graph:      # the same forward + decode + NMS + gather replayed as ONE hipGraph
            from efficientdet.pytorch_amd.graph import GraphedDetect
            try:
                gd = GraphedDetect(model, img)
                gd(); detect = gd
            except Exception as e:
                sys.stderr.write('hipGraph capture of detect failed (%s: %s); timing eager launches\n' % (type(e).__name__, e))
                graph = False
        torch.cuda.synchronize(); t1 = time.perf_counter()
        for _ in range(reps):
            dets = detect()
        torch.cuda.synchronize(); ti = (time.perf_counter() - t1) / reps
        for _ in range(2):
            model.forward_raw(img)
        torch.cuda.synchronize(); t1 = time.perf_counter()
        for _ in range(reps):
            model.forward_raw(img)
        torch.cuda.synchronize(); tf = (time.perf_counter() - t1) / reps
    kept = int(dets[0][0].numel())
    roof = inference_roofline(model, img, mode) if want_roofline else None
    del model, detect, dets
    torch.cuda.empty_cache()
    return round(ti * 1e3 / B, 4), round(tf * 1e3 / B, 4), kept, roof


def result_line(a, world, leg, cfg, ddp_note=None):
    d0_512 = a.network == 'efficientdet-d0' and a.size == 512
    out = {
        'metric': 'images/sec EfficientDet-D0 512px fwd+bwd', 'value': round(leg['value'], 2), 'unit': 'images/sec', 'n_gpus': world,
        'steps': a.steps, 'warmup': a.warmup, 'ms_per_step': round(leg['ms_per_step'], 3), 'higher_is_better': True, 'scaling': 'weak',
        'vs_baseline': None, 'dtype': a.dtype, 'data': 'synthetic',
        'config': {'workload': 'EfficientDet-D0 train step (fwd + FocalLoss/SmoothL1 + bwd + clip_grad_norm + AdamW), batch %d/GPU @ %dx%d, '
                               'synthetic COCO-shape targets, 80 classes, random-init, W_bifpn=%d D_bifpn=%d, drop_connect 0.2 active'
                               % (a.batch, a.size, a.size, cfg['W_bifpn'], cfg['D_bifpn']),
                   'network': a.network, 'global_batch': a.batch * world, 'image_size': a.size,
                   'parallelism': 'dp%d' % world + (' (world_size-1 RCCL group: ddp.wrap + bucketed all-reduce on the one GPU)' if a.ddp_single else ''),
                   'ddp_graph': ddp_note,
                   'arithmetic': MODE_NOTE[a.dtype],
                   'final_loss': round(leg['final_loss'], 4),
                   'launch': 'hipGraph replay (one graph launch per step)' if leg['graphed'] else 'eager launches',
                   'graph_self_check': leg.get('self_check')},
        'algorithmic_tflops_per_gpu': round(TRAIN_GFLOP_PER_IMG * a.batch / leg['ms_per_step'], 2) if d0_512 else None,
        # host time to ISSUE one step, per rank (wall time per step is ms_per_step): host ~= wall means the launch path, not the GPU, is the bound
        'host_ms_per_step': leg['host_ms'],
    }
    if leg.get('roofline') is not None:
        out['roofline'] = leg['roofline']
    return out


def single_gpu_main(a):
    """N = 1, in one process: the headline leg; with --full also the other arithmetic modes, inference (configs[1], configs[4]) and the
    CPU baseline."""
    import torch
    from efficientdet.pytorch_amd import EFFICIENTDET
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    cfg = EFFICIENTDET[a.network]
    d0_512 = a.network == 'efficientdet-d0' and a.size == 512
    others = [m for m in ('f32_hf16x3_bwd_bf16x3', 'f32_bwd_bf16x3', 'f32', 'f32_bf16x3', 'bf16') if m != a.dtype]
    leg = train_leg(a, a.dtype, a.steps, a.warmup, 0, 1, 0, dev, not a.no_roofline, dump_dir=a.dump_outputs)
    img = leg.pop('img')
    out = result_line(a, 1, leg, cfg)
    if not a.no_extra_modes:
        # the SAME workload in the other arithmetic modes, >= 20 timed steps each, with their own rooflines
        # (exact fp32 against the 157.3 TFLOP/s fp32 MFMA peak, bf16 against 2500, bf16x3 against 2500 / 3 algorithmic)
        for mode in others:
            r = train_leg(a, mode, a.extra_steps, a.extra_warmup, 0, 1, 0, dev, not a.no_roofline)
            r.pop('img')
            out[EXTRA_KEY[mode]] = {'dtype': mode, 'value': round(r['value'], 2), 'unit': 'images/sec', 'ms_per_step': round(r['ms_per_step'], 3),
                                    'steps': a.extra_steps, 'warmup': a.extra_warmup, 'final_loss': round(r['final_loss'], 4),
                                    'algorithmic_tflops_per_gpu': round(TRAIN_GFLOP_PER_IMG * a.batch / r['ms_per_step'], 2) if d0_512 else None,
                                    'launch': 'hipGraph replay' if r['graphed'] else 'eager launches', 'note': MODE_NOTE[mode], 'roofline': r['roofline']}
    if not a.no_inference:
        fm = FWD_MODE[a.dtype]
        fwd_others = [m for m in ('f32', 'f32_bf16x3', 'bf16') if m != fm]
        ti, tf, kept, iroof = inference_leg(a.network, fm, dev, img, reps=a.infer_reps, graph=not a.no_graph, want_roofline=not a.no_roofline)
        gf = INFER_GFLOP_PER_IMG.get((a.network, a.size))
        out['inference'] = {'workload': 'configs[1]: D0 eval batch %d @ %d: forward + decode + per-image NMS (thr 0.01, IoU 0.5)' % (a.batch, a.size),
                            'dtype': fm, 'note': 'the forward arithmetic of the headline mode (%s)' % a.dtype,
                            'ms_per_img': ti, 'forward_only_ms_per_img': tf, 'kept_boxes_img0': kept, 'reps': a.infer_reps,
                            'forward_tflops': round(gf / tf, 2) if gf else None, 'roofline': iroof,
                            'launch': 'eager launches' if a.no_graph else 'forward + decode + NMS + gather as ONE hipGraph replay (end-to-end number; forward_only is eager)'}
        if not a.no_extra_modes:
            for mode in fwd_others:
                ti, tf, kept, _ = inference_leg(a.network, mode, dev, img, reps=a.infer_reps, graph=not a.no_graph)
                out['inference'][EXTRA_KEY[mode]] = {'dtype': mode, 'ms_per_img': ti, 'forward_only_ms_per_img': tf, 'kept_boxes_img0': kept,
                                                     'reps': a.infer_reps}
        del img
        torch.cuda.empty_cache()
        if not a.no_d4:
            from efficientdet.pytorch_amd.synthetic import synthetic_batch
            img4 = synthetic_batch(8, 1024, seed=1, num_classes=80)[0].to(dev)
            ti, tf, kept, iroof = inference_leg('efficientdet-d4', fm, dev, img4, reps=a.infer_reps, graph=not a.no_graph, want_roofline=not a.no_roofline)
            out['inference_d4'] = {'workload': 'configs[4]: D4 eval batch 8 @ 1024: forward + decode + per-image NMS (thr 0.01, IoU 0.5)',
                                   'dtype': fm, 'ms_per_img': ti, 'forward_only_ms_per_img': tf, 'kept_boxes_img0': kept, 'reps': a.infer_reps,
                                   'forward_tflops': round(455.596 / tf, 2), 'roofline': iroof}
            if not a.no_extra_modes:
                for mode in fwd_others:
                    ti, tf, kept, _ = inference_leg('efficientdet-d4', mode, dev, img4, reps=max(a.infer_reps // 2, 2), graph=not a.no_graph)
                    out['inference_d4'][EXTRA_KEY[mode]] = {'dtype': mode, 'ms_per_img': ti, 'forward_only_ms_per_img': tf, 'kept_boxes_img0': kept,
                                                            'reps': max(a.infer_reps // 2, 2)}
    if not a.no_cpu_baseline:
        out['cpu_baseline'] = cpu_baseline(a.network, a.size)
    print(json.dumps(out), flush=True)
    return 0


# ------------------------------------------------------------------------------------------------ N > 1: legs in child processes
def leg_main(a):
    """One rank of ONE DDP leg (child of a supervisor rank, which gives it RANK / LOCAL_RANK / WORLD_SIZE / MASTER_*).
    'graph': captured DDP step + self-check; 'eager': eager launches under DDP; 'dry': process-group plumbing only -- the CPU-tier
    tests of the supervisor's control flow (EFFDET_BENCH_DRYRUN=1; EFFDET_BENCH_FAIL_LEG=<path> makes the last rank of that path die)."""
    rank = int(os.environ['RANK']); world = int(os.environ['WORLD_SIZE']); local = int(os.environ.get('LOCAL_RANK', 0))
    import torch
    import torch.distributed as dist
    if a.leg == 'dry':
        if os.environ.get('EFFDET_BENCH_FAIL_LEG') == os.environ.get('EFFDET_BENCH_DRY_PATH') and rank == world - 1:
            sys.stderr.write('simulated failure of the %s leg on rank %d\n' % (os.environ.get('EFFDET_BENCH_DRY_PATH'), rank))
            return 7
        dist.init_process_group('gloo', init_method='env://')
        t = torch.tensor([float(rank + 1)])
        dist.all_reduce(t)
        ok = float(t.item()) == world * (world + 1) / 2
        if rank == 0:
            print(LEG_MARK + json.dumps({'dry_run': True, 'path': os.environ.get('EFFDET_BENCH_DRY_PATH'), 'world': world, 'allreduce_ok': ok}), flush=True)
        dist.barrier()
        dist.destroy_process_group()
        return 0 if ok else 1
    from efficientdet.pytorch_amd import ddp
    ndev = torch.cuda.device_count()
    backend = os.environ.get('EFFDET_BENCH_BACKEND', 'nccl')                             # 'nccl' IS RCCL on ROCm
    if local >= ndev:      # debug only (EFFDET_BENCH_BACKEND=gloo, or EFFDET_BENCH_SHARE_GPU=1 with RCCL): several ranks sharing one GPU to exercise the N>1 path
        if (backend != 'gloo' and os.environ.get('EFFDET_BENCH_SHARE_GPU') != '1') or ndev == 0:
            sys.stderr.write('rank %d has no GPU of its own (%d visible)\n' % (local, ndev))
            return 2
        local %= ndev
    torch.cuda.set_device(local)
    dev = torch.device('cuda', local)
    ddp.init_process_group_from_env(backend, for_capture=(a.leg == 'graph'))
    try:
        leg = train_leg(a, a.dtype, a.steps, a.warmup, rank, world, local, dev, not a.no_roofline, use_ddp=True,
                        ddp_graph=(a.leg == 'graph' and backend == 'nccl'), dump_dir=a.dump_outputs)
    except DdpSelfCheckFailed as e:
        sys.stderr.write('%s\n' % e)
        sys.stderr.flush()
        os._exit(3)
    leg.pop('img')
    if rank == 0:
        print(LEG_MARK + json.dumps(leg), flush=True)
    dist.barrier()
    torch.cuda.synchronize()
    sys.stdout.flush(); sys.stderr.flush()
    os._exit(0)        # the result is out; skip the teardown (destroying a group whose collectives live in a hipGraph may abort)


def run_attempt(a, path, attempt, rank, world, local, base_port, store, dry):
    """This rank's child of one attempt -> (ok, result dict of the rank-0 child or None, reason it failed or None).
    The children's rendezvous port: rank 0 asks the OS for a free one per attempt and publishes it through the supervisors' store (an
    arithmetic offset from the launcher's port may be taken -- every rank's child would then fail or hang until --leg-timeout); without
    a store (never the case under a launcher) the offset rule remains."""
    port = None
    if store is not None:
        key = 'effdet_port_%d' % attempt
        try:
            if rank == 0:
                store.set(key, str(free_port()))
            store.wait([key])
            port = int(store.get(key))
        except Exception:
            port = None
    if port is None:
        port = base_port + 101 + 13 * attempt
        if port >= 65000:
            port = base_port - 101 - 13 * attempt
    env = {k: v for k, v in os.environ.items() if not k.startswith(('TORCHELASTIC_', 'GROUP_', 'ROLE_', 'LOCAL_WORLD'))}
    env.update(RANK=str(rank), LOCAL_RANK=str(local), WORLD_SIZE=str(world), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port),
               HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY', '0'), EFFDET_BENCH_DRY_PATH=path)
    if path == 'graph':
        env.setdefault('TORCH_NCCL_ASYNC_ERROR_HANDLING', '0')       # torch's recipe for DDP inside a captured graph (the capture leg only)
    argv = [x for x in sys.argv[1:] if x != '--ddp-single'] + (['--dump-outputs', a.dump_outputs] if a.dump_outputs else [])
    cmd = [sys.executable, os.path.abspath(__file__)] + argv + ['--_leg', 'dry' if dry else path]
    t0 = time.time()
    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True, cwd=ROOT)
    bufs = {'out': [], 'err': []}          # reader threads: a child that fills a pipe must not block while this rank polls it and its peers
    readers = [threading.Thread(target=lambda f=proc.stdout, b=bufs['out']: b.append(f.read()), daemon=True),
               threading.Thread(target=lambda f=proc.stderr, b=bufs['err']: b.append(f.read()), daemon=True)]
    for t in readers:
        t.start()
    abort_key, why = 'effdet_abort_%d' % attempt, None
    while proc.poll() is None:
        time.sleep(0.25)
        if time.time() - t0 > a.leg_timeout:
            why = 'timed out after %.0f s' % a.leg_timeout
        elif store is not None:
            try:
                if store.check([abort_key]):
                    why = 'stopped: the child of another rank failed'
            except Exception:
                pass
        if why:
            try:
                os.killpg(proc.pid, 9)      # (its own session: the pid is the process-group id -- exactly the processes this rank started)
            except Exception:
                proc.kill()
            proc.wait()
    for t in readers:
        t.join(timeout=5)
    so, se = ''.join(bufs['out']), ''.join(bufs['err'])
    ok, result = why is None and proc.returncode == 0, None
    if ok and rank == 0:
        lines = [l for l in so.splitlines() if l.startswith(LEG_MARK)]
        if lines:
            result = json.loads(lines[-1][len(LEG_MARK):])
        else:
            ok, why = False, 'no result line from the rank-0 child'
    if not ok:
        why = why or 'child exit code %s%s' % (proc.returncode, ' (self-check: captured step != eager step)' if proc.returncode == 3 else '')
        if store is not None and not why.startswith('stopped'):
            try:
                store.set(abort_key, '1')           # peers stop waiting for a collective that will never complete
            except Exception:
                pass
        tail = [l for l in se.strip().splitlines() if l.strip()][-8:]
        sys.stderr.write('[bench rank %d] attempt %d (%s) failed: %s\n%s\n' % (rank, attempt + 1, PATH_NAME[path], why, '\n'.join('    ' + l for l in tail)))
    elif rank == 0 and os.environ.get('EFFDET_BENCH_VERBOSE'):
        sys.stderr.write(se[-3000:])
    return ok, result, why


class Agreement:
    """What the supervising ranks need from each other -- a verdict per attempt (MIN over ranks), an abort key, a final barrier -- on the
    launcher's own key-value store (env:// rendezvous: under torch.distributed.run the agent hosts it, started by hand rank 0 does).  No
    process group: nothing of a collective library prints to stdout next to the ONE JSON line, and there is no communicator to tear down."""

    def __init__(self, rank, world, timeout_s):
        import datetime
        from torch.distributed import rendezvous
        self.store, _, _ = next(rendezvous('env://', rank=rank, world_size=world))
        self.store.set_timeout(datetime.timedelta(seconds=timeout_s))
        self.rank, self.world = rank, world

    def gather(self, tag, value):
        """-> the values every rank gave for `tag` (blocks until all have)."""
        self.store.set('effdet_%s_%d' % (tag, self.rank), str(int(value)))
        keys = ['effdet_%s_%d' % (tag, r) for r in range(self.world)]
        self.store.wait(keys)
        return [int(self.store.get(k)) for k in keys]


def supervisor_main(a, rank, world, local):
    """A rank as the launcher started it: never touches the GPU.  Runs its share of each attempt in a child process, agrees with the
    other supervisors (over the launcher's store) on whether the attempt worked EVERYWHERE, and moves on to the next path if it did not."""
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', str(free_port()))
    base_port = int(os.environ['MASTER_PORT'])
    ag = Agreement(rank, world, a.leg_timeout + 180.0)
    store = ag.store
    dry = os.environ.get('EFFDET_BENCH_DRYRUN') == '1'
    backend = os.environ.get('EFFDET_BENCH_BACKEND', 'nccl')
    eager_only = a.no_ddp_graph or a.no_graph or a.torch_optim or (backend != 'nccl' and not dry)
    plan = ['eager'] if eager_only else ['graph', 'eager']
    history, result = [], None
    for attempt, path in enumerate(plan):
        t0 = time.time()
        ok, mine, why = run_attempt(a, path, attempt, rank, world, local, base_port, store, dry)
        all_ok = min(ag.gather('ok%d' % attempt, 1 if ok else 0)) == 1       # every rank agrees on the verdict of the attempt
        history.append({'attempt': attempt + 1, 'path': PATH_NAME[path], 'ok_on_every_rank': all_ok, 'rank0_note': why,
                        'seconds': round(time.time() - t0, 1)})
        if all_ok:
            result = mine
            break
    rc = 0
    if rank == 0:
        if result is None:
            sys.stderr.write('[bench] every attempt failed: %s\n' % json.dumps(history))
            rc = 1
        elif result.get('dry_run'):
            print(json.dumps({'dry_run': True, 'n_gpus': world, 'value': None, 'path': result.get('path'), 'attempts': history}), flush=True)
        else:
            from efficientdet.pytorch_amd.config import EFFICIENTDET
            note = {'captured': bool(result['graphed']), 'attempts': history, 'self_check': result.get('self_check'),
                    'supervised': 'each rank ran its leg in a child process; a failed attempt is re-run on the next path in fresh processes'}
            print(json.dumps(result_line(a, world, result, EFFICIENTDET[a.network], note)), flush=True)
    return max(ag.gather('done', rc))                             # (also the final barrier: nobody leaves before rank 0 has printed)


def self_launch(a):
    """`python bench.py --gpus N` (N > 1) started by hand: become the launcher (one process per GPU; train.py:311-326 self-spawns too)."""
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(a.gpus), '--master-addr', '127.0.0.1',
           '--master-port', str(free_port()), os.path.abspath(__file__)] + sys.argv[1:] + (['--dump-outputs', a.dump_outputs] if a.dump_outputs else [])
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY', '0'))
    return subprocess.call(cmd, env=env, cwd=ROOT)


def main():
    a = parse()
    if a.leg:
        return leg_main(a)
    if a.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        return self_launch(a)
    rank = int(os.environ.get('RANK', 0)); world = int(os.environ.get('WORLD_SIZE', 1)); local = int(os.environ.get('LOCAL_RANK', 0))
    if world != a.gpus:
        sys.stderr.write('bench.py --gpus %d was started with WORLD_SIZE=%d: launch one process per GPU, or run plain `python bench.py --gpus %d` '
                         '(it launches them itself)\n' % (a.gpus, world, a.gpus))
        return 2
    if world == 1 and not a.ddp_single:
        return single_gpu_main(a)
    return supervisor_main(a, rank, world, local)


if __name__ == '__main__':
    sys.exit(main())
