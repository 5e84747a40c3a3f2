"""The launch sequence of the RetinaHead, pinned (functional.head_fwd / head_bwd).

The equality tests of the head's switches compare its paths with each other; this one compares every path with a recording.  One step of
D0, 8 classes, B = 2 @512 (the smallest standard pyramid the split-layout head takes) runs under ops.LaunchProfile, and the (kernel symbol,
shape note) pairs recorded inside head_fwd and inside head_bwd must be those of tests/golden/head_launch_sequence.json, in order:
which kernel every launch of the head is, how many maps it covers and where in the sequence it leaves.

The fixture is this module's own recording (`python -m tests.test_gpu_head_launch_sequence [FILE]` writes it): a change that moves, merges
or replans a head launch has to regenerate it and say so; one that only restates the code must leave it as it is."""
import json
import os
import sys

import pytest
import torch

from oracle import effdet_oracle as O

pytestmark = pytest.mark.gpu

HEADLINE = 'f32_hf16x3_bwd_bf16x3'
NET, NC, B, S = 'efficientdet-d0', 8, 2, 512
# run -> (f32_arith, compute dtype, head switches of functional.py to turn off, training step?)
RUNS = {
    'f32': ('f32', torch.float32, (), True),
    'bf16x3': ('bf16x3', torch.float32, (), True),
    'f32_bwd_bf16x3': ('f32_bwd_bf16x3', torch.float32, (), True),
    HEADLINE: (HEADLINE, torch.float32, (), True),
    'bf16': ('f32', torch.bfloat16, (), True),
    'pair_towers_off': (HEADLINE, torch.float32, ('HEAD_PAIR_TOWERS',), True),
    'pair_wgrad_off': (HEADLINE, torch.float32, ('HEAD_PAIR_WGRAD',), True),
    'sparse_reg_off': (HEADLINE, torch.float32, ('HEAD_SPARSE_REG', 'HEAD_SPARSE_REG_FWD'), True),
    'inference': (HEADLINE, torch.float32, (), False),
}
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'head_launch_sequence.json')
_INPUTS = {}


def _inputs():
    if not _INPUTS:
        _INPUTS['sd'] = O.make_state_dict(NET, NC, seed=3)
        _INPUTS['img'], _INPUTS['ann'] = (t.cuda() for t in O.synthetic_batch(B, S, seed=2, num_classes=NC))
    return _INPUTS['sd'], _INPUTS['img'], _INPUTS['ann']


def collect(run):
    """One step of RUNS[run] under a LaunchProfile -> {'head_fwd': [[symbol, note], ...], 'head_bwd': [...]}: the launches recorded
    between entry and exit of functional.head_fwd / head_bwd (an inference run has no backward: an empty list)."""
    from efficientdet.pytorch_amd import EfficientDet, EFFICIENTDET, ops, functional as Fn
    arith, dtype, off, train = RUNS[run]
    sd, img, ann = _inputs()
    c = EFFICIENTDET[NET]
    m = EfficientDet(NC, network=NET, W_bifpn=c['W_bifpn'], D_bifpn=c['D_bifpn'], D_class=c['D_class'], compute_dtype=dtype, f32_arith=arith,
                     is_training=train)
    m.load_state_dict(sd); m.backbone.drop_connect_rate = 0.0
    m = m.cuda()
    spans = {'head_fwd': [], 'head_bwd': []}
    old = {k: getattr(Fn, k) for k in off + ('head_fwd', 'head_bwd')}
    old_profile, old_arith = ops.PROFILE, (ops.F32_ARITH, ops.F32_ARITH_BWD, ops.F32_ARITH_HEAD)

    def noting(name):
        def call(*a, **kw):
            n0 = len(ops.PROFILE.records)
            try:
                return old[name](*a, **kw)
            finally:
                spans[name].append((n0, len(ops.PROFILE.records)))
        return call
    try:
        ops.PROFILE = ops.LaunchProfile()
        for k in off:
            setattr(Fn, k, False)
        Fn.head_fwd, Fn.head_bwd = noting('head_fwd'), noting('head_bwd')
        if train:
            m.train(); m.is_training = True; m.freeze_bn()
            cl, rl = m([img, ann])
            (cl.mean() + rl.mean()).backward()
        else:
            m.eval(); m.is_training = False
            with torch.no_grad():
                m.forward_raw(img)
        torch.cuda.synchronize()
        records = ops.PROFILE.records
    finally:
        for k, v in old.items():
            setattr(Fn, k, v)
        ops.PROFILE = old_profile
        ops.F32_ARITH, ops.F32_ARITH_BWD, ops.F32_ARITH_HEAD = old_arith
    assert len(spans['head_fwd']) == 1 and len(spans['head_bwd']) == (1 if train else 0), spans
    return {name: [[r[0], r[4]] for a, b in sp for r in records[a:b]] for name, sp in spans.items()}


@pytest.fixture(scope='module')
def expected():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_fixture_covers_every_run(expected):
    assert sorted(expected) == sorted(RUNS)
    for run, (_, _, _, train) in RUNS.items():
        assert len(expected[run]['head_fwd']) >= 6 and bool(expected[run]['head_bwd']) == train, run


@pytest.mark.parametrize('run', list(RUNS))
def test_head_launches_leave_in_the_recorded_order(expected, run):
    got = collect(run)
    for part in ('head_fwd', 'head_bwd'):
        want = expected[run][part]
        assert len(got[part]) == len(want), (run, part, len(got[part]), len(want))
        diff = [(i, g, w) for i, (g, w) in enumerate(zip(got[part], want)) if g != w]
        assert not diff, (run, part, diff[:4])


if __name__ == '__main__':
    out = {run: collect(run) for run in RUNS}
    for run, parts in out.items():
        print(run, {k: len(v) for k, v in parts.items()})
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    with open(path, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', path)
