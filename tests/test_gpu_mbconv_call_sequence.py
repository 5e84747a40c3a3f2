"""The call sequence of the sixteen MBConv blocks, pinned (functional.mbconv_fwd / mbconv_bwd).

The equality tests of the MBConv switches compare the block's paths with each other; this one compares every path with a recording.  One
step of D0, 8 classes, B = 4 @512, drop_connect active (tests/mbconv_path_cases.py: why this shape, and the runs) is taken with every
function of ops that the two functions reach replaced by a recorder, and what each block called -- [name, rendered arguments, returned
None?], in order -- must be what tests/golden/mbconv_call_sequence.json holds.  Calls are recorded, not ops.PROFILE entries: the
elementwise launches (channel_scale, the squeeze-excite ops, act_bwd, the unpacks) do not pass through the launch profile.  Arguments are
rendered without addresses: a Map as BxHxWxC:dtype, a tensor as its shape and dtype, None as null, numbers, bools and strings as
themselves, keyword arguments by name.  Host-only planner queries (ops.conv2d_gated_ok, ...) are not recorded and may move.

The fixture is this module's own recording (`python -m tests.test_gpu_mbconv_call_sequence [FILE]` writes it): a change that moves, adds,
drops or re-parameterises a call of a block has to regenerate it and say so; one that only restates the code must leave it as it is."""
import json
import sys

import pytest
import torch

from tests.mbconv_path_cases import B, FIXTURE, HEADLINE, NBLOCKS, NC, NET, OPS, RUNS, S, load_fixture, pack_fixture

pytestmark = pytest.mark.gpu

_INPUTS, _MODELS = {}, {}


def _inputs():
    from oracle import effdet_oracle as O
    if not _INPUTS:
        _INPUTS['sd'] = O.make_state_dict(NET, NC, seed=3)
        _INPUTS['img'], _INPUTS['ann'] = (t.cuda() for t in O.synthetic_batch(B, S, seed=2, num_classes=NC))
    return _INPUTS['sd'], _INPUTS['img'], _INPUTS['ann']


def _model(arith, storage, train):
    from efficientdet.pytorch_amd import EfficientDet, EFFICIENTDET
    key = (arith, storage, train)
    if key not in _MODELS:
        c = EFFICIENTDET[NET]
        m = EfficientDet(NC, network=NET, W_bifpn=c['W_bifpn'], D_bifpn=c['D_bifpn'], D_class=c['D_class'],
                         compute_dtype=torch.bfloat16 if storage == 'bf16' else torch.float32, f32_arith=arith, is_training=train)
        m.load_state_dict(_inputs()[0])
        m.backbone.drop_connect_rate = 0.2
        m.backbone.drop_masks = {i: (torch.rand(B, generator=torch.Generator().manual_seed(100 + i)) > 0.3).float() for i in range(NBLOCKS)}
        _MODELS[key] = m.cuda()
    return _MODELS[key]


def render(v):
    from efficientdet.pytorch_amd.ops import Map
    if isinstance(v, Map):
        return '%dx%dx%dx%d:%s' % (v.B, v.H, v.W, v.C, str(v.dtype).replace('torch.', ''))
    if isinstance(v, torch.Tensor):
        return '%s:%s' % (list(v.shape), str(v.dtype).replace('torch.', ''))
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if isinstance(v, torch.dtype):
        return str(v).replace('torch.', '')
    if isinstance(v, (list, tuple)):
        return [render(e) for e in v]
    raise TypeError('an argument the recording cannot render: %r' % (type(v),))


def collect(run):
    """One step of RUNS[run] -> [{'fwd': [[name, [positional ..., {keyword: value}], returned None?], ...], 'bwd': [...]} per block]: the
    calls into ops made between entry and exit of functional.mbconv_fwd / mbconv_bwd (what a recorded function calls itself is its own
    business).  The backward runs the blocks last to first; an inference run has no backward: empty lists."""
    from efficientdet.pytorch_amd import ops, functional as Fn, efficientdet as E
    r = RUNS[run]
    _, img, ann = _inputs()
    m = _model(r['arith'], r['storage'], r['train'])
    where = lambda k: E if k == 'STEM_LINK' else Fn
    touched = sorted(set(r['before']) | set(r['between']))
    old_sw = {k: getattr(where(k), k) for k in touched}
    old_fn = {k: getattr(Fn, k) for k in ('mbconv_fwd', 'mbconv_bwd')}
    old_ops = {k: getattr(ops, k) for k in OPS}
    old_arith, old_prep = (ops.F32_ARITH, ops.F32_ARITH_BWD, ops.F32_ARITH_HEAD), ops.get_prep()
    spans = {'mbconv_fwd': [], 'mbconv_bwd': []}
    state = {'into': None, 'depth': 0}

    def span(name):
        def call(*a, **kw):
            assert state['into'] is None
            state['into'] = []
            try:
                return old_fn[name](*a, **kw)
            finally:
                spans[name].append(state['into']); state['into'] = None
        return call

    def recorder(name):
        def call(*a, **kw):
            top = state['into'] is not None and state['depth'] == 0
            state['depth'] += 1
            try:
                out = old_ops[name](*a, **kw)
            finally:
                state['depth'] -= 1
            if top:
                state['into'].append([name, [render(v) for v in a] + [{k: render(kw[k]) for k in sorted(kw)}], out is None])
            return out
        return call
    try:
        for k, v in r['before'].items():
            setattr(where(k), k, v)
        Fn.mbconv_fwd, Fn.mbconv_bwd = span('mbconv_fwd'), span('mbconv_bwd')
        for k in OPS:
            setattr(ops, k, recorder(k))
        if r['train']:
            m.train(); m.is_training = True; m.freeze_bn()
            m.zero_grad(set_to_none=True)
            cl, rl = m([img, ann])
            for k, v in r['between'].items():
                setattr(where(k), k, v)
            (cl.mean() + rl.mean()).backward()
        else:
            m.eval(); m.is_training = False
            with torch.no_grad():
                m.forward_raw(img)
        torch.cuda.synchronize()
    finally:
        for k, v in old_ops.items():
            setattr(ops, k, v)
        for k, v in old_fn.items():
            setattr(Fn, k, v)
        for k, v in old_sw.items():
            setattr(where(k), k, v)
        ops.set_prep(old_prep)
        ops.F32_ARITH, ops.F32_ARITH_BWD, ops.F32_ARITH_HEAD = old_arith
    assert len(spans['mbconv_fwd']) == NBLOCKS and len(spans['mbconv_bwd']) == (NBLOCKS if r['train'] else 0), {k: len(v) for k, v in spans.items()}
    bwd = spans['mbconv_bwd'][::-1] if r['train'] else [[]] * NBLOCKS
    return json.loads(json.dumps([{'fwd': f, 'bwd': b} for f, b in zip(spans['mbconv_fwd'], bwd)]))


@pytest.fixture(scope='module')
def expected():
    return load_fixture()


def _calls(blocks, part, name):
    return [e for blk in blocks for e in blk[part] if e[0] == name]


def test_the_fixture_covers_every_run_and_every_path(expected):
    """Every run is there with its 16 blocks, and the default headline run holds what the pin is for: both operand-gated launches, each of
    the three fused backward kernels both serving and refusing, and a channel_scale pass; the inference run holds the fused expand."""
    assert sorted(expected) == sorted(RUNS)
    for run, r in RUNS.items():
        assert len(expected[run]) == NBLOCKS, run
        assert all(blk['fwd'] and bool(blk['bwd']) == r['train'] for blk in expected[run]), run
    head = expected[HEADLINE]
    assert any(e[1][-1].get('a_gate') is not None for e in _calls(head, 'fwd', 'conv2d'))
    assert any(e[1][-1].get('a_gate') is not None for e in _calls(head, 'bwd', 'conv2d_wgrad'))
    for name in ('pw_bwd', 'pw_dgrad_se', 'dwconv_bwd'):
        served = [e[2] for e in _calls(head, 'bwd', name)]
        assert True in served and False in served, (name, served)
    assert _calls(head, 'fwd', 'channel_scale')
    assert _calls(expected['inference'], 'fwd', 'expand_dw_fwd')


@pytest.mark.parametrize('run', list(RUNS))
def test_mbconv_calls_are_the_recorded_ones(expected, run):
    got = collect(run)
    for i, (g, w) in enumerate(zip(got, expected[run])):
        for part in ('fwd', 'bwd'):
            assert [e[0] for e in g[part]] == [e[0] for e in w[part]], (run, i, part)
            diff = [(j, a, b) for j, (a, b) in enumerate(zip(g[part], w[part])) if a != b]
            assert not diff, (run, i, part, diff[:3])


if __name__ == '__main__':
    out = {run: collect(run) for run in RUNS}
    for run, blocks in out.items():
        print(run, [(len(b['fwd']), len(b['bwd'])) for b in blocks])
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    with open(path, 'w') as f:
        json.dump(pack_fixture(out), f, separators=(',', ':'), sort_keys=True)
        f.write('\n')
    print('wrote', path)
