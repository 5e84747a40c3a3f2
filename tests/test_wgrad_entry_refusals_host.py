"""CPU tier: the return codes with which the weight-gradient entry points (effdet_conv2d_wgrad, _gated, _gated_kernel, _live, _pair)
refuse a call before anything is enqueued, and which refusal wins where several apply.  The pointers are fake and never dereferenced:
every row is refused before the first HIP call.  The expected codes are those of the library before the plan carried its launchers
(recorded there; this file passed against it unchanged).

No row has a split-layout plan whose mchunk is no multiple of 32: the planner cuts the bf16 view of a split-layout level into ranges of
whole 64-pixel K-steps, so neither tests/wgrad_plan_cases.py nor any other descriptor reaches that EINVAL of _live / _pair; the test
holds the case table to that."""
import ctypes as C

EINVAL, EUNSUPPORTED = -1, -3
WS, GATE, LIVE, BIG = 0x70000000, 0x60000000, 0x68000000, 1 << 40


def test_refusal_table_of_the_wgrad_entry_points():
    from efficientdet.pytorch_amd import build, _lib
    from tests.host_util import wgrad_desc
    from tests import wgrad_plan_cases as P
    build.build(verbose=False)
    L = _lib.require('effdet_conv2d_wgrad', 'effdet_conv2d_wgrad_gated', 'effdet_conv2d_wgrad_gated_kernel', 'effdet_conv2d_wgrad_live',
                     'effdet_conv2d_wgrad_pair', 'effdet_conv2d_wgrad_plan_info', 'effdet_conv2d_wgrad_workspace_bytes')
    ref = lambda d: C.byref(d) if d is not None else None
    NONE, RELU, SWISH = _lib.ACT_NONE, _lib.ACT_RELU, _lib.ACT_SWISH

    def plan(d):
        info = _lib.WgradPlanInfo()
        rc = int(L.effdet_conv2d_wgrad_plan_info(ref(d), C.byref(info)))
        return rc, info

    def without(d, field):
        setattr(d, field, None)
        return d

    # the descriptors, each held against the plan it is meant to have
    pw = lambda dt=_lib.F32, cin=144, cout=24, sizes=((16, 16),), img=1, **kw: wgrad_desc(dt, 2, cin, cout, list(sizes), image_splits=img, **kw)
    pyr = lambda dt=_lib.F32_SPLIT, B=3, cin=256, cout=256: wgrad_desc(dt, B, cin, cout, [(16, 16), (8, 8), (4, 4)], k=3, pad=1)
    tiled, x3, bf16, k3, no_img = pw(), pw(_lib.F32_BF16X3), pw(_lib.BF16), pw(k=3, pad=1), pw(img=0)
    two, two_img = pw(sizes=((16, 16), (8, 8)), img=0), pw(sizes=((16, 16), (8, 8)))
    remainder = pw(cout=22)                                        # dz rows too narrow for the DMA-staged kernel's 4-channel pieces
    thin = pw(cin=32, cout=16, sizes=((128, 128),))
    stem = pw(cin=4, cout=32, sizes=((256, 256),), k=3, stride=2, pad=1)
    split = pyr()
    refused = pw(cin=6)                                            # the planner's own refusal: no whole 4-channel pieces
    for d, path in ((tiled, 0), (x3, 0), (bf16, 0), (k3, 0), (no_img, 0), (two, 0), (remainder, 0), (thin, 1), (stem, 3), (split, 2)):
        assert plan(d)[0] == path, (path, plan(d)[0])
    assert plan(refused)[0] == EUNSUPPORTED and plan(two_img)[0] == EUNSUPPORTED
    assert plan(tiled)[1].nfast == plan(tiled)[1].splits and plan(remainder)[1].nfast == 0 < plan(remainder)[1].splits
    need = lambda d: int(L.effdet_conv2d_wgrad_workspace_bytes(ref(d)))
    assert min(need(d) for d in (tiled, thin, stem, split)) > 0
    for c in P.CASES:                                              # (see the module docstring)
        assert c.kind != 'split' or P.plan(c)['mchunk'] % 32 == 0, c.name

    wgrad = lambda d, ws=WS, n=BIG: L.effdet_conv2d_wgrad(ref(d), ws, n, None)
    gated = lambda d, g=GATE, act=NONE, ws=WS, n=BIG: L.effdet_conv2d_wgrad_gated(ref(d), g, act, ws, n, None)
    gkern = lambda d, g=GATE, act=NONE: L.effdet_conv2d_wgrad_gated_kernel(ref(d), g, act)
    live = lambda d, fl=LIVE, ws=WS, n=BIG: L.effdet_conv2d_wgrad_live(ref(d), ws, n, fl, None)
    pair = lambda a, b, fl=None, ws=WS, n=BIG: L.effdet_conv2d_wgrad_pair(ref(a), ref(b), ws, n, fl, None)
    got = {}

    def row(what, rc, want):
        assert what not in got, what
        got[what] = (int(rc), want)

    # ---- null handling: EINVAL, whatever else is wrong with the call
    row('null wgrad', wgrad(None), EINVAL)
    row('null gated', gated(None), EINVAL)
    row('null gated_kernel', gkern(None), EINVAL)
    row('null live', live(None), EINVAL)
    row('null pair a', pair(None, split), EINVAL)
    row('null pair b', pair(split, None), EINVAL)
    for f in ('x', 'dz'):
        row('no %s wgrad' % f, wgrad(without(pw(), f)), EINVAL)
        row('no %s gated' % f, gated(without(pw(), f)), EINVAL)
        row('no %s live' % f, live(without(pyr(), f)), EINVAL)
        row('no %s pair a' % f, pair(without(pyr(), f), split), EINVAL)
        row('no %s pair b' % f, pair(split, without(pyr(), f), LIVE), EINVAL)
    row('no workspace wgrad', wgrad(tiled, None), EINVAL)
    row('no workspace gated', gated(tiled, ws=None), EINVAL)
    row('no workspace live', live(split, ws=None), EINVAL)
    row('no workspace pair', pair(split, split, ws=None), EINVAL)
    row('null gate gated', gated(tiled, None), EINVAL)
    row('null gate gated swish', gated(thin, None, SWISH), EINVAL)
    row('null gate gated_kernel', gkern(tiled, None), EINVAL)
    row('null flags live', live(split, None), EINVAL)
    row('null flags live, tiled plan', live(tiled, None), EINVAL)

    # ---- which refusal wins
    # the call's own arguments before the planner ...
    row('refused wgrad, no workspace', wgrad(refused, None), EINVAL)
    row('refused gated, no workspace', gated(refused, ws=None), EINVAL)
    row('refused gated, null gate', gated(refused, None), EINVAL)
    row('refused gated_kernel, null gate', gkern(refused, None), EINVAL)
    row('refused live, no workspace', live(refused, ws=None), EINVAL)
    row('refused live, null flags', live(refused, None), EINVAL)
    row('refused pair, no workspace', pair(refused, refused, ws=None), EINVAL)
    # ... the gate's activation code before the descriptor ...
    row('refused gated relu', gated(refused, act=RELU), EINVAL)
    row('refused gated_kernel relu', gkern(refused, act=RELU), EINVAL)
    # ... then the planner's code, with everything else valid ...
    row('refused wgrad', wgrad(refused), EUNSUPPORTED)
    row('refused gated', gated(refused), EUNSUPPORTED)
    row('refused gated_kernel', gkern(refused), EUNSUPPORTED)
    row('refused live', live(refused), EUNSUPPORTED)
    row('refused pair a', pair(refused, split), EUNSUPPORTED)
    row('refused pair b', pair(split, refused), EUNSUPPORTED)
    row('refused wgrad, two levels with image splits', wgrad(two_img), EUNSUPPORTED)
    # ... and a short workspace before the flags a plan cannot take
    for name, d in (('tiled', tiled), ('thin', thin), ('stem', stem)):
        row('%s live, workspace one byte short' % name, live(d, n=need(d) - 1), EINVAL)

    # ---- flags on a plan that is not the split-layout kernel's
    for name, d in (('tiled', tiled), ('bf16x3', x3), ('bf16', bf16), ('thin', thin), ('stem', stem)):
        row(name + ' live', live(d), EUNSUPPORTED)

    # ---- the operand gate: the query returns what the launch would
    for name, d, act, g, want in (('relu', tiled, RELU, GATE, EINVAL), ('thin relu', thin, RELU, GATE, EINVAL),
                                  ('sigmoid', x3, _lib.ACT_SIGMOID, GATE, EINVAL),
                                  ('3x3', k3, SWISH, GATE, EUNSUPPORTED), ('two levels', two, NONE, GATE, EUNSUPPORTED),
                                  ('two levels with image splits', two_img, NONE, GATE, EUNSUPPORTED),
                                  ('no image splits', no_img, SWISH, GATE, EUNSUPPORTED), ('stem', stem, NONE, GATE, EUNSUPPORTED),
                                  ('split', split, SWISH, GATE, EUNSUPPORTED), ('bf16', bf16, NONE, GATE, EUNSUPPORTED),
                                  ('remainder', remainder, SWISH, GATE, EUNSUPPORTED), ('odd gate address', tiled, NONE, GATE + 2, EUNSUPPORTED),
                                  ('thin, odd gate address', thin, SWISH, GATE + 1, EUNSUPPORTED)):
        row(name + ' gated', gated(d, g, act), want)
        row(name + ' gated_kernel', gkern(d, g, act), want)

    # ---- workspace: one byte short
    for name, d in (('tiled', tiled), ('bf16x3', x3), ('thin', thin), ('stem', stem), ('split', split)):
        row(name + ' wgrad, workspace one byte short', wgrad(d, n=need(d) - 1), EINVAL)
    row('tiled gated, workspace one byte short', gated(tiled, act=SWISH, n=need(tiled) - 1), EINVAL)
    row('thin gated, workspace one byte short', gated(thin, n=need(thin) - 1), EINVAL)
    row('split live, workspace one byte short', live(split, n=need(split) - 1), EINVAL)
    row('pair, workspace one byte short of the sum', pair(split, split, n=2 * need(split) - 1), EINVAL)
    row('pair, workspace of one problem', pair(split, split, n=need(split)), EINVAL)
    row('flagged pair, workspace one byte short of the sum', pair(split, split, LIVE, n=2 * need(split) - 1), EINVAL)

    # ---- pair: both problems on the split-layout kernel, one geometry
    for name, other in (('f32', pyr(_lib.F32)), ('bf16x3', pyr(_lib.F32_BF16X3)), ('bf16', pyr(_lib.BF16)),
                        ('Cout 128', pyr(cout=128)), ('Cin 64', pyr(cin=64)), ('B 2', pyr(B=2))):
        row('pair a %s' % name, pair(other, split), EUNSUPPORTED)
        row('pair b %s' % name, pair(split, other), EUNSUPPORTED)
    row('flagged pair b Cout 128', pair(split, pyr(cout=128), LIVE), EUNSUPPORTED)
    row('pair b Cout 128, workspace short', pair(split, pyr(cout=128), n=1), EUNSUPPORTED)

    wrong = {k: v for k, v in got.items() if v[0] != v[1]}
    assert not wrong and len(got) == 100, (wrong, len(got))
