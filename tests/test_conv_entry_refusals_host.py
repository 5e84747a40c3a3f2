"""CPU tier: the return codes with which the six forward conv entry points (effdet_conv2d, _gated, _live, _needed, _live_units,
_needed_units) refuse a call before anything is enqueued, and which refusal wins where several apply.  The expected codes are those of
the library before the entry points shared one launch function (recorded there; this file passed against it unchanged)."""
import ctypes as C

EINVAL, EUNSUPPORTED = -1, -3


def _desc(_lib, a, dtype, **fields):
    """A valid 3x3, stride 1, pad 1 descriptor on one 4x4 map of 32 -> 32 channels; a lends its address to every tensor."""
    d = _lib.ConvDesc()
    d.x = d.w = d.y = a
    d.dtype, d.B, d.Cin, d.Cout, d.KH, d.KW, d.stride, d.pad_t, d.pad_l, d.ldx, d.ldy = dtype, 1, 32, 32, 3, 3, 1, 1, 1, 32, 32
    d.nseg = 1
    s = d.seg[0]
    s.H = s.W = s.Ho = s.Wo = 4
    s.in_off = s.out_off = 0
    s.in_bstride = s.out_bstride = 16 * 32
    for k, v in fields.items():
        setattr(d, k, v)
    return d


def test_refusal_table_of_the_conv_entry_points():
    from efficientdet.pytorch_amd import build, _lib
    build.build(verbose=False)
    L = _lib.require('effdet_conv2d', 'effdet_conv2d_gated', 'effdet_conv2d_live', 'effdet_conv2d_needed', 'effdet_conv2d_live_units',
                     'effdet_conv2d_needed_units', 'effdet_conv2d_kernel')
    buf = C.create_string_buffer(4096)
    a = C.addressof(buf)                   # never dereferenced: every call below is refused first
    split, hsplit = _desc(_lib, a, _lib.F32_SPLIT), _desc(_lib, a, _lib.F32_HSPLIT)
    assert int(L.effdet_conv2d_kernel(C.byref(split))) == 9 and int(L.effdet_conv2d_kernel(C.byref(hsplit))) == 31      # both valid
    biased = _desc(_lib, a, _lib.F32_SPLIT, shift=a)                   # still kernel 9, but a launch that takes no liveness flags
    assert int(L.effdet_conv2d_kernel(C.byref(biased))) == 9
    refused = _desc(_lib, a, _lib.F32_SPLIT, Cin=16, ldx=16)           # the planner's own refusal: half a 32-channel group
    assert int(L.effdet_conv2d_kernel(C.byref(refused))) == EUNSUPPORTED
    empty = _lib.ConvDesc()                                            # all zero: no x / w / y
    ref = C.byref

    got = {}

    def row(what, rc, want):
        got[what] = (int(rc), want)

    # null and empty descriptors: EINVAL everywhere, whatever else is wrong with the call
    for name, p in (('null', None), ('empty', ref(empty))):
        row(name + ' conv2d', L.effdet_conv2d(p, None), EINVAL)
        row(name + ' gated', L.effdet_conv2d_gated(p, a, _lib.ACT_NONE, None), EINVAL)
        row(name + ' gated, null gate', L.effdet_conv2d_gated(p, None, _lib.ACT_NONE, None), EINVAL)
        for fl in (a, None):
            row(name + ' live %s' % fl, L.effdet_conv2d_live(p, fl, 0, None), EINVAL)
            row(name + ' needed %s' % fl, L.effdet_conv2d_needed(p, fl, 0, None), EINVAL)
        row(name + ' live_units', L.effdet_conv2d_live_units(p, a, a, a, a, 0, None), EINVAL)
        row(name + ' needed_units', L.effdet_conv2d_needed_units(p, a, a, a, a, 0, None), EINVAL)

    # the planner's refusal comes first: its code, not the EINVAL of the call's own arguments ...
    row('refused live, tile0 -1', L.effdet_conv2d_live(ref(refused), a, -1, None), EUNSUPPORTED)
    row('refused needed, tile0 -1', L.effdet_conv2d_needed(ref(refused), a, -1, None), EUNSUPPORTED)
    row('refused live_units, null lists', L.effdet_conv2d_live_units(ref(refused), None, None, None, None, -1, None), EUNSUPPORTED)
    row('refused needed_units, null lists', L.effdet_conv2d_needed_units(ref(refused), None, None, None, None, -1, None), EUNSUPPORTED)
    row('refused conv2d', L.effdet_conv2d(ref(refused), None), EUNSUPPORTED)
    # ... except for the null gate, which is looked at before the descriptor
    row('refused gated, null gate', L.effdet_conv2d_gated(ref(refused), None, _lib.ACT_NONE, None), EINVAL)

    for dn, d, units, other_units in (('split', split, L.effdet_conv2d_live_units, L.effdet_conv2d_needed_units),
                                      ('hsplit', hsplit, L.effdet_conv2d_needed_units, L.effdet_conv2d_live_units)):
        # a negative first tile, with and without flags, on the form's own kind of flag and on the other one
        for fl in (a, None):
            row('%s live %s, tile0 -1' % (dn, fl), L.effdet_conv2d_live(ref(d), fl, -1, None), EINVAL)
            row('%s needed %s, tile0 -1' % (dn, fl), L.effdet_conv2d_needed(ref(d), fl, -1, None), EINVAL)
        row(dn + ' units, tile0 -1', units(ref(d), a, a, a, a, -1, None), EINVAL)
        row(dn + ' other units, tile0 -1', other_units(ref(d), a, a, a, a, -1, None), EINVAL)
        # each device array of the gathered form missing: EINVAL, also where the launch would take no such flags anyway
        for hole in range(4):
            args = [a, a, a, a]
            args[hole] = None
            row('%s units, null argument %d' % (dn, hole), units(ref(d), *args, 0, None), EINVAL)
            row('%s other units, null argument %d' % (dn, hole), other_units(ref(d), *args, 0, None), EINVAL)
        # the other form's unit lists: no dense launch on flagged data
        row(dn + ' other units', other_units(ref(d), a, a, a, a, 0, None), EUNSUPPORTED)
        # the operand gate: null gate, a gate on a 3x3 (no gate form), an activation the gate does not know
        row(dn + ' gated, null gate', L.effdet_conv2d_gated(ref(d), None, _lib.ACT_NONE, None), EINVAL)
        row(dn + ' gated 3x3', L.effdet_conv2d_gated(ref(d), a, _lib.ACT_NONE, None), EUNSUPPORTED)
        row(dn + ' gated 3x3 swish', L.effdet_conv2d_gated(ref(d), a, _lib.ACT_SWISH, None), EUNSUPPORTED)
        row(dn + ' gated 3x3, relu', L.effdet_conv2d_gated(ref(d), a, _lib.ACT_RELU, None), EINVAL)
    row('f32 gated 3x3', L.effdet_conv2d_gated(ref(_desc(_lib, a, _lib.F32)), a, _lib.ACT_NONE, None), EUNSUPPORTED)

    # liveness unit lists on a launch with a bias: refused, but only after the call's own arguments
    row('biased live_units', L.effdet_conv2d_live_units(ref(biased), a, a, a, a, 0, None), EUNSUPPORTED)
    row('biased live_units, tile0 -1', L.effdet_conv2d_live_units(ref(biased), a, a, a, a, -1, None), EINVAL)
    row('biased live_units, null flags', L.effdet_conv2d_live_units(ref(biased), None, a, a, a, 0, None), EINVAL)
    row('biased needed_units', L.effdet_conv2d_needed_units(ref(biased), a, a, a, a, 0, None), EUNSUPPORTED)

    wrong = {k: v for k, v in got.items() if v[0] != v[1]}
    assert not wrong and len(got) == 67, (wrong, len(got))
