"""CPU tier: include/effdet_needed_tiles.h against the binding (_lib.NEEDED_SIGNATURES) and the built library, and the refusals its three
entry points make without device work."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_needed_signatures_match_the_header_and_the_library():
    """The table against the header's prototypes, parsed as tests/test_live_tiles_host.py parses effdet_live_tiles.h's: the same names,
    return kind, parameter count and kinds in order; the built library exports them and lib() binds them with the table's types; none of
    the names is in effdet_hip.h's or effdet_live_tiles.h's table."""
    from efficientdet.pytorch_amd import build, _lib
    h = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'effdet_needed_tiles.h')).read(), flags=re.S)
    scalar = {'int': 'i', 'long long': 'q', 'float': 'f', 'effdet_stream_t': 'p'}
    ret = {'int': 'i', 'long long': 'q'}
    protos = {}
    for r, name, params in re.findall(r'^([a-z][a-z ]*?\*?)\s*\b(effdet_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', h, flags=re.M):
        kinds = []
        for p in params.split(','):
            p = ' '.join(p.split())
            kinds.append('p' if '*' in p else scalar[p.rsplit(' ', 1)[0]])
        protos[name] = (ret[' '.join(r.split())], kinds)
    assert sorted(_lib.NEEDED_SIGNATURES) == sorted(protos) and len(protos) == 3
    assert not set(protos) & set(_lib.SIGNATURES) and not set(protos) & set(_lib.LIVE_SIGNATURES)
    build.build(verbose=False)
    L = _lib.require(*protos)
    for name, (r, kinds) in protos.items():
        sig = _lib.NEEDED_SIGNATURES[name]
        assert sig[1] == ':' and sig[0] == r, (name, sig, r)
        assert list(sig[2:].replace('s', 'p')) == kinds, (name, sig, ''.join(kinds))
        f = getattr(L, name)
        assert f.restype is _lib._CTYPE[sig[0]] and list(f.argtypes) == [_lib._CTYPE[c] for c in sig[2:]], name


def test_refusals_without_device_work():
    """Null pointers and bad geometry come back as EFFDET_EINVAL (-1) before anything is enqueued (no GPU here: a launch would fail
    with another code)."""
    from efficientdet.pytorch_amd import build, _lib
    build.build(verbose=False)
    L = _lib.require(*_lib.NEEDED_SIGNATURES)
    EINVAL = -1
    sizes = [(16, 16), (8, 8), (4, 4)]
    n = len(sizes)
    H, W = (C.c_int * n)(*[h for h, _ in sizes]), (C.c_int * n)(*[w for _, w in sizes])
    A = 9 * sum(h * w for h, w in sizes)
    buf = C.create_string_buffer(4096)
    a = C.addressof(buf)                   # never dereferenced: every call below is refused first

    pm = L.effdet_positive_pixel_map
    assert int(pm(None, a, 3, A, 4, n, H, W, a, None)) == EINVAL
    assert int(pm(a, None, 3, A, 4, n, H, W, a, None)) == EINVAL
    assert int(pm(a, a, 3, A, 4, n, H, W, None, None)) == EINVAL
    assert int(pm(a, a, 3, A, 4, n, None, W, a, None)) == EINVAL
    assert int(pm(a, a, 0, A, 4, n, H, W, a, None)) == EINVAL                  # no image
    assert int(pm(a, a, 3, A, 0, n, H, W, a, None)) == EINVAL                  # no annotation row
    assert int(pm(a, a, 3, A, 4, 0, H, W, a, None)) == EINVAL and int(pm(a, a, 3, A, 4, 6, H, W, a, None)) == EINVAL
    assert int(pm(a, a, 3, A - 9, 4, n, H, W, a, None)) == EINVAL              # the anchor table is not 9 per pixel of these levels
    Hz = (C.c_int * n)(16, 0, 4)
    assert int(pm(a, a, 3, A, 4, n, Hz, W, a, None)) == EINVAL

    fm = L.effdet_live_tiles_from_map
    assert int(fm(None, 3, n, H, W, a, a, a, None)) == EINVAL
    assert int(fm(a, 3, n, H, W, None, a, a, None)) == EINVAL
    assert int(fm(a, 3, n, H, W, a, None, a, None)) == EINVAL
    assert int(fm(a, 3, n, H, W, a, a, None, None)) == EINVAL
    assert int(fm(a, 0, n, H, W, a, a, a, None)) == EINVAL
    assert int(fm(a, 3, n, Hz, W, a, a, a, None)) == EINVAL
    assert int(fm(a, 3, 6, H, W, a, a, a, None)) == EINVAL

    cn = L.effdet_conv2d_needed
    assert int(cn(None, a, 0, None)) == EINVAL
    d = _lib.ConvDesc()                                                         # all zero: no x / w / y
    assert int(cn(C.byref(d), a, 0, None)) == EINVAL
    d.x = d.w = d.y = a
    d.dtype, d.B, d.Cin, d.Cout, d.KH, d.KW, d.stride, d.pad_t, d.pad_l, d.ldx, d.ldy = _lib.F32_HSPLIT, 1, 32, 32, 3, 3, 1, 1, 1, 32, 32
    d.nseg = 1
    s = d.seg[0]
    s.H = s.W = s.Ho = s.Wo = 4
    s.in_off = s.out_off = 0
    s.in_bstride = s.out_bstride = 16 * 32
    assert int(L.effdet_conv2d_kernel(C.byref(d))) == 31                        # a valid f16x3 descriptor (host-side query) ...
    assert int(cn(C.byref(d), a, -1, None)) == EINVAL                           # ... and a negative first flagged tile
