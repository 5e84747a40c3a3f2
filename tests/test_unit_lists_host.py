"""CPU tier: include/effdet_unit_lists.h against the binding (_lib.UNIT_LISTS_SIGNATURES) and the built library, and the refusals its
three entry points make without device work."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_unit_lists_signatures_match_the_header_and_the_library():
    """The table against the header's prototypes, parsed as tests/test_needed_tiles_host.py parses effdet_needed_tiles.h's: the same
    names, return kind, parameter count and kinds in order; the built library exports them and lib() binds them with the table's types;
    none of the names is in another table; EFFDET_UNIT_COUNTS is the binding's."""
    from efficientdet.pytorch_amd import build, _lib
    src = open(os.path.join(ROOT, 'include', 'effdet_unit_lists.h')).read()
    h = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    scalar = {'int': 'i', 'long long': 'q', 'float': 'f', 'effdet_stream_t': 'p'}
    ret = {'int': 'i', 'long long': 'q'}
    protos = {}
    for r, name, params in re.findall(r'^([a-z][a-z ]*?\*?)\s*\b(effdet_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', h, flags=re.M):
        kinds = []
        for p in params.split(','):
            p = ' '.join(p.split())
            kinds.append('p' if '*' in p else scalar[p.rsplit(' ', 1)[0]])
        protos[name] = (ret[' '.join(r.split())], kinds)
    assert sorted(_lib.UNIT_LISTS_SIGNATURES) == sorted(protos) and len(protos) == 3
    others = [getattr(_lib, n) for n in dir(_lib) if n.endswith('SIGNATURES') and n != 'UNIT_LISTS_SIGNATURES']
    assert len(others) >= 12 and not any(set(protos) & set(t) for t in others)
    assert int(re.search(r'#define EFFDET_UNIT_COUNTS (\d+)', src).group(1)) == _lib.UNIT_COUNTS
    build.build(verbose=False)
    L = _lib.require(*protos)
    for name, (r, kinds) in protos.items():
        sig = _lib.UNIT_LISTS_SIGNATURES[name]
        assert sig[1] == ':' and sig[0] == r, (name, sig, r)
        assert list(sig[2:].replace('s', 'p')) == kinds, (name, sig, ''.join(kinds))
        f = getattr(L, name)
        assert f.restype is _lib._CTYPE[sig[0]] and list(f.argtypes) == [_lib._CTYPE[c] for c in sig[2:]], name


def _hsplit_desc(_lib, a, dtype, cout=32):
    d = _lib.ConvDesc()
    d.x = d.w = d.y = a
    d.dtype, d.B, d.Cin, d.Cout, d.KH, d.KW, d.stride, d.pad_t, d.pad_l, d.ldx, d.ldy = dtype, 1, 32, cout, 3, 3, 1, 1, 1, 32, cout
    d.nseg = 1
    s = d.seg[0]
    s.H = s.W = s.Ho = s.Wo = 4
    s.in_off = s.out_off = 0
    s.in_bstride, s.out_bstride = 16 * 32, 16 * cout
    return d


def test_refusals_without_device_work():
    """Null pointers and bad geometry come back as EFFDET_EINVAL (-1), a launch that takes no flags as EFFDET_EUNSUPPORTED (-3) -- never a
    dense launch on flagged data -- before anything is enqueued (no GPU here: a launch would fail with another code)."""
    from efficientdet.pytorch_amd import build, _lib
    build.build(verbose=False)
    L = _lib.require(*_lib.UNIT_LISTS_SIGNATURES)
    EINVAL, EUNSUPPORTED = -1, -3
    buf = C.create_string_buffer(4096)
    a = C.addressof(buf)                   # never dereferenced: every call below is refused first

    ul = L.effdet_unit_lists
    assert int(ul(None, a, 8, 2, a, a, None)) == EINVAL
    assert int(ul(a, None, 8, 2, a, a, None)) == EINVAL
    assert int(ul(a, a, 8, 2, None, a, None)) == EINVAL
    assert int(ul(a, a, 8, 2, a, None, None)) == EINVAL
    assert int(ul(a, a, 0, 0, a, a, None)) == EINVAL                            # no step
    assert int(ul(a, a, 2, 8, a, a, None)) == EINVAL                            # more tiles than steps
    assert int(ul(a, a, 1 << 30, 1 << 28, a, a, None)) == EUNSUPPORTED          # indices past int32's comfortable range

    for name, dtype, other in (('effdet_conv2d_needed_units', _lib.F32_HSPLIT, _lib.F32_SPLIT),
                               ('effdet_conv2d_live_units', _lib.F32_SPLIT, _lib.F32_HSPLIT)):
        f = getattr(L, name)
        assert int(f(None, a, a, a, a, 0, None)) == EINVAL
        assert int(f(C.byref(_lib.ConvDesc()), a, a, a, a, 0, None)) == EINVAL  # all zero: no x / w / y
        d = _hsplit_desc(_lib, a, dtype)
        assert int(L.effdet_conv2d_kernel(C.byref(d))) in (9, 31)               # a valid descriptor of the flagged kernels (host-side query) ...
        assert int(f(C.byref(d), a, a, a, a, -1, None)) == EINVAL               # ... and a negative first flagged tile
        for hole in range(4):                                                   # ... and each of the four device arrays missing
            args = [a, a, a, a]
            args[hole] = None
            assert int(f(C.byref(d), *args, 0, None)) == EINVAL
        assert int(f(C.byref(_hsplit_desc(_lib, a, other)), a, a, a, a, 0, None)) == EUNSUPPORTED      # the other layout's kernel takes no such flags
