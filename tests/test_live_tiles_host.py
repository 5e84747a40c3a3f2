"""CPU tier: include/effdet_live_tiles.h against the binding (_lib.LIVE_SIGNATURES) and the built library, and the host-only geometry
query of the liveness flags."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_live_signatures_match_the_header_and_the_library():
    """The table against the header's prototypes, parsed as tests/test_abi.py parses effdet_hip.h's: the same names, return kind,
    parameter count and kinds in order; the built library exports them and lib() binds them with the table's types; none of the names
    is in effdet_hip.h's table, whose ABI generation is unchanged."""
    from efficientdet.pytorch_amd import build, _lib
    h = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'effdet_live_tiles.h')).read(), flags=re.S)
    scalar = {'int': 'i', 'long long': 'q', 'float': 'f', 'effdet_stream_t': 'p'}
    ret = {'int': 'i', 'long long': 'q'}
    protos = {}
    for r, name, params in re.findall(r'^([a-z][a-z ]*?\*?)\s*\b(effdet_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', h, flags=re.M):
        kinds = []
        for p in params.split(','):
            p = ' '.join(p.split())
            kinds.append('p' if '*' in p else scalar[p.rsplit(' ', 1)[0]])
        protos[name] = (ret[' '.join(r.split())], kinds)
    assert sorted(_lib.LIVE_SIGNATURES) == sorted(protos) and len(protos) == 4
    assert not set(protos) & set(_lib.SIGNATURES)
    build.build(verbose=False)
    L = _lib.require(*protos)
    for name, (r, kinds) in protos.items():
        sig = _lib.LIVE_SIGNATURES[name]
        assert sig[1] == ':' and sig[0] == r, (name, sig, r)
        assert list(sig[2:].replace('s', 'p')) == kinds, (name, sig, ''.join(kinds))
        f = getattr(L, name)
        assert f.restype is _lib._CTYPE[sig[0]] and list(f.argtypes) == [_lib._CTYPE[c] for c in sig[2:]], name
    assert int(re.search(r'#define\s+EFFDET_LIVE_RADII\s+(\d+)', h).group(1)) == _lib.LIVE_RADII == 6


def test_live_tiles_counts():
    """Steps of 32 and tiles of 128 pixels per level, each level rounded up on its own; refusals without device work."""
    from efficientdet.pytorch_amd import build, _lib
    build.build(verbose=False)
    L = _lib.require('effdet_live_tiles_counts', 'effdet_live_tiles')

    def counts(B, sizes):
        n = len(sizes)
        H, W = (C.c_int * n)(*[h for h, _ in sizes]), (C.c_int * n)(*[w for _, w in sizes])
        s, t = C.c_longlong(-1), C.c_longlong(-1)
        return int(L.effdet_live_tiles_counts(B, n, H, W, C.byref(s), C.byref(t))), s.value, t.value

    assert counts(3, [(16, 16), (8, 8), (4, 4)]) == (1008, 24 + 6 + 2, 6 + 2 + 1)
    assert counts(32, [(64 >> i, 64 >> i) for i in range(5)]) == (174592, 5456, 1364)
    assert counts(1, [(1, 1)]) == (1, 1, 1)
    assert counts(0, [(4, 4)])[0] == -1 and counts(2, [(4, 0)])[0] == -1 and counts(2, [(4, 4)] * 6)[0] == -1      # EFFDET_EINVAL
    one = (C.c_int * 1)(4)
    assert int(L.effdet_live_tiles(None, _lib.F32, 64, 1, 1, one, one, None, None, None, None)) == -1            # null pointers
