"""CPU tier: include/effdet_wgrad_pair.h against the binding (_lib.WGRAD_PAIR_SIGNATURES) and the built library, and the refusals of the
paired weight-gradient launch that need no device (they return before the first HIP call)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pair_signature_matches_the_header_and_the_library():
    """The table against the header's prototype, parsed as tests/test_abi.py parses effdet_hip.h's; the built library exports the name
    and lib() binds it with the table's types; the name is not in effdet_hip.h's table, whose ABI generation is unchanged."""
    from efficientdet.pytorch_amd import build, _lib
    h = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'effdet_wgrad_pair.h')).read(), flags=re.S)
    scalar = {'int': 'i', 'long long': 'q', 'float': 'f', 'effdet_stream_t': 'p'}
    ret = {'int': 'i', 'long long': 'q'}
    protos = {}
    for r, name, params in re.findall(r'^([a-z][a-z ]*?\*?)\s*\b(effdet_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', h, flags=re.M):
        kinds = []
        for p in params.split(','):
            p = ' '.join(p.split())
            kinds.append('p' if '*' in p else scalar[p.rsplit(' ', 1)[0]])
        protos[name] = (ret[' '.join(r.split())], kinds)
    assert sorted(_lib.WGRAD_PAIR_SIGNATURES) == sorted(protos) == ['effdet_conv2d_wgrad_pair']
    assert not set(protos) & set(_lib.SIGNATURES)
    build.build(verbose=False)
    L = _lib.require(*protos)
    for name, (r, kinds) in protos.items():
        sig = _lib.WGRAD_PAIR_SIGNATURES[name]
        assert sig[1] == ':' and sig[0] == r, (name, sig, r)
        assert list(sig[2:].replace('s', 'p')) == kinds, (name, sig, ''.join(kinds))
        f = getattr(L, name)
        assert f.restype is _lib._CTYPE[sig[0]] and list(f.argtypes) == [_lib._CTYPE[c] for c in sig[2:]], name
    assert int(L.effdet_abi_version()) == _lib.ABI_VERSION


def test_pair_refusals_on_the_host():
    """Null arguments, problems that do not plan to the split-layout kernel, unequal geometry and a short workspace are refused by the planner, before any device work (the pointers are fake)."""
    from efficientdet.pytorch_amd import build, _lib
    from tests.host_util import wgrad_desc
    build.build(verbose=False)
    L = _lib.require('effdet_conv2d_wgrad_pair')
    sizes = [(16, 16), (8, 8), (4, 4)]
    mk = lambda dt=_lib.F32_SPLIT, B=3, cin=256, cout=256, sz=sizes: wgrad_desc(dt, B, cin, cout, sz, k=3, pad=1)
    pair = lambda a, b, nbytes=1 << 40: int(L.effdet_conv2d_wgrad_pair(C.byref(a) if a else None, C.byref(b) if b else None, 0x70000000, nbytes, None, None))
    EINVAL, EUNSUPPORTED = -1, -3
    good = mk()
    assert pair(None, good) == EINVAL and pair(good, None) == EINVAL
    assert int(L.effdet_conv2d_wgrad_pair(C.byref(good), C.byref(good), None, 1 << 40, None, None)) == EINVAL
    for other in (mk(cout=128), mk(cin=64), mk(B=2), mk(dt=_lib.F32), mk(dt=_lib.F32_BF16X3)):
        assert pair(good, other) == EUNSUPPORTED and pair(other, good) == EUNSUPPORTED
    need = int(L.effdet_conv2d_wgrad_workspace_bytes(C.byref(good)))
    assert need > 0 and pair(good, good, 2 * need - 1) == EINVAL
