"""CPU tier of the ATSS matcher (include/effdet_atss.h): the float32 mirror of tests/atss_restated.py against the hand-derived cases, the
cases' margins and tags, the binding against the header, the host-only entry point and the Python options."""
import ctypes
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import atss_cases as AC
from tests import atss_restated as AR
from tests import loss_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ['effdet_loss_atss_fwd', 'effdet_loss_atss_fwd_grad', 'effdet_loss_atss_workspace_bytes']


# --------------------------------------------------------------------------- the mirror against the hand-derived cases
def test_hand_case_candidates_threshold_positives_and_codes():
    c = AC.get('hand')
    r = AR.row_view(c, 0, 1)
    assert r['cand'] == AC.HAND_CAND
    want = [Fraction(i, u) for i, u in AC.HAND_IOU]
    assert np.allclose(r['iou'], [float(v) for v in want], rtol=0, atol=1e-7)
    mean = sum(want) / 24                                                                 # exact rational arithmetic
    thr = float(mean) + float(sum((v - mean) ** 2 for v in want) / 23) ** 0.5
    assert abs(thr - AC.HAND_THR) < 1e-6 and abs(float(r['thr']) - thr) < 1e-6
    assert [a for a, p in zip(r['cand'], r['pos']) if p] == AC.HAND_POS
    i157 = r['cand'].index(157)
    assert float(r['iou'][i157]) == 0.5 and float(r['inside'][i157]) == 0.0 and not r['pos'][i157]      # over thr, centre ON the side
    codes = AC.codes('hand')
    assert torch.nonzero(codes[0] >= 0).reshape(-1).tolist() == AC.HAND_POS and bool((codes[0, AC.HAND_POS] == 1).all())
    assert int((codes == LC.CODE_NEG).sum()) == 180 - 2


def test_small_levels_one_candidate_and_the_unbiased_std():
    c = AC.get('small_level')
    for n in range(3):
        cand = AR.row_view(c, 0, n)['cand']
        assert len(cand) == 4 * 16 + 9
        assert sorted(cand[-9:]) == list(range(3060, 3069))
    c = AC.get('single')
    for n in range(3):
        r = AR.row_view(c, 0, n)
        assert len(r['cand']) == 1 and float(r['thr']) == float(r['iou'][0])           # m = 1: std 0, thr the IoU itself
        assert bool(r['pos'][0]) == bool(r['inside'][0] > 0.01)
    assert int((AC.codes('single') >= 0).sum()) == 3
    v = [np.float32(0.25), np.float32(0.5), np.float32(0.75)]
    assert abs(float(AR.threshold(v)) - (0.5 + 0.25)) < 1e-7                              # var = 0.125 / 2 (unbiased), std 0.25
    assert float(AR.threshold(v[:1])) == 0.25


def test_dup_none_and_nested_by_construction():
    c, codes = AC.get('dup'), AC.codes('dup')
    pos = [a for _, a in c['exact']]
    assert len(pos) >= 3 and bool((codes[0, pos] == 0).all()) and int((codes >= 0).sum()) == len(pos)      # the FIRST row wins the tie
    r0, r2 = AR.row_view(c, 0, 0), AR.row_view(c, 0, 2)
    assert r0['cand'] == r2['cand'] and float(r0['thr']) == float(r2['thr']) and np.array_equal(r0['iou'], r2['iou'])
    c, codes = AC.get('none'), AC.codes('none')
    assert bool((codes[0] == LC.CODE_NEG).all()) and bool((codes[1] == LC.CODE_NEG).all()) and bool((codes[2] == LC.CODE_IGN).all())
    r = AR.row_view(c, 0, 1)
    assert len(r['cand']) == 45 and float(r['inside'].max()) < 0.01 and bool((r['iou'] >= r['thr']).any())
    r = AR.row_view(c, 1, 0)
    assert float(r['thr']) == 0.0 and float(r['iou'].max()) == 0.0 and float(r['inside'].max()) < 0.0
    c, codes = AC.get('nested'), AC.codes('nested')
    r0, r1 = AR.row_view(c, 0, 0), AR.row_view(c, 0, 1)
    p0 = {a: v for a, v, p in zip(r0['cand'], r0['iou'], r0['pos']) if p}
    p1 = {a: v for a, v, p in zip(r1['cand'], r1['iou'], r1['pos']) if p}
    both = set(p0) & set(p1)
    assert len(both) == 7 and set(r0['cand']) & set(r1['cand'])
    for a in both:
        assert int(codes[0, a]) == (0 if p0[a] > p1[a] else 1) and p0[a] != p1[a]
    assert {int(codes[0, a]) for a in both} == {0, 1}
    assert int((codes[0] == 0).sum()) > sum(int(codes[0, a]) == 0 for a in both)         # either row keeps positives of its own
    assert int((codes[0] == 1).sum()) > sum(int(codes[0, a]) == 1 for a in both)


def _key_error(a, box):
    a, box = a.astype(np.float64), box.astype(np.float64)
    u, cmax = 2.0 ** -24, max(float(np.abs(a).max()), float(np.abs(box).max()))
    dx, dy = abs(0.5 * (a[0] + a[2]) - 0.5 * (box[0] + box[2])), abs(0.5 * (a[1] + a[3]) - 0.5 * (box[1] + box[3]))
    return 2 * (dx + dy) * (2 * u * cmax + u * max(dx, dy)) + 3 * u * (dx * dx + dy * dy)


@pytest.mark.parametrize('name', sorted(AC.CASES))
def test_float32_candidates_equal_float64_away_from_key_ties(name):
    """Per (row, level): where the float64 keys on either side of the cut (the last candidate's and the first anchor's left out) are
    further apart than the float32 key's own rounding can bridge, the float32 mirror selects the float64 form's set (a level that is
    taken whole has no cut).  On the integer table every key is exact and the two selections are equal outright, ties included.
    The rounding of a float32 key, with c = the largest |coordinate| and u = 2^-24: a centre 0.5 (x1 + x2) carries u c, so dx carries
    2 u c + u |dx|, dx dx carries 2 |dx| times that + u dx dx, and the sum u d2 more:
        E(a) = 2 (|dx| + |dy|) (2 u c + u max(|dx|, |dy|)) + 3 u d2
    and two keys can change order only if they are within E(a) + E(a') of each other.  (An absolute 1e-9 is no such bound: on the model's
    table the nine anchors of a pixel have centres that agree to ~1e-6 only, because their corners are rounded to fp32.)"""
    c = AC.get(name)
    anc = c['anc'][0].numpy()
    compared = 0
    if 'integer_table' in c['tags']:                                                      # every key exact in either precision: ties included
        for b in range(c['ann'].shape[0]):
            for n in AR.rows_of(c, b):
                box = c['ann'][b, n, :4].numpy()
                assert AR.candidates(anc, box, c['level_start'], c['topk']) == AR.candidates(anc, box, c['level_start'], c['topk'], np.float64)
        return
    for b in range(c['ann'].shape[0]):
        for n in AR.rows_of(c, b):
            box = c['ann'][b, n, :4].numpy()
            d64 = AR.d2(anc, box, np.float64)
            c32, c64 = AR.candidates(anc, box, c['level_start'], c['topk']), AR.candidates(anc, box, c['level_start'], c['topk'], np.float64)
            at = 0
            for lo, hi in zip(c['level_start'][:-1], c['level_start'][1:]):
                k = min(c['topk'], hi - lo)
                order = np.argsort(d64[lo:hi], kind='stable')
                s = d64[lo:hi][order]
                clear = k == hi - lo or s[k] - s[k - 1] > _key_error(anc[lo + order[k - 1]], box) + _key_error(anc[lo + order[k]], box)
                if clear:
                    assert set(c32[at:at + k]) == set(c64[at:at + k]), (name, b, n, lo)
                    compared += 1
                at += k
    assert compared > 0 or 'seeded' not in c['tags']          # (topk 1 never has a clear cut: the nine anchors of a pixel share a centre)


@pytest.mark.parametrize('name', sorted(AC.CASES))
def test_every_case_keeps_its_margin(name):
    c = AC.get(name)
    m = AC.margin(c)
    print('\n%s: margin %.3g' % (name, m))
    assert m >= AC.MARGIN, (name, m)


def test_cases_reach_what_they_are_tagged_with():
    tags = {name: set(AC.get(name)['tags']) for name in AC.CASES}
    assert set().union(*tags.values()) >= {'integer_table', 'level_start_not_64', 'four_way_tie', 'winners_in_two_waves', 'centre_on_side',
                                           'topk_above_level_size', 'one_candidate', 'one_level', 'tail_workgroup', 'chunk_crossing',
                                           'pads_between', 'empty_image', 'shared_candidates', 'loser_keeps_others', 'exact_tie',
                                           'no_positive', 'far_box', 'seeded'}
    c = AC.get('hand')
    assert c['level_start'][1] % 64 != 0 and c['anc'].shape[1] % 9 == 0 and bool((c['anc'] == c['anc'].round()).all())
    d = AR.d2(c['anc'][0].numpy(), c['ann'][0, 1, :4].numpy())
    assert int((d[:144] == d[:144].min()).sum()) == 36 and {a // 64 for a in AC.HAND_CAND[:12]} == {0, 1}      # 4 pixels tie; two waves
    c = AC.get('straddle')
    assert c['anc'].shape[1] == 261 and c['ann'].shape[1] == 65 and c['level_start'] == [0, 252, 261]
    rows = AR.rows_of(c, 0)
    assert rows[-1] == 64 and any(b - a > 1 for a, b in zip(rows[:-1], rows[1:])) and AR.rows_of(c, 1) == []
    codes = AC.codes('straddle')
    assert bool((codes[0, 256:] >= 0).any()) and bool((codes[0] == 64).any())            # positives in the tail workgroup, and of row 64
    assert AC.S128_LEVELS[2] % 256 != 0 and AC.get('s128_nc80')['cls'].shape[2] == 80
    for name in ('s128_nc4', 's128_nc80'):
        codes = AC.codes(name)
        assert all(int((codes[b] >= 0).sum()) >= 8 for b in range(2)), name
        lev = np.searchsorted(AC.S128_LEVELS, torch.nonzero(codes >= 0)[:, 1].numpy(), side='right') - 1
        assert len(set(lev.tolist())) >= 2, name                                          # positives on more than one level


# --------------------------------------------------------------------------- binding
def _prototypes():
    h = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'effdet_atss.h')).read(), flags=re.S)
    scalar = {'int': 'i', 'long long': 'q', 'float': 'f', 'effdet_stream_t': 'p'}
    protos = {}
    for r, name, params in re.findall(r'^([a-z][a-z ]*?\*?)\s*\b(effdet_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', h, flags=re.M):
        kinds = ['p' if '*' in p else scalar[' '.join(p.split()).rsplit(' ', 1)[0]] for p in params.split(',')]
        assert name not in protos, name
        protos[name] = ({'int': 'i', 'long long': 'q'}[' '.join(r.split())], kinds)
    assert sorted(protos) == sorted(set(re.findall(r'\b(effdet_[a-z0-9_]+)\s*\(', h)))
    return protos


def _atss(topk, starts, num_levels=None):
    from efficientdet.pytorch_amd import _lib
    t = _lib.Atss(topk, len(starts) - 1 if num_levels is None else num_levels)
    for i, v in enumerate(starts):
        t.level_start[i] = v
    return t


def test_atss_signatures_match_the_companion_header_and_workspace_bytes():
    from efficientdet.pytorch_amd import build, _lib
    protos = _prototypes()
    assert sorted(protos) == ENTRY_POINTS == sorted(_lib.ATSS_SIGNATURES)
    assert not set(protos) & (set(_lib.SIGNATURES) | set(_lib.BOX_LOSS_SIGNATURES) | set(_lib.LOSS_OPTS_SIGNATURES))
    build.build(verbose=False)
    L = _lib.require(*protos)
    for name, (r, kinds) in protos.items():
        sig = _lib.ATSS_SIGNATURES[name]
        assert sig[1] == ':' and sig[0] == r, (name, sig, r)
        assert list(sig[2:].replace('s', 'p')) == kinds, (name, sig, ''.join(kinds))
        f = getattr(L, name)
        assert f.restype is _lib._CTYPE[sig[0]] and list(f.argtypes) == [_lib._CTYPE[c] for c in sig[2:]], name
    O = _lib.LOSS_OPTS_SIGNATURES
    assert _lib.ATSS_SIGNATURES['effdet_loss_atss_fwd'] == O['effdet_loss_opts_fwd'][:-1] + 'ps'
    assert _lib.ATSS_SIGNATURES['effdet_loss_atss_fwd_grad'] == O['effdet_loss_opts_fwd_grad'][:-1] + 'ps'
    assert _lib.ATSS_SIGNATURES['effdet_loss_atss_workspace_bytes'] == O['effdet_loss_opts_workspace_bytes'] + 'p'
    # host-only: the existing layout first, then kth [B][N][8] 64-bit and thr [B][N]; monotone in N; negative for a bad struct
    B, A, nc = 3, 261, 4
    good = _atss(9, [0, 252, 261])
    head = int(L.effdet_loss_workspace_bytes(B, A, nc))
    al = lambda n: (n + 255) // 256 * 256      # noqa: E731
    sizes = [int(L.effdet_loss_atss_workspace_bytes(B, A, nc, N, ctypes.byref(good))) for N in (1, 2, 65, 66, 200)]
    assert sizes[2] == head + al(8 * 8 * B * 65) + al(4 * B * 65)
    assert sizes == sorted(sizes) and sizes[0] >= head and sizes[-1] > sizes[0]
    for bad in (_atss(0, [0, 252, 261]), _atss(17, [0, 252, 261]), _atss(9, [0, 252, 260]), _atss(9, [0, 252, 252, 261]), _atss(9, [1, 252, 261]),
                _atss(9, [0, 261, 252, 261]), _atss(9, [0]), _atss(9, list(range(0, 9 * 29, 29)), num_levels=9)):
        assert int(L.effdet_loss_atss_workspace_bytes(B, A, nc, 65, ctypes.byref(bad))) == -1
    assert int(L.effdet_loss_atss_workspace_bytes(B, A, nc, 65, None)) == -1
    # an invalid struct or low_quality is refused before anything else (null device pointers: EINVAL either way)
    d = _lib.LossOpts(0.25, 2.0, 0.0, 1.0 / 9.0, 1.0, 0.5, 0.4, 0, 0, 1.0)
    assert L.effdet_loss_atss_fwd(None, None, None, None, None, None, 0, 1, 261, 4, 1, ctypes.byref(d), ctypes.byref(good), None) == -1


def test_struct_matches_the_header_as_gcc_sees_it(tmp_path):
    from efficientdet.pytorch_amd import _lib
    fields = [n for n, _ in _lib.Atss._fields_]
    assert fields == ['topk', 'num_levels', 'level_start'] and ctypes.sizeof(_lib.Atss) == 8 + 8 * 9
    assert (_lib.ATSS_MAX_LEVELS, _lib.ATSS_MAX_TOPK) == (8, 16)
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    src = tmp_path / 'sz.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "effdet_atss.h"\nint main(void){printf("%zu\\n", sizeof(effdet_atss_t));'
                   + ''.join('printf("%%zu\\n", offsetof(effdet_atss_t, %s));' % f for f in fields)
                   + 'printf("%d\\n%d\\n", EFFDET_ATSS_MAX_LEVELS, EFFDET_ATSS_MAX_TOPK);return 0;}\n')
    exe = tmp_path / 'sz'
    subprocess.run(['gcc', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == ctypes.sizeof(_lib.Atss) and out[-2:] == [_lib.ATSS_MAX_LEVELS, _lib.ATSS_MAX_TOPK]
    for f, off in zip(fields, out[1:]):
        assert getattr(_lib.Atss, f).offset == off, f


# --------------------------------------------------------------------------- the Python options
def test_atss_options_validate_their_arguments():
    from efficientdet.pytorch_amd import ATSSOptions, LossOptions, ops
    from efficientdet.pytorch_amd.efficientdet import FocalLoss
    o = ATSSOptions()
    assert o.topk == 9 and o == ATSSOptions(9) and o != ATSSOptions(8) and o != None and hash(o) == hash(ATSSOptions(topk=9))      # noqa: E711
    assert o.key() == (9,) and repr(ATSSOptions(12)) == 'ATSSOptions(topk=12)'
    assert ATSSOptions(1).topk == 1 and ATSSOptions(16).topk == 16
    for bad in (0, 17, -1, 9.0, '9', None, True):
        with pytest.raises(ValueError):
            ATSSOptions(bad)
    t = ops._atss_struct(o, [2304, 576, 144, 36, 9], 3069)
    assert (t.topk, t.num_levels, list(t.level_start)[:6]) == (9, 5, AC.S128_LEVELS)
    for levels, A in (([2304, 576], 3069), ([], 0), ([1] * 9, 9), ([5, 0, 4], 9), (None, 9)):
        with pytest.raises(ValueError):
            ops._atss_struct(o, levels, A)
    with pytest.raises(TypeError):
        ops.check_matcher('atss', None)
    with pytest.raises(TypeError):
        FocalLoss(matcher=9)
    assert FocalLoss().matcher is None and FocalLoss(matcher=o).matcher is o and FocalLoss(loss=LossOptions(gamma=1.5), matcher=o).matcher is o
    # the default-valued struct on the options path
    s = ops._loss_opts_struct(None, None, force=True)
    d = LossOptions()
    assert (s.alpha, s.gamma, s.label_smoothing, s.beta, s.reg_weight, s.low_quality, s.box_kind) == (0.25, 2.0, 0.0, d.beta, 1.0, 0, 0)
    assert ops._loss_opts_struct(d, None, force=True).gamma == 2.0 and ops._loss_opts_struct(d) is None


def test_bands_or_low_quality_with_a_matcher_raise_where_the_second_is_set():
    from efficientdet.pytorch_amd import ATSSOptions, EfficientDet, LossOptions
    from efficientdet.pytorch_amd.efficientdet import FocalLoss
    o = ATSSOptions()
    for kw in (dict(low_quality=True), dict(pos_iou=0.6), dict(neg_iou=0.3), dict(pos_iou=0.75, neg_iou=0.25)):
        bad = LossOptions(**kw)
        m = EfficientDet(num_classes=4)
        m.set_loss(bad)
        with pytest.raises(ValueError) as e:
            m.set_matcher(o)
        assert 'ATSSOptions' in str(e.value) and 'LossOptions' in str(e.value)
        assert m.matcher is None and m.criterion.matcher is None
        m = EfficientDet(num_classes=4)
        m.set_matcher(o)
        with pytest.raises(ValueError) as e:
            m.set_loss(bad)
        assert 'ATSSOptions' in str(e.value) and 'LossOptions' in str(e.value)
        assert m.loss_options is None and m.matcher is o
        with pytest.raises(ValueError):
            FocalLoss(loss=bad, matcher=o)
    m = EfficientDet(num_classes=4)
    assert m.matcher is None and m.set_matcher(o) is m and m.matcher is o and m.criterion.matcher is o
    assert m.set_loss(LossOptions(gamma=1.5, beta=0.1, reg_weight=50.0)) is m                # what a matcher does not replace
    with pytest.raises(TypeError):
        m.set_matcher(9)
    assert m.set_matcher(None).matcher is None and m.criterion.matcher is None


def test_a_model_pickled_before_the_option_loads_without_a_matcher():
    import pickle
    from efficientdet.pytorch_amd import ATSSOptions, EfficientDet
    m = EfficientDet(num_classes=4).set_matcher(ATSSOptions(7))
    m2 = pickle.loads(pickle.dumps(m))
    assert m2.matcher == ATSSOptions(7) and m2.criterion.matcher == ATSSOptions(7)
    del m.__dict__['matcher'], m.criterion.__dict__['matcher']                              # as such a model's state has it
    m3 = pickle.loads(pickle.dumps(m))
    assert getattr(m3, 'matcher', None) is None and getattr(m3.criterion, 'matcher', None) is None


def test_without_a_matcher_the_entry_points_are_todays():
    from efficientdet.pytorch_amd import ATSSOptions, BoxLossOptions, LossOptions, build, ops
    build.build(verbose=False)
    o, box = LossOptions(gamma=1.5), BoxLossOptions('giou', 2.0)
    for stem in ('fwd', 'fwd_grad', 'bwd_reg'):
        assert ops._loss_entry(stem)[1] == 'effdet_focal_loss_' + stem and ops._loss_entry(stem)[2] == ()
        assert ops._loss_entry(stem, LossOptions())[1] == 'effdet_focal_loss_' + stem
        assert ops._loss_entry(stem, None, box)[1:3] == ('effdet_box_loss_' + stem, (2, 2.0))
        assert ops._loss_entry(stem, o, box)[1] == 'effdet_loss_opts_' + stem and ops._loss_entry(stem, o, box)[3] is True
        assert ops._loss_entry(stem, matcher=None, atss=None)[1] == 'effdet_focal_loss_' + stem
    assert ops._loss_entry('bwd_cls', o)[1] == 'effdet_loss_opts_bwd_cls'
    # with one: the atss forward calls, and the options' backward calls although the values are the defaults
    m = ATSSOptions()
    t = ops._atss_struct(m, [252, 9], 261)
    for stem in ('fwd', 'fwd_grad'):
        fn, name, extra, opts, _ = ops._loss_entry(stem, None, None, m, t)
        assert name == 'effdet_loss_atss_' + stem and len(extra) == 2 and opts is True
    for stem in ('bwd_cls', 'bwd_reg'):
        fn, name, extra, opts, _ = ops._loss_entry(stem, None, None, m)
        assert name == 'effdet_loss_opts_' + stem and len(extra) == 1 and opts is True
