"""CPU checks of tests/loss_cases.py: every case reaches the branch of loss.hip it is named for, its hand-derived states are the
oracle's, and the oracle says the same in fp32 and fp64 (so the fp64 reference of tests/test_gpu_loss_edges.py is the reference of
the fp32 kernels too).  If a case stops reaching its branch -- N <= 64, A*nc % 4 == 0, <= 192 partials, no clamped positive, a
skip set over its cap -- a test here fails."""
import pytest
import torch

from oracle import effdet_oracle as O
from tests import loss_cases as LC

SKIP_CAP = 1e-3                          # the state comparison of `chunks` may skip at most 0.1 % of an image's anchors


@pytest.fixture(scope='module')
def cases():
    return {k: f() for k, f in LC.CASES.items()}


def _valid_rows(case, b):
    return torch.nonzero(case['ann'][b, :, 4] != -1).reshape(-1)


@pytest.mark.parametrize('name', sorted(LC.CASES))
def test_case_is_well_formed_and_the_oracle_agrees_with_itself(cases, name):
    c = cases[name]
    B, A, nc = c['cls'].shape
    assert c['anc'].shape == (1, A, 4) and c['reg'].shape == (B, A, 4) and c['ann'].shape[0] == B and c['ann'].shape[2] == 5
    assert A == LC.anchors(c['S']).shape[1] and A % 9 == 0
    lab = c['ann'][:, :, 4]
    assert bool(((lab == -1) | ((lab >= 0) & (lab < nc) & (lab == lab.floor()))).all())
    assert all(t.dtype == torch.float32 for t in (c['cls'], c['reg'], c['anc'], c['ann']))
    s32, s64 = LC.oracle_states(c, torch.float32), LC.oracle_states(c, torch.float64)
    differ = s32 != s64
    if c['state_check'] == 'exact':
        assert not bool(differ.any())
    else:
        assert not bool((differ & ~LC.skip_mask(c)).any())
    l32 = torch.cat(O.focal_loss(c['cls'], c['reg'], c['anc'], c['ann']))
    l64 = torch.cat(O.focal_loss(c['cls'].double(), c['reg'].double(), c['anc'].double(), c['ann'].double()))
    assert bool(torch.isfinite(l64).all()) and float(l64[0]) > 0 and float(l64[1]) > 0
    assert bool(((l32.double() - l64).abs() <= 2e-4 * l64.abs()).all()), (l32, l64)
    # hand-derived expectations are what the oracle computes
    for b, a, state, row in c['expect']:
        assert int(s64[b, a]) == LC.state_code(state, row), (name, b, a, state, row, int(s64[b, a]))
    for b, state in c['expect_all'].items():
        assert bool((s64[b] == LC.state_code(state, None)).all()), (name, b, state)


def test_chunks_reaches_the_chunk_loop_the_interspersed_pads_and_the_scalar_tail(cases):
    c = cases['chunks']
    B, A, nc = c['cls'].shape
    N = c['ann'].shape[1]
    assert N > 2 * LC.CHUNK and (A * nc) % 4 != 0 and A * nc == 15345
    v0, v1 = _valid_rows(c, 0), _valid_rows(c, 1)
    assert len(v0) == 90
    for v in (v0, v1):                                                  # pads between valid rows, not only behind them
        assert int(v[-1]) - int(v[0]) + 1 > len(v)
    for k in range(3):                                                  # image 0: every chunk has valid rows AND pads
        n = int(((v0 >= k * 64) & (v0 < (k + 1) * 64)).sum())
        assert 0 < n < min(64, N - k * 64) or (k == 2 and n > 0)
    assert int(((v1 >= 64) & (v1 < 128)).sum()) == 0                    # image 1: an empty middle chunk
    assert int((v1 < 64).sum()) > 0 and int((v1 >= 128).sum()) > 0
    assert bool((c['ann'][0, v0, :4] != c['ann'][0, v0, :4].round()).any())        # fractional coordinates
    s = LC.oracle_states(c, torch.float64)
    for b, v in ((0, v0), (1, v1)):
        won = s[b][s[b] >= 0]
        assert int((won >= 64).sum()) > 0 and int((won < 64).sum()) > 0             # winners in the first chunk and in later ones
        # compaction matters: a winner whose index among the valid rows differs from its row
        rank = {int(r): i for i, r in enumerate(v)}
        assert any(rank[int(r)] != int(r) for r in won.unique())
    assert int((s[1] >= 128).sum()) > 0                                 # past the empty chunk
    assert int((s == LC.CODE_IGN).sum()) > 0 and int((s == LC.CODE_NEG).sum()) > 0
    skip = LC.skip_mask(c)
    for b in range(B):
        assert int(skip[b].sum()) <= SKIP_CAP * A, (b, int(skip[b].sum()))


@pytest.mark.parametrize('N', sorted(LC.TIE_VARIANTS))
def test_chunk_ties_tie_and_mirror(cases, N):
    c = cases['chunk_ties_N%d' % N]
    late = LC.TIE_VARIANTS[N]
    ann = c['ann']
    assert ann.shape[1] == N and late == (N - 1 if N <= 65 else 70) and (late >= 64) == (N > 64)
    assert torch.equal(ann[0, 3, :4], ann[0, late, :4]) and float(ann[0, 3, 4]) != float(ann[0, late, 4])
    assert float(ann[1, 3, 4]) != float(ann[1, late, 4])
    s = LC.oracle_states(c, torch.float64)
    assert int((s[0] == 3).sum()) > 1 and int((s[0] == late).sum()) == 0            # the earlier twin wins everywhere
    t = LC.int_anchor(8, 8)
    iou, rows = LC.oracle_iou(c, 1, torch.float64)
    r = {int(x): i for i, x in enumerate(rows)}
    assert float(iou[t, r[3]]) == 17.0 / 32.0 and float(iou[t, r[late]]) == 1.0     # the mirror: both positive, the later one better
    assert int((ann[:, :, 4] == -1).sum()) > 0 and int(_valid_rows(c, 0)[0]) > 0    # pads in front of and between the rows


@pytest.mark.parametrize('nested', [False, True])
def test_thresholds_sit_exactly_on_the_thresholds(cases, nested):
    c = cases['thresholds_nested' if nested else 'thresholds']
    t = LC.int_anchor(8, 8)
    anc = c['anc'][0]
    assert t == 1227 and anc[t].tolist() == [52.0, 52.0, 84.0, 84.0]
    assert anc[1155].tolist() == [-12.0, 52.0, 20.0, 84.0]
    integer = (anc == anc.round()).all(dim=1)
    assert int(integer.sum()) == 341
    assert bool((c['ann'][:, 1, :4] == c['ann'][:, 1, :4].round()).all())
    want = [0.5, 544.0 / 1024.0, 480.0 / 1024.0, 0.4, 1024.0 / 2528.0, 1024.0 / 2592.0] if nested else \
        [0.5, 800.0 / 1536.0, 736.0 / 1536.0, 0.4, 800.0 / 1920.0, 736.0 / 1920.0]
    for b, w in enumerate(want):
        for dt in (torch.float32, torch.float64):
            iou, _ = LC.oracle_iou(c, b, dt)
            assert float(iou[t, 0]) == float(torch.tensor(w, dtype=torch.float64).to(dt)), (b, dt)
    i32 = LC.oracle_iou(c, 3, torch.float32)[0][t, 0]
    assert float(i32) == float(torch.tensor(0.4, dtype=torch.float32)) and not bool(i32 < 0.4)
    assert bool(LC.oracle_iou(c, 0, torch.float32)[0][t, 0] >= 0.5)
    # every other anchor is either integer-valued (exact whatever the contraction) or clear of both thresholds
    skip = LC.skip_mask(c) & ~integer[None]
    if nested:       # nested boxes also nest the pixel's ratio-0.5 / ratio-2 anchors (area 1024 up to rounding): within 2e-8, not exact
        assert 0 < int(skip.sum()) <= 6 and not bool(skip[:, t].any())
    else:
        assert not bool(skip.any())
    s = LC.oracle_states(c, torch.float64)
    states = [int(s[b, t]) for b in range(len(want))]
    assert states == [1, 1, LC.CODE_IGN, LC.CODE_IGN, LC.CODE_IGN, LC.CODE_NEG]


def test_tiny_box_has_a_positive_whose_target_width_clamps(cases):
    c = cases['tiny_box']
    s = LC.oracle_states(c, torch.float64)
    pos = torch.nonzero(s[0] >= 0).reshape(-1)
    assert sorted(pos.tolist()) == sorted(LC.TINY_ANCHORS)
    g = c['ann'][0, s[0, pos]]
    gw, gh = g[:, 2] - g[:, 0], g[:, 3] - g[:, 1]
    assert bool((gw < 1).any()) and bool((gh < 1).any())
    assert bool((s[0][s[0] < 0] == LC.CODE_NEG).all())
    # the near-duplicate would also make the anchor positive: only the argmax tells them apart
    iou, rows = LC.oracle_iou(c, 0, torch.float64)
    assert rows.tolist() == [0, 2] and bool((iou[pos] >= 0.5).all())
    std = O.anchors_for_image(128, 128)[0]
    assert float((std[:, 2:] - std[:, :2]).min()) > 22.0             # why the model's own table cannot reach the clamp


@pytest.mark.parametrize('nc', LC.TAIL_NC)
def test_tails_take_the_scalar_path(cases, nc):
    c = cases['tails_nc%d' % nc]
    B, A, k = c['cls'].shape
    assert k == nc and (A * nc) % 4 != 0
    assert (A * 6) % 4 == 2
    assert int((LC.oracle_states(c, torch.float64) >= 0).sum()) > 0


def test_many_images_needs_a_second_pass_of_the_image_loop(cases):
    c = cases['many_images']
    B, A, nc = c['cls'].shape
    assert B == 18 and B > 16 and nc == 4
    assert len(_valid_rows(c, 16)) == 0 and len(_valid_rows(c, 17)) > 0
    s = LC.oracle_states(c, torch.float64)
    assert int((s[17] >= 0).sum()) == 0 and int((s[:16] >= 0).sum()) > 0
    assert int((s[0] >= 0).sum()) > 0                                 # image 0 and image 16 share a wave: both must count


@pytest.mark.parametrize('path', sorted(LC.MANY_PARTIALS))
def test_many_partials_exceed_the_four_chain_threshold(cases, path):
    c = cases['many_partials_%s' % path]
    B, A, nc = c['cls'].shape
    ncb = LC.ncb_fwd_grad(A, nc) if path == 'fwd_grad' else LC.ncb_fwd(A, nc)
    assert ncb > LC.LANE_SUM_CHAINS, ncb
    assert ncb == {'fwd_grad': 256, 'fwd': 270}[path]
    assert nc % 4 == 0 and (A * nc) % 4 == 0
