"""Shared inputs of the output-path edge tests (tests/test_detect_out_cases_host.py on the CPU, tests/test_gpu_detect_out_edges.py on
the device): seeded builders for anchors -> decode_score -> nms -> gather_dets -> finalize_dets and head_out_bwd at the sizes and
values where the kernels of postprocess.hip / pipeline.hip take another path, plus the small restatements the two tiers share (a
float64 decode, the eval consumer in NumPy, the kept-box grid's cell arithmetic).  Everything is an fp32 / integer CPU tensor; the
host tier proves that each case reaches what it is named for, the device tier only calls ops.* on them."""
import functools
import math

import numpy as np
import torch

from oracle import effdet_oracle as O
from tests.test_gpu_post_loss import _nms_ref as nms_ref          # THE keep-list recipe of the suite: threshold, oracle, map back

# postprocess.hip constants the host tier reasons with
QUAD = 4                                             # lanes that scan one anchor's class row in decode_score_kernel
DECODE_BLOCK = 64                                    # anchors per decode_score_kernel block
KG_CAP = 8                                           # kept boxes per (octave, cell) of the grid; more go to the overflow list
SB_MIN, SB_MAX = 4, 40                               # octave clamp


def round_size(A):
    """Candidates per greedy round."""
    return 4096 if A > 65536 else 2048


def close_metric(got, ref):
    """gpu_util.assert_close's measure as a number (float64): max |got - ref| / max(|ref|, 1e-2 * max |ref|)."""
    got, ref = got.detach().double(), ref.detach().double()
    floor = 1e-2 * float(ref.abs().max()) + 1e-30
    return float(((got - ref).abs() / ref.abs().clamp_min(floor)).max())


# --------------------------------------------------------------------------- 1. anchors
ANCHOR_SIZES = [(1, 1), (7, 130), (100, 333), (129, 127), (513, 511)]


def num_anchors_restated(H, W):
    return sum(9 * (-(-H // (1 << l))) * (-(-W // (1 << l))) for l in range(3, 8))


# --------------------------------------------------------------------------- 2. decode_score
IMG_H, IMG_W = 333, 500                              # non-square; see decode_case for why just below a power of two
DECODE_SHAPES = [(1, 1, 1), (1, 77, 2), (2, 63, 3), (1, 50, 5), (3, 65, 6), (1, 64, 20), (2, 200, 80), (1, 130, 90), (2, 100, 91)]
FAMILIES = ('distinct', 'eighths', 'zeros_last')
EXTREME = 200.0                                      # regression input whose dw = 0.2 * input is 40
REG_PATTERNS = ((EXTREME, EXTREME), (-EXTREME, -EXTREME), (EXTREME, -EXTREME), None)       # (raw dw, raw dh); None: all four deltas zero


def special_rows(n):
    """-> [(flat row, pattern)]: up to 8 rows of the n = B * A, cycling through REG_PATTERNS, spread over the whole range."""
    k = min(8, n // 4)
    return [(int(r), REG_PATTERNS[j % 4]) for j, r in enumerate(np.linspace(0, n - 1, k).round().astype(int))] if k else []


@functools.lru_cache(maxsize=None)
def decode_case(B, A, nc, family):
    """-> dict(anc [1, A, 4], reg [B, A, 4], cls [B, A, nc]).  Anchors are caller-made (random centres inside the IMG_W x IMG_H image,
    sides 8..200): the op takes any [A, 4] table.  The image is 500 x 333 so that the largest coordinate sits just under a power
    of two: one ulp of a 256..512 intermediate is 3.1e-5, i.e. 6.1e-6 of assert_close's floor 1e-2 * 500 -- inside the 1e-5 the
    decode is held to -- whereas at 257 px the same ulp would be 1.2e-5 of the floor."""
    g = torch.Generator().manual_seed(1000 * nc + 10 * A + B + 7 * FAMILIES.index(family))
    ctr = torch.rand(A, 2, generator=g) * torch.tensor([float(IMG_W), float(IMG_H)])
    wh = 8.0 + torch.rand(A, 2, generator=g) * 192.0
    anc = torch.cat([ctr - 0.5 * wh, ctr + 0.5 * wh], 1)[None].contiguous()
    reg = torch.randn(B, A, 4, generator=g) * 2.0
    flat = reg.view(-1, 4)
    for r, pat in special_rows(B * A):
        if pat is None:
            flat[r] = 0.0
        else:
            flat[r, 2], flat[r, 3] = pat
    u = torch.rand(B, A, nc, generator=g)
    if family == 'distinct':                         # a permutation of the nc slots (1/nc wide) + jitter inside the slot: no tie in a row
        cls = (torch.argsort(u, dim=2).float() + 0.25 + 0.5 * torch.rand(B, A, nc, generator=g)) / nc
    elif family == 'eighths':                        # 0, 1/8 .. 7/8, skewed to the top so that short rows tie at their maximum too
        cls = (u.sqrt() * 8.0).floor().clamp(max=7.0) / 8.0
    else:                                            # even flat rows all zero, odd ones zero but for the last class
        cls = torch.zeros(B, A, nc)
        odd = (torch.arange(B * A) % 2 == 1).view(B, A)
        cls[:, :, nc - 1] = torch.where(odd, 0.125 + 0.75 * u[:, :, 0], torch.zeros(B, A))
    return {'anc': anc, 'reg': reg, 'cls': cls}


def later_lane_tie_rows(cls):
    """-> bool [B, A]: rows holding a tied maximum whose FIRST index k1 and a later tied index k2 have k1 % 4 > k2 % 4 -- the quad
    merge then meets the first index in a later lane than another tied one, and only the `oa < arg` rule keeps it."""
    m = cls.max(dim=2, keepdim=True)[0]
    tied = cls == m
    nc = cls.shape[2]
    k = torch.arange(nc)
    first = tied.float().argmax(dim=2, keepdim=True)                                   # (argmax of 0/1: the first 1)
    return (tied & (k[None, None] > first) & ((k % QUAD)[None, None] < (first % QUAD))).any(dim=2)


def decode_clip_f64(anc, reg, H, W):
    """BBoxTransform + ClipBoxes in float64 on the fp32 inputs (the std constants are the reference's float32 0.1 / 0.2, widened)."""
    a, r = anc.double(), reg.double()
    s1, s2 = float(np.float32(0.1)), float(np.float32(0.2))
    w = a[:, :, 2] - a[:, :, 0]; h = a[:, :, 3] - a[:, :, 1]
    cx = a[:, :, 0] + 0.5 * w; cy = a[:, :, 1] + 0.5 * h
    pcx = cx + r[:, :, 0] * s1 * w; pcy = cy + r[:, :, 1] * s1 * h
    pw = torch.exp(r[:, :, 2] * s2) * w; ph = torch.exp(r[:, :, 3] * s2) * h
    return torch.stack([(pcx - 0.5 * pw).clamp(min=0), (pcy - 0.5 * ph).clamp(min=0),
                        (pcx + 0.5 * pw).clamp(max=W), (pcy + 0.5 * ph).clamp(max=H)], dim=2)


# --------------------------------------------------------------------------- 3. greedy NMS
THR = 0.05                                           # score threshold of every NMS case
COUNTS_N = (0, 1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097)
COUNTS_LOW_IOU = (2048, 2049, 4097)                  # also at IoU 0.3: the brute-force cross kernel only runs from round 1 on
DENSITY = 14.0                                       # side of the square the dense boxes fall into = DENSITY * sqrt(n) px


def _dense_boxes(g, n, extent):
    """n boxes with fractional corners, sides 24..48, top-left corners uniform in [0, extent)^2."""
    xy = torch.rand(n, 2, generator=g) * extent
    wh = 24.0 + torch.rand(n, 2, generator=g) * 24.0
    return torch.cat([xy, xy + wh], 1)


def _distinct_scores(g, n, hi=0.99, lo=0.06):
    """n distinct scores in [lo, hi] in random order (an even ladder: neighbours differ by far more than an fp32 ulp)."""
    return torch.linspace(hi, lo, n)[torch.randperm(n, generator=g)] if n else torch.zeros(0)


def _image(g, A, n):
    """One image: n candidates (distinct scores above THR, dense boxes) scattered over A slots; the others score <= THR -- one of
    them exactly THR, which `>` drops."""
    boxes = _dense_boxes(g, A, DENSITY * math.sqrt(max(n, 16)))
    score = torch.rand(A, generator=g) * 0.04
    slots = torch.randperm(A, generator=g)
    score[slots[:n]] = _distinct_scores(g, n)
    if n < A:
        score[slots[n]] = THR
    return boxes, score


def _nms_case(boxes, score, ious, seed):
    """-> the case dict; label is a non-trivial int32 tensor for gather_dets."""
    g = torch.Generator().manual_seed(seed)
    label = torch.randint(0, 91, score.shape, generator=g, dtype=torch.int32)
    return {'boxes': boxes.float().contiguous(), 'score': score.float().contiguous(), 'label': label, 'thr': THR, 'ious': tuple(ious)}


def counts(n):
    g = torch.Generator().manual_seed(3000 + n)
    boxes, score = _image(g, n + 9, n)
    return _nms_case(boxes[None], score[None], (0.5, 0.3) if n in COUNTS_LOW_IOU else (0.5,), n)


def all_survive_full_rounds():
    """A = 4096 = two full rounds, every slot a candidate, 4096 pairwise disjoint 10 x 10 boxes (pitch 12): S == RND in both rounds."""
    g = torch.Generator().manual_seed(41)
    i = torch.arange(4096)
    xy = torch.stack([(i % 64).float(), (i // 64).float()], 1) * 12.0 + 3.5
    return _nms_case(torch.cat([xy, xy + 10.0], 1)[None], _distinct_scores(g, 4096)[None], (0.5, 0.3), 41)


def all_identical():
    """2100 copies of one box: one kept; the 52 candidates of round 1 die in the cross phase."""
    g = torch.Generator().manual_seed(42)
    box = torch.tensor([100.25, 50.5, 164.75, 99.0])
    return _nms_case(box.repeat(2100, 1)[None], _distinct_scores(g, 2100)[None], (0.5, 0.3), 42)


OVF_IOU = 0.92
OVF_ANCHORS, OVF_FILLERS = 64, 2100


def overflow_single_suppressor():
    """64 kept 64 x 64 boxes (area 2^12) whose centres share one 32-px cell -> 56 of them live in the overflow list; 2100 disjoint
    fillers push the 64 copies (each anchor shifted by 1 px: IoU 0.969 with its anchor, <= 0.91 with every other) into round 1, where
    the only way to find a copy's single suppressor is the grid cell or -- for at least 56 of them -- the overflow scan.
    -> (case, group [A]: 0 anchor / 1 filler / 2 copy)."""
    g = torch.Generator().manual_seed(43)
    i = torch.arange(OVF_ANCHORS)
    ctr = torch.stack([994.0 + 4.0 * (i % 8).float(), 994.0 + 4.0 * (i // 8).float()], 1)
    anchors = torch.cat([ctr - 32.0, ctr + 32.0], 1)
    j = torch.arange(OVF_FILLERS)
    fxy = torch.stack([3000.0 + 12.0 * (j % 50).float(), 3000.0 + 12.0 * (j // 50).float()], 1)
    fillers = torch.cat([fxy, fxy + 10.0], 1)
    copies = anchors + torch.tensor([1.0, 0.0, 1.0, 0.0])
    boxes = torch.cat([anchors, fillers, copies])
    score = torch.cat([torch.linspace(0.99, 0.9, OVF_ANCHORS), torch.linspace(0.8, 0.5, OVF_FILLERS), torch.linspace(0.4, 0.3, OVF_ANCHORS)])
    group = torch.cat([torch.zeros(OVF_ANCHORS), torch.ones(OVF_FILLERS), torch.full((OVF_ANCHORS,), 2.0)]).long()
    p = torch.randperm(len(boxes), generator=g)
    return _nms_case(boxes[p][None], score[p][None], (OVF_IOU,), 43), group[p]


R4096_A, R4096_N = 65537, (9000, 4097)


@functools.lru_cache(maxsize=None)
def round4096():
    """A > 65536: rounds of 4096.  Image 0: 9000 candidates (three rounds), image 1: 4097 (a second round of one)."""
    g = torch.Generator().manual_seed(44)
    imgs = [_image(g, R4096_A, n) for n in R4096_N]
    return _nms_case(torch.stack([b for b, _ in imgs]), torch.stack([s for _, s in imgs]), (0.5,), 44)


def round4096_low_iou():
    """Image 0 of round4096 alone at IoU 0.3: the brute-force cross kernel at RND = 4096."""
    c = round4096()
    return {'boxes': c['boxes'][:1].contiguous(), 'score': c['score'][:1].contiguous(), 'label': c['label'][:1].contiguous(), 'thr': THR, 'ious': (0.3,)}


MIXED_A, MIXED_N = 5000, (5000, 0, 1, 2049, 300)


def batch_mixed_counts():
    """Images that finish in different rounds (3 / 0 / 1 / 2 / 1) in one call."""
    g = torch.Generator().manual_seed(45)
    imgs = [_image(g, MIXED_A, n) for n in MIXED_N]
    return _nms_case(torch.stack([b for b, _ in imgs]), torch.stack([s for _, s in imgs]), (0.5, 0.3), 45)


SMALL_N = {1: (1, 0), 7: (7, 3)}                     # A -> candidates of the two images


def small_A(A):
    g = torch.Generator().manual_seed(46 + A)
    imgs = [_image(g, A, n) for n in SMALL_N[A]]
    return _nms_case(torch.stack([b for b, _ in imgs]), torch.stack([s for _, s in imgs]), (0.5, 0.3), 46 + A)


NMS_CASES = {'counts_n%d' % n: functools.partial(counts, n) for n in COUNTS_N}
NMS_CASES.update({'all_survive_full_rounds': all_survive_full_rounds, 'all_identical': all_identical,
                  'overflow_single_suppressor': lambda: overflow_single_suppressor()[0], 'round4096': round4096,
                  'round4096_low_iou': round4096_low_iou, 'batch_mixed_counts': batch_mixed_counts})
NMS_CASES.update({'small_A%d' % a: functools.partial(small_A, a) for a in SMALL_N})


@functools.lru_cache(maxsize=None)
def nms_reference(name, iou):
    """-> per image the int64 keep list (anchor indices in keep order) by the oracle; computed once per (case, IoU)."""
    c = NMS_CASES[name]()
    return tuple(nms_ref(c['boxes'][b], c['score'][b], c['thr'], iou) for b in range(c['score'].shape[0]))


def sorted_candidates(score, thr=THR):
    """-> anchor indices of the candidates in the kernel's order: descending score, ties by index."""
    idx = torch.nonzero(score > thr).flatten()
    return idx[torch.argsort(-score[idx], stable=True)]


def iou_matrix(a, b):
    """IoU [len(a), len(b)] in the oracle's fp32 arithmetic (nms_greedy's, vectorised over both sides)."""
    a, b = a.numpy().astype(np.float32), b.numpy().astype(np.float32)
    aa = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]); ab = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    iw = np.maximum(np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0]), np.float32(0))
    ih = np.maximum(np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1]), np.float32(0))
    inter = iw * ih
    with np.errstate(divide='ignore', invalid='ignore'):
        return inter / (aa[:, None] + ab[None, :] - inter)


# the kept-box grid's filing rule (octave / inv_cell / cell_of of postprocess.hip; NOT its hash)
def octave(area):
    return min(max(math.frexp(float(area))[1] - 1, SB_MIN), SB_MAX)


def inv_cell(lvl):
    return 2.0 ** (1 - (lvl >> 1))


def cell_of(v, inv):
    return int(math.floor(float(np.float32(v) * np.float32(inv))))


def grid_cell(box):
    """-> (octave, cell x, cell y) a kept box is filed under."""
    x1, y1, x2, y2 = (np.float32(v) for v in box.tolist())
    lvl = octave((x2 - x1) * (y2 - y1))
    inv = inv_cell(lvl)
    return lvl, cell_of(np.float32(0.5) * (x1 + x2), inv), cell_of(np.float32(0.5) * (y1 + y2), inv)


# --------------------------------------------------------------------------- 4. finalize_dets
FIN_B, FIN_A = 6, 600
FIN_COUNT = (0, 1, 255, 256, 257, 600)
FIN_SCALE = (0.3, 1.0, 1.7, 2.5, 1.0 / 3.0, 0.8125)
FIN_MAX_DET = (1, 100, 256, 257, 1000)
FIN_TIE = 0.5                                        # the score that occurs three times in a row
FIN_RUN = {1: 0, 2: 10, 3: 97, 4: 254, 5: 300}       # image -> first row of its run of FIN_TIE (image 1: its only row IS the tie)
FIN_THRESHOLDS = {'below': 0.05, 'above': 0.95, 'tied': FIN_TIE}
FIN_STRIDE = 256                                     # threads of finalize_dets_kernel


@functools.lru_cache(maxsize=None)
def finalize_case():
    """-> dict(score [6, 600] descending per image over ALL 600 rows (0.9 .. 0.1: rows past `count` would pass the low threshold),
    label int64 0..90, boxes, count int32, scale fp32).  Image b's scores cross FIN_TIE at rows FIN_RUN[b] .. + 2."""
    g = torch.Generator().manual_seed(51)
    score = torch.empty(FIN_B, FIN_A)
    for b in range(FIN_B):
        p = FIN_RUN.get(b, 300)
        score[b, :p] = torch.linspace(0.9, 0.51, p) if p else torch.zeros(0)
        score[b, p:p + 3] = FIN_TIE
        score[b, p + 3:] = torch.linspace(0.49, 0.1, FIN_A - p - 3)
    xy = torch.rand(FIN_B, FIN_A, 2, generator=g) * 400.0
    wh = 1.0 + torch.rand(FIN_B, FIN_A, 2, generator=g) * 111.0
    return {'score': score, 'label': torch.randint(0, 91, (FIN_B, FIN_A), generator=g), 'boxes': torch.cat([xy, xy + wh], 2).contiguous(),
            'count': torch.tensor(FIN_COUNT, dtype=torch.int32), 'scale': torch.tensor(FIN_SCALE, dtype=torch.float32)}


def finalize_restated(score, label, boxes, count, scale, thr, max_det, xywh):
    """finalize_dets in NumPy -> (out [B, max_det, 6] fp32, out_count [B] int32): of the first min(count, max_det) rows the prefix with
    score > thr (xywh: >= thr, the `< threshold: break` of the reference's COCO writer), boxes / scale as a float32 true division,
    xywh: x2 -= x1, y2 -= y1; the other rows (0, 0, 0, 0, 0, -1)."""
    score, label, boxes = score.numpy(), label.numpy(), boxes.numpy()
    B = score.shape[0]
    out = np.zeros((B, max_det, 6), dtype=np.float32); out[:, :, 5] = -1.0
    oc = np.zeros(B, dtype=np.int32)
    t = np.float32(thr)
    for b in range(B):
        n = min(int(count[b]), max_det)
        s = score[b, :n]
        ok = (s >= t) if xywh else (s > t)
        keep = int(ok.sum())
        assert bool(ok[:keep].all())                                                   # descending scores: the kept set is a prefix
        bx = boxes[b, :keep] / np.float32(scale[b])
        assert bx.dtype == np.float32
        if xywh:
            bx[:, 2] -= bx[:, 0]; bx[:, 3] -= bx[:, 1]
        out[b, :keep, :4] = bx; out[b, :keep, 4] = s[:keep]; out[b, :keep, 5] = label[b, :keep].astype(np.float32)
        oc[b] = keep
    return out, oc


# --------------------------------------------------------------------------- 5. head_out_bwd
HOB_SHAPES = [(1, 1), (3, 5), (4, 4), (5, 3), (1023, 1025), (1024, 1024), (1025, 1023), (4 * 256 * 3 + 2, 4 * 256 + 1)]
HOB_WG = 256                                         # threads per workgroup, one 4-element group each
BF16_TIES = (1.00390625, 1.01171875, -1.00390625, 3.0517578125e-05 * 1.00390625)      # halfway between two bf16 values: even wins


@functools.lru_cache(maxsize=None)
def head_out_bwd_case(ncls, nreg):
    """-> dict(dprob [ncls], prob [ncls], dreg [nreg], marks {name: class index}) fp32.  prob is a sigmoid of randn * 3 with an exact
    0 (first lane of the first vector group, or of the tail) and an exact 1 (the last element: the scalar tail when ncls % 4);
    dprob has a NaN lane, an Inf lane, a -Inf lane and an Inf where prob == 0 (-> NaN) as far as ncls has room; dreg carries values
    that lie exactly between two bf16 neighbours."""
    g = torch.Generator().manual_seed(6000 + 7 * ncls + nreg)
    prob = torch.sigmoid(torch.randn(ncls, generator=g) * 3.0)
    dprob = torch.randn(ncls, generator=g) * torch.exp(torch.randn(ncls, generator=g) * 3.0)
    dreg = torch.randn(nreg, generator=g) * torch.exp(torch.randn(nreg, generator=g) * 3.0)
    marks = {}
    if ncls >= 3:
        prob[0] = 0.0; marks['zero'] = 0
        prob[ncls - 1] = 1.0; marks['one'] = ncls - 1
        dprob[1] = float('nan'); marks['nan'] = 1
    elif ncls == 1:
        prob[0] = 1.0; marks['one'] = 0
    if ncls >= 4:
        dprob[2] = float('inf'); marks['inf'] = 2
    if ncls >= 8:
        prob[4] = 0.0; dprob[4] = float('inf'); marks['inf_times_zero'] = 4
        dprob[ncls - 2] = -float('inf'); marks['-inf'] = ncls - 2
    for k, v in enumerate(BF16_TIES[:max(0, nreg - 1)]):
        dreg[k + 1] = v
    if nreg >= 8:
        dreg[nreg - 1] = BF16_TIES[1]
    return {'dprob': dprob, 'prob': prob, 'dreg': dreg, 'marks': marks}


def head_out_bwd_reference(case, dtype):
    """torch's own fp32 (dprob * prob) * (1 - prob) -- no product feeds an add, so there is nothing to contract -- and dreg, both
    rounded to `dtype` by torch."""
    dl = (case['dprob'] * case['prob']) * (1.0 - case['prob'])
    return dl.to(dtype), case['dreg'].to(dtype)
