"""Seeded inputs of the weighted-boxes-fusion tests at the smallest sizes where the kernel can still go wrong.  The kernel runs one
1024-thread workgroup per image and a thread owns the clusters tid, tid + 1024, ..: 63 / 64 / 65 candidates straddle a wave, 1023 /
1024 / 1025 the workgroup, the all-singleton case and the 4096 one give a thread a second (third, fourth) cluster.  Boxes lie in a
512-pixel frame; a later view mostly holds jittered copies of view 0's boxes (what a mirror view or a second detector produces), so
clusters of several members are the rule.  Every view carries DECOY rows past its count (score 0.999): a kernel that read them would
emit them.

A case is a dict: name, views [(score [B,A_v] f32, label [B,A_v] int64, boxes [B,A_v,4] f32, count [B] int32)], weights, flips (per
view None or a width), muls, iou_thr, skip_thr, top_n, n (candidate rows of the largest image)."""
import numpy as np

EXTENT = 512.0


def _boxes(rng, n, extent=EXTENT, lo=8.0, hi=98.0):
    xy = rng.uniform(0, extent - hi, size=(n, 2))
    wh = rng.uniform(lo, hi, size=(n, 2))
    return np.concatenate([xy, xy + wh], 1).astype(np.float32)


def _jitter(rng, boxes, px=2.0):
    return (boxes + rng.uniform(-px, px, size=boxes.shape)).astype(np.float32)


def _scores(rng, n):
    return np.sort(rng.permutation(np.linspace(0.06, 0.999, max(2 * n, 1)))[:n])[::-1].astype(np.float32)      # distinct, descending


def _image(rng, boxes, score, label, pad):
    """One image's rows of a view: the given rows, then `pad` decoys."""
    n = len(score)
    b = np.concatenate([np.asarray(boxes, np.float32).reshape(n, 4), _boxes(rng, pad)])
    s = np.concatenate([np.asarray(score, np.float32), np.full(pad, 0.999, np.float32)])
    l = np.concatenate([np.asarray(label, np.int64), np.zeros(pad, np.int64)])
    return s, l, b, n


def _view(images, A=None):
    """[(s, l, b, n) per image] -> the view's batch arrays, padded to A rows with decoys' zeros."""
    A = A or max(len(s) for s, _, _, _ in images)
    B = len(images)
    S = np.zeros((B, A), np.float32); Lb = np.zeros((B, A), np.int64); Bx = np.zeros((B, A, 4), np.float32)
    for i, (s, l, b, _) in enumerate(images):
        S[i, :len(s)] = s; Lb[i, :len(s)] = l; Bx[i, :len(s)] = b
    return S, Lb, Bx, np.array([n for _, _, _, n in images], np.int32)


def _case(name, views, top_n=1000, weights=None, flips=None, muls=None, iou_thr=0.55, skip_thr=0.0):
    V = len(views)
    n = int(max(sum(min(int(v[3][b]), top_n) for v in views) for b in range(len(views[0][3]))))
    return dict(name=name, views=views, weights=weights or [1.0] * V, flips=flips or [None] * V, muls=muls or [1.0] * V,
                iou_thr=iou_thr, skip_thr=skip_thr, top_n=top_n, n=n)


def _copies(rng, base, labels, counts, pad=5, px=2.0):
    """Views of one image: view 0 holds `base`'s first counts[0] rows; a later view holds counts[v] rows under fresh scores, every
    other one a jittered copy of a row of `base` (label kept), the rest boxes of its own."""
    out = []
    for v, n in enumerate(counts):
        b, l = base[:n].copy(), labels[:n].copy()
        if v:
            b = _jitter(rng, b, px)
            b[1::2] = _boxes(rng, len(b[1::2])); l[1::2] = rng.integers(0, 4, size=len(l[1::2]))
            p = rng.permutation(n)
            b, l = b[p], l[p]
        out.append(_image(rng, b, _scores(rng, n), l, pad))
    return out


def _random(name, seed, counts, top_n=1000, pad=5, **kw):
    rng = np.random.default_rng(seed)
    m = max(max(counts), 1)
    return _case(name, [_view([im]) for im in _copies(rng, _boxes(rng, m), rng.integers(0, 4, size=m), counts, pad)], top_n, **kw)


def make_cases():
    cases = []
    for n in (0, 1, 2, 63, 64, 65, 1023, 1024, 1025):                      # candidate totals, split over two views
        cases.append(_random('n%d' % n, 100 + n, [(n + 1) // 2, n // 2]))
    cases.append(_random('n4096_v4', 1, [1024] * 4, top_n=1024, pad=0))     # the cap exactly; A_v == top_n == count
    cases.append(_random('count_exceeds_top_n', 2, [80, 30], top_n=50))     # view 0 is cut to its first 50 rows BEFORE the merge
    cases.append(_random('v1_n300', 3, [300]))
    cases.append(_random('v3', 4, [100, 90, 110], weights=[1.0, 0.7, 1.3]))
    cases.append(_random('v8_top512', 5, [40, 35, 30, 25, 20, 15, 10, 5], top_n=512))
    # all singletons: 1100 boxes of 8 x 8 in the cells of a 14-pixel grid -- clusters = candidates, 1100 > 1024 of them
    rng = np.random.default_rng(6)
    g = rng.permutation(36 * 36)[:1100]
    xy = np.stack([g % 36, g // 36], 1).astype(np.float32) * 14.0 + 3.0
    grid = np.concatenate([xy, xy + 8.0], 1)
    lab = rng.integers(0, 4, size=1100)
    cases.append(_case('all_singletons_1100', [_view([_image(rng, grid[:550], _scores(rng, 550), lab[:550], 5)]),
                                               _view([_image(rng, grid[550:], _scores(rng, 550), lab[550:], 5)])]))
    # one cluster of 300 identical boxes over two views (cnt > V: the min(cnt, V) clamp) beside ordinary rows
    rng = np.random.default_rng(7)
    one = np.tile(np.array([[100.0, 120.0, 180.0, 220.0]], np.float32), (150, 1))
    other = _boxes(rng, 20)
    other[:, [0, 2]] = other[:, [0, 2]] * 0.25 + 300.0                      # (away from the cluster)
    views = []
    for v in range(2):
        s = _scores(rng, 170)
        views.append(_view([_image(rng, np.concatenate([one, other]), s, np.concatenate([np.full(150, 2), rng.integers(0, 4, size=20)]), 5)]))
    cases.append(_case('one_cluster_of_300_identical', views))
    # identical boxes under four labels in two views: a box fuses with its own label's copy only
    rng = np.random.default_rng(8)
    b = np.repeat(_boxes(rng, 40), 4, axis=0)
    l = np.tile(np.arange(4), 40)
    cases.append(_case('identical_boxes_different_labels', [_view([_image(rng, b, _scores(rng, 160), l, 5)]) for _ in range(2)]))
    # equal conf across views and rows (16 score levels): the order is by view, then row
    rng = np.random.default_rng(9)
    base = _boxes(rng, 120); lab = rng.integers(0, 3, size=120)
    views = []
    for v in range(3):
        s = np.sort(np.floor(rng.uniform(0, 1, 120) * 16 + 1) / 16)[::-1].astype(np.float32)
        views.append(_view([_image(rng, _jitter(rng, base) if v else base, s, lab, 5)]))
    cases.append(_case('equal_conf_across_views', views))
    # a candidate mirror-symmetric between two same-label clusters on power-of-two coordinates: the two IoUs (128 / 640) are bitwise
    # equal, cluster 0 must win -- against cluster 100, which another WAVE owns; fillers far below keep the cluster indices apart
    fill = np.stack([np.arange(99) * 4.0, np.full(99, 64.0), np.arange(99) * 4.0 + 2.0, np.full(99, 66.0)], 1)
    b = np.concatenate([[[0, 0, 16, 16]], fill, [[32, 0, 48, 16]], [[8, 0, 40, 16]]]).astype(np.float32)
    s = np.concatenate([[0.96875], np.linspace(0.9, 0.5, 99), [0.25], [0.125]]).astype(np.float32)
    rng = np.random.default_rng(10)
    cases.append(_case('mirror_symmetric_tie', [_view([_image(rng, b, s, np.zeros(102), 3)])], iou_thr=0.125))
    # transforms: view 1 is stored mirrored about 512, view 2 at half scale; A_v differ
    rng = np.random.default_rng(11)
    base = _boxes(rng, 150); lab = rng.integers(0, 4, size=150)
    v0 = _image(rng, base[:120], _scores(rng, 120), lab[:120], 0)
    j1 = _jitter(rng, base[:77])
    v1 = _image(rng, np.stack([512.0 - j1[:, 2], j1[:, 1], 512.0 - j1[:, 0], j1[:, 3]], 1), _scores(rng, 77), lab[:77], 0)
    v2 = _image(rng, _jitter(rng, base) * 0.5, _scores(rng, 150), lab, 50)
    cases.append(_case('flip_mul_unequal_A', [_view([v0]), _view([v1]), _view([v2])], weights=[2.0, 1.0, 0.5], flips=[None, 512.0, None],
                       muls=[1.0, 1.0, 2.0]))
    # B = 3: different counts per image and view, image 1 empty in both views, image 2 empty in view 1
    rng = np.random.default_rng(12)
    ims = [_copies(rng, _boxes(rng, 200), rng.integers(0, 4, size=200), c) for c in ([200, 150], [0, 0], [37, 0])]
    cases.append(_case('batch3_one_empty', [_view([im[v] for im in ims]) for v in range(2)]))
    # NaN scores, zero-area, inverted, infinite and NaN boxes among ordinary rows; a score below, at and above skip_thr
    rng = np.random.default_rng(13)
    base = _boxes(rng, 90); lab = rng.integers(0, 2, size=90)
    views = []
    for v in range(2):
        s, l, b, n = _image(rng, _jitter(rng, base) if v else base.copy(), _scores(rng, 90), lab, 5)
        b[3, 2:] = b[3, :2]                                                 # zero area
        b[5, 2] = b[5, 0]                                                   # zero width
        b[7, 2] = b[7, 0] - 5.0                                             # inverted in x: negative area
        b[9, 2:] = b[9, :2] - 5.0                                           # inverted in x and y: positive product, overlaps nothing
        b[11, 2] = np.inf; b[13] = np.nan; b[15] = [0.0, 0.0, 3.0e19, 3.0e19]
        s[17] = np.nan; s[19] = np.inf; s[21] = -1.0; s[23] = 0.0
        s[80:90] = [0.2501, 0.25, 0.25, 0.2499, 0.2, 0.1, 0.09, 0.08, 0.07, 0.06]
        views.append(_view([(s, l, b, n)]))
    cases.append(_case('degenerate_nan_and_skip_thr', views, skip_thr=0.25))
    return cases


CASES = make_cases()
