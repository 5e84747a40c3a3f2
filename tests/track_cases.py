"""Seeded builders of short synthetic sequences for the tracker (include/effdet_track.h): boxes in a 512 x 512 frame, B <= 3 streams,
8-16 slots, at most 12 detections a frame, 6-40 frames -- and one case at the caps (256 slots, 128 valid rows, two frames).  A case is
a dict: name, options (tests/track_restated.Options), dets [F, B, max_det, 6] float32 (x1, y1, x2, y2, score, label; score-descending
rows are NOT required by the tracker and not kept here), counts [F, B] int32, resets {frame: streams reset before it}, tie (the case
holds a deliberate exact tie), tags (what tests/test_track_host.py proves the case reaches).

EPS_SIM is the recorded float32 error of the rule itself: the largest |float32 - float64| over every similarity and every Kalman mean
(pixels) of every case, both run through the restatement (tests/test_track_host.py measures it again and holds it to this record).  The
GPU tier's tolerance is 8 * EPS_SIM and every float64 decision of every case clears its alternative by 16 * EPS_SIM.

EPS_COV is the same record for the stored covariance numbers: the largest RELATIVE |float32 - float64| over the 12 covariance numbers
of every slot in every case's final state (a number that is exactly 0 in float64 is exactly 0 in float32).  The GPU tier holds the
stored covariances to 8 * EPS_COV relative."""
import numpy as np

from tests.track_restated import Options

EPS_COV = 2.5e-6                   # measured 2.16e-6 (resets)
EPS_SIM = 5e-5                     # measured 4.52e-5 (gap_short: a centre near 400 px, where one fp32 ulp is 3.1e-5)


def _box(cx, cy, w, h, score, label=0.0):
    return [cx - w / 2.0, cy - h / 2.0, cx + w / 2.0, cy + h / 2.0, score, label]


class _Seq:
    def __init__(self, name, F, B, max_det, options, tags, tie=False, seed=0):
        self.case = dict(name=name, options=options, dets=np.zeros((F, B, max_det, 6), dtype=np.float32),
                         counts=np.zeros((F, B), dtype=np.int32), resets={}, tie=tie, tags=tuple(tags))
        self.case['dets'][..., 5] = -1.0                                           # finalize_dets' padding rows
        self.rng = np.random.RandomState(seed)

    def put(self, f, b, rows):
        d, c = self.case['dets'], self.case['counts']
        for r in rows:
            d[f, b, c[f, b]] = r
            c[f, b] += 1

    def jitter(self, sigma=0.4):
        return self.rng.uniform(-sigma, sigma)


def crossing():
    """Two objects on crossing constant-velocity paths (they overlap around frame 15); stream 1 never has a detection."""
    s = _Seq('crossing', 30, 2, 8, Options(max_tracks=8), ('ids_survive', 'never_a_detection', 'frame1'), seed=1)
    for f in range(30):
        s.put(f, 0, [_box(100 + 10 * f + s.jitter(), 250 + s.jitter(), 40, 80, 0.9, 1),
                     _box(400 - 10 * f + s.jitter(), 260 + f + s.jitter(), 50, 70, 0.8, 2)])
    return s.case


def gap_short():
    """A detection missing for 5 frames (< track_buffer): lost, then back with its id and tracklet_len 0.  Stream 1: a lone low detection."""
    s = _Seq('gap_short', 16, 2, 4, Options(max_tracks=8), ('refound', 'lone_low'), seed=2)
    for f in range(16):
        if not 6 <= f <= 10:
            s.put(f, 0, [_box(150 + 3 * f + s.jitter(), 200 + s.jitter(), 60, 90, 0.85, 3)])
        s.put(f, 0, [_box(400, 400, 50, 50, 0.7, 1)])
        s.put(f, 1, [_box(300, 300, 50, 50, 0.3, 1)])
    return s.case


def gap_long():
    """A detection missing for 8 frames with track_buffer 5: removed, and the returning object gets a new id."""
    s = _Seq('gap_long', 20, 1, 4, Options(max_tracks=8, track_buffer=5), ('removed_new_id',), seed=3)
    for f in range(20):
        if not 5 <= f <= 12:
            s.put(f, 0, [_box(150 + s.jitter(), 200 + s.jitter(), 60, 90, 0.85, 3)])
        s.put(f, 0, [_box(400, 100, 50, 50, 0.7, 1)])
    return s.case


def dip():
    """A score dipping between low_thr and track_thr for three frames: kept by the second association.  Two objects dip together, so
    that association has two picks; a third dips below low_thr and is ignored."""
    s = _Seq('dip', 12, 1, 6, Options(max_tracks=8), ('second_association',), seed=4)
    for f in range(12):
        low = 5 <= f <= 7
        s.put(f, 0, [_box(120 + 4 * f + s.jitter(), 150 + s.jitter(), 50, 100, 0.3 if low else 0.9, 1),
                     _box(350 + s.jitter(), 350 - 3 * f + s.jitter(), 80, 60, 0.25 if low else 0.75, 2),
                     _box(100, 420, 40, 40, 0.05 if low else 0.8, 2)])
    return s.case


def false_positive():
    """A one-frame false positive on frame 4: unconfirmed for a frame, never output, removed.  Two objects appear together on frame 6
    and stay: the third association has two picks."""
    s = _Seq('false_positive', 10, 1, 6, Options(max_tracks=8), ('false_positive', 'third_association'), seed=5)
    for f in range(10):
        s.put(f, 0, [_box(200 + s.jitter(), 200 + s.jitter(), 70, 70, 0.9, 0)])
        if f == 3:
            s.put(f, 0, [_box(420, 80, 40, 60, 0.7, 5)])
        if f >= 5:
            s.put(f, 0, [_box(80 + s.jitter(), 400, 50, 60, 0.8, 1), _box(400 + s.jitter(), 400, 60, 50, 0.7, 2)])
    return s.case


def overflow():
    """12 new detections for 8 slots: the last four rows are dropped every frame (overflow counts them); one object vanishes, its slot
    is freed after track_buffer = 2 frames and the first of the dropped rows takes it."""
    s = _Seq('overflow', 9, 1, 12, Options(max_tracks=8, track_buffer=2), ('overflow', 'slot_reused'), seed=6)
    for f in range(9):
        rows = [_box(40 + 80 * (i % 6), 100 + 200 * (i // 6), 50, 80, 0.95 - 0.02 * i, i % 3) for i in range(12)]
        if f >= 2:
            del rows[2]
        s.put(f, 0, rows)
    return s.case


def _classes(name, aware):
    s = _Seq(name, 8, 1, 4, Options(max_tracks=8, class_aware=aware), ('class_aware_on' if aware else 'class_aware_off',), seed=7)
    for f in range(8):
        if f < 4:
            s.put(f, 0, [_box(200, 200, 80, 80, 0.9, 1)])
        else:                                                                      # another class stands where the track was; the track's
            s.put(f, 0, [_box(200, 200, 80, 80, 0.9, 2), _box(230, 200, 80, 80, 0.85, 1)])      # own class next to it (IoU 0.45)
    return s.case


def classes_on():
    """Overlapping boxes with different labels, class_aware: the track follows its own class."""
    return _classes('classes_on', True)


def classes_off():
    """The same rows without class_aware: the track takes the better-overlapping box of the other class."""
    return _classes('classes_off', False)


def _fuse(name, on):
    s = _Seq(name, 6, 1, 4, Options(max_tracks=8, fuse_score=on), ('fuse_on' if on else 'fuse_off',), seed=8)
    for f in range(6):
        if f < 3:
            s.put(f, 0, [_box(250, 250, 80, 80, 0.9, 1)])
        else:                                                                      # IoU 0.905 at score 0.55 against IoU 0.67 at score 0.95
            s.put(f, 0, [_box(250 + 4 * (f - 2), 250, 80, 80, 0.55, 1), _box(250 - 16 * (f - 2), 250, 80, 80, 0.95, 1)])
    return s.case


def fuse_on():
    """fuse_score flips a greedy pick: the better-scoring, worse-overlapping detection wins."""
    return _fuse('fuse_on', True)


def fuse_off():
    """The same rows on plain IoU: the better-overlapping detection wins."""
    return _fuse('fuse_off', False)


def _duplicate(name, a_start, b_start, tag):
    """Object A walks at constant velocity across the place where object B was last seen (B is lost there): on the frame it stands
    exactly there, the two are a tracked / lost pair above IoU 0.85."""
    s = _Seq(name, 24, 1, 4, Options(max_tracks=8), (tag,), seed=9)
    for f in range(24):
        if f >= a_start:
            s.put(f, 0, [_box(160 + 12 * (f - a_start), 300, 60, 60, 0.9, 1)])
        if b_start <= f < 8:
            s.put(f, 0, [_box(308, 300, 60, 60, 0.8, 1)])         # (4 px beside A's path: A's own track stays the better match)
    return s.case


def duplicate_tracked_older():
    return _duplicate('duplicate_tracked_older', 0, 3, 'dup_lost_removed')


def duplicate_tracked_younger():
    return _duplicate('duplicate_tracked_younger', 3, 0, 'dup_tracked_removed')


def duplicate_equal_age():
    return _duplicate('duplicate_equal_age', 0, 0, 'dup_equal_age')


def tie():
    """Bit-identical detection rows: two tracks with equal states, every pair of the next frames an exact tie -- the lower row goes to
    the lower slot.  Some frames are empty."""
    s = _Seq('tie', 8, 1, 4, Options(max_tracks=8), ('tie', 'empty_frames'), tie=True, seed=10)
    for f in range(8):
        if f not in (3, 6):
            s.put(f, 0, [_box(200, 220, 64, 96, 0.875, 1)] * 2)
    return s.case


def resets():
    """Three streams with the same moving object; stream 0 is reset before frame 5, stream 2 before frame 9."""
    s = _Seq('resets', 12, 3, 4, Options(max_tracks=8), ('reset_mask',), seed=11)
    for f in range(12):
        for b in range(3):
            s.put(f, b, [_box(100 + 6 * f + 20 * b, 150 + 30 * b, 60, 80, 0.9 - 0.05 * b, b),
                         _box(380, 380 - 5 * f, 70, 50, 0.75, 4)])
    s.case['resets'] = {5: (0,), 9: (2,)}
    return s.case


def skipped():
    """Rows the tracker must skip between valid ones: a NaN coordinate, an infinite one, inverted and empty boxes, a NaN score."""
    s = _Seq('skipped', 6, 1, 8, Options(max_tracks=8), ('skipped_rows',), seed=12)
    nan, inf = float('nan'), float('inf')
    for f in range(6):
        s.put(f, 0, [[nan, 10, 50, 60, 0.9, 1], _box(150 + 5 * f, 150, 60, 60, 0.9, 1), [300, 300, 250, 360, 0.9, 1],
                     [300, 300, 360, 300, 0.9, 1], [10, 10, inf, 60, 0.9, 1], _box(350, 150 + 5 * f, 60, 60, 0.8, 2),
                     [400, 400, 450, 450, nan, 1]])
    return s.case


def cap():
    """The caps: 256 slots, 128 valid rows, two frames.  Frame 1 starts 128 tracks; on frame 2 the even rows follow their objects (64
    picks in one association) and the odd rows are new objects elsewhere (64 unconfirmed tracks, 64 tracks lost)."""
    s = _Seq('cap', 2, 1, 128, Options(max_tracks=256), ('cap',), seed=13)
    score = 0.65 + 0.3 * s.rng.permutation(128) / 128.0
    for f in range(2):
        rows = []
        for i in range(128):
            cx, cy = 16 + 32 * (i % 16), 28 + 60 * (i // 16)
            if f == 1:
                cx, cy = (cx + 1, cy + 1) if i % 2 == 0 else (cx, cy + 30)
            rows.append(_box(cx, cy, 24, 40 if f == 0 or i % 2 == 0 else 16, score[i], i % 5))
        s.put(f, 0, rows)
    return s.case


BUILDERS = (crossing, gap_short, gap_long, dip, false_positive, overflow, classes_on, classes_off, fuse_on, fuse_off,
            duplicate_tracked_older, duplicate_tracked_younger, duplicate_equal_age, tie, resets, skipped, cap)
_CACHE = {}


def case(name):
    if name not in _CACHE:
        _CACHE[name] = {b.__name__: b for b in BUILDERS}[name]()
    return _CACHE[name]


NAMES = tuple(b.__name__ for b in BUILDERS)
