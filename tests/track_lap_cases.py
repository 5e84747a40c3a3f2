"""Seeded multi-frame scenes for the tracker with assignment='optimal' (include/effdet_assign.h), in the form of tests/track_cases.py: a
dict with name, options, dets [F, B, max_det, 6], counts [F, B], resets, tags.  Most scenes are built from one piece of geometry, the
PAIR: two objects that stand still for some frames (their tracks settle on them exactly, the Kalman innovation being zero), then both
detections move at once to where a crossing would put them.  With boxes of 40 x 80 on one horizontal line and centres, relative to
the pair's origin, at
    track 1: -8,  detection 0: 0,  track 0: 5,  detection 1: 13
the plain IoUs on the frame of the move are  [[0.778, 0.667], [0.667, 0.311]]  (track x detection): the structure of the header's
example.  (1 - IoU is a metric, so the fourth number cannot be much smaller while the other three stay this large.)  With a gate g
between 0.311 and 0.667 + 0.667 - 0.778 = 0.556 the greedy rule takes (0, 0) and strands track 1 and detection 1 -- a track lost and a
new id started -- while the optimum is (0, 1), (1, 0), better by 0.556 - g.  The scenes use g = 0.43 (0.5 in the second association).
IoU does not depend on scale, so the cap scene uses the pair at half size.

EPS_SIM is the recorded float32 error of the rule on these scenes, as in tests/track_cases.py: the largest |float32 - float64| over every
similarity and every Kalman mean (pixels); tests/test_track_lap_host.py measures it again.  The GPU tier's tolerance is 8 * EPS_SIM."""
import numpy as np

from tests.track_restated import Options
from tests.track_cases import _Seq, _box

EPS_SIM = 2e-5                     # measured 1.57e-5 (agree: a centre near 350 px, where one fp32 ulp is 3.1e-5)

T0, T1, D0, D1 = (5.0, 0.0), (-8.0, 0.0), (0.0, 0.0), (13.0, 0.0)
GATE = 0.43


def _pair(cx, cy, moved, scores=(0.9, 0.8), labels=(1, 2), scale=1.0):
    """the pair's two rows before (moved False) or after the move"""
    a, b = (D0, D1) if moved else (T0, T1)
    return [_box(cx + scale * a[0], cy + scale * a[1], 40 * scale, 80 * scale, scores[0], labels[0]),
            _box(cx + scale * b[0], cy + scale * b[1], 40 * scale, 80 * scale, scores[1], labels[1])]


def crossing():
    """The pair: five still frames, the move on frame 6, four frames after it."""
    s = _Seq('crossing', 10, 1, 4, Options(max_tracks=8, match_sim=GATE, fuse_score=False), ('differs', 'first_association'))
    for f in range(10):
        s.put(f, 0, _pair(200, 200, f >= 5))
    return s.case


def three_cross():
    """Three paths crossing at once, the pair's idea one link longer.  On one line (boxes 40 x 80): track c at -7, detection 0 at 0,
    track a at 5, detection 1 at 12, track b at 18, detection 2 at 25.  Neighbours overlap by 0.702 / 0.778 / 0.702 / 0.739 / 0.702,
    everything further apart is below the gate.  Greedy takes (a, 0) and (b, 1) and strands track c and detection 2; the optimum
    moves all three: (c, 0), (a, 1), (b, 2)."""
    s = _Seq('three_cross', 10, 1, 6, Options(max_tracks=8, match_sim=GATE, fuse_score=False), ('differs', 'first_association'))
    for f in range(10):
        xs = (0.0, 12.0, 25.0) if f >= 5 else (5.0, 18.0, -7.0)
        s.put(f, 0, [_box(200 + x, 200, 40, 80, sc, lb) for x, sc, lb in zip(xs, (0.9, 0.85, 0.8), (1, 2, 0))])
    return s.case


def crowd6():
    """Six objects close together stand still for five frames, then every detection moves towards ANOTHER object's place (a cyclic
    shift plus noise), scores fused: a seeded crowd in which the two rules part."""
    n = 6
    s = _Seq('crowd6', 10, 1, 2 * n, Options(max_tracks=16, match_sim=GATE), ('differs', 'first_association'), seed=39)
    rng = s.rng
    P = np.stack([200 + rng.uniform(-16, 16, n), 200 + rng.uniform(-26, 26, n)], axis=1)
    Q = np.roll(P, 1, axis=0) * 0.55 + P * 0.45 + np.stack([rng.uniform(-3, 3, n), rng.uniform(-5, 5, n)], axis=1)
    score = np.sort(rng.uniform(0.7, 0.95, n))[::-1]
    for f in range(10):
        at = Q if f >= 5 else P
        s.put(f, 0, [_box(at[i, 0], at[i, 1], 40, 80, score[i], i % 3) for i in range(n)])
    return s.case


def crowd():
    """Two pairs.  Pair A is confirmed; on frame 7 it moves AND its scores dip into the low band: the second association (plain IoU,
    gate 0.5) decides.  Pair B first appears on frame 6, so on frame 7, when it moves, its tracks are unconfirmed: the third
    association (gate 0.43, fused with scores 0.95 / 0.9: 0.739, 0.600 / 0.633, 0.280) decides.  The first association of that frame sees only pairs 200 px apart."""
    s = _Seq('crowd', 11, 1, 8, Options(max_tracks=8, unconfirmed_sim=GATE), ('differs', 'second_association', 'third_association'))
    for f in range(11):
        s.put(f, 0, _pair(100, 120, f >= 6, scores=(0.3, 0.35) if f == 6 else (0.9, 0.8)))
        if f >= 5:
            s.put(f, 0, _pair(320, 330, f >= 6, scores=(0.95, 0.9), labels=(3, 4)))
    return s.case


def _classes(name, aware):
    """After the move detection 0 carries track 1's label and detection 1 track 0's: with class_aware only the crossed pairs are
    allowed (both rules take them); without, greedy takes (0, 0)."""
    s = _Seq(name, 10, 1, 4, Options(max_tracks=8, match_sim=GATE, fuse_score=False, class_aware=aware), ('class_aware_on',) if aware else ('differs', 'class_aware_off'))
    for f in range(10):
        s.put(f, 0, _pair(200, 200, f >= 5, labels=(2, 1) if f >= 5 else (1, 2)))
    return s.case


def classes_on():
    return _classes('classes_on', True)


def classes_off():
    return _classes('classes_off', False)


def _fuse(name, on):
    """Scores 0.95 and 0.7 after the move: fused, the four similarities are 0.739, 0.467 / 0.633, 0.218 and (0, 0) alone is the
    optimum too (0.309 against 0.240); on the plain IoUs the rules part."""
    s = _Seq(name, 10, 1, 4, Options(max_tracks=8, match_sim=GATE, fuse_score=on), ('fuse_on',) if on else ('differs', 'fuse_off'))
    for f in range(10):
        s.put(f, 0, _pair(200, 200, f >= 5, scores=(0.95, 0.7)))
    return s.case


def fuse_on():
    return _fuse('fuse_on', True)


def fuse_off():
    return _fuse('fuse_off', False)


def refound():
    """Object 1 is not detected on frames 5-7 (its track is lost); on frame 8 both detections are where the move puts them.  Greedy
    gives detection 0 to track 0 and starts a new id for detection 1; the optimum re-finds the lost track."""
    s = _Seq('refound', 12, 1, 4, Options(max_tracks=8, match_sim=GATE, fuse_score=False), ('differs', 'refound'))
    for f in range(12):
        rows = _pair(200, 200, f >= 7)
        s.put(f, 0, rows[:1] if 4 <= f <= 6 else rows)
    return s.case


def cap():
    """The caps: 256 slots, 128 rows -- 64 half-size pairs on an 8 x 8 grid, far apart, so every association falls into components of
    at most two rows and two columns.  Two still frames, the move on the third."""
    s = _Seq('cap', 3, 1, 128, Options(max_tracks=256, match_sim=GATE, fuse_score=False), ('differs', 'cap'), seed=21)
    score = 0.65 + 0.3 * s.rng.permutation(128) / 128.0
    for f in range(3):
        for k in range(64):
            s.put(f, 0, _pair(32 + 64 * (k % 8), 34 + 64 * (k // 8), f >= 2, scores=(score[2 * k], score[2 * k + 1]), labels=(k % 5, k % 3), scale=0.5))
    return s.case


def agree():
    """Two objects far apart on straight paths: both rules agree on every frame."""
    s = _Seq('agree', 10, 1, 4, Options(max_tracks=8), ('agrees',), seed=22)
    for f in range(10):
        s.put(f, 0, [_box(100 + 4 * f + s.jitter(), 150 + s.jitter(), 50, 90, 0.9, 1), _box(350 + s.jitter(), 300 - 3 * f + s.jitter(), 70, 60, 0.8, 2)])
    return s.case


BUILDERS = (crossing, three_cross, crowd6, crowd, classes_on, classes_off, fuse_on, fuse_off, refound, cap, agree)
NAMES = tuple(b.__name__ for b in BUILDERS)
_CACHE = {}


def case(name):
    if name not in _CACHE:
        _CACHE[name] = {b.__name__: b for b in BUILDERS}[name]()
    return _CACHE[name]
