"""CPU tier of the detector wrappers (evaluate.EnsembleDetector / SlicedDetector / TrackedDetector) and of the options classes of
ops.py: what the shared bases must keep.  Stub models only (num_classes, f32_arith, forward_raw, eval, train, parameters); nothing is
launched."""
import re

import pytest

from efficientdet.pytorch_amd import evaluate as E
from efficientdet.pytorch_amd import ops


class Stub:
    """What the wrappers ask of an EfficientDet before any launch."""

    def __init__(self, name, num_classes=3, f32_arith='f32'):
        self.name, self.num_classes, self.f32_arith = name, num_classes, f32_arith
        self.calls = []
        self.params = [object()]

    def forward_raw(self, images):
        raise AssertionError('the host tier launches nothing')

    def eval(self):
        self.calls.append('eval')
        return self

    def train(self, mode=True):
        self.calls.append(('train', mode))
        return self

    def parameters(self):
        return iter(self.params)

    def __repr__(self):
        return 'Stub(%s)' % self.name


def _f16x3_name():
    names = [k for k, v in ops.MODEL_ARITH.items() if v[2] == 'f16x3']
    assert names, 'MODEL_ARITH names no f16x3 arithmetic'
    return names[0]


def _compositions():
    a, b, c = Stub('a'), Stub('b'), Stub('c')
    ens = E.EnsembleDetector([a, b])
    sliced = E.SlicedDetector(E.EnsembleDetector([a, b]))
    nested = E.TrackedDetector(E.SlicedDetector(E.EnsembleDetector([a, b])))
    return a, b, c, ens, sliced, nested


def test_leaf_models_in_order():
    a, b, c, ens, sliced, nested = _compositions()
    assert E.leaf_models(a) == [a]
    assert E.leaf_models(ens) == [a, b]
    assert E.leaf_models(sliced) == [a, b]
    assert E.leaf_models(nested) == [a, b]
    assert E.leaf_models(E.EnsembleDetector([b, a])) == [b, a]
    assert E.leaf_models(E.SlicedDetector(c)) == [c] and E.leaf_models(E.TrackedDetector(c)) == [c]
    # an ensemble of wrappers: the leaves in member order, depth first
    mixed = E.EnsembleDetector([E.SlicedDetector(c), E.EnsembleDetector([b, a])])
    assert E.leaf_models(mixed) == [c, b, a]


def test_f16x3_leaf_is_found_at_any_depth():
    f16 = _f16x3_name()
    plain = [k for k, v in ops.MODEL_ARITH.items() if v[2] != 'f16x3']
    for depth_wrap in (lambda m: E.EnsembleDetector([Stub('p'), m]),
                       lambda m: E.SlicedDetector(m),
                       lambda m: E.TrackedDetector(m),
                       lambda m: E.SlicedDetector(E.EnsembleDetector([Stub('p'), m])),
                       lambda m: E.TrackedDetector(E.SlicedDetector(E.EnsembleDetector([Stub('p'), m]))),
                       lambda m: E.EnsembleDetector([Stub('p'), E.SlicedDetector(E.EnsembleDetector([m]))])):
        assert depth_wrap(Stub('h', f32_arith=f16))._f16x3() is True
        for name in plain:
            assert depth_wrap(Stub('h', f32_arith=name))._f16x3() is False
    # a member without the attribute computes in the default arithmetic
    bare = Stub('n')
    del bare.f32_arith
    assert E.SlicedDetector(bare)._f16x3() is False


def test_eval_and_train_reach_every_leaf_and_return_the_wrapper():
    for pick in (3, 4, 5):
        parts = _compositions()
        a, b, w = parts[0], parts[1], parts[pick]
        assert w.eval() is w
        assert a.calls == ['eval'] and b.calls == ['eval']
        assert w.train(False) is w
        assert a.calls == ['eval', ('train', False)] and b.calls == ['eval', ('train', False)]
        assert w.train() is w
        assert a.calls[-1] == ('train', True) and b.calls[-1] == ('train', True)
        assert list(w.parameters()) == a.params + b.params
        assert w.num_classes == 3
    c = Stub('c', num_classes=7)
    for w in (E.SlicedDetector(c), E.TrackedDetector(c)):
        assert w.model is c and w.num_classes == 7 and list(w.parameters()) == c.params and next(w.parameters(), None) is c.params[0]


def test_only_the_list_detectors_have_detect():
    assert E.EnsembleDetector.detect is E.SlicedDetector.detect
    assert not hasattr(E.TrackedDetector, 'detect')
    assert hasattr(E.TrackedDetector, 'update') and hasattr(E.TrackedDetector, 'tracks')


def _raises(kind, text, fn):
    with pytest.raises(kind, match='^' + re.escape(text) + '$'):
        fn()


def test_constructor_refusals_keep_type_and_text():
    a, b = Stub('a'), Stub('b')
    V, N = ops.WBF_MAX_VIEWS, ops.WBF_MAX_IN
    _raises(ValueError, 'EnsembleDetector: 1..%d members, got 0' % V, lambda: E.EnsembleDetector([]))
    _raises(ValueError, 'EnsembleDetector: 1..%d members, got %d' % (V, V + 1), lambda: E.EnsembleDetector([a] * (V + 1)))
    _raises(ValueError, 'EnsembleDetector: members must share num_classes, got [3, 4]',
            lambda: E.EnsembleDetector([a, Stub('d', num_classes=4)]))
    top_n = N // 2 + 1
    _raises(ValueError, 'EnsembleDetector: members * fusion.top_n must be <= %d' % N,
            lambda: E.EnsembleDetector([a, b], fusion=ops.WBFOptions(top_n=top_n)))
    _raises(ValueError, 'EnsembleDetector: 1 weights for 2 views', lambda: E.EnsembleDetector([a, b], weights=[1.0]))
    _raises(ValueError, 'EnsembleDetector: weights must be positive and finite', lambda: E.EnsembleDetector([a, b], weights=[1.0, 0.0]))
    _raises(ValueError, 'EnsembleDetector: 1 scales for 2 members', lambda: E.EnsembleDetector([a, b], scales=[1.25]))
    _raises(ValueError, 'EnsembleDetector: scales must be positive and finite (or None), got (None, -2.0)',
            lambda: E.EnsembleDetector([a, b], scales=[None, -2.0]))
    ok = E.EnsembleDetector([a, b], weights=[2, 1], scales=[None, 1.0])
    assert ok.models == [a, b] and ok.weights == (2.0, 1.0) and ok.scales is None and ok.fusion == ops.WBFOptions() and ok.num_classes == 3
    assert E.EnsembleDetector([a, b], scales=(None, 1.25)).scales == (None, 1.25)

    no_pass = object()
    _raises(TypeError, 'SlicedDetector: options must be a SliceOptions, not 5', lambda: E.SlicedDetector(a, 5))
    _raises(TypeError, 'SlicedDetector: model must be an EfficientDet or an EnsembleDetector, not %r' % (no_pass,),
            lambda: E.SlicedDetector(no_pass))

    class NoClasses:
        def forward_raw(self, images):
            raise AssertionError

        def __repr__(self):
            return 'NoClasses()'
    _raises(TypeError, 'SlicedDetector: model must be an EfficientDet or an EnsembleDetector, not NoClasses()',
            lambda: E.SlicedDetector(NoClasses()))
    s = E.SlicedDetector(a)
    assert s.model is a and s.options == ops.SliceOptions() and s.num_classes == 3

    _raises(TypeError, 'TrackedDetector: options must be a TrackOptions, not 5', lambda: E.TrackedDetector(a, 5))
    _raises(TypeError, 'TrackedDetector: model must be an EfficientDet, an EnsembleDetector or a SlicedDetector, not %r' % (no_pass,),
            lambda: E.TrackedDetector(no_pass))
    for bad in (0, ops.TRACK_MAX_DET + 1):
        _raises(ValueError, 'TrackedDetector: max_detections must be in 1..%d' % ops.TRACK_MAX_DET,
                lambda: E.TrackedDetector(a, max_detections=bad))
    for bad in (float('inf'), float('nan')):
        _raises(ValueError, 'TrackedDetector: score_threshold must be finite', lambda: E.TrackedDetector(a, score_threshold=bad))
    # the options are checked before the model, the model before the numbers
    _raises(TypeError, 'TrackedDetector: options must be a TrackOptions, not 5', lambda: E.TrackedDetector(no_pass, 5, max_detections=0))
    _raises(TypeError, 'SlicedDetector: options must be a SliceOptions, not 5', lambda: E.SlicedDetector(no_pass, 5))
    t = E.TrackedDetector(a, ops.TrackOptions(low_thr=0.2), max_detections=50)
    assert t.model is a and t.options == ops.TrackOptions(low_thr=0.2) and t.score_threshold == ops.TrackOptions(low_thr=0.2).low_thr
    assert t.max_detections == 50 and t.num_classes == 3 and t.state is None
    assert E.TrackedDetector(a, score_threshold=0.3).score_threshold == 0.3


# (class, arguments, other arguments, repr of the first, repr of the second): the strings are the ones these constructions gave before the
# classes shared a base
OPTION_CASES = [
    ('NMSOptions', {}, {'method': 'gaussian', 'sigma': 0.25},
     "NMSOptions(method='hard', sigma=0.5, class_aware=False, pre_nms_top_n=1000, max_det=100)",
     "NMSOptions(method='gaussian', sigma=0.25, class_aware=False, pre_nms_top_n=1000, max_det=100)"),
    ('WBFOptions', {}, {'conf_type': 'max', 'top_n': 300},
     "WBFOptions(iou_thr=0.55, skip_box_thr=0.0, conf_type='avg', top_n=1000)",
     "WBFOptions(iou_thr=0.55, skip_box_thr=0.0, conf_type='max', top_n=300)"),
    ('TTAOptions', {}, {'hflip': False, 'scales': (1.25,)},
     "TTAOptions(hflip=True, weights=None, fusion=WBFOptions(iou_thr=0.55, skip_box_thr=0.0, conf_type='avg', top_n=1000))",
     "TTAOptions(hflip=False, weights=None, fusion=WBFOptions(iou_thr=0.55, skip_box_thr=0.0, conf_type='avg', top_n=1000), scales=(1.25,))"),
    ('SliceMergeOptions', {}, {'method': 'nms', 'metric': 'iou'},
     "SliceMergeOptions(method='nmm', metric='ios', thr=0.5, class_aware=True, skip_thr=0.0, top_n=256, max_det=300)",
     "SliceMergeOptions(method='nms', metric='iou', thr=0.5, class_aware=True, skip_thr=0.0, top_n=256, max_det=300)"),
    ('SliceOptions', {}, {'slice': (256, 384), 'full_view': False},
     "SliceOptions(slice=(512, 512), overlap=(0.2, 0.2), full_view=True, tile_batch=32, merge=SliceMergeOptions(method='nmm', metric='ios', "
     "thr=0.5, class_aware=True, skip_thr=0.0, top_n=256, max_det=300))",
     "SliceOptions(slice=(256, 384), overlap=(0.2, 0.2), full_view=False, tile_batch=32, merge=SliceMergeOptions(method='nmm', metric='ios', "
     "thr=0.5, class_aware=True, skip_thr=0.0, top_n=256, max_det=300))"),
    ('BoxLossOptions', {}, {'kind': 'giou', 'weight': 2.0},
     "BoxLossOptions(kind='smooth_l1', weight=1.0)",
     "BoxLossOptions(kind='giou', weight=2.0)"),
    ('LossOptions', {}, {'gamma': 1.5, 'low_quality': True},
     'LossOptions(alpha=0.25, gamma=2.0, label_smoothing=0.0, beta=0.1111111119389534, reg_weight=1.0, pos_iou=0.5, '
     'neg_iou=0.4000000059604645, low_quality=False)',
     'LossOptions(alpha=0.25, gamma=1.5, label_smoothing=0.0, beta=0.1111111119389534, reg_weight=1.0, pos_iou=0.5, '
     'neg_iou=0.4000000059604645, low_quality=True)'),
    ('ATSSOptions', {}, {'topk': 7},
     'ATSSOptions(topk=9)',
     'ATSSOptions(topk=7)'),
    ('TaskAlignedOptions', {}, {'topk': 10, 'aligned_target': False},
     'TaskAlignedOptions(topk=13, alpha=1.0, beta=6.0, aligned_target=True)',
     'TaskAlignedOptions(topk=10, alpha=1.0, beta=6.0, aligned_target=False)'),
    ('QualityLossOptions', {}, {'kind': 'vfl'},
     "QualityLossOptions(kind='qfl', beta=2.0, alpha=0.75, gamma=2.0)",
     "QualityLossOptions(kind='vfl', beta=2.0, alpha=0.75, gamma=2.0)"),
    ('TrackOptions', {}, {'assignment': 'optimal', 'track_buffer': 10},
     'TrackOptions(track_thr=0.5, low_thr=0.1, new_thr=0.6000000238418579, match_sim=0.2, second_sim=0.5, unconfirmed_sim=0.3, '
     'track_buffer=30, fuse_score=True, class_aware=False, max_tracks=128)',
     "TrackOptions(track_thr=0.5, low_thr=0.1, new_thr=0.6000000238418579, match_sim=0.2, second_sim=0.5, unconfirmed_sim=0.3, "
     "track_buffer=10, fuse_score=True, class_aware=False, max_tracks=128, assignment='optimal')"),
]


def test_the_cases_name_every_options_class_of_ops():
    found = sorted(n for n, v in vars(ops).items() if isinstance(v, type) and n.endswith('Options') and not n.startswith('_'))
    assert found == sorted(c[0] for c in OPTION_CASES)
    for n in found:
        assert issubclass(getattr(ops, n), ops._Options) and '__eq__' not in vars(getattr(ops, n)) and '__hash__' not in vars(getattr(ops, n))


@pytest.mark.parametrize('name,first,second,repr_first,repr_second', OPTION_CASES, ids=[c[0] for c in OPTION_CASES])
def test_options_equality_hash_and_repr(name, first, second, repr_first, repr_second):
    cls = getattr(ops, name)
    x, y, z = cls(**first), cls(**first), cls(**second)
    assert x == y and not (x != y) and hash(x) == hash(y) and x.key() == y.key()
    assert x != z and not (x == z) and x.key() != z.key()
    assert z == cls(**second) and hash(z) == hash(cls(**second))
    assert {x: 1}[y] == 1 and z not in {x: 1}
    assert x != None and x != x.key()                                                          # noqa: E711
    # another options class whose key() is the same tuple is still another thing
    other_cls = ops.ATSSOptions if cls is not ops.ATSSOptions else ops.NMSOptions
    for mine in (x, z):
        twin = other_cls()
        twin.key = mine.key
        assert twin.key() == mine.key() and hash(twin) == hash(mine)
        assert mine != twin and twin != mine and not (mine == twin)
    assert repr(x) == repr_first and repr(z) == repr_second


def test_options_that_extend_their_key_only_off_the_default():
    assert len(ops.TrackOptions().key()) == 10 and ops.TrackOptions(assignment='optimal').key()[10:] == ('optimal',)
    assert ops.TrackOptions(assignment='greedy') == ops.TrackOptions()
    t = ops.TTAOptions()
    assert t.key() == (True, None, ops.WBFOptions().key()) and ops.TTAOptions(scales=(1.25,)).key()[3:] == ((1.25,),)
    assert ops.TTAOptions(scales=()) == t
