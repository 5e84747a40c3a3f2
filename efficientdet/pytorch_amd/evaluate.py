"""Batched evaluation consumer: what the reference's eval.py does per image on the host
(_get_detections :96-127, evaluate_coco :279-306: D2H of every detection, numpy threshold + argsort + top-100, box
rescale) done for the whole batch on the device, ONE device->host copy of [B, max_det, 6] + counts.

Output formats are the reference's: ``all_detections[image][label] -> ndarray [n, 5] (x1,y1,x2,y2,score)`` and the
MS-COCO result dicts {'image_id', 'category_id', 'score', 'bbox': [x, y, w, h]}.

The VOC metric itself (eval.py:165-257 `evaluate` after `_get_detections`) runs on the device too: ``VOCMeanAP`` keeps one record per
detection slot on the GPU across the dataset (csrc/voc_map.hip) and the host receives the per-class APs once, in ``compute``;
``evaluate_voc`` is the drop-in for ``evaluate(generator, model)``.  The COCO box metric (pycocotools' ``COCOeval`` as eval.py:260-338
`evaluate_coco` runs it) is on the device the same way: ``COCOMeanAP`` (csrc/coco_map.hip) and the drop-in ``evaluate_coco``.
``OperatingPoint`` / ``evaluate_operating_point`` (csrc/op_point.hip; the reference has no counterpart) answer where to cut the
detections: precision / recall / F1 against a grid of confidence thresholds and a confusion matrix, over the VOC meter's records.
``TrackedDetector`` (csrc/track.hip; the reference's camera mode has no counterpart) gives the boxes of a video identities: ByteTrack over
finalize_device's rows, one tracker per image of the batch, state and outputs on the device."""
import numpy as np
import torch

from . import ops


def postprocess(model, cls, reg, anc, H, W):
    """models/efficientdet.py:69-86 for every image of the batch, on the device: decode + clip + class max + threshold + NMS.
    -> (scores [B,A], labels [B,A] int64, boxes [B,A,4], count [B] int32): score-descending rows, count[b] of them valid."""
    boxes, score, label = ops.decode_score(anc, reg, cls, H, W)
    return ops.model_nms(model, boxes, score, label)


def default_max_detections(xywh, A, num_classes=None):
    """eval.py:104-117 (_get_detections, the VOC path) keeps the 100 best detections per image; eval.py:279-306 (evaluate_coco)
    emits EVERY detection scoring >= the threshold and leaves the capping to COCOeval.  finalize_dets' cap is a per-image top-K by
    score, so any cap below the NMS output size A could truncate whole low-scoring categories the reference would have emitted:
    the xywh / COCO path is therefore UNCAPPED by default (A rows), whatever num_classes is."""
    return int(A) if xywh else 100


def _scales_tensor(scales, device):
    """finalize_dets' resize factors (tensor, array or list) -> contiguous fp32 on device."""
    return torch.as_tensor(np.asarray(scales, dtype=np.float32) if not torch.is_tensor(scales) else scales,
                           dtype=torch.float32, device=device).contiguous()


def finalize(s, l, b, count, scales, score_threshold=0.05, max_detections=None, xywh=False, num_classes=None):
    """eval.py:104-117 / :279-292 for the batch on the device -> (dets [B,max_detections,6], counts [B]) on the HOST.
    max_detections=None: default_max_detections (100 per image for the VOC rows, every detection for the COCO rows)."""
    if max_detections is None:
        max_detections = default_max_detections(xywh, s.shape[1], num_classes)
    out, oc = ops.finalize_dets(s, l, b, count, _scales_tensor(scales, s.device), score_threshold, max_detections, xywh)
    # counts first (a few bytes), then ONLY the filled rows: the uncapped COCO default makes `out` [B, A, 6] -- 1.18 MB per D0 image,
    # 4.7 MB per D4 image, nearly all of it padding rows past the count (zeros with label -1, as the kernel writes them) -- which the
    # host array reproduces without transferring them
    counts = oc.cpu().numpy()
    k = int(counts.max()) if counts.size else 0
    host = np.zeros((out.shape[0], max_detections, 6), dtype=np.float32)
    host[:, :, 5] = -1.0
    if k:
        host[:, :k] = out[:, :k].cpu().numpy()
    return host, counts


def finalize_device(s, l, b, count, scales, score_threshold=0.05, max_detections=100):
    """finalize (the VOC rows: x1, y1, x2, y2, score, label, boxes / scale) without the copy -> (out [B, max_detections, 6] fp32,
    counts [B] int32), both left on the device; rows past counts[b] are zero with label -1."""
    return ops.finalize_dets(s, l, b, count, _scales_tensor(scales, s.device), score_threshold, int(max_detections), False)


def detections_batched(model, images, scales, score_threshold=0.05, max_detections=None, xywh=False):
    """-> (dets [B, max_detections, 6] fp32 on the HOST: x1,y1,x2,y2 (or x,y,w,h), score, label; counts [B] ints).
    images: NCHW fp32 batch or PackedImages; scales: [B] resize factors (tensor, array or list); model: an EfficientDet (its set_nms /
    set_tta apply) or an EnsembleDetector."""
    with torch.no_grad():
        s, l, b, count = ops.model_detections(model, images, int(images.shape[2]), int(images.shape[3]))
        return finalize(s, l, b, count, scales, score_threshold, max_detections, xywh, getattr(model, 'num_classes', None))


def leaf_models(model):
    """The models with a pass of their own (forward_raw) under ``model``, in order: an EnsembleDetector's members, a SlicedDetector's
    or a TrackedDetector's model, at any depth; a model that wraps nothing is its own only leaf."""
    inner = getattr(model, 'models', None) or ([model.model] if hasattr(model, 'model') and not hasattr(model, 'forward_raw') else None)
    return [model] if inner is None else [x for i in inner for x in leaf_models(i)]


class _DetectorWrapper:
    """What EnsembleDetector, SlicedDetector and TrackedDetector share: they stand in for a model (num_classes, eval, train,
    parameters) over ``models`` or ``model``, and know whether a leaf computes in f16x3 (whose range flag they clear and check)."""

    def _take_model(self, model, kinds):
        if not hasattr(model, 'num_classes') or not (hasattr(model, 'forward_raw') or hasattr(model, 'detections')):
            raise TypeError('%s: model must be %s, not %r' % (type(self).__name__, kinds, model))
        self.model = model
        self.num_classes = int(model.num_classes)

    def _inner(self):
        return self.models if hasattr(self, 'models') else [self.model]

    def eval(self):
        for m in self._inner():
            m.eval()
        return self

    def train(self, mode=True):
        for m in self._inner():
            m.train(mode)
        return self

    def parameters(self):
        return (p for m in self._inner() for p in m.parameters())

    def _f16x3(self):
        return any(ops.MODEL_ARITH[getattr(m, 'f32_arith', 'f32')][2] == 'f16x3' for m in leaf_models(self))


class _ListDetector(_DetectorWrapper):
    """A wrapper whose ``detections(images, H, W)`` is one pass: EfficientDet's ``detect`` over it."""

    def detect(self, images):
        """-> list of (scores[K], labels[K] int64, boxes[K,4]) per image, score-descending, as EfficientDet.detect."""
        f16x3 = self._f16x3()
        if f16x3:
            ops.clear_range_flag(images.device)
        with torch.no_grad():
            s, l, b, count = self.detections(images, int(images.shape[2]), int(images.shape[3]))
        counts = count.tolist()
        if f16x3 and not torch.cuda.is_current_stream_capturing():
            ops.check_range_flag(s.device)
        return [(s[i, :n], l[i, :n], b[i, :n]) for i, n in enumerate(counts)]


class EnsembleDetector(_ListDetector):
    """Several detectors as one: every member runs its own detection pass on the batch (its own set_nms and set_tta included) and the
    lists are merged on the device by weighted boxes fusion (ops.fuse_detections) under the members' weights.  Has ``detect(images)``
    like EfficientDet and is taken as ``model`` by detections_batched, evaluate_voc and evaluate_coco.  Members may differ in family
    (D0 with D1, raw with EMA weights) but share num_classes.  scales: None, or one entry per member: None or 1.0 gives the member the
    image tensor as it is, and none of its boxes is rescaled; any other s gives it the batch resampled to (H * s, W * s)
    (ops.resample_images; both sides whole multiples of 128, checked at the call before anything is launched) -- D0 at 512 next to D1 at
    640 is scales=(None, 1.25) -- and its boxes are multiplied by H / (H * s) in the fusion.  A member's own set_tta applies to the
    input that member sees."""

    def __init__(self, models, weights=None, fusion=None, scales=None):
        self.models = list(models)
        self.fusion = ops.WBFOptions() if fusion is None else fusion
        V = len(self.models)
        if not 1 <= V <= ops.WBF_MAX_VIEWS:
            raise ValueError('EnsembleDetector: 1..%d members, got %d' % (ops.WBF_MAX_VIEWS, V))
        if len({int(m.num_classes) for m in self.models}) != 1:
            raise ValueError('EnsembleDetector: members must share num_classes, got %s' % [int(m.num_classes) for m in self.models])
        if V * self.fusion.top_n > ops.WBF_MAX_IN:
            raise ValueError('EnsembleDetector: members * fusion.top_n must be <= %d' % ops.WBF_MAX_IN)
        self.weights = ops._view_weights(weights, V, 'EnsembleDetector')
        if scales is not None:
            scales = tuple(None if s is None or float(s) == 1.0 else float(s) for s in scales)
            if len(scales) != V:
                raise ValueError('EnsembleDetector: %d scales for %d members' % (len(scales), V))
            if not all(s is None or 0.0 < s < float('inf') for s in scales):
                raise ValueError('EnsembleDetector: scales must be positive and finite (or None), got %r' % (scales,))
            if all(s is None for s in scales):
                scales = None
        self.scales = scales
        self.num_classes = int(self.models[0].num_classes)

    def detections(self, images, H, W):
        """ops.model_detections' tuple for the ensemble (what that function asks a model with its own pass for)."""
        scales = getattr(self, 'scales', None)                 # (an ensemble pickled before the option existed has no such attribute)
        if scales is None:
            return ops.fuse_detections([ops.model_detections(m, images, H, W) for m in self.models], self.weights, None, None, self.fusion)
        sizes = [(H, W) if s is None else ops.scaled_size(H, W, s, 'EnsembleDetector') for s in scales]   # (every refusal before a launch)
        views = [ops.model_detections(m, images if s is None else ops.resample_images(images, hw), hw[0], hw[1])
                 for m, s, hw in zip(self.models, scales, sizes)]
        muls = [float(np.float32(float(H) / float(hw[0]))) for hw in sizes]
        return ops.fuse_detections(views, self.weights, None, muls, self.fusion)


class SlicedDetector(_ListDetector):
    """A detector for images larger than its network input (sliced inference, SAHI): the batch is cut into overlapping tiles of
    options.slice on the device (ops.slice_images), the tiles go through ``model``'s own detection pass tile_batch at a time (its
    set_nms and set_tta apply per tile), with options.full_view the whole image resampled to the tile size (ops.resample_images) goes
    through one more pass of batch B, and the lists are moved into the image's frame and merged on the device (ops.merge_slices).
    ``model``: an EfficientDet or an EnsembleDetector.  Has ``detect(images)`` like EfficientDet and is taken as ``model`` by
    detections_batched, evaluate_voc and evaluate_coco.  images: an NCHW fp32 batch or a PackedImages of any H x W >= the slice, one
    size per batch; the tiles are PackedImages of the batch's dtype (fp32 for an NCHW batch), which the model must compute in.  A batch
    of exactly the slice's size is one tile: it goes through ``model``'s own pass as it is and nothing is merged."""

    def __init__(self, model, options=None):
        options = ops.SliceOptions() if options is None else options
        if not isinstance(options, ops.SliceOptions):
            raise TypeError('SlicedDetector: options must be a SliceOptions, not %r' % (options,))
        self._take_model(model, 'an EfficientDet or an EnsembleDetector')
        self.options = options

    def detections(self, images, H, W):
        """ops.model_detections' tuple for the sliced pass (what that function asks a model with its own pass for)."""
        o = self.options
        h, w = o.slice
        plan = ops.slice_plan(H, W, o)                                # (first: every refusal comes before any launch)
        if len(plan) == 1:                                            # the image is one tile: the model's own pass, nothing to merge
            return ops.model_detections(self.model, images, H, W)
        full = o.full_view and (int(H), int(W)) != (h, w)             # (slice_plan's rule: its last record is then the whole image)
        B, TPI = int(images.shape[0]), len(plan)
        T = TPI - (1 if full else 0)
        table = ops.slice_table(plan, images.device)
        cut = ops.slice_table(plan[:T], images.device)                # (the flat tile index counts the T tiles: the full view is not one)
        parts = []
        for t0 in range(0, B * T, o.tile_batch):
            tiles = ops.slice_images(images, cut, (h, w), t0, min(t0 + o.tile_batch, B * T))
            parts.append(ops.model_detections(self.model, tiles, h, w))
        whole = ops.model_detections(self.model, ops.resample_images(images, (h, w)), h, w) if full else None
        R = min(o.merge.top_n, int(parts[0][0].shape[1]))

        def gather(i, tail):
            t = torch.cat([p[i][:, :R] for p in parts]).reshape((B, T, R) + tail)
            return t if whole is None else torch.cat([t, whole[i][:, None, :R]], dim=1)
        count = torch.cat([p[3] for p in parts]).reshape(B, T)
        if whole is not None:
            count = torch.cat([count, whole[3][:, None]], dim=1)
        return ops.merge_slices((gather(0, ()), gather(1, ()), gather(2, (4,)), count), table, H, W, o.merge)


class TrackedDetector(_DetectorWrapper):
    """A detector for video: every image of the batch is one camera stream, and each call is the streams' next frame.  ``update`` runs
    ``model``'s own detection pass (an EfficientDet, an EnsembleDetector or a SlicedDetector: its NMS and TTA settings apply), the eval
    consumer on the device (finalize_device; score_threshold None: options.low_thr, because ByteTrack needs the low detections) and ONE
    ops.track_step (csrc/track.hip, include/effdet_track.h): ByteTrack, state on the device, no host read.  Each association is greedy
    by descending similarity by default; options = TrackOptions(assignment='optimal') solves it as the published tracker does, as a
    linear assignment problem (include/effdet_assign.h) -- the wrapper only passes its options on.  The
    state is allocated at the first update for that batch size; another batch size later raises (reset() and a new wrapper are the ways
    to start over).  options is read at every update; its max_tracks is fixed once the state exists (ops.track_step refuses another).

    Capture.  update reads nothing back, so the caller can capture it in a torch.cuda.graph over a static image buffer -- with the
    recipe of any captured forward here: two warm-up updates on a side stream (the first allocates the state and records the model's
    parameter-preparation jobs, the second builds their device tables; neither may happen under capture), then reset() (the warm-up
    frames advanced frame_id and next_id), then the capture; scales must be None or a device tensor (a host list would be uploaded
    under capture).  The three tensors the captured call returned are rewritten by every replay.  For an f16x3 model the range flag
    is cleared inside update (a node of the graph) and checked by tracks(), the form that reads back; after a replay
    ops.check_range_flag(device) is the caller's:

        side = torch.cuda.Stream(); side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            tracker.update(static); tracker.update(static)
        torch.cuda.current_stream().wait_stream(side); tracker.reset()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            rows, ids, count = tracker.update(static)
        static.copy_(frame); graph.replay()                   # per frame"""

    def __init__(self, model, options=None, score_threshold=None, max_detections=100):
        options = ops.TrackOptions() if options is None else options
        if not isinstance(options, ops.TrackOptions):
            raise TypeError('TrackedDetector: options must be a TrackOptions, not %r' % (options,))
        self._take_model(model, 'an EfficientDet, an EnsembleDetector or a SlicedDetector')
        if not 1 <= int(max_detections) <= ops.TRACK_MAX_DET:
            raise ValueError('TrackedDetector: max_detections must be in 1..%d' % ops.TRACK_MAX_DET)
        score_threshold = options.low_thr if score_threshold is None else float(score_threshold)
        if not abs(score_threshold) < float('inf'):
            raise ValueError('TrackedDetector: score_threshold must be finite')
        self.options, self.score_threshold, self.max_detections = options, score_threshold, int(max_detections)
        self.state = None

    def detections_device(self, images, scales=None):
        """The detection half of update -> finalize_device's (dets [B, max_detections, 6], counts [B]) on the device."""
        B = int(images.shape[0])
        if self._f16x3():
            ops.clear_range_flag(images.device)
        if scales is None:
            scales = torch.ones(B, dtype=torch.float32, device=images.device)
        with torch.no_grad():
            s, l, b, count = ops.model_detections(self.model, images, int(images.shape[2]), int(images.shape[3]))
            return finalize_device(s, l, b, count, scales, self.score_threshold, self.max_detections)

    def update(self, images, scales=None):
        """The streams' next frame -> ops.track_step's (rows [B, max_tracks, 8], ids [B, max_tracks] int32, count [B] int32), all on the
        device.  scales: finalize's resize factors (None: 1, boxes in the input's pixels)."""
        B = int(images.shape[0])
        if self.state is not None and self.state.B != B:
            raise ValueError('TrackedDetector: the tracker holds %d streams, this batch has %d' % (self.state.B, B))
        if self.state is None:
            self.state = ops.track_state(B, self.options.max_tracks, images.device)
        dets, counts = self.detections_device(images, scales)
        return ops.track_step(dets, counts, self.state, self.options)

    def tracks(self, images, scales=None):
        """update, read back -> per image (ids[K] int64, scores[K], labels[K] int64, boxes[K, 4])."""
        rows, ids, count = self.update(images, scales)
        counts = count.tolist()
        if self._f16x3() and not torch.cuda.is_current_stream_capturing():
            ops.check_range_flag(rows.device)
        return [(ids[i, :n].to(torch.int64), rows[i, :n, 4], rows[i, :n, 5].to(torch.int64), rows[i, :n, :4]) for i, n in enumerate(counts)]

    def reset(self, streams=None):
        """Forget the tracks of every stream (None) or of the listed stream indices; ids start at 1 again there."""
        if self.state is None:
            return
        if streams is None:
            ops.track_reset(self.state)
            return
        mask = [0] * self.state.B
        for b in streams:
            if not 0 <= int(b) < self.state.B:
                raise ValueError('TrackedDetector.reset: stream %r of %d' % (b, self.state.B))
            mask[int(b)] = 1
        ops.track_reset(self.state, mask)


class Annotator:
    """Paints detections or tracks into uint8 RGB frames on the device (ops.draw_detections, csrc/draw.hip; include/effdet_draw.h
    holds the drawing rule): names -- the class names, tabled on the device at the first call and kept; options -- an
    ops.DrawOptions; palette -- uint8 [P, 3] (None: ops.draw_palette(64)).  Takes TrackedDetector.update's (rows, ids, count) and
    finalize_device's (dets, counts) as they are, and reads nothing back:

        rows, ids, count = tracker.update(images)
        painted = annotator(frames, rows, count, ids, box_scale)       # frames: uint8 [B, H, W, 3] on the device"""

    def __init__(self, names, options=None, palette=None):
        options = ops.DrawOptions() if options is None else options
        if not isinstance(options, ops.DrawOptions):
            raise TypeError('Annotator: options must be a DrawOptions, not %r' % (options,))
        self.names = None if names is None else list(names)
        ops.draw_names(self.names, 'cpu')                                # (the refusals now, not at the first frame)
        self.options, self.palette = options, palette
        self._tables = {}

    def __call__(self, frames, rows, counts, ids=None, box_scale=None, inplace=False, max_hw=None):
        """-> the painted frames (ops.draw_detections' arguments and result).  box_scale: (sx, sy) from the rows' pixels to the frames',
        one pair or a [B, 2] device tensor."""
        dev = rows.device
        if dev not in self._tables:
            pal = ops.draw_palette(64, dev) if self.palette is None else torch.as_tensor(self.palette, dtype=torch.uint8).to(dev).contiguous()
            self._tables[dev] = (ops.draw_names(self.names, dev), pal)
        table, pal = self._tables[dev]
        return ops.draw_detections(frames, rows, counts, table, ids, box_scale, pal, self.options, inplace, max_hw)


def all_detections_rows(dets, counts, num_classes):
    """eval.py:118-123: per image, per label -> [n,5] arrays (boxes + score)."""
    rows = []
    for d, n in zip(dets, counts):
        d = d[:int(n)]
        rows.append([d[d[:, 5] == c, :5] if n else np.zeros((0, 5)) for c in range(num_classes)])
    return rows


def coco_results(dets_xywh, counts, image_ids, label_to_coco_label=lambda c: c):
    """eval.py:296-306: one dict per detection (dets must come from detections_batched(..., xywh=True))."""
    res = []
    for d, n, iid in zip(dets_xywh, counts, image_ids):
        for k in range(int(n)):
            res.append({'image_id': iid, 'category_id': label_to_coco_label(int(d[k, 5])), 'score': float(d[k, 4]),
                        'bbox': [float(v) for v in d[k, :4]]})
    return res


def _check_dets(dets, counts, device):
    """dets [B, max_det, 6] and counts [B] of finalize_dets -> (fp32 dets, int32 counts), contiguous on device."""
    dets = torch.as_tensor(dets).to(device, torch.float32).contiguous()
    counts = torch.as_tensor(counts).to(device, torch.int32).contiguous()
    if dets.dim() != 3 or dets.shape[2] != 6 or counts.dim() != 1 or counts.shape[0] != dets.shape[0]:
        raise ValueError('dets must be [B, max_det, 6] with counts [B], got %s and %s' % (tuple(dets.shape), tuple(counts.shape)))
    return dets, counts


def _check_gt_rows(G, max_gt):
    if G > max_gt:
        raise ValueError('at most %d ground-truth rows per image, got %d' % (max_gt, G))


def _pad_ground_truth(rows, B, cols, what, max_gt, check=None):
    """B per-image [n, cols] arrays (label in column 4; an empty one counts as (0, cols)) -> fp64 [B, G, cols] with G >= 1 (the
    kernels want a row: all empty gives one padding row), padding rows zero with label -1.  check(a) sees each image's array."""
    if len(rows) != B:
        raise ValueError('%d ground-truth arrays for %d images' % (len(rows), B))
    arrays = []
    for a in rows:
        a = np.asarray(a, dtype=np.float64)
        if a.size == 0:
            a = a.reshape(0, cols)
        if a.ndim != 2 or a.shape[1] != cols:
            raise ValueError('ground truth per image must be [n, %d] %s, got %s' % (cols, what, a.shape))
        if check is not None:
            check(a)
        arrays.append(a)
    G = max([1] + [len(a) for a in arrays])
    _check_gt_rows(G, max_gt)
    h = np.zeros((B, G, cols), dtype=np.float64)
    h[:, :, 4] = -1
    for i, a in enumerate(arrays):
        h[i, :len(a)] = a
    return h


class _RecordMeter:
    """What the two meters share: one record per detection slot, held in the 1-D device tensors `_rec` (one per entry of
    RECORD_DTYPES) that grow by doubling; `num_records` of their `capacity` are filled.  A subclass extends reset()."""

    INITIAL_CAPACITY = 1 << 16            # records; the buffers double when a batch does not fit
    RECORD_DTYPES = ()

    def __init__(self, device):
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        self.reset()

    def reset(self):
        self.num_records = 0
        self._rec = self._alloc(self.INITIAL_CAPACITY)

    def _alloc(self, n):
        return tuple(torch.empty(n, dtype=dt, device=self.device) for dt in self.RECORD_DTYPES)

    @property
    def capacity(self):
        return self._rec[0].numel()

    def _reserve(self, need):
        cap = self.capacity
        if need <= cap:
            return
        while cap < need:
            cap *= 2
        rec = self._alloc(cap)
        for new, old in zip(rec, self._rec):
            new[:self.num_records].copy_(old[:self.num_records])          # device to device, stream-ordered
        self._rec = rec


class VOCMeanAP(_RecordMeter):
    """The reference's VOC metric (eval.py:185-257) accumulated on the device.

    ``add(dets, counts, gt)`` matches one batch of finalize_device's rows against its ground truth and appends one record per detection
    slot to a device buffer (no device->host transfer); ``compute()`` sorts every record by (class, descending score) and returns
    ``(mean AP, {label: (ap, num_annotations)})`` with the reference's types: ``(0, 0)`` for a class without ground truth, else
    ``(np.float64, float)``.  Ties: detections of one class with equal scores are ranked in insertion order (image, then score order
    within the image); the reference's np.argsort is unstable there, so AP can differ from it only when tied scores mix TP and FP.
    ``gt`` is either a list of per-image [n, 5] arrays (x1, y1, x2, y2, label; the generator's load_annotations, (0, 5) allowed) or a
    pair of device tensors (boxes fp64 [B, G, 4], labels int32 [B, G], -1 = pad)."""

    RECORD_DTYPES = (torch.int64, torch.uint8)                     # sort key (class << 32 | score key), TP byte

    def __init__(self, num_classes, iou_threshold=0.5, device=None):
        num_classes = int(num_classes)
        if not 1 <= num_classes <= 65535:
            raise ValueError('num_classes must be in [1, 65535], got %d' % num_classes)
        self.num_classes = num_classes
        self.iou_threshold = float(iou_threshold)
        super().__init__(device)

    def reset(self):
        super().reset()
        self._gt_count = torch.zeros(self.num_classes, dtype=torch.int32, device=self.device)

    def _ground_truth(self, gt, B):
        if isinstance(gt, tuple) and len(gt) == 2 and torch.is_tensor(gt[0]) and torch.is_tensor(gt[1]) and gt[0].dim() == 3:
            boxes, labels = gt
            if boxes.dim() != 3 or boxes.shape[0] != B or boxes.shape[2] != 4 or tuple(labels.shape) != tuple(boxes.shape[:2]):
                raise ValueError('device ground truth must be boxes [B, G, 4] and labels [B, G], got %s and %s'
                                 % (tuple(boxes.shape), tuple(labels.shape)))
            if boxes.dtype != torch.float64 or labels.dtype != torch.int32:
                raise ValueError('device ground truth must be float64 boxes and int32 labels')
            _check_gt_rows(boxes.shape[1], ops.VOC_MAX_GT)
            if boxes.shape[1] > 0:
                return boxes.to(self.device).contiguous(), labels.to(self.device).contiguous()
            gt = [()] * B                                               # G = 0: one padding row
        h = _pad_ground_truth(gt, B, 5, '(x1, y1, x2, y2, label)', ops.VOC_MAX_GT)
        lab = h[:, :, 4]
        # eval.py:157 selects rows by `annotations[:, 4] == label` for label in range(num_classes): any other value is no row
        ok = (lab >= 0) & (lab < self.num_classes) & (lab == np.floor(lab))
        return (torch.from_numpy(np.ascontiguousarray(h[:, :, :4])).to(self.device),
                torch.from_numpy(np.where(ok, lab, -1).astype(np.int32)).to(self.device))

    def add(self, dets, counts, gt):
        """dets [B, max_det, 6] fp32 and counts [B] of finalize_device (device tensors); gt: see the class docstring."""
        dets, counts = _check_dets(dets, counts, self.device)
        B, M = int(dets.shape[0]), int(dets.shape[1])
        if B == 0 or M == 0:
            return
        boxes, labels = self._ground_truth(gt, B)
        self._reserve(self.num_records + B * M)
        n = self.num_records
        ops.voc_match(dets, counts, boxes, labels, self.num_classes, self.iou_threshold, self._rec[0][n:], self._rec[1][n:],
                      self._gt_count)
        self.num_records = n + B * M

    def compute(self, curves=False):
        """-> (mean AP, {label: (ap, num_annotations)}) as eval.py:243-257 returns them; with curves=True also
        {label: (recall, precision)}: the sorted fp64 arrays eval.py:241 hands to _compute_ap (labels without ground truth: absent)."""
        out, recall, precision, seg = ops.voc_ap(*self._rec, self.num_records, self._gt_count, self.num_classes)
        host = out.cpu().numpy()                                    # the one device->host copy: 2 x num_classes doubles
        average_precisions = {}
        for c in range(self.num_classes):
            if host[1, c] == 0:
                average_precisions[c] = 0, 0
            else:
                average_precisions[c] = np.float64(host[0, c]), float(host[1, c])
        mean = np.mean([average_precisions[c][0] for c in range(self.num_classes)])
        if not curves:
            return mean, average_precisions
        sg, r, p = seg.cpu().numpy(), recall.cpu().numpy(), precision.cpu().numpy()
        cv = {c: (r[sg[c, 0]:sg[c, 1]].copy(), p[sg[c, 0]:sg[c, 1]].copy()) for c in range(self.num_classes) if host[1, c] != 0}
        return mean, average_precisions, cv


def _image_batches(generator, batch_size):
    """Consecutive images of identical H x W, at most batch_size per batch (padding would change the detections)."""
    batch = []
    for i in range(len(generator)):
        data = generator[i]
        img = torch.as_tensor(data['img'])
        if batch and (len(batch) == batch_size or batch[0][1].shape != img.shape):
            yield batch
            batch = []
        batch.append((i, img, data['scale']))
    if batch:
        yield batch


def _model_device(model):
    p = next(model.parameters(), None)
    return p.device if p is not None else torch.device('cuda', torch.cuda.current_device())


def _detect_batch(model, batch, device):
    """One batch of _image_batches (HWC images of one size) through ops.model_detections
    -> (scores, labels, boxes, count, number of classes of the head)."""
    x = torch.stack([img.permute(2, 0, 1) for _, img, _ in batch]).to(device).float().contiguous()
    return ops.model_detections(model, x, int(x.shape[2]), int(x.shape[3]), num_classes=True)


def evaluate_voc(generator, model, iou_threshold=0.5, score_threshold=0.05, max_detections=100, batch_size=1):
    """Drop-in for eval.py:165-257 `evaluate(generator, retinanet)`: the same generator protocol (len, [i] -> {'img' HWC, 'scale'},
    load_annotations, num_classes, label_to_name), the same summary lines and return value; detections, matching, sort and AP on
    the device.  batch_size > 1 batches consecutive images of the same size."""
    model.eval()
    device = _model_device(model)
    meter = VOCMeanAP(generator.num_classes(), iou_threshold, device)
    with torch.no_grad():
        for batch in _image_batches(generator, max(1, int(batch_size))):
            s, l, b, count, _ = _detect_batch(model, batch, device)
            dets, counts = finalize_device(s, l, b, count, [sc for _, _, sc in batch], score_threshold, max_detections)
            meter.add(dets, counts, [generator.load_annotations(i) for i, _, _ in batch])
    mean, average_precisions = meter.compute()
    print('\nmAP:')
    for label in range(generator.num_classes()):
        print('{}: {}'.format(generator.label_to_name(label), average_precisions[label][0]))
    print('avg mAP: {}'.format(mean))
    return mean, average_precisions


# ------------------------------------------------------------------------------------------------ operating point
class OperatingPoint(VOCMeanAP):
    """Where to cut the detections: precision / recall / F1 of every class against a grid of confidence thresholds, the threshold
    with the best F1, and a confusion matrix, accumulated on the device over VOCMeanAP's records (include/effdet_op_point.h,
    csrc/op_point.hip).

    ``add(dets, counts, gt)`` takes what VOCMeanAP.add takes (finalize_device's rows, score-descending per image -- the curves rely on
    that order); besides the VOC records it adds the batch to the confusion matrix: the predictions are the rows with
    score > conf_threshold, matched to the objects at IoU > confusion_iou whatever their labels (Ultralytics' process_batch with its
    ties decided: a prediction keeps its best object, the first of equals; an object keeps its best prediction, the lowest row of
    equals).  No device->host transfer.  ``compute()`` returns a dict:

      thresholds            the grid, fp32 [M] (default i / 1000, i = 0..1000)
      tp, npred             int32 [C, M]: TPs (at iou_threshold, VOC matching) and detections of the class with score > threshold
      precision, recall, f1 fp64 [C, M]: tp / npred (1 without detections), tp / annotations (0 without), 2PR / (P + R) (0 for 0 / 0)
      mean                  fp64 [3, M]: their means over the classes with annotations
      num_annotations       int64 [C]
      per_class             {label: (threshold, P, R, F1)} at the class's own best F1 (the lowest such threshold); classes without
                            annotations are absent
      overall               (threshold, P, R, F1) at the best mean F1; (None, 0.0, 0.0, 0.0) when no class has annotations
      ap, mean_ap           VOC AP per class (fp64 [C]) at iou_threshold and their mean, as VOCMeanAP.compute gives them
      confusion             int64 [C + 1, C + 1]: row = predicted class, column = true class, index C = background

    Only these tables are copied to the host.  Unlike Ultralytics the F1 curve is not smoothed and the thresholds are a fixed grid, not
    interpolated over all confidences."""

    def __init__(self, num_classes, iou_threshold=0.5, conf_threshold=0.25, confusion_iou=0.45, thresholds=None, device=None):
        self.thresholds = ops.op_thresholds(thresholds)
        self.conf_threshold, self.confusion_iou = float(conf_threshold), float(confusion_iou)
        if self.conf_threshold != self.conf_threshold or self.confusion_iou != self.confusion_iou:
            raise ValueError('conf_threshold and confusion_iou must not be NaN')
        super().__init__(num_classes, iou_threshold, device)

    def reset(self):
        super().reset()
        self._confusion = torch.zeros((self.num_classes + 1, self.num_classes + 1), dtype=torch.int64, device=self.device)

    def add(self, dets, counts, gt):
        """dets [B, max_det, 6] fp32 and counts [B] of finalize_device (device tensors); gt: see VOCMeanAP."""
        dets, counts = _check_dets(dets, counts, self.device)
        B, M = int(dets.shape[0]), int(dets.shape[1])
        if B == 0 or M == 0:
            return
        boxes, labels = self._ground_truth(gt, B)
        self._reserve(self.num_records + B * M)
        n = self.num_records
        ops.voc_match(dets, counts, boxes, labels, self.num_classes, self.iou_threshold, self._rec[0][n:], self._rec[1][n:],
                      self._gt_count)
        ops.confusion_match(dets, counts, boxes, labels, self.num_classes, self.conf_threshold, self.confusion_iou, self._confusion)
        self.num_records = n + B * M

    def compute(self):
        """-> the dict of the class docstring."""
        C = self.num_classes
        cur = ops.op_curves(*self._rec, self.num_records, self._gt_count, C, self.thresholds)
        mean_ap, aps = super().compute()
        out = {k: cur[k].cpu().numpy() for k in ('tp', 'npred', 'precision', 'recall', 'f1', 'mean')}
        best = cur['best'].cpu().numpy()
        th = self.thresholds.copy()
        out['thresholds'] = th
        out['num_annotations'] = self._gt_count.cpu().numpy().astype(np.int64)
        out['per_class'] = {c: (float(th[int(best[c, 0])]), best[c, 1], best[c, 2], best[c, 3]) for c in range(C) if best[c, 0] >= 0}
        j = int(best[C, 0])
        out['overall'] = (float(th[j]), best[C, 1], best[C, 2], best[C, 3]) if j >= 0 else (None, 0.0, 0.0, 0.0)
        out['ap'] = np.array([aps[c][0] for c in range(C)], dtype=np.float64)
        out['mean_ap'] = mean_ap
        out['confusion'] = self._confusion.cpu().numpy()
        return out


def operating_point_lines(result, names):
    """The summary evaluate_operating_point prints for an OperatingPoint.compute() dict: one line per class (P, R and F1 at the overall
    threshold, the class's own best threshold, AP), then the overall line."""
    t = result['overall'][0]
    j = -1 if t is None else int(np.flatnonzero(result['thresholds'] == np.float32(t))[0])      # (the grid is strictly ascending)
    lines = []
    for c, name in enumerate(names):
        p, r, f = (result['precision'][c, j], result['recall'][c, j], result['f1'][c, j]) if j >= 0 else (0.0, 0.0, 0.0)
        own = result['per_class'][c][0] if c in result['per_class'] else None
        lines.append('{}: annotations {} P {:.4f} R {:.4f} F1 {:.4f} best threshold {} AP {}'.format(
            name, int(result['num_annotations'][c]), p, r, f, own, result['ap'][c]))
    t, p, r, f = result['overall']
    lines.append('overall: threshold {} P {:.4f} R {:.4f} F1 {:.4f} mAP {}'.format(t, p, r, f, result['mean_ap']))
    return lines


def evaluate_operating_point(generator, model, iou_threshold=0.5, score_threshold=0.05, max_detections=100, batch_size=1,
                             conf_threshold=0.25, confusion_iou=0.45, thresholds=None):
    """The operating point of ``model`` on ``generator``: evaluate_voc's generator protocol, batching and models (an EfficientDet, an
    EnsembleDetector or a SlicedDetector), an OperatingPoint meter instead of the VOC one.  Prints one line per class (annotations; P, R
    and F1 at the overall threshold; the class's own best threshold; AP) and the overall line, and returns OperatingPoint.compute()'s
    dict.  ``overall[0]`` is the score threshold with the best mean F1: assigning it to ``model.threshold`` is the intended use; this
    function does not do it.  The detections are cut at score_threshold and max_detections before the meter sees them, so every
    threshold of the grid below score_threshold sees the same detections as score_threshold itself, and the confusion matrix is that of
    max(conf_threshold, score_threshold)."""
    model.eval()
    device = _model_device(model)
    meter = OperatingPoint(generator.num_classes(), iou_threshold, conf_threshold, confusion_iou, thresholds, device)
    with torch.no_grad():
        for batch in _image_batches(generator, max(1, int(batch_size))):
            s, l, b, count, _ = _detect_batch(model, batch, device)
            dets, counts = finalize_device(s, l, b, count, [sc for _, _, sc in batch], score_threshold, max_detections)
            meter.add(dets, counts, [generator.load_annotations(i) for i, _, _ in batch])
    result = meter.compute()
    print('\noperating point:')
    for line in operating_point_lines(result, [generator.label_to_name(c) for c in range(generator.num_classes())]):
        print(line)
    return result


# ------------------------------------------------------------------------------------------------ COCO box metric
# COCOeval's default Params for iouType='bbox', computed the way COCOeval computes them (np.linspace: iouThrs[8] is
# 0.8999999999999999, and 10 of the 101 recThrs differ from i / 100)
COCO_IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
COCO_REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
COCO_AREA_RNG = np.array([[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]], dtype=np.float64)
COCO_AREA_LBL = ['all', 'small', 'medium', 'large']
COCO_MAX_DETS = [1, 10, 100]
# summarize()'s 12 rows: (ap, iouThr or None, area label, index into maxDets)
_COCO_SUMMARY = [(1, None, 'all', 2), (1, .5, 'all', 2), (1, .75, 'all', 2), (1, None, 'small', 2), (1, None, 'medium', 2),
                 (1, None, 'large', 2), (0, None, 'all', 0), (0, None, 'all', 1), (0, None, 'all', 2), (0, None, 'small', 2),
                 (0, None, 'medium', 2), (0, None, 'large', 2)]


def summarize_lines(stats):
    """The 12 lines COCOeval.summarize() prints for these stats (default Params)."""
    lines = []
    for (ap, thr, area, mi), v in zip(_COCO_SUMMARY, stats):
        iou = '{:0.2f}:{:0.2f}'.format(COCO_IOU_THRS[0], COCO_IOU_THRS[-1]) if thr is None else '{:0.2f}'.format(thr)
        lines.append(' {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}'.format(
            'Average Precision' if ap else 'Average Recall', '(AP)' if ap else '(AR)', iou, area, COCO_MAX_DETS[mi], v))
    return lines


class COCOMeanAP(_RecordMeter):
    """pycocotools' COCOeval (iouType='bbox', default Params, useCats=1) accumulated on the device.

    ``add(dets, counts, image_ids, gt)`` matches one batch of finalize_dets' xywh rows (category index in column 5, rows of an image
    score-descending) against its ground truth and appends the records of the detections COCOeval would keep (the first 100 per
    image and category) to a device buffer -- no device->host transfer.  ``image_ids`` are host integers in [0, 2^31), each seen
    once per accumulation.  ``gt`` is either a list of per-image [g, 7] arrays (x, y, w, h, category index, iscrowd, annotation
    area; annotation order) or a device tensor [B, G, 7] fp64 whose rows with a category outside [0, num_categories) are padding.
    ``compute()`` returns ``stats`` (np.float64[12], summarize()'s order); ``compute(full=True)`` also returns
    ``{'precision': [T, R, K, A, M], 'recall': [T, K, A, M]}`` as ``COCOeval.eval`` holds them.

    Deviations from COCOeval: a matched detection is flagged rather than labelled with the matched GT's annotation id (COCOeval
    reads id 0 as "no match", which COCO's positive ids never produce); no ``eval['scores']``; the category list is the
    ``num_categories`` indices (evaluate_coco maps the dataset's sorted category ids onto them)."""

    RECORD_DTYPES = (torch.int64, torch.int32, torch.uint8, torch.int64, torch.int64)      # key, image, rank, match, ignore

    def __init__(self, num_categories, device=None):
        num_categories = int(num_categories)
        if not 1 <= num_categories <= ops.COCO_MAX_CATEGORIES:
            raise ValueError('num_categories must be in [1, %d], got %d' % (ops.COCO_MAX_CATEGORIES, num_categories))
        self.num_categories = num_categories
        super().__init__(device)

    def reset(self):
        super().reset()
        self.max_image_id = 0
        self._seen = set()
        self._npig = torch.zeros((self.num_categories, len(COCO_AREA_RNG)), dtype=torch.int32, device=self.device)

    def _image_ids(self, image_ids, B):
        if torch.is_tensor(image_ids) and image_ids.device.type != 'cpu':
            raise ValueError('image_ids must be host integers (the meter checks them for duplicates)')
        ids = np.asarray(image_ids).reshape(-1)
        if ids.shape[0] != B:
            raise ValueError('%d image ids for %d images' % (ids.shape[0], B))
        if ids.size and (ids.dtype.kind not in 'iu' and not np.all(ids == np.floor(ids))):
            raise ValueError('image ids must be integers')
        ids = ids.astype(np.int64)
        if ids.size and (ids.min() < 0 or ids.max() >= 2 ** 31):
            raise ValueError('image ids must be in [0, 2^31)')
        if len(set(ids.tolist())) != B or self._seen.intersection(ids.tolist()):
            raise ValueError('an image id was added twice')
        return ids

    def _ground_truth(self, gt, B):
        K = self.num_categories
        if torch.is_tensor(gt):
            if gt.dim() != 3 or gt.shape[0] != B or gt.shape[2] != 7:
                raise ValueError('device ground truth must be [B, G, 7], got %s' % (tuple(gt.shape),))
            if gt.dtype != torch.float64:
                raise ValueError('device ground truth must be float64')
            _check_gt_rows(gt.shape[1], ops.COCO_MAX_GT)
            if gt.shape[1] > 0:
                return gt.to(self.device).contiguous()
            gt = [()] * B                                               # G = 0: one padding row

        def in_range(a):
            c = a[:, 4]
            if not np.all((c >= 0) & (c < K) & (c == np.floor(c))):
                raise ValueError('ground-truth category out of range [0, %d)' % K)
        h = _pad_ground_truth(gt, B, 7, '(x, y, w, h, category, iscrowd, area)', ops.COCO_MAX_GT, in_range)
        return torch.from_numpy(h).to(self.device)

    def add(self, dets, counts, image_ids, gt):
        """dets [B, max_det, 6] fp32 (x, y, w, h, score, category index) and counts [B] (device tensors); image_ids: B host ints;
        gt: see the class docstring."""
        dets, counts = _check_dets(dets, counts, self.device)
        B, M = int(dets.shape[0]), int(dets.shape[1])
        ids = self._image_ids(image_ids, B)
        g = self._ground_truth(gt, B)
        if B == 0:
            return
        if M == 0:                                                  # no detection rows: the ground truth still counts
            dets = torch.zeros((B, 1, 6), dtype=torch.float32, device=self.device)
            counts = torch.zeros(B, dtype=torch.int32, device=self.device)
            M = 1
        S = ops.coco_slots(M, self.num_categories, COCO_MAX_DETS[-1])
        self._reserve(self.num_records + B * S)
        n = self.num_records
        ops.coco_match(dets, counts, torch.from_numpy(ids.astype(np.int32)).to(self.device), g, self.num_categories, COCO_IOU_THRS,
                       COCO_AREA_RNG, COCO_MAX_DETS[-1], tuple(t[n:] for t in self._rec), self._npig)
        self.num_records = n + B * S
        self._seen.update(ids.tolist())
        self.max_image_id = max(self.max_image_id, int(ids.max()))

    def compute(self, full=False):
        """-> stats (np.float64[12]); with full=True -> (stats, {'precision', 'recall'}) in COCOeval.eval's shapes."""
        precision, recall, stats = ops.coco_accumulate(self._rec, self.num_records, self.max_image_id, self._npig, self.num_categories,
                                                       COCO_IOU_THRS, COCO_REC_THRS, len(COCO_AREA_RNG), COCO_MAX_DETS)
        host = stats.cpu().numpy()                                  # the one device->host copy: 12 doubles
        if not full:
            return host
        return host, {'precision': precision.cpu().numpy(), 'recall': recall.cpu().numpy()}


def evaluate_coco(dataset, model, threshold=0.05, batch_size=1):
    """Drop-in for eval.py:260-338 `evaluate_coco(dataset, model, threshold)`: the same dataset protocol (len, [i] -> {'img' HWC,
    'scale'}, image_ids, label_to_coco_label, coco) and the same 12 summary lines; detections, matching, accumulation and the
    summary on the device.  Returns the 12 stats (the reference returns None), or None without a summary when no image has a
    detection, as the reference does.  The ground truth is read through coco.getCatIds / getAnnIds(imgIds=[id]) / loadAnns:
    every annotation (crowd and sub-pixel boxes included) with its bbox, category_id, iscrowd and area.  No results JSON is
    written: a submission still goes through detections_batched(..., xywh=True) and coco_results.  batch_size > 1 batches
    consecutive images of the same size."""
    model.eval()
    device = _model_device(model)
    coco = dataset.coco
    cat_ids = sorted(coco.getCatIds())
    cat_index = {c: i for i, c in enumerate(cat_ids)}
    meter = COCOMeanAP(len(cat_ids), device)
    lut, total = None, torch.zeros((), dtype=torch.int64, device=device)
    with torch.no_grad():
        for batch in _image_batches(dataset, max(1, int(batch_size))):
            s, l, b, count, nc = _detect_batch(model, batch, device)
            if lut is None:                                         # model label -> index into the sorted category ids (-1: none)
                lut = torch.tensor([cat_index.get(dataset.label_to_coco_label(c), -1) for c in range(nc)],
                                   dtype=torch.float32, device=device)
            sc = torch.as_tensor(np.asarray([sc for _, _, sc in batch], dtype=np.float32), device=device)
            dets, counts = ops.finalize_dets(s, l, b, count, sc, threshold, int(s.shape[1]), True)     # uncapped, as the reference
            lab = dets[:, :, 5]
            dets[:, :, 5] = torch.where(lab >= 0, lut[lab.clamp(min=0).long()], lab)
            total += counts.sum()
            ids = [int(dataset.image_ids[i]) for i, _, _ in batch]
            gts = []
            for iid in ids:
                rows = [[*a['bbox'], cat_index[a['category_id']], a['iscrowd'], a['area']]
                        for a in coco.loadAnns(coco.getAnnIds(imgIds=[iid])) if a['category_id'] in cat_index]
                gts.append(np.asarray(rows, dtype=np.float64).reshape(-1, 7))
            meter.add(dets, counts, ids, gts)
    if int(total) == 0:
        return None
    stats = meter.compute()
    for line in summarize_lines(stats):
        print(line)
    model.train()
    return stats
