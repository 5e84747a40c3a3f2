"""Batched evaluation consumer: what the reference's eval.py does per image on the host
(_get_detections :96-127, evaluate_coco :279-306: D2H of every detection, numpy threshold + argsort + top-100, box
rescale) done for the whole batch on the device, ONE device->host copy of [B, max_det, 6] + counts.

Output formats are the reference's: ``all_detections[image][label] -> ndarray [n, 5] (x1,y1,x2,y2,score)`` and the
MS-COCO result dicts {'image_id', 'category_id', 'score', 'bbox': [x, y, w, h]}.

The VOC metric itself (eval.py:165-257 `evaluate` after `_get_detections`) runs on the device too: ``VOCMeanAP`` keeps one record per
detection slot on the GPU across the dataset (csrc/voc_map.hip) and the host receives the per-class APs once, in ``compute``;
``evaluate_voc`` is the drop-in for ``evaluate(generator, model)``."""
import numpy as np
import torch

from . import ops


def postprocess(model, cls, reg, anc, H, W):
    """models/efficientdet.py:69-86 for every image of the batch, on the device: decode + clip + class max + threshold + NMS.
    -> (scores [B,A], labels [B,A] int64, boxes [B,A,4], count [B] int32): score-descending rows, count[b] of them valid."""
    boxes, score, label = ops.decode_score(anc, reg, cls, H, W)
    idx, count = ops.nms(boxes, score, float(model.threshold), float(model.iou_threshold))
    s, l, b = ops.gather_dets(boxes, score, label, idx, count)
    return s, l, b, count


def default_max_detections(xywh, A, num_classes=None):
    """eval.py:104-117 (_get_detections, the VOC path) keeps the 100 best detections per image; eval.py:279-306 (evaluate_coco)
    emits EVERY detection scoring >= the threshold and leaves the capping to COCOeval.  finalize_dets' cap is a per-image top-K by
    score, so any cap below the NMS output size A could truncate whole low-scoring categories the reference would have emitted:
    the xywh / COCO path is therefore UNCAPPED by default (A rows), whatever num_classes is."""
    return int(A) if xywh else 100


def finalize(s, l, b, count, scales, score_threshold=0.05, max_detections=None, xywh=False, num_classes=None):
    """eval.py:104-117 / :279-292 for the batch on the device -> (dets [B,max_detections,6], counts [B]) on the HOST.
    max_detections=None: default_max_detections (100 per image for the VOC rows, every detection for the COCO rows)."""
    if max_detections is None:
        max_detections = default_max_detections(xywh, s.shape[1], num_classes)
    sc = torch.as_tensor(np.asarray(scales, dtype=np.float32) if not torch.is_tensor(scales) else scales,
                         dtype=torch.float32, device=s.device).contiguous()
    out, oc = ops.finalize_dets(s, l, b, count, sc, score_threshold, max_detections, xywh)
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
    sc = torch.as_tensor(np.asarray(scales, dtype=np.float32) if not torch.is_tensor(scales) else scales,
                         dtype=torch.float32, device=s.device).contiguous()
    return ops.finalize_dets(s, l, b, count, sc, score_threshold, int(max_detections), False)


def detections_batched(model, images, scales, score_threshold=0.05, max_detections=None, xywh=False):
    """-> (dets [B, max_detections, 6] fp32 on the HOST: x1,y1,x2,y2 (or x,y,w,h), score, label; counts [B] ints).
    images: NCHW fp32 batch or PackedImages; scales: [B] resize factors (tensor, array or list)."""
    with torch.no_grad():
        cls, reg, anc = model.forward_raw(images)
        s, l, b, count = postprocess(model, cls, reg, anc, int(images.shape[2]), int(images.shape[3]))
        return finalize(s, l, b, count, scales, score_threshold, max_detections, xywh, getattr(model, 'num_classes', None))


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


class VOCMeanAP:
    """The reference's VOC metric (eval.py:185-257) accumulated on the device.

    ``add(dets, counts, gt)`` matches one batch of finalize_device's rows against its ground truth and appends one record per detection
    slot to a device buffer (no device->host transfer); ``compute()`` sorts every record by (class, descending score) and returns
    ``(mean AP, {label: (ap, num_annotations)})`` with the reference's types: ``(0, 0)`` for a class without ground truth, else
    ``(np.float64, float)``.  Ties: detections of one class with equal scores are ranked in insertion order (image, then score order
    within the image); the reference's np.argsort is unstable there, so AP can differ from it only when tied scores mix TP and FP.
    ``gt`` is either a list of per-image [n, 5] arrays (x1, y1, x2, y2, label; the generator's load_annotations, (0, 5) allowed) or a
    pair of device tensors (boxes fp64 [B, G, 4], labels int32 [B, G], -1 = pad)."""

    INITIAL_CAPACITY = 1 << 16            # records; the buffer doubles when a batch does not fit

    def __init__(self, num_classes, iou_threshold=0.5, device=None):
        num_classes = int(num_classes)
        if not 1 <= num_classes <= 65535:
            raise ValueError('num_classes must be in [1, 65535], got %d' % num_classes)
        self.num_classes = num_classes
        self.iou_threshold = float(iou_threshold)
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        self.reset()

    def reset(self):
        self.num_records = 0
        self._key = torch.empty(self.INITIAL_CAPACITY, dtype=torch.int64, device=self.device)
        self._tp = torch.empty(self.INITIAL_CAPACITY, dtype=torch.uint8, device=self.device)
        self._gt_count = torch.zeros(self.num_classes, dtype=torch.int32, device=self.device)

    @property
    def capacity(self):
        return self._key.numel()

    def _reserve(self, need):
        cap = self._key.numel()
        if need <= cap:
            return
        while cap < need:
            cap *= 2
        key = torch.empty(cap, dtype=torch.int64, device=self.device)
        tp = torch.empty(cap, dtype=torch.uint8, device=self.device)
        key[:self.num_records].copy_(self._key[:self.num_records])          # device to device, stream-ordered
        tp[:self.num_records].copy_(self._tp[:self.num_records])
        self._key, self._tp = key, tp

    def _ground_truth(self, gt, B):
        if isinstance(gt, tuple) and len(gt) == 2 and torch.is_tensor(gt[0]) and torch.is_tensor(gt[1]) and gt[0].dim() == 3:
            boxes, labels = gt
            if boxes.dim() != 3 or boxes.shape[0] != B or boxes.shape[2] != 4 or tuple(labels.shape) != tuple(boxes.shape[:2]):
                raise ValueError('device ground truth must be boxes [B, G, 4] and labels [B, G], got %s and %s'
                                 % (tuple(boxes.shape), tuple(labels.shape)))
            if boxes.dtype != torch.float64 or labels.dtype != torch.int32:
                raise ValueError('device ground truth must be float64 boxes and int32 labels')
            boxes, labels = boxes.to(self.device).contiguous(), labels.to(self.device).contiguous()
        else:
            if len(gt) != B:
                raise ValueError('%d ground-truth arrays for %d images' % (len(gt), B))
            rows = []
            for a in gt:
                a = np.asarray(a, dtype=np.float64)
                if a.size == 0:
                    a = a.reshape(0, 5)
                if a.ndim != 2 or a.shape[1] != 5:
                    raise ValueError('ground truth per image must be [n, 5] (x1, y1, x2, y2, label), got %s' % (a.shape,))
                rows.append(a)
            G = max([1] + [len(a) for a in rows])
            hb = np.zeros((B, G, 4), dtype=np.float64)
            hl = np.full((B, G), -1, dtype=np.int32)
            for i, a in enumerate(rows):
                lab = a[:, 4]
                # eval.py:157 selects rows by `annotations[:, 4] == label` for label in range(num_classes): any other value is no row
                ok = (lab >= 0) & (lab < self.num_classes) & (lab == np.floor(lab))
                hb[i, :len(a)] = a[:, :4]
                hl[i, :len(a)] = np.where(ok, lab, -1).astype(np.int32)
            boxes = torch.from_numpy(hb).to(self.device)
            labels = torch.from_numpy(hl).to(self.device)
        if boxes.shape[1] > ops.VOC_MAX_GT:
            raise ValueError('at most %d ground-truth rows per image, got %d' % (ops.VOC_MAX_GT, boxes.shape[1]))
        if boxes.shape[1] == 0:                                     # (the kernel wants G >= 1: one padding row)
            boxes = torch.zeros((B, 1, 4), dtype=torch.float64, device=self.device)
            labels = torch.full((B, 1), -1, dtype=torch.int32, device=self.device)
        return boxes, labels

    def add(self, dets, counts, gt):
        """dets [B, max_det, 6] fp32 and counts [B] of finalize_device (device tensors); gt: see the class docstring."""
        dets = torch.as_tensor(dets).to(self.device, torch.float32).contiguous()
        counts = torch.as_tensor(counts).to(self.device, torch.int32).contiguous()
        if dets.dim() != 3 or dets.shape[2] != 6 or counts.dim() != 1 or counts.shape[0] != dets.shape[0]:
            raise ValueError('dets must be [B, max_det, 6] with counts [B], got %s and %s' % (tuple(dets.shape), tuple(counts.shape)))
        B, M = int(dets.shape[0]), int(dets.shape[1])
        if B == 0 or M == 0:
            return
        boxes, labels = self._ground_truth(gt, B)
        self._reserve(self.num_records + B * M)
        n = self.num_records
        ops.voc_match(dets, counts, boxes, labels, self.num_classes, self.iou_threshold, self._key[n:], self._tp[n:], self._gt_count)
        self.num_records = n + B * M

    def compute(self, curves=False):
        """-> (mean AP, {label: (ap, num_annotations)}) as eval.py:243-257 returns them; with curves=True also
        {label: (recall, precision)}: the sorted fp64 arrays eval.py:241 hands to _compute_ap (labels without ground truth: absent)."""
        out, recall, precision, seg = ops.voc_ap(self._key, self._tp, self.num_records, self._gt_count, self.num_classes)
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


def evaluate_voc(generator, model, iou_threshold=0.5, score_threshold=0.05, max_detections=100, batch_size=1):
    """Drop-in for eval.py:165-257 `evaluate(generator, retinanet)`: the same generator protocol (len, [i] -> {'img' HWC, 'scale'},
    load_annotations, num_classes, label_to_name), the same summary lines and return value; detections, matching, sort and AP on
    the device.  batch_size > 1 batches consecutive images of the same size."""
    model.eval()
    p = next(model.parameters(), None)
    device = p.device if p is not None else torch.device('cuda', torch.cuda.current_device())
    meter = VOCMeanAP(generator.num_classes(), iou_threshold, device)
    with torch.no_grad():
        for batch in _image_batches(generator, max(1, int(batch_size))):
            x = torch.stack([img.permute(2, 0, 1) for _, img, _ in batch]).to(device).float().contiguous()
            cls, reg, anc = model.forward_raw(x)
            s, l, b, count = postprocess(model, cls, reg, anc, int(x.shape[2]), int(x.shape[3]))
            dets, counts = finalize_device(s, l, b, count, [sc for _, _, sc in batch], score_threshold, max_detections)
            meter.add(dets, counts, [generator.load_annotations(i) for i, _, _ in batch])
    mean, average_precisions = meter.compute()
    print('\nmAP:')
    for label in range(generator.num_classes()):
        print('{}: {}'.format(generator.label_to_name(label), average_precisions[label][0]))
    print('avg mAP: {}'.format(mean))
    return mean, average_precisions
