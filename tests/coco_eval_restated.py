"""A NumPy restatement of the COCO box metric (pycocotools' ``COCOeval`` with ``iouType='bbox'``, default ``Params``, ``useCats=1``):
``evaluate`` / ``accumulate`` / ``summarize`` written from the published algorithm, on COCO-format dicts, with the loops kept in the
same shape as ``COCOeval``'s so that each step can be read against it.  The GPU tests hold the device metric
(``evaluate.COCOMeanAP``) to these arrays bit for bit; the CPU tests pin the restatement on hand-derived cases.

One documented deviation, shared with the device: a matched detection is marked by a flag, not by the matched ground truth's
annotation ``id`` (``COCOeval`` reads id 0 as "no match", which COCO's positive ids never hit)."""
import numpy as np

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
MAX_DETS = [1, 10, 100]
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
AREA_LBL = ['all', 'small', 'medium', 'large']


def bb_iou(d, g, iscrowd):
    """maskApi.c bbIou: d [m, 4], g [n, 4] xywh (fp64), iscrowd [n] -> [m, n], in the C operation order."""
    o = np.zeros((len(d), len(g)))
    for j in range(len(g)):
        G = g[j]
        ga = G[2] * G[3]
        for i in range(len(d)):
            D = d[i]
            da = D[2] * D[3]
            w = min(D[2] + D[0], G[2] + G[0]) - max(D[0], G[0])
            if w <= 0:
                continue
            h = min(D[3] + D[1], G[3] + G[1]) - max(D[1], G[1])
            if h <= 0:
                continue
            inter = w * h
            u = da if iscrowd[j] else da + ga - inter
            o[i, j] = inter / u
    return o


class COCOEvalRestated:
    """gt: {'annotations': [{'id', 'image_id', 'category_id', 'bbox', 'area', 'iscrowd'}], 'categories': [{'id'}]};
    dt: result dicts {'image_id', 'category_id', 'score', 'bbox'} in result order; img_ids: the evaluated images."""

    def __init__(self, gt, dt, img_ids):
        self.img_ids = list(np.unique(img_ids))
        self.cat_ids = sorted(c['id'] for c in gt['categories'])
        self.iou_thrs, self.rec_thrs, self.max_dets, self.area_rng = IOU_THRS, REC_THRS, MAX_DETS, AREA_RNG
        cats, imgs = set(self.cat_ids), set(self.img_ids)
        self._gts, self._dts = {}, {}
        for g in gt['annotations']:                                    # _prepare: getAnnIds order, ignore = iscrowd
            if g['image_id'] in imgs and g['category_id'] in cats:
                g = dict(g)
                g['ignore'] = int(bool(g.get('iscrowd', 0)))
                self._gts.setdefault((g['image_id'], g['category_id']), []).append(g)
        for i, d in enumerate(dt):                                     # loadRes: id = 1-based, area = w * h
            if d['image_id'] in imgs and d['category_id'] in cats:
                d = dict(d)
                d['id'] = i + 1
                d['area'] = d['bbox'][2] * d['bbox'][3]
                self._dts.setdefault((d['image_id'], d['category_id']), []).append(d)

    # ------------------------------------------------------------------------------------------------ evaluate
    def compute_iou(self, img_id, cat_id):
        gt = self._gts.get((img_id, cat_id), [])
        dt = self._dts.get((img_id, cat_id), [])
        if len(gt) == 0 and len(dt) == 0:
            return []
        inds = np.argsort([-d['score'] for d in dt], kind='mergesort')
        dt = [dt[i] for i in inds]
        if len(dt) > self.max_dets[-1]:
            dt = dt[0:self.max_dets[-1]]
        if len(dt) == 0 or len(gt) == 0:
            return []
        return bb_iou(np.array([d['bbox'] for d in dt], dtype=np.float64), np.array([g['bbox'] for g in gt], dtype=np.float64),
                      [int(o['iscrowd']) for o in gt])

    def evaluate_img(self, img_id, cat_id, a_rng, max_det):
        gt = self._gts.get((img_id, cat_id), [])
        dt = self._dts.get((img_id, cat_id), [])
        if len(gt) == 0 and len(dt) == 0:
            return None
        for g in gt:
            g['_ignore'] = 1 if (g['ignore'] or (g['area'] < a_rng[0] or g['area'] > a_rng[1])) else 0
        gtind = np.argsort([g['_ignore'] for g in gt], kind='mergesort')
        gt = [gt[i] for i in gtind]
        dtind = np.argsort([-d['score'] for d in dt], kind='mergesort')
        dt = [dt[i] for i in dtind[0:max_det]]
        iscrowd = [int(o['iscrowd']) for o in gt]
        ious = self.ious[img_id, cat_id]
        ious = ious[:, gtind] if len(ious) > 0 else ious
        T, G, D = len(self.iou_thrs), len(gt), len(dt)
        gtm = np.zeros((T, G))
        dtm = np.zeros((T, D))                                         # 1 = matched (the flag that replaces the GT id)
        gt_ig = np.array([g['_ignore'] for g in gt])
        dt_ig = np.zeros((T, D))
        if not len(ious) == 0:
            for tind, t in enumerate(self.iou_thrs):
                for dind, d in enumerate(dt):
                    iou = min([t, 1 - 1e-10])
                    m = -1
                    for gind, g in enumerate(gt):
                        if gtm[tind, gind] > 0 and not iscrowd[gind]:
                            continue
                        if m > -1 and gt_ig[m] == 0 and gt_ig[gind] == 1:
                            break
                        if ious[dind, gind] < iou:
                            continue
                        iou = ious[dind, gind]
                        m = gind
                    if m == -1:
                        continue
                    dt_ig[tind, dind] = gt_ig[m]
                    dtm[tind, dind] = 1
                    gtm[tind, m] = d['id']
        a = np.array([d['area'] < a_rng[0] or d['area'] > a_rng[1] for d in dt]).reshape((1, len(dt)))
        dt_ig = np.logical_or(dt_ig, np.logical_and(dtm == 0, np.repeat(a, T, 0)))
        return {'dtMatches': dtm, 'dtScores': [d['score'] for d in dt], 'gtIgnore': gt_ig, 'dtIgnore': dt_ig}

    def evaluate(self):
        self.ious = {(i, c): self.compute_iou(i, c) for i in self.img_ids for c in self.cat_ids}
        self.eval_imgs = [self.evaluate_img(i, c, a, self.max_dets[-1])
                          for c in self.cat_ids for a in self.area_rng for i in self.img_ids]

    # ------------------------------------------------------------------------------------------------ accumulate
    def accumulate(self):
        T, R, K, A, M = len(self.iou_thrs), len(self.rec_thrs), len(self.cat_ids), len(self.area_rng), len(self.max_dets)
        precision = -np.ones((T, R, K, A, M))
        recall = -np.ones((T, K, A, M))
        I0, A0 = len(self.img_ids), len(self.area_rng)
        for k in range(K):
            Nk = k * A0 * I0
            for a in range(A):
                Na = a * I0
                for m, max_det in enumerate(self.max_dets):
                    E = [self.eval_imgs[Nk + Na + i] for i in range(I0)]
                    E = [e for e in E if e is not None]
                    if len(E) == 0:
                        continue
                    dt_scores = np.concatenate([e['dtScores'][0:max_det] for e in E])
                    inds = np.argsort(-dt_scores, kind='mergesort')
                    dtm = np.concatenate([e['dtMatches'][:, 0:max_det] for e in E], axis=1)[:, inds]
                    dt_ig = np.concatenate([e['dtIgnore'][:, 0:max_det] for e in E], axis=1)[:, inds]
                    gt_ig = np.concatenate([e['gtIgnore'] for e in E])
                    npig = np.count_nonzero(gt_ig == 0)
                    if npig == 0:
                        continue
                    tps = np.logical_and(dtm, np.logical_not(dt_ig))
                    fps = np.logical_and(np.logical_not(dtm), np.logical_not(dt_ig))
                    tp_sum = np.cumsum(tps, axis=1).astype(dtype=np.float64)
                    fp_sum = np.cumsum(fps, axis=1).astype(dtype=np.float64)
                    for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                        tp, fp = np.array(tp), np.array(fp)
                        nd = len(tp)
                        rc = tp / npig
                        pr = tp / (fp + tp + np.spacing(1))
                        q = np.zeros((R,))
                        recall[t, k, a, m] = rc[-1] if nd else 0
                        pr, q = pr.tolist(), q.tolist()
                        for i in range(nd - 1, 0, -1):
                            if pr[i] > pr[i - 1]:
                                pr[i - 1] = pr[i]
                        inds = np.searchsorted(rc, self.rec_thrs, side='left')
                        for ri, pi in enumerate(inds):
                            if pi >= len(pr):
                                break
                            q[ri] = pr[pi]
                        precision[t, :, k, a, m] = np.array(q)
        self.eval = {'precision': precision, 'recall': recall}

    # ------------------------------------------------------------------------------------------------ summarize
    def _summarize(self, ap=1, iou_thr=None, area_rng='all', max_dets=100):
        aind = [i for i, l in enumerate(AREA_LBL) if l == area_rng]
        mind = [i for i, d in enumerate(self.max_dets) if d == max_dets]
        s = self.eval['precision'] if ap == 1 else self.eval['recall']
        if iou_thr is not None:
            s = s[np.where(iou_thr == self.iou_thrs)[0]]
        s = s[:, :, :, aind, mind] if ap == 1 else s[:, :, aind, mind]
        return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])

    def summarize(self):
        md = self.max_dets
        self.stats = np.array([
            self._summarize(1), self._summarize(1, iou_thr=.5, max_dets=md[2]), self._summarize(1, iou_thr=.75, max_dets=md[2]),
            self._summarize(1, area_rng='small', max_dets=md[2]), self._summarize(1, area_rng='medium', max_dets=md[2]),
            self._summarize(1, area_rng='large', max_dets=md[2]),
            self._summarize(0, max_dets=md[0]), self._summarize(0, max_dets=md[1]), self._summarize(0, max_dets=md[2]),
            self._summarize(0, area_rng='small', max_dets=md[2]), self._summarize(0, area_rng='medium', max_dets=md[2]),
            self._summarize(0, area_rng='large', max_dets=md[2])], dtype=np.float64)
        return self.stats


def coco_eval(gt, dt, img_ids):
    """-> (stats [12], precision [T, R, K, A, M], recall [T, K, A, M])."""
    e = COCOEvalRestated(gt, dt, img_ids)
    e.evaluate()
    e.accumulate()
    return e.summarize(), e.eval['precision'], e.eval['recall']
