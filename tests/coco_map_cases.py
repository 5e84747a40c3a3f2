"""Shared inputs of the COCO metric tests: the hand-derived cases (their expected numbers are derived in
tests/test_coco_map_host.py), a seeded COCO-scale generator, and the conversion of COCO-format dicts into the meter's per-image
rows.  A case is (gt, dt, img_ids, num_categories): gt {'annotations', 'categories'}, dt result dicts in result order, img_ids in
the order the images are added."""
import numpy as np

V = 1.0 / (1.0 + np.spacing(1))            # the precision of one TP and no FP: 0.9999999999999998


def _ann(i, img, cat, bbox, crowd=0, area=None):
    return {'id': i, 'image_id': img, 'category_id': cat, 'bbox': [float(v) for v in bbox], 'iscrowd': crowd,
            'area': float(bbox[2] * bbox[3] if area is None else area)}


def _det(img, cat, bbox, score):
    return {'image_id': img, 'category_id': cat, 'bbox': [float(v) for v in bbox], 'score': float(np.float32(score))}


def _case(anns, dets, img_ids, cats=(1,)):
    return {'annotations': anns, 'categories': [{'id': c} for c in cats]}, dets, list(img_ids), len(cats)


def hand_cases():
    c = {}
    box = [0, 0, 10, 10]
    c['perfect'] = _case([_ann(1, 1, 1, box)], [_det(1, 1, box, 0.9)], [1])
    c['iou_0.6'] = _case([_ann(1, 1, 1, [0, 0, 6, 10])], [_det(1, 1, box, 0.9)], [1])
    c['iou_0.9'] = _case([_ann(1, 1, 1, [0, 0, 9, 10])], [_det(1, 1, box, 0.9)], [1])
    c['area_edges'] = _case([_ann(1, 1, 1, [0, 0, 32, 32], area=1024.0), _ann(2, 1, 1, [100, 100, 96, 96], area=9216.0)],
                            [_det(1, 1, [0, 0, 32, 32], 0.9), _det(1, 1, [100, 100, 96, 96], 0.8)], [1])
    c['crowd'] = _case([_ann(1, 1, 1, [0, 0, 100, 100], crowd=1), _ann(2, 1, 1, [200, 200, 10, 10])],
                       [_det(1, 1, [0, 0, 10, 10], 0.9), _det(1, 1, [20, 20, 10, 10], 0.8), _det(1, 1, [50, 50, 10, 10], 0.7),
                        _det(1, 1, [200, 200, 10, 10], 0.6)], [1])
    c['ignored_break'] = _case([_ann(1, 1, 1, box), _ann(2, 1, 1, box, crowd=1)], [_det(1, 1, box, 0.9), _det(1, 1, box, 0.8)], [1])
    c['ties_desc_ids'] = _case([_ann(1, 3, 1, box), _ann(2, 2, 1, [50, 50, 10, 10])],
                               [_det(3, 1, box, 0.5), _det(2, 1, box, 0.5)], [3, 2])
    c['rank_cut_150'] = _case([_ann(i + 1, 1, 1, [20 * i, 0, 10, 10]) for i in range(150)],
                              [_det(1, 1, [20 * i, 0, 10, 10], 1 - i / 1000) for i in range(150)], [1])
    c['cat_without_dets'] = _case([_ann(1, 1, 1, box), _ann(2, 1, 2, [50, 50, 10, 10])], [_det(1, 1, box, 0.9)], [1], cats=(1, 2))
    c['img_without_gt'] = _case([_ann(1, 1, 1, box)], [_det(1, 1, box, 0.9), _det(5, 1, box, 0.95)], [1, 5])
    return c


def per_image_rows(gt, dt, img_ids):
    """-> (dets [n, 6] per image: x, y, w, h, score, category index in result order; gts [g, 7] per image: x, y, w, h, category
    index, iscrowd, area in annotation order), both in img_ids order."""
    cats = sorted(c['id'] for c in gt['categories'])
    ci = {c: i for i, c in enumerate(cats)}
    dets, gts = [], []
    for iid in img_ids:
        dets.append(np.array([d['bbox'] + [d['score'], ci[d['category_id']]] for d in dt if d['image_id'] == iid],
                             dtype=np.float64).reshape(-1, 6))
        gts.append(np.array([a['bbox'] + [ci[a['category_id']], a['iscrowd'], a['area']] for a in gt['annotations']
                             if a['image_id'] == iid], dtype=np.float64).reshape(-1, 7))
    return dets, gts


def random_case(n_img=300, K=80, max_rows=400, seed=0):
    """A seeded COCO-scale set: 0-40 GTs per image (1 in 30 crowd, some sub-pixel, some huge, areas around the range edges),
    0-max_rows score-descending detections per image, coarse scores so that ties across images are common; image ids shuffled."""
    rng = np.random.RandomState(seed)
    ids = rng.permutation(np.arange(1, 3 * n_img))[:n_img] * 7 + 3
    cat_ids = sorted(rng.choice(np.arange(1, 200), K, replace=False).tolist())
    anns, dets, aid = [], [], 1
    for iid in ids:
        ng = rng.randint(0, 41)
        gb = []
        for _ in range(ng):
            kind = rng.rand()
            if kind < 0.1:
                w, h = rng.uniform(0.05, 1.0, 2)                       # sub-pixel
            elif kind < 0.2:
                w, h = rng.uniform(300, 900, 2)                        # huge
            else:
                w, h = np.exp(rng.uniform(np.log(4), np.log(200), 2))
            x, y = rng.uniform(0, 640, 2)
            cat = cat_ids[rng.randint(0, min(K, 12))] if rng.rand() < 0.7 else cat_ids[rng.randint(0, K)]
            area = w * h * rng.choice([1.0, 0.7, 1.3]) if rng.rand() < 0.5 else rng.choice([1024.0, 9216.0, w * h])
            anns.append({'id': aid, 'image_id': int(iid), 'category_id': int(cat), 'bbox': [float(x), float(y), float(w), float(h)],
                         'iscrowd': int(rng.rand() < 1 / 30), 'area': float(area)})
            gb.append((x, y, w, h, cat))
            aid += 1
        nd = rng.randint(0, max_rows + 1)
        sc = np.sort(rng.randint(1, 400, nd).astype(np.float32) / np.float32(400))[::-1]
        for k in range(nd):
            if gb and rng.rand() < 0.6:
                x, y, w, h, cat = gb[rng.randint(0, len(gb))]
                j = rng.normal(0, 0.15, 4)
                bx = [x + j[0] * w, y + j[1] * h, w * (1 + j[2]), h * (1 + j[3])]
                if rng.rand() < 0.2:
                    cat = cat_ids[rng.randint(0, K)]
            else:
                x, y = rng.uniform(0, 640, 2)
                bx = [x, y] + list(np.exp(rng.uniform(np.log(2), np.log(300), 2)))
                cat = cat_ids[rng.randint(0, min(K, 12))]
            bx = [float(np.float32(v)) for v in bx]                       # the rows are fp32 on the device
            bx[2], bx[3] = max(bx[2], 0.0), max(bx[3], 0.0)
            dets.append({'image_id': int(iid), 'category_id': int(cat), 'bbox': bx, 'score': float(sc[k])})
    return {'annotations': anns, 'categories': [{'id': c} for c in cat_ids]}, dets, [int(i) for i in ids], K
