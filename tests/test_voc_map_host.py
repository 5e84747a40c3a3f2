"""CPU tier of the device VOC metric (csrc/voc_map.hip, evaluate.VOCMeanAP / evaluate_voc): the new entry points are declared and
bound, the meter refuses bad arguments before any device work, and tests/golden/voc_map.npz is self-consistent."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compute_ap(recall, precision):
    """eval.py:46-73 restated: sentinels, envelope from the right, sum of (delta recall) * envelope where recall changes."""
    mrec = np.concatenate(([0.], recall, [1.]))
    mpre = np.concatenate(([0.], precision, [0.]))
    for i in range(mpre.size - 1, 0, -1):
        mpre[i - 1] = np.maximum(mpre[i - 1], mpre[i])
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])


def test_voc_entry_points_are_declared_and_bound():
    from efficientdet.pytorch_amd import _lib, build, evaluate, ops
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'effdet_hip.h')).read(), flags=re.S)
    for name in ('effdet_voc_match', 'effdet_voc_ap', 'effdet_voc_ap_workspace_bytes'):
        assert re.search(r'\b%s\s*\(' % name, hdr), name
        assert name in _lib.SYMBOLS, name
    assert _lib.ABI_VERSION == 11
    assert '-ffp-contract=off' in build.PER_FILE['voc_map.hip']          # fp64 IoUs at exactly the threshold: no FMA contraction
    for f in (ops.voc_match, ops.voc_ap, evaluate.finalize_device, evaluate.evaluate_voc):
        assert callable(f)
    L = _lib.lib()
    assert L.effdet_voc_ap_workspace_bytes.restype is ctypes.c_longlong
    assert L.effdet_voc_ap_workspace_bytes(ctypes.c_longlong(495200)) >= 495200 * 24      # sort ping-pong: 2 x (8 B key + 4 B index)


def test_voc_meter_rejects_bad_arguments():
    from efficientdet.pytorch_amd.evaluate import VOCMeanAP
    with pytest.raises(ValueError):
        VOCMeanAP(0, device='cpu')
    with pytest.raises(ValueError):
        VOCMeanAP(70000, device='cpu')
    m = VOCMeanAP(20, device='cpu')
    dets, counts = torch.zeros(2, 100, 6), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match=r'\[n, 5\]'):
        m.add(dets, counts, [np.zeros((3, 4)), np.zeros((0, 5))])           # wrong width
    with pytest.raises(ValueError, match='ground-truth arrays'):
        m.add(dets, counts, [np.zeros((0, 5))])                              # one array for two images
    with pytest.raises(ValueError, match='at most'):
        m.add(dets, counts, [np.zeros((2049, 5)), np.zeros((0, 5))])
    with pytest.raises(ValueError, match='float64'):
        m.add(dets, counts, (torch.zeros(2, 3, 4), torch.zeros(2, 3, dtype=torch.int32)))
    with pytest.raises(ValueError, match=r'\[B, max_det, 6\]'):
        m.add(torch.zeros(2, 100, 5), counts, [np.zeros((0, 5))] * 2)
    assert m.num_records == 0                                               # nothing was appended


def test_voc_golden_is_self_consistent(golden_dir):
    """The recorded recall / precision arrays (what the reference's evaluate handed _compute_ap) give the recorded APs and mean."""
    g = np.load(os.path.join(golden_dir, 'voc_map.npz'), allow_pickle=False)
    NC = int(g['num_classes'])
    ap, nann, classes = g['ap'], g['num_annotations'], [int(c) for c in g['curve_classes']]
    assert classes == [c for c in range(NC) if nann[c] > 0]
    assert any(nann == 0) and any(len(g['recall%d' % c]) == 0 for c in classes)      # a class without GT; one without detections
    for c in classes:
        r, p = g['recall%d' % c], g['precision%d' % c]
        assert r.dtype == np.float64 and p.dtype == np.float64 and r.shape == p.shape
        assert np.all(np.diff(r) >= 0) and (len(r) == 0 or r[-1] <= 1.0)
        assert _compute_ap(r, p) == ap[c], c
    assert all(ap[c] == 0 for c in range(NC) if nann[c] == 0)
    assert np.mean(list(ap)) == g['mean_ap']
