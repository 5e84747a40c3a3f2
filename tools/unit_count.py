"""Go / no-go count for compacting the regression tower's needed 32-pixel units into dense 128-pixel tiles (no GPU needed).

The flagged launches of the RetinaHead's regression tower (include/effdet_needed_tiles.h forwards, include/effdet_live_tiles.h
backwards) compute every 128-pixel flat tile that holds a flagged pixel.  If they gathered the flagged 32-PIXEL units of a launch
into dense tiles instead, they would compute ceil(units / 4) tiles.  This script restates the flag geometry of csrc/live_tiles.hip in
numpy and counts both for the benchmark's batch -- synthetic_batch(32, 512, seed=1), default matcher -- at every radius 0..5:

  map      level-major bytes, level l holding its B * H * W pixels in (b, h, w) order: 1 iff one of the pixel's 9 anchors has
           IoU >= 0.5 with its best annotation (an image without a valid annotation row has none);
  d        Chebyshev distance of a pixel to the nearest set pixel of its own image and level, capped at 6;
  live32   [6][steps]: step s of radius r is 1 iff min d over its 32 pixels <= r.  A level's steps cover its linear pixel index
           M = B * H * W, the last one possibly partial; levels are concatenated;
  live128  [6][tiles] likewise over 128 pixels;
  units    [r]: the indices of the set live32 flags, ascending (level-major, the order of the flags), n_units[r] their count.

16-pixel units are printed as a note only.  One JSON document on stdout.

    python tools/unit_count.py > profiles/unit_count_b32_512.json"""
import json
import os
import sys

import numpy as np

RADII = 6                                    # EFFDET_LIVE_RADII


def level_sizes(S, nlev=5):
    return [(S >> (3 + i), S >> (3 + i)) for i in range(nlev)]


def positive_pixel_map(anc, ann, sizes):
    """anc [A][4] fp32 with A = 9 * sum H*W (anchor 9 * pixel + k, pixels level-major within an image), ann [B][N][5] (label -1 = pad
    row) -> the level-major byte map.  IoU in separately rounded fp32 steps, as the loss's assign pass computes it."""
    anc = np.asarray(anc, dtype=np.float32).reshape(-1, 4)
    ann = np.asarray(ann, dtype=np.float32)
    B = ann.shape[0]
    apix = sum(h * w for h, w in sizes)
    assert anc.shape[0] == 9 * apix
    pos = np.zeros((B, apix), dtype=np.uint8)
    aarea = (anc[:, 2] - anc[:, 0]) * (anc[:, 3] - anc[:, 1])
    for b in range(B):
        box = ann[b][ann[b, :, 4] != -1][:, :4]
        if len(box) == 0:
            continue
        barea = (box[:, 2] - box[:, 0]) * (box[:, 3] - box[:, 1])
        iw = np.maximum(np.minimum(anc[:, None, 2], box[None, :, 2]) - np.maximum(anc[:, None, 0], box[None, :, 0]), np.float32(0))
        ih = np.maximum(np.minimum(anc[:, None, 3], box[None, :, 3]) - np.maximum(anc[:, None, 1], box[None, :, 1]), np.float32(0))
        ua = np.maximum(aarea[:, None] + barea[None, :] - iw * ih, np.float32(1e-8))
        best = (iw * ih / ua).max(axis=1)
        pos[b] = (best >= np.float32(0.5)).reshape(apix, 9).any(axis=1)
    out, o = [], 0
    for h, w in sizes:
        out.append(pos[:, o:o + h * w].reshape(-1))
        o += h * w
    return np.concatenate(out)


def chebyshev(m):
    """m [B][H][W] bool -> int [B][H][W]: distance to the nearest set pixel of the same image, capped at RADII"""
    d = np.full(m.shape, RADII, dtype=np.int64)
    cur = m.astype(bool)
    d[cur] = 0
    for r in range(1, RADII):
        p = np.pad(cur, ((0, 0), (1, 1), (1, 1)))
        nxt = np.zeros_like(cur)
        for dy in range(3):
            for dx in range(3):
                nxt |= p[:, dy:dy + m.shape[1], dx:dx + m.shape[2]]
        d[nxt & ~cur] = r
        cur = nxt
    return d


def unit_flags(pmap, B, sizes, unit):
    """-> uint8 [RADII][units over all levels] for units of `unit` pixels of each level's linear index (32: live32, 128: live128)"""
    pmap = np.asarray(pmap).reshape(-1)
    assert pmap.size == B * sum(h * w for h, w in sizes)
    cols, o = [], 0
    for h, w in sizes:
        M = B * h * w
        d = chebyshev(pmap[o:o + M].reshape(B, h, w) != 0).reshape(-1)
        n = (M + unit - 1) // unit
        d = np.concatenate([d, np.full(n * unit - M, RADII, dtype=d.dtype)]).reshape(n, unit).min(axis=1)
        cols.append(np.stack([(d <= r) for r in range(RADII)]).astype(np.uint8))
        o += M
    return np.concatenate(cols, axis=1)


def unit_lists(flags32):
    """-> ([RADII] int32 arrays of the set flags' indices, ascending; [RADII] counts)"""
    units = [np.flatnonzero(flags32[r]).astype(np.int32) for r in range(flags32.shape[0])]
    return units, [int(len(u)) for u in units]


def level_of_unit(B, sizes, unit):
    """-> (first unit of each level, units over all levels)"""
    first, o = [], 0
    for h, w in sizes:
        first.append(o)
        o += (B * h * w + unit - 1) // unit
    return first, o


def count_table(pmap, B, sizes):
    """per radius: live 128-pixel tiles, live 32-pixel units, ceil(units / 4) and their ratio; the same per level; 16-pixel units as a
    note"""
    f128, f32, f16 = (unit_flags(pmap, B, sizes, u) for u in (128, 32, 16))
    t0, ntile = level_of_unit(B, sizes, 128)
    s0, nstep = level_of_unit(B, sizes, 32)
    rows = []
    for r in range(RADII):
        t, u, u16 = int(f128[r].sum()), int(f32[r].sum()), int(f16[r].sum())
        g = (u + 3) // 4
        per_level = []
        for l, (h, w) in enumerate(sizes):
            te = t0[l + 1] if l + 1 < len(sizes) else ntile
            se = s0[l + 1] if l + 1 < len(sizes) else nstep
            tl, ul = int(f128[r, t0[l]:te].sum()), int(f32[r, s0[l]:se].sum())
            per_level.append({'level': '%dx%d' % (h, w), 'tiles': te - t0[l], 'live128': tl, 'live32': ul,
                              'pixel_ratio': round(ul / (4.0 * tl), 4) if tl else None})
        rows.append({'radius': r, 'live128': t, 'live128_fraction': round(t / ntile, 4), 'live32': u, 'gathered_tiles': g,
                     'ratio': round(g / t, 4) if t else None, 'per_level': per_level,
                     'note_live16': u16, 'note_gathered_tiles_16': (u16 + 7) // 8})
    return {'tiles': ntile, 'steps': nstep, 'radii': rows}


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from efficientdet.pytorch_amd.synthetic import synthetic_batch
    from oracle.effdet_oracle import anchors_for_image
    B, S = 32, 512
    sizes = level_sizes(S)
    ann = synthetic_batch(B, S, seed=1, num_classes=80)[1].numpy()
    pmap = positive_pixel_map(anchors_for_image(S, S)[0].numpy(), ann, sizes)
    out = {'batch': 'synthetic_batch(%d, %d, seed=1), default matcher' % (B, S), 'positive_pixels': int(pmap.sum()),
           'pixels': int(pmap.size)}
    out.update(count_table(pmap, B, sizes))
    out['go'] = bool(out['radii'][3]['ratio'] <= 0.85)
    json.dump(out, sys.stdout, indent=1)
    print()


if __name__ == '__main__':
    main()
