"""Write tests/golden/jpeg_cases.npz: the JPEG streams, the OUTSIDE decoder's pixels and the restatement's coefficients that
tests/test_jpeg_host.py and tests/test_gpu_jpeg.py pin the decoder of csrc/jpeg.hip on.  Needs Pillow (with libjpeg-turbo).

    python tools/make_jpeg_golden.py

For every accepted case the tool asserts tests/jpeg_restated.decode(bytes) == Image.open(bytes).convert('RGB') exactly before it
writes anything, so the restatement is pinned on libjpeg-turbo and the goldens hold that decoder's pixels, not ours.

Keys: 'names' (accepted cases), 'rejected' (names), and per case '<name>/jpg' uint8 bytes, '<name>/rgb' uint8 [H,W,3] (Pillow),
'<name>/coef' int16 (restatement, library layout)."""
import io
import os
import sys

import numpy as np
from PIL import Image, features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import jpeg_restated as R  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'jpeg_cases.npz')
SIZES = ((1, 1), (8, 8), (16, 16), (17, 9), (19, 16), (33, 47))      # W x H


def source(w, h, seed, noise=0.5):
    """Smooth gradients plus seeded noise, uint8 [h, w, 3]; noise=1: full-contrast noise alone."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    grad = np.stack([255 * xx / max(w - 1, 1), 255 * yy / max(h - 1, 1), 255 * (xx + yy) / max(w + h - 2, 1)], -1)
    if noise >= 1:
        return (rng.randint(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    return np.clip((1 - noise) * grad + noise * rng.randint(0, 256, (h, w, 3)), 0, 255).astype(np.uint8)


def encode(img, mode='RGB', **kw):
    im = Image.fromarray(img if mode == 'RGB' else img[:, :, 0], mode)
    buf = io.BytesIO()
    kw.setdefault('quality', 85)
    kw.setdefault('progressive', False)
    im.save(buf, 'JPEG', **kw)
    return buf.getvalue()


def cases():
    out, seed = {}, 0
    for w, h in SIZES:
        for sub in (0, 1, 2):
            seed += 1
            out['%dx%d_s%d' % (w, h, sub)] = encode(source(w, h, seed), subsampling=sub)
    out['9x20_grey'] = encode(source(9, 20, 101), 'L')
    out['16x16_grey'] = encode(source(16, 16, 102), 'L')
    out['33x47_s2_rst2'] = encode(source(33, 47, 103), subsampling=2, restart_marker_blocks=2)
    out['33x47_s0_rst2'] = encode(source(33, 47, 104), subsampling=0, restart_marker_blocks=2)
    out['19x16_s2_opt'] = encode(source(19, 16, 105), subsampling=2, optimize=True)
    out['19x16_s2_noopt'] = encode(source(19, 16, 105), subsampling=2, optimize=False)
    out['33x47_s1_q100'] = encode(source(33, 47, 106, noise=0.8), subsampling=1, quality=100)
    out['33x47_s2_q5'] = encode(source(33, 47, 107, noise=1), subsampling=2, quality=5)
    qt = [[(3 + 5 * k) % 97 + 1 for k in range(64)], [(7 + 11 * k) % 61 + 2 for k in range(64)]]
    out['17x9_s2_qtables'] = encode(source(17, 9, 108), subsampling=2, qtables=qt)
    return out


def rejected():
    good = encode(source(33, 47, 201), subsampling=2)
    scan = R.parse(good).scan
    return {'progressive': encode(source(16, 16, 202), subsampling=2, progressive=True),
            'truncated_scan': good[:scan + (len(good) - scan) // 2],
            'truncated_header': good[:good.index(b'\xff\xc0') + 7]}


def main():
    print('Pillow %s, libjpeg %s (turbo: %s)' % (Image.__version__ if hasattr(Image, '__version__') else features.version('pil'),
                                                 features.version('jpg'), features.check_feature('libjpeg_turbo')))
    arrays, names = {}, []
    stuffed = restarts = 0
    for name, data in cases().items():
        hd = R.parse(data)
        assert (hd.width, hd.height) == Image.open(io.BytesIO(data)).size
        want = np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))
        got = R.decode(data)
        assert got.shape == want.shape and np.array_equal(got, want), \
            '%s: restatement != Pillow at %d pixels' % (name, int((got != want).any(-1).sum()))
        scan = data[hd.scan:]
        stuffed += b'\xff\x00' in scan
        restarts += any(bytes([0xFF, 0xD0 + k]) in scan for k in range(8))
        arrays[name + '/jpg'] = np.frombuffer(data, dtype=np.uint8)
        arrays[name + '/rgb'] = want
        arrays[name + '/coef'] = R.coefficients(data, hd)
        names.append(name)
        print('%-18s %4d B  sampling %d  restart %d' % (name, len(data), hd.sampling, hd.restart))
    assert stuffed >= 1 and restarts >= 1, (stuffed, restarts)
    bad = rejected()
    assert b'\xff\xc2' in bad['progressive']
    for name, data in bad.items():
        try:
            R.decode(data)
        except ValueError:
            pass
        else:
            raise AssertionError('%s was not rejected' % name)
        arrays[name + '/jpg'] = np.frombuffer(data, dtype=np.uint8)
    np.savez_compressed(OUT, names=np.array(names), rejected=np.array(sorted(bad)), **arrays)
    size = os.path.getsize(OUT)
    assert size < 200 * 1024, size
    print('%d accepted + %d rejected cases, %d scans with FF 00, %d with RSTn -> %s (%d bytes)'
          % (len(names), len(bad), stuffed, restarts, os.path.relpath(OUT, ROOT), size))


if __name__ == '__main__':
    main()
