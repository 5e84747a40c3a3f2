"""CPU tier: the host half of the JPEG decoder (effdet_jpeg_probe, effdet_jpeg_entropy_batch) and the NumPy restatement against the
goldens of tools/make_jpeg_golden.py (tests/golden/jpeg_cases.npz: streams, Pillow / libjpeg-turbo pixels, coefficients).  Builds and
loads the library; no GPU call.  Every comparison is exact.

Documented behaviour for a truncated or corrupt scan: that image alone fails (status EFFDET_EINVAL in its descriptor), its
coefficient range is zero and it gets no workgroups."""
import ctypes
import io
import os

import numpy as np
import pytest

from tests import jpeg_restated as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'jpeg_cases.npz')
EINVAL, EUNSUPPORTED = -1, -3
CANARY = 0xA5
PAD = 64                                            # canary bytes in front of and behind every image's coefficient range


@pytest.fixture(scope='module')
def G():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


@pytest.fixture(scope='module')
def ops():
    from efficientdet.pytorch_amd import build, ops
    build.build(verbose=False)
    return ops


def names(G):
    return [str(n) for n in G['names']]


def stream(G, name):
    return G[name + '/jpg'].tobytes()


def run_batch(ops, streams, threads, sizes=None):
    """-> (status, totals, coef buffer with canaries, offsets, sizes, descriptor bytes)."""
    if sizes is None:
        sizes = []
        for s in streams:
            st, info = ops.jpeg_probe(s)
            assert st == 0
            sizes.append(int(info.coef_bytes))
    offs, end = [], 0
    for n in sizes:
        offs.append(end + PAD)
        end += PAD + n
    coef = np.full(end + PAD, CANARY, dtype=np.uint8)
    desc = np.zeros(len(streams) * ops.JPEG_DESC_BYTES, dtype=np.uint8)
    status, totals = ops.jpeg_entropy_batch(streams, coef, offs, desc, threads)
    return status, totals, coef, offs, sizes, desc


def canaries_intact(coef, offs, sizes):
    keep = np.ones(coef.size, dtype=bool)
    for o, n in zip(offs, sizes):
        keep[o:o + n] = False
    return bool((coef[keep] == CANARY).all())


def test_case_list_is_the_one_the_tool_writes(G):
    ns = names(G)
    for w, h in ((1, 1), (8, 8), (16, 16), (17, 9), (19, 16), (33, 47)):
        for sub in (0, 1, 2):
            assert '%dx%d_s%d' % (w, h, sub) in ns
    for n in ('9x20_grey', '16x16_grey', '33x47_s2_rst2', '33x47_s0_rst2', '19x16_s2_opt', '19x16_s2_noopt', '33x47_s1_q100',
              '33x47_s2_q5', '17x9_s2_qtables'):
        assert n in ns
    assert sorted(str(n) for n in G['rejected']) == ['progressive', 'truncated_header', 'truncated_scan']
    assert os.path.getsize(GOLDEN) < 200 * 1024
    q5 = G['33x47_s2_q5/rgb']
    assert q5.min() == 0 and q5.max() == 255                       # the clamp at both ends is exercised
    scans = [stream(G, n)[R.parse(stream(G, n)).scan:] for n in ns]
    assert any(b'\xff\x00' in s for s in scans) and any(b'\xff\xd0' in s for s in scans)


def test_restatement_equals_the_golden_pixels(G):
    for n in names(G):
        got = R.decode(stream(G, n))
        assert got.dtype == np.uint8 and got.shape == G[n + '/rgb'].shape, n
        assert np.array_equal(got, G[n + '/rgb']), n
        assert np.array_equal(R.coefficients(stream(G, n)), G[n + '/coef']), n


def test_restatement_equals_a_fresh_pillow_decode(G):
    Image = pytest.importorskip('PIL.Image')
    for n in names(G):
        want = np.asarray(Image.open(io.BytesIO(stream(G, n))).convert('RGB'))
        assert np.array_equal(R.decode(stream(G, n)), want), n


def test_restatement_rejects_the_rejected(G):
    with pytest.raises(R.Unsupported):
        R.decode(stream(G, 'progressive'))
    for n in ('truncated_header', 'truncated_scan'):
        with pytest.raises(ValueError):
            R.decode(stream(G, n))


def test_entry_points_are_declared_and_bound(ops):
    from efficientdet.pytorch_amd import _lib, build, data
    for name in ('effdet_jpeg_probe', 'effdet_jpeg_entropy_batch', 'effdet_jpeg_reconstruct'):
        assert name in _lib.SYMBOLS and hasattr(_lib.lib(), name), name
    assert 'jpeg.hip' not in build.PER_FILE                        # integer arithmetic only: no fp-contract entry
    for f in (ops.jpeg_probe, ops.jpeg_entropy_batch, ops.jpeg_reconstruct, data.decode_jpeg_batch):
        assert callable(f)
    assert issubclass(data.UnsupportedJPEG, ValueError)
    assert ctypes.sizeof(_lib.JpegDesc) % 16 == 0 and _lib.JpegDesc.qt.offset % 16 == 0        # the kernels' 16 B table loads


def test_struct_mirrors_match_the_header_as_gcc_sees_it(ops, tmp_path):
    import shutil
    import subprocess
    from efficientdet.pytorch_amd import _lib
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = ['sizeof(effdet_jpeg_info_t)', 'sizeof(effdet_jpeg_desc_t)', 'offsetof(effdet_jpeg_info_t, coef_bytes)',
              'offsetof(effdet_jpeg_desc_t, status)', 'offsetof(effdet_jpeg_desc_t, rgb_wg0)', 'offsetof(effdet_jpeg_desc_t, coef_off)',
              'offsetof(effdet_jpeg_desc_t, qt)']
    src = tmp_path / 'sz.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "effdet_hip.h"\nint main(void){' +
                   ''.join('printf("%%zu\\n", %s);' % f for f in fields) + 'return 0;}\n')
    subprocess.run(['gcc', '-I', os.path.join(root, 'include'), str(src), '-o', str(tmp_path / 'sz')], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / 'sz')], capture_output=True, text=True, check=True).stdout.split()]
    I, D = _lib.JpegInfo, _lib.JpegDesc
    assert got == [ctypes.sizeof(I), ctypes.sizeof(D), I.coef_bytes.offset, D.status.offset, D.rgb_wg0.offset, D.coef_off.offset, D.qt.offset]


def test_probe_fields(G, ops):
    for n in names(G):
        s = stream(G, n)
        hd = R.parse(s)
        st, info = ops.jpeg_probe(s)
        assert st == 0 and info.reason == 0, n
        h, w = G[n + '/rgb'].shape[:2]
        assert (info.width, info.height) == (w, h) == (hd.width, hd.height), n
        assert info.ncomp == len(hd.comps) and info.sampling == hd.sampling, n
        assert info.restart_interval == hd.restart, n
        assert (info.mcus_x, info.mcus_y) == (hd.mcus_x, hd.mcus_y), n
        blocks = hd.blocks + [(0, 0)] * (3 - len(hd.blocks))
        assert [(info.blocks_h[c], info.blocks_w[c]) for c in range(3)] == blocks, n
        assert info.coef_bytes == 128 * sum(r * c for r, c in blocks) == 2 * G[n + '/coef'].size, n
    # the grids, spelled out for one case per sampling class: 33 x 47
    want = {'33x47_s0': (ops.JPEG_444, 5, 6, [5, 5, 5], [6, 6, 6]), '33x47_s1': (ops.JPEG_422, 3, 6, [6, 3, 3], [6, 6, 6]),
            '33x47_s2': (ops.JPEG_420, 3, 3, [6, 3, 3], [6, 3, 3]), '9x20_grey': (ops.JPEG_GREY, 2, 3, [2, 0, 0], [3, 0, 0])}
    for n, (sampling, mx, my, bw, bh) in want.items():
        _, info = ops.jpeg_probe(stream(G, n))
        assert (info.sampling, info.mcus_x, info.mcus_y, list(info.blocks_w), list(info.blocks_h)) == (sampling, mx, my, bw, bh), n
    assert ops.jpeg_probe(stream(G, '33x47_s2_rst2'))[1].restart_interval == 2
    assert ops.jpeg_probe(stream(G, '33x47_s2'))[1].restart_interval == 0


def test_probe_refusals(G, ops):
    st, info = ops.jpeg_probe(stream(G, 'progressive'))
    assert st == EUNSUPPORTED and info.reason == 1 and 'progressive' in ops.JPEG_REASONS[info.reason]
    st, info = ops.jpeg_probe(stream(G, 'truncated_header'))
    assert st == EINVAL
    good = stream(G, '33x47_s2')
    for cut in (0, 1, 2, 3, 4, 20, R.parse(good).scan - 1):       # every prefix that ends inside the header
        assert ops.jpeg_probe(good[:cut])[0] == EINVAL, cut
    assert ops.jpeg_probe(b'\x89PNG\r\n\x1a\n' + bytes(64))[0] == EINVAL
    assert ops.jpeg_probe(stream(G, 'truncated_scan'))[0] == 0    # the header is whole: the scan fails in the entropy stage

    def patched(at, value):
        b = bytearray(good)
        b[at] = value
        return bytes(b)
    sof = good.index(b'\xff\xc0')
    for at, value, reason in ((sof + 1, 0xC1, 2), (sof + 1, 0xC9, 2), (sof + 1, 0xC3, 2), (sof + 4, 12, 3), (sof + 9, 4, 5),
                              (sof + 11, 0x12, 6), (sof + 11, 0x41, 6), (good.index(b'\xff\xdb') + 4, 0x10, 4),
                              (good.index(b'\xff\xda') + 4, 1, 7)):
        st, info = ops.jpeg_probe(patched(at, value))
        assert (st, info.reason) == (EUNSUPPORTED, reason), (at, value, st, info.reason)


def test_coefficients_and_tables_equal_the_restatement(G, ops):
    ns = names(G)
    streams = [stream(G, n) for n in ns]
    status, totals, coef, offs, sizes, desc = run_batch(ops, streams, 4)
    assert status == 0
    ds = ops.jpeg_descs(desc, len(ns))
    wg1 = wg2 = 0
    for b, n in enumerate(ns):
        d = ds[b]
        assert d.status == 0, n
        assert np.array_equal(coef[offs[b]:offs[b] + sizes[b]].view(np.int16), G[n + '/coef']), n
        assert np.array_equal(np.array(d.qt, dtype=np.uint16), R.quant_tables(streams[b])), n
        h, w = G[n + '/rgb'].shape[:2]
        hd = R.parse(streams[b])
        assert (d.height, d.width, d.ncomp, d.sampling) == (h, w, len(hd.comps), hd.sampling), n
        nblk = [r * c for r, c in hd.blocks] + [0, 0]
        assert list(d.coef_off) == [offs[b], offs[b] + 128 * nblk[0], offs[b] + 128 * (nblk[0] + nblk[1])], n
        assert (d.idct_wg0, d.rgb_wg0) == (wg1, wg2), n
        wg1 += -(-sum(nblk) // 32)
        wg2 += -(-h * w * 3 // 4096)
    assert totals == (wg1, wg2)
    assert canaries_intact(coef, offs, sizes)


def test_thread_counts_agree(G, ops):
    ns = (names(G) * 2)[5:17]                                      # 12 images
    assert len(ns) == 12
    streams = [stream(G, n) for n in ns]
    runs = {t: run_batch(ops, streams, t) for t in (1, 3, 16, 0, 1000)}          # 0 and 1000 are clamped to 1 and 16
    for t, r in runs.items():
        assert r[0] == 0 and canaries_intact(r[2], r[3], r[4]), t
        assert np.array_equal(r[2], runs[1][2]) and np.array_equal(r[5], runs[1][5]) and r[1] == runs[1][1], t


def test_truncated_scan_fails_that_image_alone(G, ops):
    good = [stream(G, '33x47_s2'), stream(G, '17x9_s1')]
    bad = stream(G, 'truncated_scan')
    streams = [good[0], bad, good[1]]
    status, totals, coef, offs, sizes, desc = run_batch(ops, streams, 2)
    assert status == EINVAL
    ds = ops.jpeg_descs(desc, 3)
    assert [d.status for d in ds] == [0, EINVAL, 0]
    assert not coef[offs[1]:offs[1] + sizes[1]].any()              # the failed image's range is zero ...
    assert ds[1].idct_wg0 == ds[2].idct_wg0 and ds[1].rgb_wg0 == ds[2].rgb_wg0        # ... and it owns no workgroups
    alone = run_batch(ops, [good[0], good[1]], 1)
    assert totals == alone[1]
    for b, n in ((0, '33x47_s2'), (2, '17x9_s1')):
        assert np.array_equal(coef[offs[b]:offs[b] + sizes[b]].view(np.int16), G[n + '/coef'])
    assert canaries_intact(coef, offs, sizes)


def test_no_write_outside_the_range_under_corrupt_input(G, ops):
    """Truncations at every length and seeded byte damage inside the scan: each image decodes or fails, and in both cases only its
    own coefficient range changes."""
    base = stream(G, '33x47_s2_rst2')
    scan = R.parse(base).scan
    size = int(ops.jpeg_probe(base)[1].coef_bytes)
    variants = [base[:n] for n in range(scan, len(base), 7)]
    rng = np.random.RandomState(0)
    for _ in range(64):
        b = bytearray(base)
        for at in rng.randint(scan, len(base), size=3):
            b[at] = rng.randint(0, 256)
        variants.append(bytes(b))
    variants += [stream(G, 'truncated_scan'), stream(G, 'truncated_header'), stream(G, 'progressive')]
    status, _, coef, offs, sizes, desc = run_batch(ops, variants, 8, sizes=[size] * len(variants))
    assert status in (EINVAL, EUNSUPPORTED)
    assert canaries_intact(coef, offs, sizes)
    ds = ops.jpeg_descs(desc, len(variants))
    assert [d.status for d in ds[len(variants) - 3:]] == [EINVAL, EINVAL, EUNSUPPORTED]
    assert all(d.status in (0, EINVAL, EUNSUPPORTED) for d in ds)
    assert all(d.status == EINVAL for d in ds[:len(range(scan, len(base) - 2, 7))])   # a scan cut before its last bytes never decodes
    for b, d in enumerate(ds):                                    # a failed scan leaves zeros, a refused header leaves the range alone
        own = coef[offs[b]:offs[b] + sizes[b]]
        if d.status != 0:
            assert (own == CANARY).all() if b >= len(variants) - 2 else not own.any(), b


def test_range_too_small_is_refused_without_a_write(G, ops):
    s = stream(G, '33x47_s0')
    size = int(ops.jpeg_probe(s)[1].coef_bytes)
    coef = np.full(size - 128, CANARY, dtype=np.uint8)
    desc = np.zeros(ops.JPEG_DESC_BYTES, dtype=np.uint8)
    status, _ = ops.jpeg_entropy_batch([s], coef, [0], desc, 1)
    assert status == EINVAL and (coef == CANARY).all()
