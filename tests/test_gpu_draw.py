"""GPU tier of the device renderer (csrc/draw.hip, ops.draw_detections): every case of tests/draw_cases.py, painted on the device inside
a sentinel-filled buffer, equals the sequential restatement (tests/draw_restated.py) byte for byte -- guards included.  Also: two calls
give equal bytes, a frame with count 0 is its input, the out-of-place form leaves the input alone, the Python refusals come before a
launch, and a captured call replays on new frames and rows."""
import numpy as np
import pytest
import torch

from tests import draw_cases as C

pytestmark = pytest.mark.gpu
GUARD, SENTINEL = 253, 0xA5                                                        # an odd guard: frames start at odd addresses


def _dev():
    return torch.device('cuda', 0)


def _layout(c):
    """-> (host buffer with guards before, between and after the frames, offsets of the frames in it)."""
    gap = GUARD if c['mixed'] else 0                                               # the dense form is one [B, H, W, 3] block
    offs, n = [], GUARD
    for f in c['frames']:
        offs.append(n)
        n += f.size + gap
    n += GUARD - gap
    buf = np.full(n, SENTINEL, dtype=np.uint8)
    return buf, offs


def _filled(c, frames):
    buf, offs = _layout(c)
    for off, f in zip(offs, frames):
        buf[off:off + f.size] = f.reshape(-1)
    return buf, offs


def _tables(c, dev):
    from efficientdet.pytorch_amd import ops
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    return dict(rows=t(c['rows']), counts=t(c['counts']), ids=t(c['ids']), box_scale=t(c['scale']), names=ops.draw_names(c['names'], dev),
                palette=t(c['palette']), options=ops.DrawOptions(**c['opts']))


def _run(c, frames=None, tables=None):
    """Paints c's frames (or `frames`) in place inside the guarded buffer -> the whole buffer back on the host."""
    from efficientdet.pytorch_amd import ops
    dev = _dev()
    host, offs = _filled(c, c['frames'] if frames is None else frames)
    buf = torch.from_numpy(host).to(dev)
    tb = _tables(c, dev) if tables is None else tables
    if c['mixed']:
        off = torch.tensor(offs, dtype=torch.int64, device=dev)
        hw = torch.tensor(c['sizes'], dtype=torch.int32, device=dev)
        out = ops.draw_detections((buf, off, hw), inplace=True, max_hw=c['max_hw'], **tb)
        assert out is buf
    else:
        (H, W), B = c['sizes'][0], len(c['sizes'])
        view = buf[GUARD:GUARD + B * H * W * 3].view(B, H, W, 3)
        out = ops.draw_detections(view, inplace=True, **tb)
        assert out is view
    return buf.cpu().numpy()


@pytest.mark.parametrize('name', C.NAMES_OF_CASES)
def test_the_device_equals_the_restatement(name):
    c = C.case(name)
    want, _ = _filled(c, C.expected(name))
    got = _run(c)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError('%s: %d bytes differ, first at %d (got %d, want %d)' % (name, bad.size, bad[0], got[bad[0]], want[bad[0]]))
    assert np.array_equal(_run(c), got)                                            # two calls on equal input give equal bytes


def test_a_frame_with_no_rows_is_its_input():
    c = C.case('counts')
    painted = C.expected('counts')
    for b in (0, 1):                                                               # counts 0 and -3
        assert np.array_equal(painted[b], c['frames'][b])
    assert not np.array_equal(painted[2], c['frames'][2]) and not np.array_equal(painted[2], painted[3])      # counts 8 (> K) and 2


def test_out_of_place_and_the_python_refusals():
    from efficientdet.pytorch_amd import ops
    c, dev = C.case('alpha128'), _dev()
    tb = _tables(c, dev)
    frames = torch.from_numpy(np.stack(c['frames'])).to(dev)
    keep = frames.clone()
    out = ops.draw_detections(frames, **tb)
    assert out is not frames and torch.equal(frames, keep) and np.array_equal(out.cpu().numpy(), np.stack(C.expected('alpha128')))
    no_ids = dict(tb, ids=None)
    for bad in (dict(options=ops.DrawOptions(show_id=True)), dict(options=ops.DrawOptions(color_by='id'))):
        with pytest.raises(ValueError):
            ops.draw_detections(frames, inplace=True, **dict(no_ids, **bad))
    with pytest.raises(ValueError):
        ops.draw_detections(frames, inplace=True, **dict(tb, rows=tb['rows'][:, :, :5].contiguous()))
    with pytest.raises(ValueError):
        ops.draw_detections(frames, inplace=True, **dict(tb, rows=torch.zeros((1, 1025, 6), device=dev)))
    with pytest.raises(ValueError):
        ops.draw_detections(frames, inplace=True, **dict(tb, palette=torch.zeros((0, 3), dtype=torch.uint8, device=dev)))
    with pytest.raises(ValueError):
        ops.draw_detections(frames, inplace=True, max_hw=(64, 64), **tb)
    with pytest.raises(TypeError):
        ops.draw_detections(frames, inplace=True, **dict(tb, options=dict(thickness=1)))
    assert torch.equal(frames, keep)                                               # every refusal came before a launch
    # the default palette and a host (sx, sy) pair
    d = dict(tb, palette=None, box_scale=(0.5, 0.75))
    want = C.paint_case(dict(c, palette=ops.draw_palette_host(64), scale=np.array([[0.5, 0.75]], dtype=np.float32)))
    assert np.array_equal(ops.draw_detections(frames, **d).cpu().numpy(), np.stack(want))


def test_a_captured_call_replays_on_new_frames_and_rows():
    from efficientdet.pytorch_amd import ops
    a, b, dev = C.case('alpha128'), C.case('t0_label'), _dev()                      # same frame size and K, other pixels and rows
    assert a['sizes'] == b['sizes'] and a['rows'].shape == b['rows'].shape
    opts = dict(a['opts'])
    tb = _tables(a, dev)
    static = torch.from_numpy(np.stack(a['frames'])).to(dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.draw_detections(static.clone(), inplace=True, **tb)                    # warm-up: the library and the kernel are loaded
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.draw_detections(static, inplace=True, **tb)
    assert out is static
    static.copy_(torch.from_numpy(np.stack(b['frames'])))
    tb['rows'].copy_(torch.from_numpy(b['rows']))
    tb['counts'].copy_(torch.from_numpy(b['counts']))
    graph.replay()
    torch.cuda.synchronize()
    eager = ops.draw_detections(torch.from_numpy(np.stack(b['frames'])).to(dev), inplace=True, **tb)
    want = C.paint_case(dict(b, opts=opts))                                        # b's frames and rows under the captured options
    assert torch.equal(static, eager) and np.array_equal(static.cpu().numpy(), np.stack(want))
