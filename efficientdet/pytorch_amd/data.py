"""Device-side input pipeline: the work of the reference's Normalizer -> Augmenter -> Resizer ->
collater chain (datasets/augmentation.py:69-150) as ONE HIP launch per batch.

The host only concatenates the decoded uint8 HWC images into a pinned staging buffer (one memcpy per image) and issues
one async H2D copy; bilinear resize to the common size, /255, mean/std normalisation, horizontal flip, zero padding, the
NHWC / compute-dtype / channel-padded pack the stem conv reads, and the annotation rescale all happen on the GPU
(csrc/pipeline.hip::preprocess_kernel).  The float64 512x512x3 canvas of augmentation.py:111, the NCHW permute of the
collater and the model-side NCHW -> NHWC repack disappear.  There is no CPU fallback: the collater needs the GPU.

Samples may carry the file itself ({'jpeg': bytes}) instead of decoded pixels: decode_jpeg_batch then replaces the staging of the
pixels -- Huffman decode on host threads inside the library, coefficients over the same pinned double buffer, and the rest of the
decoder as two HIP launches (csrc/jpeg.hip) that write the uint8 HWC layout the kernels above read."""
import math

import numpy as np
import torch

from . import ops
from .efficientdet import PackedImages
from .functional import chunk_elems

MEAN = (0.485, 0.456, 0.406)       # datasets/augmentation.py:141-142
STD = (0.229, 0.224, 0.225)


class UnsupportedJPEG(ValueError):
    """A valid JPEG outside what csrc/jpeg.hip decodes (one-scan 8-bit baseline, grey or YCbCr 4:4:4 / 4:2:2 / 4:2:0), met without a
    fallback decoder.  index: position in the batch; reason: ops.JPEG_REASONS code."""

    def __init__(self, index, reason):
        super().__init__('JPEG %d of the batch is not baseline (%s) and no decode_fallback was given'
                         % (index, ops.JPEG_REASONS.get(reason, 'reason %d' % reason)))
        self.index, self.reason = index, reason


def _align(n, a=128):
    return (int(n) + a - 1) // a * a


def _decode_jpeg_batch(streams, stager, threads, fallback):
    """decode_jpeg_batch on `stager`'s pinned double buffer -> (src, src_off, src_hw, host hw [B,2] int32)."""
    dev = stager.device
    B = len(streams)
    infos, fb = [], {}
    for b, st in enumerate(streams):                               # 1. probe (host): every refusal is raised before anything is staged
        status, info = ops.jpeg_probe(st)
        if status == -3 and fallback is not None:
            px = np.ascontiguousarray(fallback(st))
            if px.dtype != np.uint8 or px.ndim != 3 or px.shape[2] != 3:
                raise ValueError('decode_fallback must return uint8 [H,W,3] RGB (JPEG %d of the batch)' % b)
            fb[b] = px
        elif status == -3:
            raise UnsupportedJPEG(b, info.reason)
        elif status != 0:
            raise ValueError('JPEG %d of the batch is corrupt: not a JPEG, or its header is cut short' % b)
        infos.append(info)
    dec = [b for b in range(B) if b not in fb]
    hw = np.array([fb[b].shape[:2] if b in fb else (infos[b].height, infos[b].width) for b in range(B)], dtype=np.int32).reshape(B, 2)
    nd = len(dec)
    # one staging block = one H2D copy: [descriptors | planes_off | dst_off | src_off | src_hw | coefficients | fallback pixels]; the
    # device buffer continues with the decoded images, and src starts at the fallback pixels
    o_desc = 0
    o_poff = _align(o_desc + nd * ops.JPEG_DESC_BYTES)
    o_doff = _align(o_poff + 8 * nd)
    o_soff = _align(o_doff + 8 * nd)
    o_shw = _align(o_soff + 8 * B)
    o_coef = _align(o_shw + 8 * B)
    coef_off = o_coef + np.concatenate([[0], np.cumsum([infos[b].coef_bytes for b in dec])]).astype(np.int64)    # whole blocks: 128 B each
    o_fb = _align(coef_off[-1])
    src_off = np.zeros(B, dtype=np.int64)
    end = o_fb
    for b in fb:
        src_off[b] = end - o_fb
        end += _align(fb[b].size, 16)
    n_stage = _align(end)
    for b in dec:
        src_off[b] = end - o_fb
        end += _align(int(hw[b, 0]) * int(hw[b, 1]) * 3, 16)
    slot, stage = stager._pinned(n_stage)
    view = stage.numpy()
    wgs = (0, 0)
    if nd:                                                         # 2. entropy decode (host threads) straight into the pinned block
        status, wgs = ops.jpeg_entropy_batch([streams[b] for b in dec], view[:o_fb], coef_off[:-1], view[o_desc:o_poff], threads)
        if status != 0:
            bad = [b for b, d in zip(dec, ops.jpeg_descs(view[o_desc:o_poff], nd)) if d.status != 0]
            raise ValueError('JPEG %d of the batch is corrupt: its scan is truncated or damaged' % bad[0])
        view[o_poff:o_poff + 8 * nd].view(np.int64)[:] = (coef_off[:-1] - o_coef) // 2
        view[o_doff:o_doff + 8 * nd].view(np.int64)[:] = src_off[dec]
    view[o_soff:o_soff + 8 * B].view(np.int64)[:] = src_off
    view[o_shw:o_shw + 8 * B].view(np.int32)[:] = hw.reshape(-1)
    for b, px in fb.items():
        view[o_fb + src_off[b]:o_fb + src_off[b] + px.size] = px.reshape(-1)
    buf = torch.empty(int(end), dtype=torch.uint8, device=dev)
    buf[:n_stage].copy_(stage[:n_stage], non_blocking=True)       # 3. the one async H2D copy; the slot's event guards its reuse
    ev = torch.cuda.Event(); ev.record(); stager._evt[slot] = ev
    src = buf[o_fb:]
    if nd:                                                         # 4. two launches for the whole batch
        planes = torch.empty(max(int(coef_off[-1] - o_coef) // 2, 16), dtype=torch.uint8, device=dev)
        ops.jpeg_reconstruct(buf, buf[o_desc:o_poff], nd, wgs, planes, buf[o_poff:o_poff + 8 * nd].view(torch.int64), src,
                             buf[o_doff:o_doff + 8 * nd].view(torch.int64))
    return src, buf[o_soff:o_soff + 8 * B].view(torch.int64), buf[o_shw:o_shw + 8 * B].view(torch.int32).view(B, 2), hw


_default_stagers = {}


def decode_jpeg_batch(streams, device='cuda', threads=8, fallback=None):
    """Baseline JPEG streams (list of bytes) -> (src uint8, src_off [B] int64, src_hw [B,2] int32) on the device: RGB HWC pixels of
    image b at src[src_off[b]:], rows tightly packed -- the input of ops.preprocess_batch / augment_train / augment_resize.

    The host probes the headers and Huffman-decodes the batch on `threads` workers into a pinned double buffer; one async copy
    carries coefficients and descriptors over; dequantisation, inverse DCT, chroma upsampling and YCbCr -> RGB are two HIP launches
    (csrc/jpeg.hip).  The pixels are libjpeg's (islow IDCT, fancy upsampling) bit for bit; EXIF orientation is not applied.
    A stream outside the baseline subset goes through fallback(bytes) -> uint8 [H,W,3] RGB when given (its pixels ride the same
    copy), else UnsupportedJPEG is raised; a corrupt stream raises ValueError.  Nothing is launched for a batch that raises."""
    dev = torch.device(device)
    if dev not in _default_stagers:
        _default_stagers[dev] = DeviceCollater(device=dev)
    src, d_off, d_hw, _ = _decode_jpeg_batch(list(streams), _default_stagers[dev], threads, fallback)
    return src, d_off, d_hw


class DeviceCollater:
    """collate_fn replacement: ``batch = collater(samples)`` -> (PackedImages, annotations [B,M,5] fp32 device, scales [B]).

    samples: list of dicts {'img': uint8 ndarray [H,W,3] RGB, 'annot': float ndarray [n,5]} -- what the reference's
    datasets yield BEFORE its transform chain (the chain runs here, on the device).  flip_x: probability of the
    Augmenter's horizontal flip (0 disables; eval pipelines have none).
    A batch may carry {'jpeg': bytes} in place of 'img' in EVERY sample: the files are then decoded by decode_jpeg_batch
    (decode_threads host workers for the entropy stage, decode_fallback for streams that are not baseline)."""

    def __init__(self, common_size=512, dtype=torch.bfloat16, device='cuda', flip_x=0.0, seed=0, decode_threads=8, decode_fallback=None):
        self.S, self.dtype, self.device = int(common_size), dtype, torch.device(device)
        self.decode_threads, self.decode_fallback = int(decode_threads), decode_fallback
        self.flip_x = float(flip_x)
        self.rng = np.random.RandomState(seed)
        self._stage = [None, None]      # two pinned staging buffers: batch k+1 is assembled while batch k's copy is in flight
        self._evt = [None, None]
        self._slot = 0

    def _pinned(self, nbytes):
        s = self._slot; self._slot ^= 1
        if self._evt[s] is not None:
            self._evt[s].synchronize()
        if self._stage[s] is None or self._stage[s].numel() < nbytes:
            self._stage[s] = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8).pin_memory()
        return s, self._stage[s]

    def _stage_batch(self, samples):
        """-> None for a batch of {'jpeg': bytes} samples (decoded in _upload), else _stage_images(samples)."""
        n_jpeg = sum('jpeg' in s for s in samples)
        if n_jpeg and (n_jpeg != len(samples) or any('img' in s for s in samples)):
            raise ValueError("a batch carries either 'img' or 'jpeg' in every sample, not a mix")
        return None if n_jpeg else self._stage_images(samples)

    def _upload(self, samples, staged):
        """-> (src, src_off, src_hw on the device, host hw [B,2]): the staged pixels' H2D copy, or the JPEG decode."""
        if staged is None:
            return _decode_jpeg_batch([s['jpeg'] for s in samples], self, self.decode_threads, self.decode_fallback)
        stage, slot, offs, hw = staged
        return self._upload_images(stage, slot, offs, hw) + (hw,)

    def _stage_images(self, samples):
        """Concatenate the decoded images into a pinned staging buffer -> (pinned bytes, slot, offsets [B+1] int64, hw [B,2] int32)."""
        imgs = [np.ascontiguousarray(s['img']) for s in samples]
        for im in imgs:
            if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
                raise ValueError('%s takes decoded uint8 HWC RGB images' % type(self).__name__)
        sizes = [im.size for im in imgs]
        offs = np.concatenate([[0], np.cumsum([(n + 15) // 16 * 16 for n in sizes])]).astype(np.int64)
        slot, stage = self._pinned(int(offs[-1]))
        view = stage.numpy()
        for im, o, n in zip(imgs, offs[:-1], sizes):
            view[o:o + n] = im.reshape(-1)
        hw = np.array([[im.shape[0], im.shape[1]] for im in imgs], dtype=np.int32)
        return stage, slot, offs, hw

    def _upload_images(self, stage, slot, offs, hw):
        """One async H2D copy of the staged bytes (the slot's event guards its reuse) -> (src, src_off, src_hw) on the device."""
        dev = self.device
        src = stage[:int(offs[-1])].to(dev, non_blocking=True)
        ev = torch.cuda.Event(); ev.record(); self._evt[slot] = ev
        d_off = torch.from_numpy(offs[:-1].copy()).to(dev, non_blocking=True)
        d_hw = torch.from_numpy(hw).to(dev, non_blocking=True)
        return src, d_off, d_hw

    @staticmethod
    def _padded_annots(samples):
        M = max(1, max((len(s['annot']) for s in samples), default=0))
        ann = np.full((len(samples), M, 5), -1.0, dtype=np.float32)         # collater's padding (augmentation.py:78-86)
        for b, s in enumerate(samples):
            a = np.asarray(s['annot'], dtype=np.float32).reshape(-1, 5)
            ann[b, :len(a)] = a
        return ann

    def __call__(self, samples):
        B = len(samples)
        staged = self._stage_batch(samples)
        flips = (self.rng.rand(B) < self.flip_x).astype(np.uint8) if self.flip_x > 0 else None
        ann = self._padded_annots(samples)
        dev = self.device
        src, d_off, d_hw, _ = self._upload(samples, staged)
        d_flip = torch.from_numpy(flips).to(dev, non_blocking=True) if flips is not None else None
        d_ann = torch.from_numpy(ann).to(dev, non_blocking=True)
        m, scale = ops.preprocess_batch(src, d_off, d_hw, self.S, self.dtype, chunk_elems(self.dtype), MEAN, STD, d_flip, d_ann)
        return PackedImages(m), d_ann, scale


# ------------------------------------------------------------------------------------------------ get_augumentation on the device
# Columns of the per-image parameter table (include/effdet_hip.h, EFFDET_AUG_P).
AUG_COLUMNS = ('rrc', 'crop_y', 'crop_x', 'crop_h', 'crop_w', 'flip', 'flip_code', 'transpose', 'color', 'alpha', 'beta', 'gamma',
               'shift', 'r_shift', 'g_shift', 'b_shift', 'hue_shift', 'sat_shift', 'val_shift', 'clahe', 'clip_limit', 'hflip', 'vflip')
AUG = {n: i for i, n in enumerate(AUG_COLUMNS)}
COLOR_BRIGHTNESS_CONTRAST, COLOR_GAMMA, COLOR_NOOP = 1, 2, 3       # 'color' column (0: the OneOf did not fire)
SHIFT_RGB, SHIFT_HSV, SHIFT_NOOP = 1, 2, 3                         # 'shift' column


def _one_of(rng, member_p=(0.5, 0.5, 0.5), p=0.5):
    """albumentations OneOf: fires with probability p, then picks a member by its normalised probability -> 0 or 1 + member."""
    if rng.rand() >= p:
        return 0
    q = np.asarray(member_p, dtype=np.float64)
    return 1 + int(rng.choice(len(q), p=q / q.sum()))


def sample_augment_table(rng, B, S):
    """Draw the 'train' parameters of B images on an S x S canvas from rng (np.random.RandomState) -> [B, len(AUG_COLUMNS)] fp32.

    Order per image: RandomResizedCrop (p 0.3; up to 10 attempts with area scale U(0.08, 1) and log-uniform ratio in (3/4, 4/3),
    then the centre-crop fallback, which on the square canvas is the whole canvas), Flip (p 0.5, code U{-1, 0, 1}), Transpose
    (p 0.5), OneOf[RandomBrightnessContrast(0.5, 0.4), RandomGamma(50, 150), NoOp] (p 0.5, members 1/3 each; alpha = 1 + U(-0.4,
    0.4), beta = U(-0.5, 0.5), gamma = U(50, 150) / 100), OneOf[RGBShift(20, 15, 15), HueSaturationValue(5, 5, 20), NoOp] (same
    rule), CLAHE (p 0.8, clip U(1, 4)), HorizontalFlip (p 0.5), VerticalFlip (p 0.5).  A parameter is drawn only when its
    transform fires.  This is not albumentations' random stream (matching it is a non-goal), only its distributions."""
    t = np.zeros((B, len(AUG_COLUMNS)), dtype=np.float32)
    for b in range(B):
        r = t[b]
        if rng.rand() < 0.3:
            area = float(S * S)
            y = x = 0; h = w = S
            for _ in range(10):
                target = rng.uniform(0.08, 1.0) * area
                ratio = math.exp(rng.uniform(math.log(3 / 4), math.log(4 / 3)))
                cw, ch = int(round(math.sqrt(target * ratio))), int(round(math.sqrt(target / ratio)))
                if 0 < cw <= S and 0 < ch <= S:
                    h, w = ch, cw
                    y, x = rng.randint(0, S - h + 1), rng.randint(0, S - w + 1)
                    break
            r[[AUG['rrc'], AUG['crop_y'], AUG['crop_x'], AUG['crop_h'], AUG['crop_w']]] = (1, y, x, h, w)
        if rng.rand() < 0.5:
            r[AUG['flip']], r[AUG['flip_code']] = 1, rng.randint(-1, 2)
        if rng.rand() < 0.5:
            r[AUG['transpose']] = 1
        c = r[AUG['color']] = _one_of(rng)
        if c == COLOR_BRIGHTNESS_CONTRAST:
            r[AUG['alpha']] = 1.0 + rng.uniform(-0.4, 0.4)
            r[AUG['beta']] = rng.uniform(-0.5, 0.5)
        elif c == COLOR_GAMMA:
            r[AUG['gamma']] = rng.uniform(50, 150) / 100.0
        s = r[AUG['shift']] = _one_of(rng)
        if s == SHIFT_RGB:
            r[AUG['r_shift']], r[AUG['g_shift']], r[AUG['b_shift']] = rng.uniform(-20, 20), rng.uniform(-15, 15), rng.uniform(-15, 15)
        elif s == SHIFT_HSV:
            r[AUG['hue_shift']], r[AUG['sat_shift']], r[AUG['val_shift']] = rng.uniform(-5, 5), rng.uniform(-5, 5), rng.uniform(-20, 20)
        if rng.rand() < 0.8:
            r[AUG['clahe']], r[AUG['clip_limit']] = 1, rng.uniform(1, 4)
        r[AUG['hflip']] = rng.rand() < 0.5
        r[AUG['vflip']] = rng.rand() < 0.5
    return t


def check_augment_table(table, B, S):
    """Refuse a table the chain cannot mean: wrong shape, or a crop that is not an integer box inside the S x S canvas."""
    t = np.asarray(table, dtype=np.float32)
    if t.shape != (B, len(AUG_COLUMNS)):
        raise ValueError('augmentation table must be [%d, %d], got %s' % (B, len(AUG_COLUMNS), t.shape))
    crop = t[t[:, AUG['rrc']] != 0][:, [AUG['crop_y'], AUG['crop_x'], AUG['crop_h'], AUG['crop_w']]]
    if len(crop) and (np.any(crop != np.round(crop)) or np.any(crop[:, 2:] < 1) or np.any(crop[:, :2] < 0)
                      or np.any(crop[:, 0] + crop[:, 2] > S) or np.any(crop[:, 1] + crop[:, 3] > S)):
        raise ValueError('RandomResizedCrop boxes must be integer windows inside the %d x %d canvas' % (S, S))
    codes = t[t[:, AUG['flip']] != 0][:, AUG['flip_code']]
    if np.any(~np.isin(codes, (-1, 0, 1))):
        raise ValueError('Flip codes are -1, 0 or 1')
    return t


# ------------------------------------------------------------------------------------------------ Mosaic / MixUp on the device
# Columns of the per-image mosaic table (include/effdet_mosaic.h, EFFDET_MOSAIC_P), one row per OUTPUT image.
MOSAIC_COLUMNS = ('on', 'cx', 'cy', 'src0', 'src1', 'src2', 'src3', 'side0', 'side1', 'side2', 'side3', 'mix', 'mix_src', 'lam')
MOSAIC = {n: i for i, n in enumerate(MOSAIC_COLUMNS)}


def _lms_dims(h, w, S):
    """LongestMaxSize(S)'s output size of an h x w image (Python's round: half to even, as the kernels' rint)."""
    scale = S / max(h, w)
    return int(round(h * scale)), int(round(w * scale))


class MosaicOptions:
    """Mosaic (four images of the batch around a random centre) and MixUp (a partner image blended in) in front of the 'train' chain
    of DeviceAugmentation; include/effdet_mosaic.h holds the semantics.

    p: probability that an output image is a mosaic (else it is its own source, as without the option).  centre: range of the
    centre, as fractions of the canvas side.  scale: range of each quadrant image's longest side, as fractions of the canvas side.
    fill: the background byte.  mixup_p: probability that a mosaic is blended with a partner; the blend weight is Beta(mixup_alpha,
    mixup_alpha).  Sources come from the batch itself, with replacement."""

    def __init__(self, p=1.0, centre=(0.25, 0.75), scale=(0.5, 1.0), fill=114, mixup_p=0.0, mixup_alpha=8.0):
        self.p, self.mixup_p, self.mixup_alpha = float(p), float(mixup_p), float(mixup_alpha)
        self.centre, self.scale = tuple(float(v) for v in centre), tuple(float(v) for v in scale)
        if not 0.0 <= self.p <= 1.0 or not 0.0 <= self.mixup_p <= 1.0:
            raise ValueError('p and mixup_p are probabilities in [0, 1]')
        if len(self.centre) != 2 or not 0.0 <= self.centre[0] <= self.centre[1] <= 1.0:
            raise ValueError('centre is a range (lo, hi) with 0 <= lo <= hi <= 1')
        if len(self.scale) != 2 or not 0.0 < self.scale[0] <= self.scale[1] <= 1.0:
            raise ValueError('scale is a range (lo, hi) with 0 < lo <= hi <= 1')
        if isinstance(fill, bool) or int(fill) != fill or not 0 <= int(fill) <= 255:
            raise ValueError('fill is a byte, 0 .. 255')
        self.fill = int(fill)
        if not (self.mixup_alpha > 0.0 and math.isfinite(self.mixup_alpha)):
            raise ValueError('mixup_alpha must be positive and finite')

    def key(self):
        return (self.p, self.centre, self.scale, self.fill, self.mixup_p, self.mixup_alpha)

    def __eq__(self, other):
        return isinstance(other, MosaicOptions) and self.key() == other.key()

    def __hash__(self):
        return hash(self.key())

    def __repr__(self):
        return 'MosaicOptions(p=%r, centre=%r, scale=%r, fill=%r, mixup_p=%r, mixup_alpha=%r)' % self.key()


def sample_mosaic_table(rng, B, S, opts):
    """Draw the mosaic parameters of B output images on an S x S canvas from rng (np.random.RandomState) -> [B, len(MOSAIC_COLUMNS)]
    fp32.  Order per image: on (probability p); then, only when on: cx and cy (integers in round(centre * S)), src1..3 (uniform
    over the batch, with replacement; src0 = b), side0..3 (max(1, round(U(scale) * S))), mix (probability mixup_p) and, only when
    mix, mix_src (uniform over the batch) and lam ~ Beta(mixup_alpha, mixup_alpha)."""
    t = np.zeros((B, len(MOSAIC_COLUMNS)), dtype=np.float32)
    c_lo, c_hi = int(round(opts.centre[0] * S)), int(round(opts.centre[1] * S))
    for b in range(B):
        r = t[b]
        r[MOSAIC['src0']] = b
        if rng.rand() >= opts.p:
            continue
        r[MOSAIC['on']] = 1
        r[MOSAIC['cx']], r[MOSAIC['cy']] = rng.randint(c_lo, c_hi + 1), rng.randint(c_lo, c_hi + 1)
        r[MOSAIC['src1']:MOSAIC['src3'] + 1] = rng.randint(0, B, size=3)
        for q in range(4):
            r[MOSAIC['side0'] + q] = min(S, max(1, int(round(rng.uniform(opts.scale[0], opts.scale[1]) * S))))
        if rng.rand() < opts.mixup_p:
            r[MOSAIC['mix']], r[MOSAIC['mix_src']] = 1, rng.randint(0, B)
            r[MOSAIC['lam']] = min(1.0, max(0.0, rng.beta(opts.mixup_alpha, opts.mixup_alpha)))
    return t


def check_mosaic_table(table, B, S, hw):
    """Refuse a table the mosaic stage cannot mean (include/effdet_mosaic.h, Domain): wrong shape, non-integers, sources outside the
    batch, centres or sides outside their ranges, mix without on, lam outside [0, 1], or a resized side that rounds to 0.  hw: the
    sources' (h, w) [B, 2] on the host.  Raises ValueError naming the row -> the table as fp32."""
    t = np.asarray(table, dtype=np.float32)
    if t.shape != (B, len(MOSAIC_COLUMNS)):
        raise ValueError('mosaic table must be [%d, %d], got %s' % (B, len(MOSAIC_COLUMNS), t.shape))
    hw = np.asarray(hw).reshape(-1, 2)
    if hw.shape != (B, 2):
        raise ValueError('mosaic table check needs the %d source sizes [B, 2], got %s' % (B, hw.shape))

    def bad(b, what):
        raise ValueError('mosaic table row %d: %s' % (b, what))
    for b in range(B):
        r = t[b]
        on, mix = r[MOSAIC['on']], r[MOSAIC['mix']]
        if on not in (0.0, 1.0) or mix not in (0.0, 1.0):
            bad(b, 'on and mix are 0 or 1')
        if mix and not on:
            bad(b, 'mix needs on')
        if min(_lms_dims(int(hw[b, 0]), int(hw[b, 1]), S)) < 1:
            bad(b, 'source %d (%d x %d) has a side that resizes to 0 at %d' % (b, hw[b, 0], hw[b, 1], S))
        if not on:
            continue                                               # the rest of a pass-through row is ignored
        ints = r[:MOSAIC['lam']]
        if not np.all(np.isfinite(ints)) or np.any(ints != np.round(ints)):
            bad(b, 'every column but lam is an integer')
        if not (0 <= r[MOSAIC['cx']] <= S and 0 <= r[MOSAIC['cy']] <= S):
            bad(b, 'the centre lies in [0, %d]' % S)
        for q in range(4):
            src, side = r[MOSAIC['src0'] + q], r[MOSAIC['side0'] + q]
            if not 0 <= src < B:
                bad(b, 'src%d = %d is outside the batch of %d' % (q, src, B))
            if not 1 <= side <= S:
                bad(b, 'side%d = %d is outside [1, %d]' % (q, side, S))
            if min(_lms_dims(int(hw[int(src), 0]), int(hw[int(src), 1]), int(side))) < 1:
                bad(b, 'source %d (%d x %d) has a side that resizes to 0 at side%d = %d' % (src, hw[int(src), 0], hw[int(src), 1], q, side))
        if mix:
            src, lam = r[MOSAIC['mix_src']], r[MOSAIC['lam']]
            if not 0 <= src < B:
                bad(b, 'mix_src = %d is outside the batch of %d' % (src, B))
            if not 0.0 <= lam <= 1.0:                              # (refuses NaN too)
                bad(b, 'lam = %r is outside [0, 1]' % float(lam))
            if min(_lms_dims(int(hw[int(src), 0]), int(hw[int(src), 1]), S)) < 1:
                bad(b, 'partner %d (%d x %d) has a side that resizes to 0 at %d' % (src, hw[int(src), 0], hw[int(src), 1], S))
    return t


# ------------------------------------------------------------------------------------------------ affine / perspective warp on the device
# Columns of the per-image warp table (include/effdet_affine.h, EFFDET_AFFINE_P), one row per OUTPUT image: the forward matrix F
# (source pixel -> output pixel, row-major), its inverse G and the isotropic scale in F.  The table is fp64.
AFFINE_COLUMNS = ('on',) + tuple('f%d' % i for i in range(9)) + tuple('g%d' % i for i in range(9)) + ('scale',)
AFFINE = {n: i for i, n in enumerate(AFFINE_COLUMNS)}


class AffineOptions:
    """The random affine / perspective warp (YOLOv5's random_perspective) between the mosaic stage and the 'train' chain of
    DeviceAugmentation; include/effdet_affine.h holds the semantics.

    p: probability that an image is warped (else it goes through LongestMaxSize + pad, as without the option).  degrees: rotation
    range, +-.  translate: range of the centre's offset, +- fractions of the output side.  scale: range (lo, hi) of the scale
    relative to LongestMaxSize's.  shear: range of the two shear angles, +- degrees.  perspective: range of the two perspective
    terms, +-.  fill: the border byte.  wh_thr, ar_thr, area_thr: box_candidates' thresholds (a warped box is kept if both sides
    exceed wh_thr px, its aspect ratio stays below ar_thr and its area exceeds area_thr of the scaled source box's).  canvas: 1, or 2
    with a mosaic in front: the mosaic is then composed on a canvas of twice the output side and the warp brings it down (the
    published recipe)."""

    def __init__(self, p=1.0, degrees=0.0, translate=0.1, scale=(0.5, 1.5), shear=0.0, perspective=0.0, fill=114, wh_thr=2.0,
                 ar_thr=100.0, area_thr=0.1, canvas=1):
        self.p, self.degrees, self.translate = float(p), float(degrees), float(translate)
        self.scale = tuple(float(v) for v in scale)
        self.shear, self.perspective = float(shear), float(perspective)
        self.wh_thr, self.ar_thr, self.area_thr = float(wh_thr), float(ar_thr), float(area_thr)
        if not 0.0 <= self.p <= 1.0:
            raise ValueError('p is a probability in [0, 1]')
        if not 0.0 <= self.degrees <= 180.0:
            raise ValueError('degrees is a range +- in [0, 180]')
        if not 0.0 <= self.translate <= 0.5:
            raise ValueError('translate is a range +- in [0, 0.5] of the output side')
        if len(self.scale) != 2 or not 0.0 < self.scale[0] <= self.scale[1] or not math.isfinite(self.scale[1]):
            raise ValueError('scale is a range (lo, hi) with 0 < lo <= hi, finite')
        if not 0.0 <= self.shear < 90.0:
            raise ValueError('shear is a range +- in [0, 90) degrees')
        if not (0.0 <= self.perspective and math.isfinite(self.perspective)):
            raise ValueError('perspective is a range +-, non-negative and finite')
        if isinstance(fill, bool) or int(fill) != fill or not 0 <= int(fill) <= 255:
            raise ValueError('fill is a byte, 0 .. 255')
        self.fill = int(fill)
        if not (self.wh_thr >= 0.0 and self.area_thr >= 0.0 and self.ar_thr > 0.0) or not all(
                math.isfinite(v) for v in (self.wh_thr, self.ar_thr, self.area_thr)):
            raise ValueError('wh_thr and area_thr are non-negative, ar_thr is positive, all finite')
        if isinstance(canvas, bool) or canvas not in (1, 2):
            raise ValueError('canvas is 1 or 2')
        self.canvas = int(canvas)

    def key(self):
        return (self.p, self.degrees, self.translate, self.scale, self.shear, self.perspective, self.fill, self.wh_thr, self.ar_thr,
                self.area_thr, self.canvas)

    def __eq__(self, other):
        return isinstance(other, AffineOptions) and self.key() == other.key()

    def __hash__(self):
        return hash(self.key())

    def __repr__(self):
        return ('AffineOptions(p=%r, degrees=%r, translate=%r, scale=%r, shear=%r, perspective=%r, fill=%r, wh_thr=%r, ar_thr=%r, '
                'area_thr=%r, canvas=%r)' % self.key())


def sample_affine_table(rng, B, S, hw, opts):
    """Draw the warp parameters of B output images of S x S from rng (np.random.RandomState) -> [B, len(AFFINE_COLUMNS)] fp64.  hw:
    the sources' (h, w) [B, 2].  Order per image: on (probability p); then, only when on: the two perspective terms (uniform in
    +-perspective), the angle (+-degrees), s (uniform in scale), the two shears (+-shear degrees) and the two translations
    (uniform in (0.5 +- translate) * S).  F = T . Sh . R . P . C in fp64: C moves the source centre (w / 2, h / 2) to the origin,
    P holds the perspective terms, R is the rotation with scale s * S / max(h, w) (LongestMaxSize folded in), Sh the shears, T
    moves the origin to the drawn point; G = inv(F), and the scale column is s * S / max(h, w)."""
    hw = np.asarray(hw).reshape(-1, 2)
    if hw.shape != (B, 2):
        raise ValueError('the warp table needs the %d source sizes [B, 2], got %s' % (B, hw.shape))
    t = np.zeros((B, len(AFFINE_COLUMNS)), dtype=np.float64)
    for b in range(B):
        if rng.rand() >= opts.p:
            continue
        h, w = float(hw[b, 0]), float(hw[b, 1])
        C_, P_, R_, Sh, T_ = (np.eye(3) for _ in range(5))
        C_[0, 2], C_[1, 2] = -w / 2, -h / 2
        P_[2, 0], P_[2, 1] = rng.uniform(-opts.perspective, opts.perspective), rng.uniform(-opts.perspective, opts.perspective)
        a = math.radians(rng.uniform(-opts.degrees, opts.degrees))
        k = rng.uniform(opts.scale[0], opts.scale[1]) * S / max(h, w)
        R_[0, 0], R_[0, 1], R_[1, 0], R_[1, 1] = k * math.cos(a), k * math.sin(a), -k * math.sin(a), k * math.cos(a)
        Sh[0, 1] = math.tan(math.radians(rng.uniform(-opts.shear, opts.shear)))
        Sh[1, 0] = math.tan(math.radians(rng.uniform(-opts.shear, opts.shear)))
        T_[0, 2] = rng.uniform(0.5 - opts.translate, 0.5 + opts.translate) * S
        T_[1, 2] = rng.uniform(0.5 - opts.translate, 0.5 + opts.translate) * S
        F = T_ @ Sh @ R_ @ P_ @ C_
        t[b, AFFINE['on']] = 1
        t[b, AFFINE['f0']:AFFINE['f8'] + 1] = F.reshape(-1)
        t[b, AFFINE['g0']:AFFINE['g8'] + 1] = np.linalg.inv(F).reshape(-1)
        t[b, AFFINE['scale']] = k
    return t


def check_affine_table(table, B, S):
    """Refuse a table the warp cannot mean (include/effdet_affine.h): wrong shape, `on` outside {0, 1}, and for a row that is on:
    non-finite entries, scale <= 0, or a G that is not the inverse of F (the largest absolute row sum of F.G - I above 1e-9).  The
    rest of a row that is off is ignored.  Raises ValueError naming the row -> the table as fp64."""
    t = np.asarray(table, dtype=np.float64)
    if t.shape != (B, len(AFFINE_COLUMNS)):
        raise ValueError('warp table must be [%d, %d], got %s' % (B, len(AFFINE_COLUMNS), t.shape))

    def bad(b, what):
        raise ValueError('warp table row %d: %s' % (b, what))
    for b in range(B):
        r = t[b]
        if r[AFFINE['on']] not in (0.0, 1.0):
            bad(b, 'on is 0 or 1')
        if not r[AFFINE['on']]:
            continue
        if not np.all(np.isfinite(r)):
            bad(b, 'every entry is finite')
        if not r[AFFINE['scale']] > 0.0:
            bad(b, 'scale = %r is not positive' % float(r[AFFINE['scale']]))
        F, G = r[AFFINE['f0']:AFFINE['f8'] + 1].reshape(3, 3), r[AFFINE['g0']:AFFINE['g8'] + 1].reshape(3, 3)
        err = float(np.abs(F @ G - np.eye(3)).sum(1).max())
        if not err <= 1e-9:
            bad(b, 'G is not the inverse of F (|F.G - I| = %.3g > 1e-9)' % err)
    return t


class DeviceAugmentation(DeviceCollater):
    """get_augumentation(phase, width, height, min_area, min_visibility) + detection_collate (datasets/augmentation.py:8-67) on the
    device: ``images, annotations, params = aug(samples)``.

    samples: as for DeviceCollater ({'img': uint8 [H,W,3] RGB or 'jpeg': bytes, 'annot': [n,5] pascal_voc boxes + label}).  Returns
    PackedImages (NHWC, `dtype`, the stem conv's layout), annotations [B,M,5] fp32 with each image's kept boxes first in their
    input order and -1 rows after (None for 'test'), and params: for 'train' the device table [B, len(AUG_COLUMNS)] that drove
    the chain, for 'valid' / 'test' the per-axis scales [B,2] = (width / w, height / h) (boxes / scale map back to the image).
    M = max(1, most boxes kept by one image); trim=False keeps M = max(1, longest input list) instead, which spares the
    device-to-host read of the kept counts.  The reference's detection_collate can return M = 0; this never does.
    ``aug(samples, table=...)`` runs 'train' with an explicit table (numpy or tensor, columns AUG_COLUMNS).

    The host draws the table (sample_augment_table) and copies the uint8 bytes; every pixel and box operation runs in
    csrc/augment.hip.  'train' needs width == height (the reference's transpose and crop assume a square output).

    mosaic: a MosaicOptions puts Mosaic / MixUp (csrc/mosaic.hip) in front of the 'train' chain: the batch's images are composed
    into B canvases of width x width, and the chain runs on those as if they were the dataset's images.  Annotations then have up to
    5 x the longest input list of rows before trimming.  It is a plain attribute: ``aug.mosaic = None`` switches the stage off (the
    last epochs of a schedule), and nothing of it runs then.  ``aug(samples, mosaic_table=...)`` takes an explicit table (host
    memory: numpy or CPU tensor, columns MOSAIC_COLUMNS); it always passes check_mosaic_table.

    affine: an AffineOptions puts the random affine / perspective warp (csrc/affine.hip) between the mosaic stage and the chain: each
    source (a dataset image, or a mosaic canvas) becomes one width x width image through a homography, its boxes go along and are
    filtered by box_candidates' rule, and the chain runs on the result.  With ``canvas=2`` (which needs `mosaic`) the mosaic is
    composed at twice the width, its table sampled and checked at that side, and the warp brings it down.  Like `mosaic` it is a
    plain attribute, ``aug.affine = None`` switches it off and nothing of it runs then, not even a random draw; its table is drawn
    after the mosaic's.  ``aug(samples, affine_table=...)`` takes an explicit host table (fp64, columns AFFINE_COLUMNS); it always
    passes check_affine_table."""

    PHASES = ('train', 'valid', 'test')

    def __init__(self, phase='train', width=512, height=512, min_area=0., min_visibility=0., dtype=torch.bfloat16, device='cuda',
                 seed=0, trim=True, decode_threads=8, decode_fallback=None, mosaic=None, affine=None):
        if phase not in self.PHASES:
            raise ValueError('phase must be one of %s' % (self.PHASES,))
        if phase == 'train' and (width != height or width < 8):
            raise ValueError("the 'train' chain needs width == height >= 8 (got %d x %d)" % (width, height))
        super().__init__(common_size=width, dtype=dtype, device=device, seed=seed, decode_threads=decode_threads,
                         decode_fallback=decode_fallback)
        self.phase, self.W, self.H = phase, int(width), int(height)
        self.min_area, self.min_visibility, self.trim = float(min_area), float(min_visibility), bool(trim)
        if mosaic is not None and not isinstance(mosaic, MosaicOptions):
            raise TypeError('mosaic is a MosaicOptions or None')
        if mosaic is not None and phase != 'train':
            raise ValueError("mosaic only applies to the 'train' phase")
        self.mosaic = mosaic
        if affine is not None and not isinstance(affine, AffineOptions):
            raise TypeError('affine is an AffineOptions or None')
        self._check_affine(affine, mosaic)
        self.affine = affine

    def _check_affine(self, affine, mosaic):
        if affine is not None and self.phase != 'train':
            raise ValueError("affine only applies to the 'train' phase")
        if affine is not None and affine.canvas == 2 and mosaic is None:
            raise ValueError('affine canvas=2 warps a mosaic canvas of twice the side down: it needs mosaic options')

    def __call__(self, samples, table=None, stages=None, mosaic_table=None, affine_table=None):
        """stages: optional dict that receives the uint8 intermediates of ops.augment_train / ops.augment_resize (tests), with mosaic
        'mosaic' (uint8 [B,side,side,3], side = canvas * S) and 'mosaic_table' (the device table), and with affine 'affine' (uint8
        [B,S,S,3]) and 'affine_table' (the device table, fp64)."""
        B = len(samples)
        mosaic = getattr(self, 'mosaic', None)
        affine = getattr(self, 'affine', None)
        if mosaic is not None and self.phase != 'train':
            raise ValueError("mosaic only applies to the 'train' phase")
        if mosaic_table is not None and mosaic is None:
            raise ValueError('mosaic_table was given, but this augmentation has no mosaic options')
        if mosaic_table is not None and torch.is_tensor(mosaic_table) and mosaic_table.device.type != 'cpu':
            raise ValueError('a mosaic table comes from the host (numpy or CPU tensor): it is checked before anything is launched')
        self._check_affine(affine, mosaic)
        if affine_table is not None and affine is None:
            raise ValueError('affine_table was given, but this augmentation has no affine options')
        if affine_table is not None and torch.is_tensor(affine_table) and affine_table.device.type != 'cpu':
            raise ValueError('an affine table comes from the host (numpy or CPU tensor): it is checked before anything is launched')
        if affine_table is not None:
            affine_table = check_affine_table(affine_table.numpy() if torch.is_tensor(affine_table) else affine_table, B, self.S)
        staged = self._stage_batch(samples)
        if self.phase == 'train':
            if table is None:
                table = sample_augment_table(self.rng, B, self.S)
            elif not torch.is_tensor(table) or table.device.type == 'cpu':
                table = check_augment_table(table.numpy() if torch.is_tensor(table) else table, B, self.S)
        elif table is not None:
            raise ValueError("an explicit table only applies to the 'train' phase")
        ann = self._padded_annots(samples) if self.phase != 'test' else None
        dev = self.device
        src, d_off, d_hw, hw = self._upload(samples, staged)
        d_ann = None
        if mosaic is not None:
            side = self.S * (affine.canvas if affine is not None else 1)   # canvas=2: composed at 2S, the warp brings it down to S
            if mosaic_table is None:
                mosaic_table = sample_mosaic_table(self.rng, B, side, mosaic)
            mt = check_mosaic_table(mosaic_table.numpy() if torch.is_tensor(mosaic_table) else mosaic_table, B, side, hw)
            d_mt = torch.from_numpy(np.ascontiguousarray(mt)).to(dev, non_blocking=True)
            canvas = ops.mosaic_compose(src, d_off, d_hw, d_mt, side, mosaic.fill)
            d_ann, _ = ops.mosaic_boxes(d_hw, d_mt, side, torch.from_numpy(ann).to(dev, non_blocking=True), self.min_area,
                                        self.min_visibility)
            if stages is not None:
                stages.update(mosaic=canvas, mosaic_table=d_mt)
            # the next stage takes the canvases as a batch of side x side dataset images
            src = canvas.view(-1)
            d_off = torch.arange(B, dtype=torch.int64, device=dev) * (side * side * 3)
            d_hw = torch.full((B, 2), side, dtype=torch.int32, device=dev)
            hw = np.full((B, 2), side, dtype=np.int32)
        if affine is not None:
            wt = affine_table if affine_table is not None else check_affine_table(sample_affine_table(self.rng, B, self.S, hw, affine), B, self.S)
            d_wt = torch.from_numpy(np.ascontiguousarray(wt)).to(dev, non_blocking=True)
            warped = ops.affine_warp(src, d_off, d_hw, d_wt, self.S, affine.fill)
            if d_ann is None:
                d_ann = torch.from_numpy(ann).to(dev, non_blocking=True)
            d_ann, _ = ops.affine_boxes(d_hw, d_wt, self.S, d_ann, affine.wh_thr, affine.ar_thr, affine.area_thr)
            if stages is not None:
                stages.update(affine=warped, affine_table=d_wt)
            # the chain takes the warped images as a batch of S x S dataset images
            src = warped.view(-1)
            d_off = torch.arange(B, dtype=torch.int64, device=dev) * (self.S * self.S * 3)
            d_hw = torch.full((B, 2), self.S, dtype=torch.int32, device=dev)
        if self.phase == 'train':
            params = (table if torch.is_tensor(table) else torch.from_numpy(table)).to(dev, torch.float32, non_blocking=True).contiguous()
            m = ops.augment_train(src, d_off, d_hw, params, self.S, self.dtype, chunk_elems(self.dtype), MEAN, STD, stages)
        else:
            scale = np.stack([self.W / hw[:, 1].astype(np.float64), self.H / hw[:, 0].astype(np.float64)], 1).astype(np.float32)
            params = torch.from_numpy(scale).to(dev, non_blocking=True)
            m = ops.augment_resize(src, d_off, d_hw, self.H, self.W, self.dtype, chunk_elems(self.dtype), MEAN, STD, stages)
        if ann is None:
            return PackedImages(m), None, params
        if d_ann is None:
            d_ann = torch.from_numpy(ann).to(dev, non_blocking=True)
        out, counts = ops.augment_boxes(d_hw, params if self.phase == 'train' else None, self.H, self.W, d_ann, self.min_area,
                                        self.min_visibility)
        if self.trim:
            out = out[:, :max(1, int(counts.max()))].contiguous()
        return PackedImages(m), out, params
