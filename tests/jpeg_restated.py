"""NumPy restatement of a baseline JPEG decoder: the specification csrc/jpeg.hip is tested against.  TEST INFRASTRUCTURE ONLY,
written for clarity, not speed (one Python step per Huffman symbol).

Written from ITU-T T.81 (markers, Huffman coding, zig-zag order) and the documented arithmetic of the IJG decoder family that
cv2.imread and Pillow share:
* the "slow integer" inverse DCT: 13-bit constants, columns first with 2 extra bits kept, then rows, each pass rounded once;
* "fancy" chroma upsampling: the triangle filter (3/4 near + 1/4 far) with rounding terms 1, 2 (one axis) or 8, 7 (two axes)
  alternating over the output columns, edges replicated from the last real sample of the downsampled plane; a plane of one or
  two samples across is replicated instead;
* YCbCr -> RGB through 16-bit fixed-point tables.
tools/make_jpeg_golden.py asserts decode() == Pillow (libjpeg-turbo) for every case before it writes the goldens.

Layout of coefficients(): one int16 array, component-major, [component][block_row][block_col][64] with each block in natural
(row-major, de-zigzagged) order and the block grid rounded up to whole MCUs -- the layout of effdet_jpeg_entropy_batch."""
import numpy as np

GREY, S444, S422, S420 = 0, 1, 2, 3                     # sampling classes (EFFDET_JPEG_* in include/effdet_hip.h)

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63])                 # ZIGZAG[k] = natural index of the k-th coefficient of the stream


class Unsupported(ValueError):
    pass


class Header:
    """The markers up to the scan."""

    def __init__(self, data):
        if data[:2] != b'\xff\xd8':
            raise ValueError('not a JPEG')
        self.qt, self.huff, self.restart = {}, {}, 0
        self.comps = None
        p = 2
        while True:
            if p + 4 > len(data) or data[p] != 0xFF:
                raise ValueError('header cut short')
            m = data[p + 1]
            if m == 0xFF:                               # fill byte
                p += 1
                continue
            n = (data[p + 2] << 8) | data[p + 3]
            seg = data[p + 4:p + 2 + n]
            if n < 2 or p + 2 + n > len(data):
                raise ValueError('header cut short')
            p += 2 + n
            if m == 0xC0:
                if seg[0] != 8:
                    raise Unsupported('precision')
                self.height, self.width = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4]
                self.comps = [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(seg[5])]
            elif 0xC1 <= m <= 0xCF and m not in (0xC4, 0xC8):
                raise Unsupported('SOF%d' % (m - 0xC0))
            elif m == 0xC4:
                while len(seg):
                    counts = list(seg[1:17])
                    total = sum(counts)
                    self.huff[seg[0]] = (counts, list(seg[17:17 + total]))       # key: class << 4 | id
                    seg = seg[17 + total:]
            elif m == 0xDB:
                while len(seg):
                    if seg[0] >> 4:
                        raise Unsupported('16-bit quantisation table')
                    t = np.zeros(64, dtype=np.uint16)
                    t[ZIGZAG] = np.frombuffer(seg[1:65], dtype=np.uint8)
                    self.qt[seg[0] & 15] = t
                    seg = seg[65:]
            elif m == 0xDD:
                self.restart = (seg[0] << 8) | seg[1]
            elif m == 0xDA:
                if seg[0] != len(self.comps):
                    raise Unsupported('more than one scan')
                self.tables = [(seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15) for i in range(seg[0])]
                self.scan = p
                break
        hv = [(h, v) for _, h, v, _ in self.comps]
        if len(hv) == 1:
            self.sampling, hv = GREY, [(1, 1)]
        elif len(hv) == 3 and hv[1:] == [(1, 1), (1, 1)] and hv[0] in ((1, 1), (2, 1), (2, 2)):
            self.sampling = {(1, 1): S444, (2, 1): S422, (2, 2): S420}[hv[0]]
        else:
            raise Unsupported('sampling')
        self.hv = hv
        self.mcus_x = -(-self.width // (8 * hv[0][0]))
        self.mcus_y = -(-self.height // (8 * hv[0][1]))
        self.blocks = [(self.mcus_y * v, self.mcus_x * h) for h, v in hv]       # (rows, cols) of 8x8 blocks per component


class _Bits:
    """The entropy-coded segment as a bit stream: FF 00 is a data byte FF, FF FF.. are fill bytes, any other FF xx ends it."""

    def __init__(self, data, p):
        self.d, self.p, self.acc, self.n = data, p, 0, 0

    def _byte(self):
        d = self.d
        if self.p >= len(d):
            raise ValueError('scan cut short')
        b = d[self.p]
        if b == 0xFF:
            q = self.p + 1
            while q < len(d) and d[q] == 0xFF:
                q += 1
            if q >= len(d) or d[q] != 0:
                raise ValueError('scan cut short')      # a marker where data was expected
            self.p = q
        self.p += 1
        return b

    def bit(self):
        if self.n == 0:
            self.acc, self.n = self._byte(), 8
        self.n -= 1
        return (self.acc >> self.n) & 1

    def bits(self, s):
        v = 0
        for _ in range(s):
            v = (v << 1) | self.bit()
        return v

    def restart_marker(self, k):
        self.n = 0                                      # drop the bits left in the current byte
        d = self.d
        while self.p + 1 < len(d) and d[self.p] == 0xFF and d[self.p + 1] == 0xFF:
            self.p += 1
        if self.p + 1 >= len(d) or d[self.p] != 0xFF or d[self.p + 1] != 0xD0 + (k & 7):
            raise ValueError('restart marker missing')
        self.p += 2


def _codebook(counts, symbols):
    """T.81 annex C: canonical codes in order of length -> {(length, code): symbol}."""
    book, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            book[(length, code)] = symbols[k]
            code += 1; k += 1
        code <<= 1
    return book


def _symbol(bits, book):
    code = 0
    for length in range(1, 17):
        code = (code << 1) | bits.bit()
        if (length, code) in book:
            return book[(length, code)]
    raise ValueError('bad Huffman code')


def _extend(v, s):
    return v if s == 0 or v >= (1 << (s - 1)) else v - (1 << s) + 1


def parse(data):
    return Header(bytes(data))


def coefficients(data, header=None):
    """-> int16 [total blocks * 64] in the library's layout (see the module docstring)."""
    data = bytes(data)
    hd = header or Header(data)
    planes = [np.zeros((r, c, 64), dtype=np.int16) for r, c in hd.blocks]
    dc = [_codebook(*hd.huff[t[0]]) for t in hd.tables]
    ac = [_codebook(*hd.huff[16 | t[1]]) for t in hd.tables]
    bits = _Bits(data, hd.scan)
    pred = [0] * len(planes)
    n_mcu, rst = 0, 0
    for my in range(hd.mcus_y):
        for mx in range(hd.mcus_x):
            if hd.restart and n_mcu and n_mcu % hd.restart == 0:
                bits.restart_marker(rst)
                rst += 1
                pred = [0] * len(planes)
            n_mcu += 1
            for c, (h, v) in enumerate(hd.hv):
                for by in range(v):
                    for bx in range(h):
                        blk = planes[c][my * v + by, mx * h + bx]
                        s = _symbol(bits, dc[c])
                        pred[c] += _extend(bits.bits(s), s)
                        blk[0] = pred[c]
                        k = 1
                        while k < 64:
                            rs = _symbol(bits, ac[c])
                            r, s = rs >> 4, rs & 15
                            if s == 0:
                                if r != 15:
                                    break               # end of block
                                k += 16
                                continue
                            k += r
                            if k > 63:
                                raise ValueError('coefficient index past 63')
                            blk[ZIGZAG[k]] = _extend(bits.bits(s), s)
                            k += 1
    return np.concatenate([p.reshape(-1) for p in planes])


def quant_tables(data, header=None):
    """-> uint16 [3, 64] natural order; rows past the component count are zero."""
    hd = header or Header(bytes(data))
    out = np.zeros((3, 64), dtype=np.uint16)
    for c, comp in enumerate(hd.comps):
        out[c] = hd.qt[comp[3]]
    return out


# ------------------------------------------------------------------------------------------------ inverse DCT
def _idct_1d(x, shift_in, descale):
    """One pass of the slow-integer IDCT over the first axis of x (int64 [8, ...]); even part scaled by 2^13."""
    z2, z3 = x[2], x[6]
    z1 = (z2 + z3) * 4433
    t2 = z1 - z3 * 15137
    t3 = z1 + z2 * 6270
    t0 = (x[0] + x[4]) << 13
    t1 = (x[0] - x[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = x[7], x[5], x[3], x[1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    out = np.stack([t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3])
    return (out + (1 << (descale - 1))) >> descale


def idct_blocks(coef, qt):
    """coef int16 [..., 64], qt [64] -> uint8 [..., 8, 8]."""
    x = (coef.astype(np.int64) * qt.astype(np.int64)).reshape(coef.shape[:-1] + (8, 8))
    x = np.moveaxis(x, -2, 0)                           # pass 1 down the columns: axis 0 = row index
    w = _idct_1d(x, 0, 11)
    w = np.moveaxis(w, 0, -2)
    y = _idct_1d(np.moveaxis(w, -1, 0), 0, 18)          # pass 2 along the rows
    y = np.moveaxis(y, 0, -1)
    y = y & 1023                                        # the decoder's range-limit table is indexed modulo 1024 ...
    y = np.where(y >= 512, y - 1024, y)                 # ... around the level shift of 128
    return np.clip(y + 128, 0, 255).astype(np.uint8)


def component_planes(data, header=None):
    data = bytes(data)
    hd = header or Header(data)
    coef, qt = coefficients(data, hd), quant_tables(data, hd)
    planes, o = [], 0
    for c, (r, cc) in enumerate(hd.blocks):
        px = idct_blocks(coef[o:o + r * cc * 64].reshape(r, cc, 64), qt[c])
        planes.append(px.transpose(0, 2, 1, 3).reshape(r * 8, cc * 8))
        o += r * cc * 64
    return planes


# ------------------------------------------------------------------------------------------------ upsampling and colour
def _up_h(p):
    """h2v1 triangle filter over the columns of p (int [rows, w]) -> [rows, 2w]."""
    left = np.concatenate([p[:, :1], p[:, :-1]], 1)
    right = np.concatenate([p[:, 1:], p[:, -1:]], 1)
    out = np.empty((p.shape[0], 2 * p.shape[1]), dtype=np.int64)
    out[:, 0::2] = (3 * p + left + 1) >> 2
    out[:, 1::2] = (3 * p + right + 2) >> 2
    return out


def _up_hv(p):
    """h2v2 triangle filter -> [2 rows, 2 w]: vertical sums 3 near + far first, then the horizontal step on the sums."""
    up = np.concatenate([p[:1], p[:-1]], 0)
    down = np.concatenate([p[1:], p[-1:]], 0)
    out = np.empty((2 * p.shape[0], 2 * p.shape[1]), dtype=np.int64)
    for parity, other in ((0, up), (1, down)):
        s = 3 * p + other
        left = np.concatenate([s[:, :1], s[:, :-1]], 1)
        right = np.concatenate([s[:, 1:], s[:, -1:]], 1)
        out[parity::2, 0::2] = (3 * s + left + 8) >> 4
        out[parity::2, 1::2] = (3 * s + right + 7) >> 4
    return out


def upsample(plane, sampling, height, width):
    """A chroma plane (MCU-padded) -> int [height, width]."""
    if sampling in (GREY, S444):
        return plane[:height, :width].astype(np.int64)
    dw = -(-width // 2)
    dh = -(-height // 2) if sampling == S420 else height
    p = plane[:dh, :dw].astype(np.int64)                # the real samples: the edges replicate these, not the MCU padding
    if dw <= 2:                                         # too narrow for the filter: plain replication
        p = np.repeat(p, 2, axis=1)
        if sampling == S420:
            p = np.repeat(p, 2, axis=0)
    else:
        p = _up_hv(p) if sampling == S420 else _up_h(p)
    return p[:height, :width]


def ycc_to_rgb(y, cb, cr):
    cb, cr = cb - 128, cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def decode(data):
    """-> uint8 [H, W, 3] RGB."""
    data = bytes(data)
    hd = Header(data)
    planes = component_planes(data, hd)
    H, W = hd.height, hd.width
    y = planes[0][:H, :W].astype(np.int64)
    if hd.sampling == GREY:
        return np.repeat(y[:, :, None], 3, axis=2).astype(np.uint8)
    return ycc_to_rgb(y, upsample(planes[1], hd.sampling, H, W), upsample(planes[2], hd.sampling, H, W))
