// Baseline JPEG decode in front of the input pipeline (the cv2.imread of datasets/voc0712.py / datasets/coco.py), cut at the
// coefficient buffer:
//   HOST    effdet_jpeg_probe          markers up to the scan (T.81 annex B)
//           effdet_jpeg_entropy_batch  Huffman decode of a batch on std::thread workers -> int16 coefficients + descriptors
//   DEVICE  effdet_jpeg_reconstruct    two launches for the whole minibatch:
//     1. jpeg_idct_kernel  dequantise + the 13-bit "slow integer" 8x8 inverse DCT + level shift + clamp -> uint8 component planes.
//                          8 lanes per block, 32 blocks per workgroup: lane r loads row r of the block (16 B), the two passes
//                          exchange through an LDS tile with a 9-word row pitch (conflict-free both ways), lane r stores row r
//                          of the samples (8 B; horizontally adjacent blocks of a wave complete the 64 B line).
//     2. jpeg_rgb_kernel   triangle-filter chroma upsampling + YCbCr -> RGB -> uint8 RGB HWC.  One lane per 16 output BYTES of
//                          the image's flat [H][W][3] array (5 1/3 pixels: it computes the 6 pixels it touches), one 16 B store;
//                          each chroma sample's neighbours are read from the planes, so workgroups exchange nothing.
// Both launches walk the mixed-size batch through the workgroup prefix the host stage wrote into the descriptors.  The integer
// arithmetic is the IJG decoder family's, restated in tests/jpeg_restated.py and pinned there on libjpeg-turbo bit for bit.
// Everything is int32: no floating point, so the file needs no -ffp-contract entry.
#include "common.h"

#include <atomic>
#include <cstring>
#include <thread>
#include <vector>

namespace {

const int IDCT_BLOCKS_PER_WG = 32;                 // 256 lanes / 8 lanes per block
const int RGB_BYTES_PER_WG = 256 * 16;

// ================================================================================================ host: markers
const unsigned char ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                  41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                  30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
const int LOOK = 9;                                // Huffman codes up to 9 bits resolve in one table read

struct HuffTab {
  bool defined;
  unsigned char look_len[1 << LOOK], look_sym[1 << LOOK];
  int mincode[17], maxcode[17], valptr[17];        // per code length 1..16 (maxcode -1: no code of that length)
  unsigned char vals[256];
};

struct Header {
  int width, height, ncomp, sampling, restart, mcus_x, mcus_y, reason;
  int hs[3], vs[3], bw[3], bh[3], tq[3], td[3], ta[3], id[3];
  bool have_sof, qt_defined[4];
  int adobe_transform;                             // -1: no Adobe marker
  unsigned short qt[4][64];                        // natural order
  HuffTab dc[4], ac[4];
  long long scan;                                  // first byte of the entropy-coded segment
};

// T.81 annex C: canonical codes in order of length
bool build_huff(HuffTab& t, const unsigned char counts[16], const unsigned char* symbols, int total) {
  std::memset(t.look_len, 0, sizeof t.look_len);
  std::memcpy(t.vals, symbols, (size_t)total);
  int code = 0, k = 0;
  for (int len = 1; len <= 16; ++len) {
    const int n = counts[len - 1];
    if (code + n > (1 << len)) return false;       // more codes than the length can hold
    t.mincode[len] = code; t.valptr[len] = k; t.maxcode[len] = n ? code + n - 1 : -1;
    if (len <= LOOK)
      for (int i = 0; i < n; ++i)
        for (int f = 0; f < (1 << (LOOK - len)); ++f) {
          const int at = ((code + i) << (LOOK - len)) | f;
          t.look_len[at] = (unsigned char)len; t.look_sym[at] = symbols[k + i];
        }
    code = (code + n) << 1; k += n;
  }
  t.defined = true;
  return true;
}

inline int rd16(const unsigned char* p) { return (p[0] << 8) | p[1]; }

// -> EFFDET_OK / EFFDET_EUNSUPPORTED (h.reason set) / EFFDET_EINVAL.  Every read is checked against n.
int parse_header(const unsigned char* d, long long n, Header& h) {
  h.have_sof = false; h.restart = 0; h.reason = EFFDET_JPEG_OK; h.adobe_transform = -1;
  for (int i = 0; i < 4; ++i) { h.qt_defined[i] = false; h.dc[i].defined = false; h.ac[i].defined = false; }
  if (!d || n < 4 || d[0] != 0xFF || d[1] != 0xD8) return EFFDET_EINVAL;
  long long p = 2;
  for (;;) {
    if (p + 2 > n || d[p] != 0xFF) return EFFDET_EINVAL;
    const int m = d[p + 1];
    if (m == 0xFF) { ++p; continue; }                                      // fill byte
    if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) { p += 2; continue; }       // stand-alone markers
    if (m == 0xD8 || m == 0xD9 || m == 0x00) return EFFDET_EINVAL;         // SOI again, EOI before a scan, FF 00 outside a scan
    if (p + 4 > n) return EFFDET_EINVAL;
    const int len = rd16(d + p + 2);
    if (len < 2 || p + 2 + len > n) return EFFDET_EINVAL;
    const unsigned char* s = d + p + 4;
    const int sl = len - 2;
    p += 2 + len;
    if (m >= 0xC0 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {   // SOFn
      if (sl < 6) return EFFDET_EINVAL;
      if (m != 0xC0) { h.reason = m == 0xC2 ? EFFDET_JPEG_PROGRESSIVE : (s[0] != 8 && m == 0xC1 ? EFFDET_JPEG_PRECISION : EFFDET_JPEG_FRAME_TYPE); return EFFDET_EUNSUPPORTED; }
      if (h.have_sof) return EFFDET_EINVAL;
      if (s[0] != 8) { h.reason = EFFDET_JPEG_PRECISION; return EFFDET_EUNSUPPORTED; }
      h.height = rd16(s + 1); h.width = rd16(s + 3); h.ncomp = s[5];
      if (h.width < 1 || h.height < 1) return EFFDET_EINVAL;               // a height of 0 defers to a DNL marker: not baseline practice
      if (h.ncomp != 1 && h.ncomp != 3) { h.reason = EFFDET_JPEG_COMPONENTS; return EFFDET_EUNSUPPORTED; }
      if (sl < 6 + 3 * h.ncomp) return EFFDET_EINVAL;
      for (int c = 0; c < h.ncomp; ++c) {
        h.id[c] = s[6 + 3 * c]; h.hs[c] = s[7 + 3 * c] >> 4; h.vs[c] = s[7 + 3 * c] & 15; h.tq[c] = s[8 + 3 * c];
        if (h.hs[c] < 1 || h.hs[c] > 4 || h.vs[c] < 1 || h.vs[c] > 4 || h.tq[c] > 3) return EFFDET_EINVAL;
      }
      h.have_sof = true;
    } else if (m == 0xCC) {                                                // DAC: arithmetic conditioning
      h.reason = EFFDET_JPEG_FRAME_TYPE; return EFFDET_EUNSUPPORTED;
    } else if (m == 0xC4) {                                                // DHT
      int o = 0;
      while (o < sl) {
        if (o + 17 > sl) return EFFDET_EINVAL;
        const int tc = s[o] >> 4, th = s[o] & 15;
        int total = 0;
        for (int i = 0; i < 16; ++i) total += s[o + 1 + i];
        if (tc > 1 || th > 3 || total > 256 || o + 17 + total > sl) return EFFDET_EINVAL;
        if (!build_huff(tc ? h.ac[th] : h.dc[th], s + o + 1, s + o + 17, total)) return EFFDET_EINVAL;
        o += 17 + total;
      }
    } else if (m == 0xDB) {                                                // DQT
      int o = 0;
      while (o < sl) {
        const int pq = s[o] >> 4, tq = s[o] & 15;
        if (pq > 1 || tq > 3) return EFFDET_EINVAL;
        if (pq == 1) { h.reason = EFFDET_JPEG_QUANT16; return EFFDET_EUNSUPPORTED; }
        if (o + 65 > sl) return EFFDET_EINVAL;
        for (int k = 0; k < 64; ++k) h.qt[tq][ZIGZAG[k]] = s[o + 1 + k];
        h.qt_defined[tq] = true;
        o += 65;
      }
    } else if (m == 0xDD) {                                                // DRI
      if (sl < 2) return EFFDET_EINVAL;
      h.restart = rd16(s);
    } else if (m == 0xEE) {                                                // APP14: "Adobe" + version, flags0, flags1, transform
      if (sl >= 12 && std::memcmp(s, "Adobe", 5) == 0) h.adobe_transform = s[11];
    } else if (m == 0xDA) {                                                // SOS
      if (!h.have_sof || sl < 1) return EFFDET_EINVAL;
      const int ns = s[0];
      if (ns < 1 || ns > 4 || sl < 4 + 2 * ns) return EFFDET_EINVAL;
      if (ns != h.ncomp) { h.reason = EFFDET_JPEG_MULTISCAN; return EFFDET_EUNSUPPORTED; }
      for (int c = 0; c < ns; ++c) {
        if (s[1 + 2 * c] != h.id[c]) return EFFDET_EINVAL;
        h.td[c] = s[2 + 2 * c] >> 4; h.ta[c] = s[2 + 2 * c] & 15;
        if (h.td[c] > 3 || h.ta[c] > 3 || !h.dc[h.td[c]].defined || !h.ac[h.ta[c]].defined || !h.qt_defined[h.tq[c]]) return EFFDET_EINVAL;
      }
      if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) return EFFDET_EINVAL;   // Ss, Se, Ah / Al of a sequential scan
      h.scan = p;
      break;
    }                                                                      // APPn, COM and anything else: skipped
  }
  if (h.ncomp == 1) {
    h.sampling = EFFDET_JPEG_GREY; h.hs[0] = h.vs[0] = 1;                  // a single component is never interleaved
  } else {
    if (h.adobe_transform == 0 || (h.id[0] == 'R' && h.id[1] == 'G' && h.id[2] == 'B')) { h.reason = EFFDET_JPEG_COLORSPACE; return EFFDET_EUNSUPPORTED; }
    const bool chroma11 = h.hs[1] == 1 && h.vs[1] == 1 && h.hs[2] == 1 && h.vs[2] == 1;
    if (chroma11 && h.hs[0] == 1 && h.vs[0] == 1) h.sampling = EFFDET_JPEG_444;
    else if (chroma11 && h.hs[0] == 2 && h.vs[0] == 1) h.sampling = EFFDET_JPEG_422;
    else if (chroma11 && h.hs[0] == 2 && h.vs[0] == 2) h.sampling = EFFDET_JPEG_420;
    else { h.reason = EFFDET_JPEG_SAMPLING; return EFFDET_EUNSUPPORTED; }
  }
  h.mcus_x = (h.width + 8 * h.hs[0] - 1) / (8 * h.hs[0]);
  h.mcus_y = (h.height + 8 * h.vs[0] - 1) / (8 * h.vs[0]);
  for (int c = 0; c < 3; ++c) {
    h.bw[c] = c < h.ncomp ? h.mcus_x * h.hs[c] : 0;
    h.bh[c] = c < h.ncomp ? h.mcus_y * h.vs[c] : 0;
  }
  return EFFDET_OK;
}

inline long long total_blocks(const Header& h) {
  long long t = 0;
  for (int c = 0; c < h.ncomp; ++c) t += (long long)h.bw[c] * h.bh[c];
  return t;
}

// ================================================================================================ host: entropy decode
// The entropy-coded segment as a bit stream.  FF 00 is a data byte FF, FF FF.. are fill bytes, any other FF xx (or the end of
// the stream) ends the data: from there the reader supplies zero bits and counts them, and ok() turns false as soon as one
// of them has been consumed.  p never passes end.
struct Bits {
  const unsigned char* p; const unsigned char* end;
  unsigned long long acc; int n, fake; bool stop;
  Bits(const unsigned char* b, const unsigned char* e) : p(b), end(e), acc(0), n(0), fake(0), stop(false) {}
  inline void fill() {
    while (n <= 56) {
      unsigned b = 0;
      if (!stop) {
        if (p >= end) stop = true;
        else {
          b = *p++;
          if (b == 0xFF) {
            while (p < end && *p == 0xFF) ++p;
            if (p < end && *p == 0) ++p;
            else { --p; stop = true; }             // p: the FF in front of the marker code (or the last byte)
          }
        }
      }
      if (stop) { b = 0; fake += 8; }
      acc = (acc << 8) | b; n += 8;
    }
  }
  inline unsigned peek(int k) const { return (unsigned)(acc >> (n - k)) & ((1u << k) - 1u); }
  inline void skip(int k) { n -= k; }
  inline bool ok() const { return n >= fake; }
  // byte-align at the end of a restart interval and step over RSTk; fewer than 8 real bits may be left
  bool restart(int k) {
    fill();
    if (!stop || n - fake >= 8) return false;
    if (end - p < 2 || p[0] != 0xFF || p[1] != 0xD0 + (k & 7)) return false;
    p += 2; acc = 0; n = 0; fake = 0; stop = false;
    return true;
  }
};

inline int huff_symbol(Bits& br, const HuffTab& t) {       // the caller has filled the reader (>= 57 bits)
  const unsigned look = br.peek(LOOK);
  const int l = t.look_len[look];
  if (l) { br.skip(l); return t.look_sym[look]; }
  for (int len = LOOK + 1; len <= 16; ++len) {
    const int code = (int)br.peek(len);
    if (code <= t.maxcode[len]) { br.skip(len); return t.vals[t.valptr[len] + code - t.mincode[len]]; }
  }
  return -1;
}

inline int receive_extend(Bits& br, int s) {               // T.81 F.2.2.1: s magnitude bits -> signed value
  const int v = (int)br.peek(s);
  br.skip(s);
  return v >= (1 << (s - 1)) ? v : v - (1 << s) + 1;
}

// One image.  out: the image's own range of `elems` int16 (already zero).  -> false: the scan is truncated or corrupt.
bool decode_scan(const unsigned char* d, long long n, const Header& h, short* out, long long elems) {
  Bits br(d + h.scan, d + n);
  long long base[3]; base[0] = 0;
  for (int c = 1; c < 3; ++c) base[c] = base[c - 1] + (long long)h.bw[c - 1] * h.bh[c - 1] * 64;
  int pred[3] = {0, 0, 0};
  long long mcu = 0;
  int rst = 0;
  for (int my = 0; my < h.mcus_y; ++my)
    for (int mx = 0; mx < h.mcus_x; ++mx, ++mcu) {
      if (h.restart && mcu && mcu % h.restart == 0) {
        if (!br.restart(rst++)) return false;
        pred[0] = pred[1] = pred[2] = 0;
      }
      for (int c = 0; c < h.ncomp; ++c) {
        const HuffTab& dc = h.dc[h.td[c]];
        const HuffTab& ac = h.ac[h.ta[c]];
        for (int by = 0; by < h.vs[c]; ++by)
          for (int bx = 0; bx < h.hs[c]; ++bx) {
            const long long at = base[c] + ((long long)(my * h.vs[c] + by) * h.bw[c] + (mx * h.hs[c] + bx)) * 64;
            if (at < 0 || at + 64 > elems) return false;               // cannot happen: the grid and elems come from one header
            short* blk = out + at;
            br.fill();
            int s = huff_symbol(br, dc);
            if (s < 0 || s > 11) return false;
            if (s) pred[c] += receive_extend(br, s);
            if (pred[c] < -32768 || pred[c] > 32767) return false;
            blk[0] = (short)pred[c];
            for (int k = 1; k < 64;) {
              br.fill();
              const int rs = huff_symbol(br, ac);
              if (rs < 0) return false;
              const int r = rs >> 4;
              s = rs & 15;
              if (s == 0) {
                if (r != 15) break;                                    // end of block
                k += 16;
                continue;
              }
              k += r;
              if (k > 63) return false;
              blk[ZIGZAG[k]] = (short)receive_extend(br, s);
              ++k;
            }
            if (!br.ok()) return false;
          }
      }
    }
  return true;
}

void fill_desc(effdet_jpeg_desc_t& e, const Header& h, long long off_bytes) {
  e.width = h.width; e.height = h.height; e.ncomp = h.ncomp; e.sampling = h.sampling;
  long long o = off_bytes;
  for (int c = 0; c < 3; ++c) {
    e.blocks_w[c] = h.bw[c]; e.blocks_h[c] = h.bh[c];
    e.coef_off[c] = o;
    o += (long long)h.bw[c] * h.bh[c] * 128;
    if (c < h.ncomp) std::memcpy(e.qt[c], h.qt[h.tq[c]], sizeof e.qt[c]);
  }
}

// ================================================================================================ device
// last image whose first workgroup is <= wg (images without workgroups share their successor's start, so they are never chosen)
__device__ __forceinline__ int find_image(const effdet_jpeg_desc_t* __restrict__ desc, int B, int wg, bool rgb) {
  int lo = 0, hi = B;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    const int start = rgb ? desc[mid].rgb_wg0 : desc[mid].idct_wg0;
    if (start <= wg) lo = mid; else hi = mid;
  }
  return lo;
}

// One pass of the slow-integer IDCT on 8 values: the even part scaled by 2^13, constants = round(c * 2^13), result rounded once
// and shifted down by `descale`.
__device__ __forceinline__ void idct_pass(int x[8], int descale) {
  int z1 = (x[2] + x[6]) * 4433;
  const int t2e = z1 - x[6] * 15137, t3e = z1 + x[2] * 6270;
  const int t0e = (x[0] + x[4]) << 13, t1e = (x[0] - x[4]) << 13;
  const int t10 = t0e + t3e, t13 = t0e - t3e, t11 = t1e + t2e, t12 = t1e - t2e;
  int t0 = x[7], t1 = x[5], t2 = x[3], t3 = x[1];
  z1 = t0 + t3;
  int z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
  const int z5 = (z3 + z4) * 9633;
  t0 *= 2446; t1 *= 16819; t2 *= 25172; t3 *= 12299;
  z1 *= -7373; z2 *= -20995; z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5;
  t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
  const int r = 1 << (descale - 1);
  x[0] = (t10 + t3 + r) >> descale; x[7] = (t10 - t3 + r) >> descale;
  x[1] = (t11 + t2 + r) >> descale; x[6] = (t11 - t2 + r) >> descale;
  x[2] = (t12 + t1 + r) >> descale; x[5] = (t12 - t1 + r) >> descale;
  x[3] = (t13 + t0 + r) >> descale; x[4] = (t13 - t0 + r) >> descale;
}

__device__ __forceinline__ unsigned sample_u8(int v) {     // the range-limit table: index modulo 1024 around the level shift
  v &= 1023;
  if (v >= 512) v -= 1024;
  v += 128;
  return (unsigned)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

__global__ __launch_bounds__(256) void jpeg_idct_kernel(const short* __restrict__ coef, const effdet_jpeg_desc_t* __restrict__ desc,
                                                        int B, unsigned char* __restrict__ planes,
                                                        const long long* __restrict__ planes_off) {
  __shared__ int tile[IDCT_BLOCKS_PER_WG][8][9];
  const int b = find_image(desc, B, (int)blockIdx.x, false);
  const effdet_jpeg_desc_t& d = desc[b];
  const int g = threadIdx.x >> 3, r = threadIdx.x & 7;
  const long long nb0 = (long long)d.blocks_w[0] * d.blocks_h[0], nb1 = (long long)d.blocks_w[1] * d.blocks_h[1],
                  nb2 = (long long)d.blocks_w[2] * d.blocks_h[2];
  long long blk = (long long)((int)blockIdx.x - d.idct_wg0) * IDCT_BLOCKS_PER_WG + g;
  const bool live = d.status == EFFDET_OK && blk >= 0 && blk < nb0 + nb1 + nb2;
  int c = 0;
  long long plane0 = 0;                            // byte offset of the component's plane inside the image's plane block
  if (live && blk >= nb0) { blk -= nb0; c = 1; plane0 = nb0 * 64; if (blk >= nb1) { blk -= nb1; c = 2; plane0 += nb1 * 64; } }
  int x[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (live) {                                      // row r of the block: 8 coefficients x 8 table entries, 16 B each
    const uint4 cv = *(const uint4*)((const char*)coef + d.coef_off[c] + blk * 128 + r * 16);
    const uint4 qv = *(const uint4*)(&d.qt[c][r * 8]);
    const unsigned cw[4] = {cv.x, cv.y, cv.z, cv.w}, qw[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      x[2 * i] = (int)(short)(cw[i] & 0xFFFFu) * (int)(qw[i] & 0xFFFFu);
      x[2 * i + 1] = (int)(short)(cw[i] >> 16) * (int)(qw[i] >> 16);
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) tile[g][r][j] = x[j];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; ++k) x[k] = tile[g][k][r];            // pass 1: this lane takes column r
  idct_pass(x, 13 - 2);
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; ++k) tile[g][k][r] = x[k];
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 8; ++j) x[j] = tile[g][r][j];            // pass 2: row r
  idct_pass(x, 13 + 2 + 3);
  if (!live) return;
  const int bw = d.blocks_w[c];
  const long long brow = blk / bw, bcol = blk - brow * bw;
  uint2 o;
  o.x = sample_u8(x[0]) | (sample_u8(x[1]) << 8) | (sample_u8(x[2]) << 16) | (sample_u8(x[3]) << 24);
  o.y = sample_u8(x[4]) | (sample_u8(x[5]) << 8) | (sample_u8(x[6]) << 16) | (sample_u8(x[7]) << 24);
  *(uint2*)(planes + planes_off[b] + plane0 + (brow * 8 + r) * ((long long)bw * 8) + bcol * 8) = o;
}

// one chroma sample at full resolution, pixel (y, x): P is the MCU-padded plane with `pitch` bytes per row, dw x dh its real samples
__device__ __forceinline__ int chroma_at(const unsigned char* __restrict__ P, long long pitch, int sampling, int y, int x, int dw, int dh) {
  if (sampling == EFFDET_JPEG_444) return P[y * pitch + x];
  const int i = x >> 1;
  if (sampling == EFFDET_JPEG_422) {
    if (dw <= 2) return P[y * pitch + i];                      // too narrow for the filter: replication
    const int near = P[y * pitch + i];
    return x & 1 ? (3 * near + P[y * pitch + min(i + 1, dw - 1)] + 2) >> 2 : (3 * near + P[y * pitch + max(i - 1, 0)] + 1) >> 2;
  }
  const int j = y >> 1;
  if (dw <= 2) return P[j * pitch + i];
  const int j2 = y & 1 ? min(j + 1, dh - 1) : max(j - 1, 0), i2 = x & 1 ? min(i + 1, dw - 1) : max(i - 1, 0);
  const int near = 3 * P[j * pitch + i] + P[j2 * pitch + i], far = 3 * P[j * pitch + i2] + P[j2 * pitch + i2];
  return (3 * near + far + (x & 1 ? 7 : 8)) >> 4;
}

__device__ __forceinline__ int clamp_u8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__global__ __launch_bounds__(256) void jpeg_rgb_kernel(const effdet_jpeg_desc_t* __restrict__ desc, int B,
                                                       const unsigned char* __restrict__ planes, const long long* __restrict__ planes_off,
                                                       unsigned char* __restrict__ dst, const long long* __restrict__ dst_off) {
  const int b = find_image(desc, B, (int)blockIdx.x, true);
  const effdet_jpeg_desc_t& d = desc[b];
  if (d.status != EFFDET_OK) return;
  const int H = d.height, W = d.width, sampling = d.sampling;
  const long long npix = (long long)H * W, nbytes = npix * 3;
  const long long j0 = ((long long)((int)blockIdx.x - d.rgb_wg0) * 256 + threadIdx.x) * 16;
  if (j0 < 0 || j0 >= nbytes) return;
  const unsigned char* Y = planes + planes_off[b];
  const long long pitch_y = (long long)d.blocks_w[0] * 8, pitch_c = (long long)d.blocks_w[1] * 8;
  const unsigned char* Cb = Y + (long long)d.blocks_w[0] * d.blocks_h[0] * 64;
  const unsigned char* Cr = Cb + (long long)d.blocks_w[1] * d.blocks_h[1] * 64;
  const int dw = sampling == EFFDET_JPEG_444 ? W : (W + 1) >> 1, dh = sampling == EFFDET_JPEG_420 ? (H + 1) >> 1 : H;
  long long pix = j0 / 3;
  int ch = (int)(j0 - pix * 3);                    // channel of the chunk's first byte
  int y = (int)(pix / W), x = (int)(pix - (long long)y * W);
  unsigned long long lo = 0, hi = 0;
  int n = 0;
#pragma unroll 1
  for (int it = 0; it < 6 && n < 16 && pix < npix; ++it, ++pix) {      // 16 bytes touch at most 6 pixels
    const int yy = Y[y * pitch_y + x];
    int rgb[3] = {yy, yy, yy};
    if (sampling != EFFDET_JPEG_GREY) {
      const int cb = chroma_at(Cb, pitch_c, sampling, y, x, dw, dh) - 128, cr = chroma_at(Cr, pitch_c, sampling, y, x, dw, dh) - 128;
      rgb[0] = clamp_u8(yy + ((91881 * cr + 32768) >> 16));
      rgb[1] = clamp_u8(yy + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
      rgb[2] = clamp_u8(yy + ((116130 * cb + 32768) >> 16));
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (k >= ch && n < 16) {
        if (n < 8) lo |= (unsigned long long)rgb[k] << (8 * n); else hi |= (unsigned long long)rgb[k] << (8 * (n - 8));
        ++n;
      }
    ch = 0;
    if (++x == W) { x = 0; ++y; }
  }
  unsigned char* o = dst + dst_off[b] + j0;
  if (n == 16) *(uint4*)o = make_uint4((unsigned)lo, (unsigned)(lo >> 32), (unsigned)hi, (unsigned)(hi >> 32));
  else for (int k = 0; k < n; ++k) o[k] = (unsigned char)((k < 8 ? lo >> (8 * k) : hi >> (8 * (k - 8))) & 0xFF);   // the image's last bytes
}

}  // namespace

// ================================================================================================ C ABI
extern "C" int effdet_jpeg_probe(const unsigned char* bytes, long long nbytes, effdet_jpeg_info_t* info) {
  if (!info) return EFFDET_EINVAL;
  std::memset(info, 0, sizeof *info);
  std::vector<Header> hv(1);                       // ~12 KB of Huffman tables: off the stack
  Header& h = hv[0];
  const int st = parse_header(bytes, nbytes, h);
  info->reason = st == EFFDET_EUNSUPPORTED ? h.reason : EFFDET_JPEG_OK;
  if (st != EFFDET_OK) return st;
  info->width = h.width; info->height = h.height; info->ncomp = h.ncomp; info->sampling = h.sampling;
  info->restart_interval = h.restart; info->mcus_x = h.mcus_x; info->mcus_y = h.mcus_y;
  for (int c = 0; c < 3; ++c) { info->blocks_w[c] = h.bw[c]; info->blocks_h[c] = h.bh[c]; }
  info->coef_bytes = total_blocks(h) * 128;
  return EFFDET_OK;
}

extern "C" int effdet_jpeg_entropy_batch(const unsigned char* const* streams, const long long* nbytes, int B, short* coef_out,
                                         long long coef_bytes_total, const long long* coef_off, effdet_jpeg_desc_t* desc,
                                         int threads, int wg_totals[2]) {
  if (!streams || !nbytes || !coef_out || !coef_off || !desc || !wg_totals || B < 1 || coef_bytes_total < 0) return EFFDET_EINVAL;
  for (int b = 0; b < B; ++b)
    if (!streams[b] || nbytes[b] < 0 || coef_off[b] < 0 || coef_off[b] % 16 || coef_off[b] > coef_bytes_total) return EFFDET_EINVAL;
  threads = threads < 1 ? 1 : (threads > 16 ? 16 : threads);
  if (threads > B) threads = B;
  std::atomic<int> next(0);
  auto work = [&]() {
    std::vector<Header> hv(1);
    Header& h = hv[0];
    for (int b = next.fetch_add(1); b < B; b = next.fetch_add(1)) {
      effdet_jpeg_desc_t& e = desc[b];
      std::memset(&e, 0, sizeof e);
      e.status = parse_header(streams[b], nbytes[b], h);
      if (e.status != EFFDET_OK) continue;
      const long long need = total_blocks(h) * 128;
      if (need > coef_bytes_total - coef_off[b]) { e.status = EFFDET_EINVAL; continue; }   // the caller's range is too small: write nothing
      fill_desc(e, h, coef_off[b]);
      short* out = (short*)((char*)coef_out + coef_off[b]);
      std::memset(out, 0, (size_t)need);
      if (!decode_scan(streams[b], nbytes[b], h, out, need / 2)) {
        std::memset(out, 0, (size_t)need);
        e.status = EFFDET_EINVAL;
      }
    }
  };
  std::vector<std::thread> pool;
  for (int t = 1; t < threads; ++t) pool.emplace_back(work);
  work();
  for (auto& t : pool) t.join();
  long long w1 = 0, w2 = 0;
  int first_bad = EFFDET_OK;
  for (int b = 0; b < B; ++b) {
    effdet_jpeg_desc_t& e = desc[b];
    e.idct_wg0 = (int)w1; e.rgb_wg0 = (int)w2;
    if (e.status != EFFDET_OK) { if (first_bad == EFFDET_OK) first_bad = e.status; continue; }
    long long blocks = 0;
    for (int c = 0; c < 3; ++c) blocks += (long long)e.blocks_w[c] * e.blocks_h[c];
    w1 += (blocks + IDCT_BLOCKS_PER_WG - 1) / IDCT_BLOCKS_PER_WG;
    w2 += ((long long)e.height * e.width * 3 + RGB_BYTES_PER_WG - 1) / RGB_BYTES_PER_WG;
    if (w1 > 0x7FFFFFFFLL || w2 > 0x7FFFFFFFLL) return EFFDET_EUNSUPPORTED;                  // more workgroups than a grid holds
  }
  wg_totals[0] = (int)w1; wg_totals[1] = (int)w2;
  return first_bad;
}

extern "C" int effdet_jpeg_reconstruct(const short* coef, const effdet_jpeg_desc_t* desc, int B, int idct_wgs, int rgb_wgs,
                                       unsigned char* planes, const long long* planes_off, unsigned char* dst,
                                       const long long* dst_off, effdet_stream_t stream) {
  if (!coef || !desc || !planes || !planes_off || !dst || !dst_off || B < 1 || idct_wgs < 0 || rgb_wgs < 0) return EFFDET_EINVAL;
  if (((uintptr_t)coef | (uintptr_t)desc | (uintptr_t)planes | (uintptr_t)dst) & 15) return EFFDET_EINVAL;     // 16 B loads and stores
  hipStream_t st = (hipStream_t)stream;
  if (idct_wgs) {
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)idct_wgs), dim3(256), 0, st, coef, desc, B, planes, planes_off);
    EFFDET_CHECK_LAUNCH();
  }
  if (rgb_wgs) {
    hipLaunchKernelGGL(jpeg_rgb_kernel, dim3((unsigned)rgb_wgs), dim3(256), 0, st, desc, B, (const unsigned char*)planes, planes_off,
                       dst, dst_off);
    EFFDET_CHECK_LAUNCH();
  }
  return EFFDET_OK;
}
