// effdet_draw_detections: boxes, translucent fills and text labels painted into uint8 RGB frames (include/effdet_draw.h holds the
// rule).  The painter's loop is order-dependent, so it becomes a gather: ONE 256-thread workgroup per 64 x 16 pixel tile of one
// frame; a wave owns whole tile rows (lane = x, so a wave's 64 pixels are 192 consecutive bytes whatever the row's alignment: the
// three byte accesses of a wave each fall in the same two or three cache lines) and a thread keeps its 4 pixels in registers from the one read
// to the one write.  Rows are binned 256 at a time: thread i of a pass derives row k0 + i's integers, tests its extent against the
// tile, the four waves' ballots are compacted in row order into an LDS list, and every thread walks that list over its own pixels
// (all lanes read the same entry: an LDS broadcast).  Two sweeps over the rows: fills and outlines (tested by the outline rectangle),
// then labels (tested by the label rectangle; the text of a listed row is built once, into LDS, by the thread that binned it).  A
// tile nothing touches reads and writes no pixel.  No atomics.  Built with -ffp-contract=off: x1 * sx and score * 100 + 0.5 round as
// the header says.
#include "common.h"
#include "../../../include/effdet_draw.h"

namespace {

constexpr int TW = EFFDET_DRAW_TILE_W, TH = EFFDET_DRAW_TILE_H, NT = 256, WAVES = NT / 64, PPT = TW * TH / NT;
static_assert(TW == 64 && TH % WAVES == 0, "a wave owns whole tile rows");

// The font: 95 glyphs of 5 x 8 for 0x20..0x7E, rows top to bottom as 5-bit numbers whose bit 4 is the leftmost column.
#define G(a, b, c, d, e, f, g, h)                                                                                              \
  ((unsigned long long)(a) | (unsigned long long)(b) << 5 | (unsigned long long)(c) << 10 | (unsigned long long)(d) << 15 |    \
   (unsigned long long)(e) << 20 | (unsigned long long)(f) << 25 | (unsigned long long)(g) << 30 | (unsigned long long)(h) << 35)
#define DRAW_FONT                                                                                        \
  G(0b00000, 0b00000, 0b00000, 0b00000, 0b00000, 0b00000, 0b00000, 0b00000), /* space */                 \
  G(0b00100, 0b00100, 0b00100, 0b00100, 0b00100, 0b00000, 0b00100, 0b00000), /* ! */                     \
  G(0b01010, 0b01010, 0b01010, 0b00000, 0b00000, 0b00000, 0b00000, 0b00000), /* " */                     \
  G(0b01010, 0b01010, 0b11111, 0b01010, 0b11111, 0b01010, 0b01010, 0b00000), /* # */                     \
  G(0b00100, 0b01111, 0b10100, 0b01110, 0b00101, 0b11110, 0b00100, 0b00000), /* $ */                     \
  G(0b11000, 0b11001, 0b00010, 0b00100, 0b01000, 0b10011, 0b00011, 0b00000), /* % */                     \
  G(0b01100, 0b10010, 0b10100, 0b01000, 0b10101, 0b10010, 0b01101, 0b00000), /* & */                     \
  G(0b00100, 0b00100, 0b01000, 0b00000, 0b00000, 0b00000, 0b00000, 0b00000), /* ' */                     \
  G(0b00010, 0b00100, 0b01000, 0b01000, 0b01000, 0b00100, 0b00010, 0b00000), /* ( */                     \
  G(0b01000, 0b00100, 0b00010, 0b00010, 0b00010, 0b00100, 0b01000, 0b00000), /* ) */                     \
  G(0b00000, 0b00100, 0b10101, 0b01110, 0b10101, 0b00100, 0b00000, 0b00000), /* * */                     \
  G(0b00000, 0b00100, 0b00100, 0b11111, 0b00100, 0b00100, 0b00000, 0b00000), /* + */                     \
  G(0b00000, 0b00000, 0b00000, 0b00000, 0b00000, 0b01100, 0b00100, 0b01000), /* , */                     \
  G(0b00000, 0b00000, 0b00000, 0b11111, 0b00000, 0b00000, 0b00000, 0b00000), /* - */                     \
  G(0b00000, 0b00000, 0b00000, 0b00000, 0b00000, 0b01100, 0b01100, 0b00000), /* . */                     \
  G(0b00000, 0b00001, 0b00010, 0b00100, 0b01000, 0b10000, 0b00000, 0b00000), /* / */                     \
  G(0b01110, 0b10001, 0b10011, 0b10101, 0b11001, 0b10001, 0b01110, 0b00000), /* 0 */                     \
  G(0b00100, 0b01100, 0b00100, 0b00100, 0b00100, 0b00100, 0b01110, 0b00000), /* 1 */                     \
  G(0b01110, 0b10001, 0b00001, 0b00010, 0b00100, 0b01000, 0b11111, 0b00000), /* 2 */                     \
  G(0b11111, 0b00010, 0b00100, 0b00010, 0b00001, 0b10001, 0b01110, 0b00000), /* 3 */                     \
  G(0b00010, 0b00110, 0b01010, 0b10010, 0b11111, 0b00010, 0b00010, 0b00000), /* 4 */                     \
  G(0b11111, 0b10000, 0b11110, 0b00001, 0b00001, 0b10001, 0b01110, 0b00000), /* 5 */                     \
  G(0b00110, 0b01000, 0b10000, 0b11110, 0b10001, 0b10001, 0b01110, 0b00000), /* 6 */                     \
  G(0b11111, 0b00001, 0b00010, 0b00100, 0b01000, 0b01000, 0b01000, 0b00000), /* 7 */                     \
  G(0b01110, 0b10001, 0b10001, 0b01110, 0b10001, 0b10001, 0b01110, 0b00000), /* 8 */                     \
  G(0b01110, 0b10001, 0b10001, 0b01111, 0b00001, 0b00010, 0b01100, 0b00000), /* 9 */                     \
  G(0b00000, 0b01100, 0b01100, 0b00000, 0b01100, 0b01100, 0b00000, 0b00000), /* : */                     \
  G(0b00000, 0b01100, 0b01100, 0b00000, 0b01100, 0b00100, 0b01000, 0b00000), /* ; */                     \
  G(0b00010, 0b00100, 0b01000, 0b10000, 0b01000, 0b00100, 0b00010, 0b00000), /* < */                     \
  G(0b00000, 0b00000, 0b11111, 0b00000, 0b11111, 0b00000, 0b00000, 0b00000), /* = */                     \
  G(0b01000, 0b00100, 0b00010, 0b00001, 0b00010, 0b00100, 0b01000, 0b00000), /* > */                     \
  G(0b01110, 0b10001, 0b00001, 0b00010, 0b00100, 0b00000, 0b00100, 0b00000), /* ? */                     \
  G(0b01110, 0b10001, 0b00001, 0b01101, 0b10101, 0b10101, 0b01110, 0b00000), /* @ */                     \
  G(0b01110, 0b10001, 0b10001, 0b10001, 0b11111, 0b10001, 0b10001, 0b00000), /* A */                     \
  G(0b11110, 0b10001, 0b10001, 0b11110, 0b10001, 0b10001, 0b11110, 0b00000), /* B */                     \
  G(0b01110, 0b10001, 0b10000, 0b10000, 0b10000, 0b10001, 0b01110, 0b00000), /* C */                     \
  G(0b11100, 0b10010, 0b10001, 0b10001, 0b10001, 0b10010, 0b11100, 0b00000), /* D */                     \
  G(0b11111, 0b10000, 0b10000, 0b11110, 0b10000, 0b10000, 0b11111, 0b00000), /* E */                     \
  G(0b11111, 0b10000, 0b10000, 0b11110, 0b10000, 0b10000, 0b10000, 0b00000), /* F */                     \
  G(0b01110, 0b10001, 0b10000, 0b10111, 0b10001, 0b10001, 0b01111, 0b00000), /* G */                     \
  G(0b10001, 0b10001, 0b10001, 0b11111, 0b10001, 0b10001, 0b10001, 0b00000), /* H */                     \
  G(0b01110, 0b00100, 0b00100, 0b00100, 0b00100, 0b00100, 0b01110, 0b00000), /* I */                     \
  G(0b00111, 0b00010, 0b00010, 0b00010, 0b00010, 0b10010, 0b01100, 0b00000), /* J */                     \
  G(0b10001, 0b10010, 0b10100, 0b11000, 0b10100, 0b10010, 0b10001, 0b00000), /* K */                     \
  G(0b10000, 0b10000, 0b10000, 0b10000, 0b10000, 0b10000, 0b11111, 0b00000), /* L */                     \
  G(0b10001, 0b11011, 0b10101, 0b10101, 0b10001, 0b10001, 0b10001, 0b00000), /* M */                     \
  G(0b10001, 0b10001, 0b11001, 0b10101, 0b10011, 0b10001, 0b10001, 0b00000), /* N */                     \
  G(0b01110, 0b10001, 0b10001, 0b10001, 0b10001, 0b10001, 0b01110, 0b00000), /* O */                     \
  G(0b11110, 0b10001, 0b10001, 0b11110, 0b10000, 0b10000, 0b10000, 0b00000), /* P */                     \
  G(0b01110, 0b10001, 0b10001, 0b10001, 0b10101, 0b10010, 0b01101, 0b00000), /* Q */                     \
  G(0b11110, 0b10001, 0b10001, 0b11110, 0b10100, 0b10010, 0b10001, 0b00000), /* R */                     \
  G(0b01111, 0b10000, 0b10000, 0b01110, 0b00001, 0b00001, 0b11110, 0b00000), /* S */                     \
  G(0b11111, 0b00100, 0b00100, 0b00100, 0b00100, 0b00100, 0b00100, 0b00000), /* T */                     \
  G(0b10001, 0b10001, 0b10001, 0b10001, 0b10001, 0b10001, 0b01110, 0b00000), /* U */                     \
  G(0b10001, 0b10001, 0b10001, 0b10001, 0b10001, 0b01010, 0b00100, 0b00000), /* V */                     \
  G(0b10001, 0b10001, 0b10001, 0b10101, 0b10101, 0b10101, 0b01010, 0b00000), /* W */                     \
  G(0b10001, 0b10001, 0b01010, 0b00100, 0b01010, 0b10001, 0b10001, 0b00000), /* X */                     \
  G(0b10001, 0b10001, 0b10001, 0b01010, 0b00100, 0b00100, 0b00100, 0b00000), /* Y */                     \
  G(0b11111, 0b00001, 0b00010, 0b00100, 0b01000, 0b10000, 0b11111, 0b00000), /* Z */                     \
  G(0b01110, 0b01000, 0b01000, 0b01000, 0b01000, 0b01000, 0b01110, 0b00000), /* [ */                     \
  G(0b00000, 0b10000, 0b01000, 0b00100, 0b00010, 0b00001, 0b00000, 0b00000), /* backslash */             \
  G(0b01110, 0b00010, 0b00010, 0b00010, 0b00010, 0b00010, 0b01110, 0b00000), /* ] */                     \
  G(0b00100, 0b01010, 0b10001, 0b00000, 0b00000, 0b00000, 0b00000, 0b00000), /* ^ */                     \
  G(0b00000, 0b00000, 0b00000, 0b00000, 0b00000, 0b00000, 0b11111, 0b00000), /* _ */                     \
  G(0b01000, 0b00100, 0b00010, 0b00000, 0b00000, 0b00000, 0b00000, 0b00000), /* ` */                     \
  G(0b00000, 0b00000, 0b01110, 0b00001, 0b01111, 0b10001, 0b01111, 0b00000), /* a */                     \
  G(0b10000, 0b10000, 0b10110, 0b11001, 0b10001, 0b10001, 0b11110, 0b00000), /* b */                     \
  G(0b00000, 0b00000, 0b01110, 0b10000, 0b10000, 0b10001, 0b01110, 0b00000), /* c */                     \
  G(0b00001, 0b00001, 0b01101, 0b10011, 0b10001, 0b10001, 0b01111, 0b00000), /* d */                     \
  G(0b00000, 0b00000, 0b01110, 0b10001, 0b11111, 0b10000, 0b01110, 0b00000), /* e */                     \
  G(0b00110, 0b01001, 0b01000, 0b11100, 0b01000, 0b01000, 0b01000, 0b00000), /* f */                     \
  G(0b00000, 0b00000, 0b01111, 0b10001, 0b10001, 0b01111, 0b00001, 0b01110), /* g */                     \
  G(0b10000, 0b10000, 0b10110, 0b11001, 0b10001, 0b10001, 0b10001, 0b00000), /* h */                     \
  G(0b00100, 0b00000, 0b01100, 0b00100, 0b00100, 0b00100, 0b01110, 0b00000), /* i */                     \
  G(0b00010, 0b00000, 0b00110, 0b00010, 0b00010, 0b00010, 0b10010, 0b01100), /* j */                     \
  G(0b10000, 0b10000, 0b10010, 0b10100, 0b11000, 0b10100, 0b10010, 0b00000), /* k */                     \
  G(0b01100, 0b00100, 0b00100, 0b00100, 0b00100, 0b00100, 0b01110, 0b00000), /* l */                     \
  G(0b00000, 0b00000, 0b11010, 0b10101, 0b10101, 0b10001, 0b10001, 0b00000), /* m */                     \
  G(0b00000, 0b00000, 0b10110, 0b11001, 0b10001, 0b10001, 0b10001, 0b00000), /* n */                     \
  G(0b00000, 0b00000, 0b01110, 0b10001, 0b10001, 0b10001, 0b01110, 0b00000), /* o */                     \
  G(0b00000, 0b00000, 0b11110, 0b10001, 0b10001, 0b11110, 0b10000, 0b10000), /* p */                     \
  G(0b00000, 0b00000, 0b01101, 0b10011, 0b10001, 0b01111, 0b00001, 0b00001), /* q */                     \
  G(0b00000, 0b00000, 0b10110, 0b11001, 0b10000, 0b10000, 0b10000, 0b00000), /* r */                     \
  G(0b00000, 0b00000, 0b01110, 0b10000, 0b01110, 0b00001, 0b11110, 0b00000), /* s */                     \
  G(0b01000, 0b01000, 0b11100, 0b01000, 0b01000, 0b01001, 0b00110, 0b00000), /* t */                     \
  G(0b00000, 0b00000, 0b10001, 0b10001, 0b10001, 0b10011, 0b01101, 0b00000), /* u */                     \
  G(0b00000, 0b00000, 0b10001, 0b10001, 0b10001, 0b01010, 0b00100, 0b00000), /* v */                     \
  G(0b00000, 0b00000, 0b10001, 0b10001, 0b10101, 0b10101, 0b01010, 0b00000), /* w */                     \
  G(0b00000, 0b00000, 0b10001, 0b01010, 0b00100, 0b01010, 0b10001, 0b00000), /* x */                     \
  G(0b00000, 0b00000, 0b10001, 0b10001, 0b10001, 0b01111, 0b00001, 0b01110), /* y */                     \
  G(0b00000, 0b00000, 0b11111, 0b00010, 0b00100, 0b01000, 0b11111, 0b00000), /* z */                     \
  G(0b00010, 0b00100, 0b00100, 0b01000, 0b00100, 0b00100, 0b00010, 0b00000), /* { */                     \
  G(0b00100, 0b00100, 0b00100, 0b00100, 0b00100, 0b00100, 0b00100, 0b00000), /* | */                     \
  G(0b01000, 0b00100, 0b00100, 0b00010, 0b00100, 0b00100, 0b01000, 0b00000), /* } */                     \
  G(0b00000, 0b00000, 0b01000, 0b10101, 0b00010, 0b00000, 0b00000, 0b00000)  /* ~ */

// one table in the source; the device reads its copy in constant memory, effdet_draw_glyph the host's
const unsigned long long kFontHost[95] = {DRAW_FONT};
__constant__ unsigned long long kFont[95] = {DRAW_FONT};

struct DrawArgs {
  unsigned char* pixels; const long long* pix_off; const int* pix_hw; int Hmax, Wmax;
  const float* rows; int row_stride, K; const int* counts; const int* ids; const float* box_scale;
  const unsigned char* names; const unsigned char* name_len; int n_names; const unsigned char* palette; int P;
  int thickness, fill_alpha, label, show_score, show_id, text_scale, color_by_id;
};

struct Row { int x1, y1, x2, y2, L; float score; bool ok; };

__device__ __forceinline__ bool finite_(float v) { return v - v == 0.f; }
__device__ __forceinline__ int coord_(float v) { return (int)fminf(fmaxf(v, -1048576.f), 1048576.f); }

// the header's "Coordinates" for one row
__device__ __forceinline__ Row read_row(const float* r, float sx, float sy) {
  Row g;
  const float a = r[0] * sx, b = r[1] * sy, c = r[2] * sx, d = r[3] * sy, lab = r[5];
  g.score = r[4];
  g.ok = finite_(a) && finite_(b) && finite_(c) && finite_(d) && lab >= 0.f;               // (a NaN label fails the compare)
  g.x1 = coord_(a); g.y1 = coord_(b); g.x2 = coord_(c); g.y2 = coord_(d);
  g.ok = g.ok && g.x2 >= g.x1 && g.y2 >= g.y1;
  g.L = g.ok ? (int)fminf(lab, 2147483520.f) : 0;
  return g;
}

__device__ __forceinline__ unsigned colour_of(const DrawArgs& a, int key) {               // R | G << 8 | B << 16 | black text << 24
  int i = key % a.P;
  if (i < 0) i += a.P;
  const unsigned R = a.palette[3 * i], Gc = a.palette[3 * i + 1], Bc = a.palette[3 * i + 2];
  return R | Gc << 8 | Bc << 16 | (299u * R + 587u * Gc + 114u * Bc >= 128000u ? 1u << 24 : 0u);
}

__device__ __forceinline__ int digits_(unsigned v) {
  int d = 1;
  while (v >= 10u) { v /= 10u; ++d; }
  return d;
}
__device__ __forceinline__ int put_dec(unsigned char* out, int pos, unsigned v) {
  const int d = digits_(v);
  for (int i = d - 1; i >= 0; --i) { out[pos + i] = (unsigned char)('0' + v % 10u); v /= 10u; }
  return pos + d;
}
__device__ __forceinline__ int pct_of(float score) {
  if (!finite_(score)) return 0;
  const float f = score * 100.f + 0.5f;
  return f <= 0.f ? 0 : (f >= 100.f ? 100 : (int)f);
}
// the label's characters: its length, and the text itself into out[EFFDET_DRAW_TEXT_MAX]
__device__ __forceinline__ int text_len(const DrawArgs& a, const Row& g, int id) {
  int n = g.L < a.n_names ? min((int)a.name_len[g.L], EFFDET_DRAW_NAME_MAX) : digits_((unsigned)g.L);
  if (a.show_id) n += 2 + digits_((unsigned)max(id, 0));
  if (a.show_score) n += 1 + digits_((unsigned)pct_of(g.score));
  return n;
}
__device__ __forceinline__ void text_put(const DrawArgs& a, const Row& g, int id, unsigned char* out) {
  int p = 0;
  if (a.show_id) { out[p++] = '#'; p = put_dec(out, p, (unsigned)max(id, 0)); out[p++] = ' '; }
  if (g.L < a.n_names) {
    const int n = min((int)a.name_len[g.L], EFFDET_DRAW_NAME_MAX);
    for (int i = 0; i < n; ++i) out[p++] = a.names[(long long)g.L * EFFDET_DRAW_NAME_MAX + i];
  } else {
    p = put_dec(out, p, (unsigned)g.L);
  }
  if (a.show_score) { out[p++] = ' '; p = put_dec(out, p, (unsigned)pct_of(g.score)); }
}

// Compacts the workgroup's hits in thread (= row) order: -> this thread's slot (valid where hit), total in `total`.
__device__ __forceinline__ int compact(bool hit, int* wcnt, int lane, int wave, int& total) {
  const unsigned long long m = __ballot(hit);
  __syncthreads();                                                     // (the previous pass has finished with wcnt and the lists)
  if (lane == 0) wcnt[wave] = __popcll(m);
  __syncthreads();
  int base = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) { base += w < wave ? wcnt[w] : 0; total += wcnt[w]; }
  return base + __popcll(m & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(NT) void draw_kernel(DrawArgs a) {
  __shared__ int s_rect[NT][4];                      // sweep 1: X1, Y1, X2, Y2;  sweep 2: Lx, Ly, characters, unused
  __shared__ unsigned s_col[NT];
  __shared__ unsigned char s_txt[NT][EFFDET_DRAW_TEXT_MAX];
  __shared__ int s_wcnt[WAVES];
  const int b = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int H = a.pix_hw ? a.pix_hw[2 * b] : a.Hmax, W = a.pix_hw ? a.pix_hw[2 * b + 1] : a.Wmax;
  const int tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH;
  if (tx0 >= W || ty0 >= H) return;                                    // (uniform: a tile outside a smaller frame)
  const int tx1 = min(tx0 + TW, W) - 1, ty1 = min(ty0 + TH, H) - 1;    // the tile's pixels inside the frame, inclusive
  const int n = min(max(a.counts[b], 0), a.K);
  const int t = a.thickness, o = t >> 1, s = a.text_scale, alpha = a.fill_alpha;
  const float sx = a.box_scale ? a.box_scale[2 * b] : 1.f, sy = a.box_scale ? a.box_scale[2 * b + 1] : 1.f;
  const float* rows = a.rows + (long long)b * a.K * a.row_stride;
  const int* ids = a.ids ? a.ids + (long long)b * a.K : nullptr;
  unsigned char* frame = a.pixels + (a.pix_off ? a.pix_off[b] : (long long)b * a.Hmax * a.Wmax * 3);

  const int px = tx0 + lane;
  int cr[PPT], cg[PPT], cb[PPT];
  bool live[PPT], touched[PPT];
#pragma unroll
  for (int i = 0; i < PPT; ++i) {
    const int py = ty0 + wave + WAVES * i;
    live[i] = px <= tx1 && py <= ty1;
    touched[i] = false;
    cr[i] = cg[i] = cb[i] = 0;
  }
  bool loaded = false;                                                 // (uniform) the pixels are read when the first fill needs them

  // ---- sweep 1: for k ascending, the fill and then the outline
  if (t > 0 || alpha > 0) {
    for (int k0 = 0; k0 < n; k0 += NT) {
      const int k = k0 + tid;
      Row g; g.ok = false;
      if (k < n) g = read_row(rows + (long long)k * a.row_stride, sx, sy);
      const bool hit = g.ok && g.x1 - o <= tx1 && g.x2 + o >= tx0 && g.y1 - o <= ty1 && g.y2 + o >= ty0;
      int total;
      const int slot = compact(hit, s_wcnt, lane, wave, total);
      if (hit) {
        s_rect[slot][0] = g.x1; s_rect[slot][1] = g.y1; s_rect[slot][2] = g.x2; s_rect[slot][3] = g.y2;
        s_col[slot] = colour_of(a, a.color_by_id ? ids[k] : g.L);
      }
      __syncthreads();
      if (total > 0 && alpha > 0 && !loaded) {
        loaded = true;
#pragma unroll
        for (int i = 0; i < PPT; ++i)
          if (live[i]) {
            const unsigned char* p = frame + ((long long)(ty0 + wave + WAVES * i) * W + px) * 3;
            cr[i] = p[0]; cg[i] = p[1]; cb[i] = p[2];
          }
      }
      for (int e = 0; e < total; ++e) {
        const int X1 = s_rect[e][0], Y1 = s_rect[e][1], X2 = s_rect[e][2], Y2 = s_rect[e][3];
        const unsigned c = s_col[e];
        const int R = c & 255u, Gc = (c >> 8) & 255u, Bc = (c >> 16) & 255u;
        const int hx1 = X1 - o + t, hx2 = X2 + o - t, hy1 = Y1 - o + t, hy2 = Y2 + o - t;
        const bool hole = hx1 <= hx2 && hy1 <= hy2;
#pragma unroll
        for (int i = 0; i < PPT; ++i) {
          const int py = ty0 + wave + WAVES * i;
          if (!live[i]) continue;
          if (alpha > 0 && px >= X1 && px <= X2 && py >= Y1 && py <= Y2) {
            cr[i] = (R * alpha + cr[i] * (255 - alpha) + 127) / 255;
            cg[i] = (Gc * alpha + cg[i] * (255 - alpha) + 127) / 255;
            cb[i] = (Bc * alpha + cb[i] * (255 - alpha) + 127) / 255;
            touched[i] = true;
          }
          if (t > 0 && px >= X1 - o && px <= X2 + o && py >= Y1 - o && py <= Y2 + o &&
              !(hole && px >= hx1 && px <= hx2 && py >= hy1 && py <= hy2)) {
            cr[i] = R; cg[i] = Gc; cb[i] = Bc;
            touched[i] = true;
          }
        }
      }
    }
  }

  // ---- sweep 2: for k ascending, the label
  if (a.label) {
    for (int k0 = 0; k0 < n; k0 += NT) {
      const int k = k0 + tid;
      Row g; g.ok = false;
      int id = 0, nch = 0, Lx = 0, Ly = 0;
      bool hit = false;
      if (k < n) g = read_row(rows + (long long)k * a.row_stride, sx, sy);
      if (g.ok) {
        id = ids ? ids[k] : 0;
        nch = text_len(a, g, id);
        const int width = 6 * s * nch + s;
        Lx = g.x1 - o; Ly = g.y1 - o - 9 * s;
        if (Ly < 0) Ly = g.y1 - o + t;
        Lx = max(min(Lx, W - width), 0);
        hit = Lx <= tx1 && Lx + width - 1 >= tx0 && Ly <= ty1 && Ly + 9 * s - 1 >= ty0;
      }
      int total;
      const int slot = compact(hit, s_wcnt, lane, wave, total);
      if (hit) {
        s_rect[slot][0] = Lx; s_rect[slot][1] = Ly; s_rect[slot][2] = nch; s_rect[slot][3] = 0;
        s_col[slot] = colour_of(a, a.color_by_id ? id : g.L);
        text_put(a, g, id, s_txt[slot]);
      }
      __syncthreads();
      for (int e = 0; e < total; ++e) {
        const int X = s_rect[e][0], Y = s_rect[e][1], width = 6 * s * s_rect[e][2] + s;
        const unsigned c = s_col[e];
        const int ink = (c >> 24) & 1u ? 0 : 255;
#pragma unroll
        for (int i = 0; i < PPT; ++i) {
          const int py = ty0 + wave + WAVES * i;
          const int u = px - X, v = py - Y;
          if (!live[i] || u < 0 || u >= width || v < 0 || v >= 9 * s) continue;
          bool set = false;
          if (u >= s && v >= s) {
            const int j = (u - s) / (6 * s), col = ((u - s) - j * 6 * s) / s, r = (v - s) / s;
            if (col < 5) {
              int code = s_txt[e][j];
              if (code < 0x20 || code > 0x7E) code = '?';
              set = (kFont[code - 0x20] >> (5 * r + 4 - col)) & 1ull;
            }
          }
          cr[i] = set ? ink : (int)(c & 255u);
          cg[i] = set ? ink : (int)((c >> 8) & 255u);
          cb[i] = set ? ink : (int)((c >> 16) & 255u);
          touched[i] = true;
        }
      }
    }
  }

#pragma unroll
  for (int i = 0; i < PPT; ++i)
    if (touched[i]) {                                                  // (touched implies live: inside the frame)
      unsigned char* p = frame + ((long long)(ty0 + wave + WAVES * i) * W + px) * 3;
      p[0] = (unsigned char)cr[i]; p[1] = (unsigned char)cg[i]; p[2] = (unsigned char)cb[i];
    }
}

}  // namespace

extern "C" unsigned long long effdet_draw_glyph(int code) { return kFontHost[(code < 0x20 || code > 0x7E ? '?' : code) - 0x20]; }

extern "C" int effdet_draw_detections(unsigned char* pixels, const long long* pix_off, const int* pix_hw, int B, int Hmax, int Wmax,
                                      const float* rows, int row_stride, int K, const int* counts, const int* ids, const float* box_scale,
                                      const unsigned char* names, const unsigned char* name_len, int n_names,
                                      const unsigned char* palette, int P, int thickness, int fill_alpha, int label, int show_score,
                                      int show_id, int text_scale, int color_by_id, effdet_stream_t stream) {
  if (!pixels || !rows || !counts || !palette || B < 1 || K < 1 || Hmax < 1 || Wmax < 1 || row_stride < 6 || P < 1 || n_names < 0 ||
      (n_names > 0 && (!names || !name_len)) || ((color_by_id || show_id) && !ids) || thickness < 0 || fill_alpha < 0 ||
      fill_alpha > 255 || text_scale < 1)
    return EFFDET_EINVAL;
  if (K > EFFDET_DRAW_MAX_ROWS || thickness > EFFDET_DRAW_MAX_THICKNESS || text_scale > EFFDET_DRAW_MAX_TEXT_SCALE ||
      Hmax > EFFDET_DRAW_MAX_SIDE || Wmax > EFFDET_DRAW_MAX_SIDE || B > EFFDET_DRAW_MAX_BATCH)
    return EFFDET_EUNSUPPORTED;
  const DrawArgs a{pixels, pix_off, pix_hw, Hmax, Wmax, rows, row_stride, K, counts, ids, box_scale, names, name_len, n_names, palette, P,
                   thickness, fill_alpha, label != 0, show_score != 0, show_id != 0, text_scale, color_by_id != 0};
  hipLaunchKernelGGL(draw_kernel, dim3((Wmax + TW - 1) / TW, (Hmax + TH - 1) / TH, B), dim3(NT), 0, (hipStream_t)stream, a);
  EFFDET_CHECK_LAUNCH();
  return EFFDET_OK;
}
