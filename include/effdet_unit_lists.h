/* effdet_unit_lists.h -- gathered 32-pixel units for the flagged launches of the RetinaHead's regression tower: entry points added to
 * ABI generation 11 after effdet_needed_tiles.h's set (effdet_hip.h's conventions hold: device pointers, 0 or a negative EFFDET_E*
 * code, kernels enqueued on `stream`, no memset / copy / host sync, so every call may be captured in a graph).  A library of the same
 * generation built before this header lacks the symbols, so a binding looks them up by name before the first call.
 *
 * effdet_conv2d_live / effdet_conv2d_needed compute every 128-pixel flat tile that holds a flagged pixel.  A positive pixel dilated by
 * radius r touches 3 - 6 such tiles and fills a fraction of each; counted in 32-pixel units (effdet_live_tiles' live32 flags) the
 * benchmark's batch needs 0.53 - 0.80 of the pixels the tile flags make it compute (profiles/unit_count_b32_512.json).  The launches
 * below gather the flagged units, four to a tile, into the FIRST ceil(n_units / 4) workgroup rows of the flagged segments and compute
 * those; every workgroup row also writes the zero rows of its own original tile's unflagged units.  The grid is the dense one and the
 * counts are device data: nothing depends on the host knowing them.  Each computed output element sees the operands of the dense
 * launch in its K order, so the flagged pixels hold the dense launch's bytes and everything else is zero bytes. */
#ifndef EFFDET_UNIT_LISTS_H
#define EFFDET_UNIT_LISTS_H
#include "effdet_needed_tiles.h"
#ifdef __cplusplus
extern "C" {
#endif

#define EFFDET_UNIT_COUNTS 4         /* ints per radius in `counts` */

/* From effdet_live_tiles' flags (either source: d(reg) or a pixel map) the compacted lists, per radius r = 0 .. 5:
 *   units  [6][steps] int32: units[r][i], i < n, = the indices of the set flags of live32[r], ascending (level-major, the order of the
 *          flags); entries from n on are not written;
 *   counts [6][4] int32: counts[r] = { n = set flags of live32[r], set flags of live128[r], gather, 0 } with gather = 1 iff
 *          16 * ceil(n / 4) <= 15 * (set flags of live128[r]): the gathered form computes at least 1/16 fewer tiles than the tile flags
 *          (its tiles stage their activations per tap, which costs 3.5 - 5 % of a tile against the row slabs of the flagged form).
 * One workgroup per radius, a block scan in a fixed order, plain stores: no atomics, nothing assumed about the buffers' content. */
int effdet_unit_lists(const unsigned char* live32, const unsigned char* live128, long long steps, long long tiles, int* units,
                      int* counts, effdet_stream_t stream);

/* effdet_conv2d_needed / effdet_conv2d_live in the gathered form.  flags128: that call's tile flags (one byte per 128-pixel tile from
 * tile0 on); flags32, units, counts: the SAME radius' rows of live32, `units` and `counts` (one byte / entry per 32-pixel step of the
 * flagged segments, which are the segments from tile tile0 on: one pyramid, levels in order).  With counts[2] == 0 -- read on the device
 * -- or where the launch cannot take the gathered form (other than a 3x3, stride 1, pad 1 conv on kernel ids 30 / 31 resp. 8 / 9; the
 * flagged segments not sharing weights and bias; their inputs spanning 4 GiB or more; tile0 not the first tile of a segment) it is the
 * call with flags128 alone; never a dense launch.  Otherwise workgroup row mt >= tile0 writes zero bytes to the rows of tile mt's units
 * whose flags32 byte is 0 (nothing under an in-place EFFDET_RES_ADD) and, if 4 * (mt - tile0) < counts[0], computes the tile whose four
 * 32-row groups are the units units[4 * (mt - tile0) ..+ 3] (a last one may have fewer). */
int effdet_conv2d_needed_units(const effdet_conv_t* p, const unsigned char* flags128, const unsigned char* flags32, const int* units,
                               const int* counts, int tile0, effdet_stream_t stream);
int effdet_conv2d_live_units(const effdet_conv_t* p, const unsigned char* flags128, const unsigned char* flags32, const int* units,
                             const int* counts, int tile0, effdet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EFFDET_UNIT_LISTS_H */
