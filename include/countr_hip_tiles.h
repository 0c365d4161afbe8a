/*
 * countr_hip_tiles.h -- C ABI of libcountr_hip_tiles.so: a frame counted at k times the model's height on a 2-D grid of 384 x 384 tiles.
 * countr_hip.h, countr_hip_ext.h and countr_hip_classes.h are closed; this header is the one statement of a library of its own, in the
 * same dialect (countr_amd/_lib.py::parse_header reads all four), with the same conventions: extern "C", plain pointers and sizes, 0 / a
 * size on success and < 0 on error with the text in countr_tiles_last_error() (thread-local), no allocation and no synchronisation
 * inside a call.  One build, no fp16 twin: nothing here has a 16-bit operand.  The library keeps no per-device state and needs no init
 * call.
 *
 * THE RULE (countr_amd/tiles.py restates it in torch / numpy).
 *   Zoomed size.  Hk = 384 k, Wk = 16 int((W / H Hk) / 16) for k in 1 .. 4; the zoomed image is the Pillow-exact bilinear resize of the
 *     ORIGINAL frame to (Wk, Hk) (countr_frame_resize_u8 of countr_hip.h), fp32 planar [3, Hk, Wk].
 *   Tile starts.  starts(size, stride): s = 0, stride, 2 stride, ... as long as the tile fits (s + 384 <= size); the first start whose
 *     tile would pass the end is snapped to size - 384 and closes the list, unless the tile before it already ends at size (the
 *     reference's window loop with 128 replaced by stride).  size < 384 has no starts.  Columns: starts(Wk, 128).  Rows:
 *     starts(Hk, band_stride), band_stride in {128, 192, 256, 384}.  At most COUNTR_TILES_MAX_STARTS starts per axis.  A list of starts
 *     accepted here begins at 0, increases strictly, leaves no gap (start[i] <= start[i - 1] + 384) and ends at size - 384.
 *   Tile order.  Band-major: tile (b, c) = rows [row[b], row[b] + 384) x columns [col[c], col[c] + 384) has index b * ncols + c.
 *   Stitching.  Band b's map is the sequential horizontal blend of its tiles in column order: a column that an earlier tile of the band
 *     already covered becomes old / 2 + new / 2, any other column is the new tile's.  The frame's map is the same sequential rule over
 *     the band maps along the rows, in band order.  x / 2 is exact, so the map is defined bit for bit.
 *   Sums.  sums[0] is the fp32 sum of the map; sums[1 + r] the fp32 sum over rectangle r = (y1, x1, y2, x2), corners inclusive, clipped
 *     to the map (an empty intersection sums to 0).  No floating-point atomics: a workgroup writes one partial per sum into the
 *     workspace, a second launch folds them in a fixed order.  Two runs give the same bytes.
 */
#ifndef COUNTR_HIP_TILES_H
#define COUNTR_HIP_TILES_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden: what this header declares is what it exports */

#define COUNTR_TILES_ABI_VERSION 1
#define COUNTR_TILES_SIZE 384       /* a tile is 384 x 384: the model's input */
#define COUNTR_TILES_MAX_STARTS 64  /* starts per axis of a blend, tiles of one gather */
#define COUNTR_TILES_MAX_RECTS 8
#define COUNTR_TILES_MAX_ZOOM 4
int countr_tiles_version(void);               /* COUNTR_TILES_ABI_VERSION */
const char* countr_tiles_last_error(void);    /* thread-local message of the last failing call of THIS library */

/* bytes of workspace countr_tile_blend needs for an [hk, wk] map (host only): 9 four-byte partials per workgroup, a workgroup being
 * 4 rows x 1024 columns */
int countr_tiles_workspace(int hk, int wk);

/*
 * countr_tile_gather: wins[j] = img[:, rows[j] : rows[j] + 384, cols[j] : cols[j] + 384] for j < nt <= COUNTR_TILES_MAX_STARTS, straight
 * into the forward's input batch wins [nt, 3, 384, 384] (fp32, contiguous).  img is fp32 planar [3, hk, wk]; img and wins are 16-byte
 * aligned, wk and every column start are multiples of 4: all accesses are 16 bytes.  rows / cols are HOST arrays read at call time.  A
 * tile outside the image is an error, not a launch.  One launch on `stream`.
 */
int countr_tile_gather(const float* img, int hk, int wk, const int* rows, const int* cols, int nt, float* wins, void* stream);

/*
 * countr_tile_blend: outs [nrows * ncols, 384, 384] (band-major, fp32, 16-byte aligned) -> dm [hk, wk] (16-byte aligned) by the rule
 * above, and sums [1 + nrects].  row_starts [nrows], col_starts [ncols] and rects [nrects * 4] are HOST arrays read at call time; the
 * starts must be a full cover as stated above, the column starts and wk multiples of 4.  nrects <= COUNTR_TILES_MAX_RECTS; a rectangle
 * with y2 < y1 or x2 < x1 is refused.  workspace: countr_tiles_workspace(hk, wk) bytes, 4-byte aligned.  Two launches on `stream`.
 */
int countr_tile_blend(const float* outs, int nrows, int ncols, const int* row_starts, const int* col_starts, int hk, int wk,
                      const int* rects, int nrects, float* dm, float* sums, void* workspace, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* COUNTR_HIP_TILES_H */
