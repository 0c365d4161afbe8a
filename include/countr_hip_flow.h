/*
 * countr_hip_flow.h -- C ABI of libcountr_hip_flow.so: line counts from density flux -- the luma of prepared images, a block-matching
 * motion field between two lumas, and the flux of a density map through counting lines -- on the device and on the caller's stream.  The
 * seven older headers are closed; this header is the one statement of a library of its own, in the same dialect
 * (countr_amd/_lib.py::parse_header reads all eight), with the same conventions: extern "C", plain pointers and sizes, 0 on success and
 * < 0 on error with the text in countr_flow_last_error() (thread-local), no allocation and no synchronisation inside a call.  One build, no
 * fp16 twin.  The library keeps no state and needs no init call.
 *
 * THE RULE (countr_amd/flow.py::flow_host restates it in numpy).  A density map is a mass that moves with the picture; the number of
 * objects that cross a line is the flux of that mass through the line.  No peaks, no association, no track limit.
 *   Sizes.  An image is fp32 [3, h, w] (planes R, G, B; the prepared image the forward reads), its luma uint8 [h, w], its density map fp32
 *     [h, w], its motion field int16 [h / 8, w / 8, 2]; h and w are multiples of COUNTR_FLOW_CELL in COUNTR_FLOW_CELL ..
 *     COUNTR_FLOW_MAX_SIDE (the forward's are h = 384 and w a multiple of 16, so luma and map are pixel-aligned).
 *   Luma.  q_c = (int)(fl(v_c * 255) + 0.5f) in fp32, clamped to 0 .. 255 (this recovers the resized byte of a prepared image exactly;
 *     v_c is finite), L = (77 q_R + 150 q_G + 29 q_B + 128) >> 8.
 *   Motion, of the current luma C against an earlier luma E: a backward offset per 8 x 8 cell.  The window of cell (j, i) is the 16 x 16
 *     pixels with origin (8 j - 4, 8 i - 4).  For o = (oy, ox) in [-r, r]^2 (r = search, 1 .. COUNTR_FLOW_MAX_SEARCH)
 *       S(o) = sum over the window's pixels p of |C(clamp(p)) - E(clamp(p + o))|        (uint32; clamp: each coordinate to the image)
 *     best = the first minimum of S in (oy^2 + ox^2, oy, ox) order.  If best != 0 and S(0) - S(best) < min_gain, the cell is at rest:
 *     its offset is (0, 0) and nothing below applies.  Otherwise, per axis, when both neighbours of best on that axis lie inside the search
 *     square, with S-, S0, S+ along that axis and den = max(S-, S+) - S0:
 *       f = den > 0 ? floor((16 (S- - S+) + den) / (2 den)) : 0       (the equiangular fit for SAD, rounded to 1/16 px; -8 <= f <= 8
 *                                                                      because S0 is the smallest of the three)
 *     and f = 0 otherwise.  The cell's offset is 16 best + f per axis, stored as the int16 pair (x, y).  All of it is integer arithmetic.
 *   Flux of map M with motion field V through line k = (ax, ay, bx, by), in pixel-centre coordinates of the original frame.  Everything
 *     up to g is fp64, one rounding per written operation, nothing contracted:
 *       a map pixel (cy, cx) lies at P = (sx * cx + tx, sy * cy + ty)                     (sx, sy > 0: the map's placement)
 *       e = b - a; len2 = ex * ex + ey * ey; len = sqrt(len2); a line with len2 == 0 counts nothing
 *       ux = Px - ax; uy = Py - ay; cr = ex * uy - ey * ux; t = ex * ux + ey * uy; hw = (band / 2) * len
 *       the pixel is in the band iff -hw <= cr && cr < hw && 0 <= t && t < len2           (both intervals half-open)
 *       the cell's offset (ox, oy) gives the object's move per frame: dx = -((sx * ox) / (16 * interval)), dy likewise with sy, oy
 *       vn = ((dy * ex) - (dx * ey)) / len                                                (towards side 1 of the tracker's side test)
 *       g = (vn / band) / 60
 *     A pixel in the band with vn > 0 adds the fp32 term fl32((double)M * g) to forward; with vn < 0 it adds fl32((double)M * -g) to
 *     backward.  The sums are fp32 in a fixed order: a block of 256 threads takes the 8 map rows of one cell row; wave v of its 4 takes
 *     the 64-column chunks v, v + 4, ...; a lane adds its pixels chunk by chunk and, inside a chunk, row by row; the lanes of a wave are
 *     added by one butterfly (lane ^ 1, ^ 2, half-row mirror, row mirror, ^ 16, ^ 32), the four waves in wave order, and the cell rows in
 *     ascending order.  total, the sum of all of M, is formed in the same order.  No floating-point atomics: two runs give the same bytes.
 */
#ifndef COUNTR_HIP_FLOW_H
#define COUNTR_HIP_FLOW_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden: what this header declares is what it exports */

#define COUNTR_FLOW_ABI_VERSION 1
#define COUNTR_FLOW_MAX_FRAMES 16     /* images, luma pairs or maps of one call */
#define COUNTR_FLOW_MAX_LINES 16      /* counting lines of a call */
#define COUNTR_FLOW_MAX_SEARCH 16     /* the search radius r, in pixels */
#define COUNTR_FLOW_MAX_INTERVAL 8    /* frames between the two lumas of a pair */
#define COUNTR_FLOW_CELL 8            /* a motion cell is 8 x 8 pixels, its window 16 x 16 */
#define COUNTR_FLOW_MAX_SIDE 4096     /* h and w of a call */
#define COUNTR_FLOW_OUT_FLOATS 33     /* a map's results: flux[16][2] as (forward, backward), then total */
int countr_flow_version(void);               /* COUNTR_FLOW_ABI_VERSION */
const char* countr_flow_last_error(void);    /* thread-local message of the last failing call of THIS library */

/* bytes of scratch a countr_flow_flux call of n maps of height h needs (< 0: bad arguments) */
int countr_flow_workspace(int n, int h);

/*
 * countr_flow_luma: n (1 .. COUNTR_FLOW_MAX_FRAMES) images fp32 [3, h, w] -> n lumas uint8 [h, w], one launch.  images and lumas are HOST
 * arrays of device pointers (16-byte and 4-byte aligned), read at call time.
 */
int countr_flow_luma(const void* const* images, void* const* lumas, int n, int h, int w, void* stream);

/*
 * countr_flow_motion: n (1 .. COUNTR_FLOW_MAX_FRAMES) pairs (current luma, earlier luma), uint8 [h, w] each -> n motion fields int16
 * [h / 8, w / 8, 2], one launch: a wave per cell stages the window and its (16 + 2 r)^2 search area in LDS as bytes, a lane takes a
 * candidate and compares four bytes at a time (v_sad_u8), a fixed-order minimum over the wave picks the rule's first minimum.  current,
 * earlier and motion are HOST arrays of device pointers (motion 4-byte aligned).  search in 1 .. COUNTR_FLOW_MAX_SEARCH, min_gain >= 0.
 */
int countr_flow_motion(const void* const* current, const void* const* earlier, void* const* motion, int n, int h, int w, int search,
                       int min_gain, void* stream);

/* One map of a flux call.  map (fp32 [h, w]), motion (int16 [h / 8, w / 8, 2]) and out (fp32 [COUNTR_FLOW_OUT_FLOATS]) are device
 * pointers, 4-byte aligned; sx, tx, sy, ty is the map's placement, finite with sx > 0 and sy > 0. */
typedef struct countr_flow_map {
  const void* map;
  const void* motion;
  void* out;
  double sx, tx, sy, ty;
} countr_flow_map;

/*
 * countr_flow_flux: the flux of n (1 .. COUNTR_FLOW_MAX_FRAMES) maps through L (0 .. COUNTR_FLOW_MAX_LINES) lines, and every map's total,
 * by the rule above; two launches (a block per cell row of a map, then the fold of the cell rows).  maps and lines are HOST arrays read at
 * call time: lines is fp64 [L, 4] as (ax, ay, bx, by), finite (NULL when L = 0); lines and placements travel as kernel arguments, so a
 * call uploads nothing.  band is finite and > 0 (frame pixels), interval in 1 .. COUNTR_FLOW_MAX_INTERVAL.  out[2 k], out[2 k + 1] =
 * forward, backward of line k (0 for k >= L), out[32] = total.  workspace: 4-byte aligned device scratch of countr_flow_workspace(n, h)
 * bytes.
 *
 * A refused call (a count, a size or a setting out of range, a null or misaligned pointer, a value that is not finite) launches nothing.
 */
int countr_flow_flux(const countr_flow_map* maps, int n, int h, int w, const double* lines, int L, double band, int interval,
                     void* workspace, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* COUNTR_HIP_FLOW_H */
