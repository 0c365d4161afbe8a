/*
 * countr_hip_overlay.h -- C ABI of libcountr_hip_overlay.so: an annotated frame composed on the device at the frame's own resolution
 * from the frame's own pixels -- the density map as a colour overlay, points, region outlines and a label -- as packed RGB [H, W, 3] or
 * as the 4:2:0 buffer (NV12 / NV21 / I420) a video encoder takes.  The five older headers are closed; this header is the one statement
 * of a library of its own, in the same dialect (countr_amd/_lib.py::parse_header reads all six), with the same conventions: extern "C",
 * plain pointers and sizes, 0 on success and < 0 on error with the text in countr_overlay_last_error() (thread-local), no allocation and
 * no synchronisation inside a call.  One build, no fp16 twin.  The library keeps no per-device state and needs no init call.
 *
 * THE RULE (countr_amd/overlay.py::overlay_host restates it in numpy).  Everything after step 1 is integer arithmetic.
 *   Inputs per frame: the RGB frame uint8 [H, W, 3], a density map fp32 [mh, mw] of any size, an fp32 gain, a colour table
 *     lut uint8 [256, 4] of (r, g, b, a), and optionally the marks of step 4.
 *   1 Heat.  For a map pixel m: q = clamp(floor(fl(fl(m * gain) + 0.5f)), 0, 255) -- one fp32 multiply and one fp32 add, not contracted
 *     into an fma; NaN gives 0.  Under gain_max the gain is 255.0f / max(map) -- one fp32 division of the exact maximum of the map's
 *     values above 0 -- and 0 where no value is above 0.  The maximum is found on the device.
 *   2 Upsampling to the frame: bilinear with align_corners = False, 8-bit weights, in integers.  For output row y:
 *     ny = (2 y + 1) mh - H; if ny < 0: iy = 0, fy = 0; else iy = ny / (2 H), fy = ((ny % (2 H)) * 256) / (2 H);
 *     iy1 = min(iy + 1, mh - 1), iy = min(iy, mh - 1).  Columns likewise with mw and W.
 *     h = ((q00 (256 - fx) + q01 fx) (256 - fy) + (q10 (256 - fx) + q11 fx) fy + 32768) >> 16.
 *   3 Blend.  (r, g, b, a) = lut[h]; each channel out = (frame * (255 - a) + colour * a + 127) / 255, exact integer division
 *     (v / 255 = (v * 0x8081) >> 23 for 0 <= v < 65536).  An all-zero alpha column returns the frame.
 *   4 Marks, drawn onto the blended RGB in this order: label, region outlines, points.  A later kind overwrites an earlier one; within
 *     a kind every write carries the same bytes, so overlap is order-free.
 *       Label.  One coverage patch uint8 [lh, lw] at (lx, ly), blended towards white: p = (p * (255 - m) + 255 m + 127) / 255, clipped
 *         to the frame.
 *       Region outlines.  int32 vertices.  For an edge (x0, y0) -> (x1, y1): dx = x1 - x0, dy = y1 - y0, n = max(|dx|, |dy|); pixel i
 *         in 0 .. n is (x0 + rdiv(i dx, n), y0 + rdiv(i dy, n)), rdiv(a, n) = floor((2 a + n) / (2 n)) in int64; n = 0 is one pixel.
 *         A polygon of V vertices has the V edges (v[k], v[(k + 1) % V]).  One colour a call; pixels outside the frame are skipped.
 *       Points.  int32 centres; a point is the disc of the pixels with dx^2 + dy^2 <= r^2, r in 0 .. 16, one colour a call, clipped.
 *     (The host rounds float coordinates to int32 as floor(v + 0.5) before the call.)
 *   5 Optional 4:2:0 output: one contiguous buffer per frame, Y [H, W] then the chroma plane(s), no padding, Hc = (H + 1) / 2,
 *     Wc = (W + 1) / 2: NV12 one plane [Hc, 2 Wc] of (U, V) pairs, NV21 of (V, U) pairs, I420 U [Hc, Wc] then V [Hc, Wc].
 *       Y = ((yr R + yg G + yb B + 128) >> 8) + yoff.
 *       A chroma sample: R, G, B each the sum over the block's 2 x 2 pixels, coordinates clamped to the frame (odd sizes replicate the
 *       edge), then (s + 2) >> 2;  U = clamp(((ur R + ug G + ub B + 128) >> 8) + 128, 0, 255), V likewise; arithmetic shift.
 *                           yr   yg  yb  yoff    ur   ug   ub     vr    vg   vb
 *       BT601 full          77  150  29    0    -43  -85  128    128  -107  -21
 *       BT601 limited       66  129  25   16    -38  -74  112    112   -94  -18
 *       BT709 full          54  184  18    0    -29  -99  128    128  -116  -12
 *       BT709 limited       47  157  16   16    -26  -86  112    112  -102  -10
 *     (a red or blue coefficient is floor(256 x the exact coefficient + 0.5); green takes what is left of the row's total: 256 for
 *     full-range luma, 220 for limited-range luma, 0 for the chroma rows.)
 *
 * THE PACKED UPLOAD.  One device buffer per call, copied from the host by the caller before the call on the same stream:
 *     bytes 0 .. 63       float gain[16], one per frame (ignored for a frame with gain_max)
 *     bytes 64 .. 1087    the colour table, uint8 [256, 4]
 *     from byte 1088      what the frames' offsets name: int32 (x, y) per point, int32 (x0, y0, x1, y1) per edge, the patch bytes.
 *   Offsets are in bytes from the start of the buffer; those of points and edges are multiples of 4.
 */
#ifndef COUNTR_HIP_OVERLAY_H
#define COUNTR_HIP_OVERLAY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden: what this header declares is what it exports */

#define COUNTR_OVERLAY_ABI_VERSION 1
#define COUNTR_OVERLAY_MAX_FRAMES 16    /* frames of one countr_overlay_render call */
#define COUNTR_OVERLAY_MAX_SIDE 16384   /* H, W, mh and mw are 1 .. this */
#define COUNTR_OVERLAY_MAX_POINTS 4096  /* points of a frame */
#define COUNTR_OVERLAY_MAX_POLYGONS 64  /* polygons of a frame */
#define COUNTR_OVERLAY_MAX_VERTICES 64  /* vertices of a polygon */
#define COUNTR_OVERLAY_MAX_RADIUS 16    /* point_radius is 0 .. this */
#define COUNTR_OVERLAY_PATCH_H 64       /* a label patch is at most this high */
#define COUNTR_OVERLAY_PATCH_W 256      /* and this wide */
#define COUNTR_OVERLAY_PACK_GAINS 0     /* byte offsets of the packed upload's fixed part */
#define COUNTR_OVERLAY_PACK_LUT 64
#define COUNTR_OVERLAY_PACK_HEAD 1088
#define COUNTR_OVERLAY_RGB 0
#define COUNTR_OVERLAY_NV12 1
#define COUNTR_OVERLAY_NV21 2
#define COUNTR_OVERLAY_I420 3
#define COUNTR_OVERLAY_BT601 0
#define COUNTR_OVERLAY_BT709 1
#define COUNTR_OVERLAY_LIMITED 0
#define COUNTR_OVERLAY_FULL 1
int countr_overlay_version(void);               /* COUNTR_OVERLAY_ABI_VERSION */
const char* countr_overlay_last_error(void);    /* thread-local message of the last failing call of THIS library */

/* One frame of a call.  rgb, map and out are device pointers: rgb the frame uint8 [H, W, 3] (read only), map fp32 [mh, mw], out the
 * composed RGB uint8 [H, W, 3], a buffer of its own (not rgb).  A mark's coordinates lie in -2^20 .. 2^20.  yuv is the
 * packed 4:2:0 buffer of step 5, required when the call's format is not COUNTR_OVERLAY_RGB and NULL otherwise.  poly_verts is a HOST
 * array of n_polys vertex counts, read at call time for the limits; the edges themselves are n_edges (the sum of the counts) records in
 * the packed upload.  lh = lw = 0: no label. */
typedef struct countr_overlay_frame {
  const void* rgb;
  const void* map;
  void* out;
  void* yuv;
  const void* poly_verts;
  int gain_max;
  int n_points, points_off;
  int n_polys, n_edges, edges_off;
  int lh, lw, lx, ly, patch_off;
} countr_overlay_frame;

/*
 * countr_overlay_render: n (1 .. COUNTR_OVERLAY_MAX_FRAMES) frames of ONE frame shape and ONE map shape, by the rule above, on `stream`:
 * the per-map maximum (only when a frame has gain_max; `maxbits`, n device uint32, is then required and is zeroed by the call), the
 * composition (steps 1 to 3), one launch per kind of mark present (label, edges, points), and the RGB -> 4:2:0 conversion when format
 * is not COUNTR_OVERLAY_RGB.  pack: the packed upload on the device, pack_bytes long; every offset of every frame must lie inside it.
 * point_rgb / edge_rgb: 0xRRGGBB.  16-byte loads and stores when every rgb / out (/ yuv) pointer is 16-byte aligned and W is a multiple
 * of 16, element-wise otherwise; the bytes written are the same.  A refused call (n, H, W, mh or mw out of range, an unknown format,
 * matrix or range, more points, polygons or vertices than the limits, a patch above 64 x 256, a radius out of range, an offset outside
 * the pack, a null pointer) launches nothing.
 */
int countr_overlay_render(const countr_overlay_frame* frames, int n, int H, int W, int mh, int mw, const void* pack, int pack_bytes,
                          int point_radius, int point_rgb, int edge_rgb, int format, int matrix, int range, void* maxbits, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* COUNTR_HIP_OVERLAY_H */
