/*
 * countr_hip_draw.h -- C ABI of libcountr_hip_draw.so: marks drawn in place onto packed RGB frames on the device -- thick segments, discs
 * and text, each mark in a colour of its own -- and, behind the marks, the 4:2:0 buffer (NV12 / NV21 / I420) a video encoder takes.  What
 * a tracked clip shows: every object's id and trail, every counting line's tally.  The table of the eight side libraries is closed; this
 * header is the one statement of the first library of the later table, in the same dialect (countr_amd/_lib.py::parse_header reads it),
 * with the same conventions: extern "C", plain pointers and sizes, 0 on success and < 0 on error with the text in
 * countr_draw_last_error() (thread-local), no allocation and no synchronisation inside a call.  One build, no fp16 twin.  The library
 * keeps no per-device state and needs no init call.
 *
 * THE RULE (countr_amd/draw.py::draw_host restates it in numpy).  Integers only.  A frame is uint8 [H, W, 3]; coordinates are int32 in
 * -2^20 .. 2^20, x to the right and y down, and name pixels; a colour is 0xRRGGBB.  A mark COVERS a set of pixels; pixels outside the
 * frame are skipped.
 *   Segment (x0, y0, x1, y1, half-width w in 0 .. 8, colour).  Its centres are the pixels of the edge rule of countr_hip_overlay.h:
 *     dx = x1 - x0, dy = y1 - y0, n = max(|dx|, |dy|); centre i in 0 .. n is (x0 + rdiv(i dx, n), y0 + rdiv(i dy, n)),
 *     rdiv(a, n) = floor((2 a + n) / (2 n)) in int64; n = 0 is one centre.  The segment covers, around every centre (cx, cy), the
 *     pixels (cx + u, cy + v) with u^2 + v^2 <= w^2.
 *   Disc (cx, cy, r in 0 .. 16, colour): the pixels (cx + u, cy + v) with u^2 + v^2 <= r^2, the point rule of countr_hip_overlay.h.
 *   Text (x, y, scale s in 1 .. 8, foreground, background or none, len <= 32 bytes).  Character k owns the cell
 *     [x + 6 s k, x + 6 s (k + 1)) x [y, y + 8 s).  Its glyph is 5 columns x 7 rows in the cell's top-left: pixel (x + 6 s k + u,
 *     y + v) of the cell belongs to glyph column u / s and row v / s, and is FOREGROUND when that column is below 5, that row below 7
 *     and the font has the bit set; every other pixel of the cell is BACKGROUND.  A byte outside 32 .. 126 is drawn as '?'.  The text
 *     covers its foreground pixels and, when it has a background colour, its background pixels too.
 *   The font is the table uint8 [95][7] of csrc_draw/draw.hip, drawn by hand: row r of glyph g (the character 32 + g) is font[g][r],
 *     column c is bit 4 - c.  countr_draw_font copies it out, so that the host restatement reads the one statement of it.
 *   Overlap.  Everything is opaque.  Every mark of a frame has a key: segments in the order of the call, then discs in the order of the
 *     call, then texts in the order of the call.  A pixel takes the colour the covering mark with the GREATEST key gives it, and keeps
 *     its own when no mark covers it.  (A text's background lies directly under its own foreground, so a later text covers an earlier
 *     one whole.)  Painting the marks one after another in key order gives the same frame.
 *   4:2:0 output behind the marks: step 5 of countr_hip_overlay.h, unchanged -- one contiguous buffer per frame, Y [H, W] then the
 *     chroma plane(s) of Hc = (H + 1) / 2 rows, in the layouts, coefficients and roundings stated there.
 *
 * THE DEVICE FORM.  Per frame an owner plane uint32 [H, W] that is all zero between calls.  A claim launch: every mark does an integer
 * atomicMax of 1 + its key over the pixels it covers.  A paint launch: every mark walks the same pixels, and where the owner equals
 * 1 + its key writes its colour and stores 0.  The maximum does not depend on the order, so two runs give the same bytes, and the plane
 * is clean again without a pass over the frame.
 *
 * THE PACKED UPLOAD.  One buffer per call, built on the host and copied to the device by the caller before the call on the same stream;
 * the call reads the HOST copy for its checks and the kernels read the device copy.  Every record is int32 words:
 *     segment   6 words   x0, y0, x1, y1, w, colour
 *     disc      4 words   cx, cy, r, colour
 *     text     14 words   x, y, s, foreground, background (-1: none), len, then the 32 bytes of the text (those behind len are ignored)
 *   A frame names its records by a byte offset from the start of the buffer, a multiple of 4, and a count.
 */
#ifndef COUNTR_HIP_DRAW_H
#define COUNTR_HIP_DRAW_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden: what this header declares is what it exports */

#define COUNTR_DRAW_ABI_VERSION 1
#define COUNTR_DRAW_MAX_FRAMES 16        /* frames of one countr_draw_paint call */
#define COUNTR_DRAW_MAX_SIDE 16384       /* H and W are 1 .. this */
#define COUNTR_DRAW_MAX_SEGMENTS 65600   /* segments of a frame: 4096 trails of 16 steps, and 64 more */
#define COUNTR_DRAW_MAX_DISCS 4096       /* discs of a frame */
#define COUNTR_DRAW_MAX_TEXTS 4160       /* texts of a frame: 4096 tags, and 64 more */
#define COUNTR_DRAW_MAX_HALF_WIDTH 8     /* a segment's w is 0 .. this */
#define COUNTR_DRAW_MAX_RADIUS 16        /* a disc's r is 0 .. this */
#define COUNTR_DRAW_MAX_SCALE 8          /* a text's s is 1 .. this */
#define COUNTR_DRAW_TEXT_BYTES 32        /* a text's len is 0 .. this */
#define COUNTR_DRAW_MAX_COORD 1048576    /* coordinates are -this .. this */
#define COUNTR_DRAW_SEGMENT_WORDS 6      /* int32 words of a record */
#define COUNTR_DRAW_DISC_WORDS 4
#define COUNTR_DRAW_TEXT_WORDS 14
#define COUNTR_DRAW_FONT_FIRST 32        /* the font's first character */
#define COUNTR_DRAW_FONT_GLYPHS 95       /* 32 .. 126 */
#define COUNTR_DRAW_FONT_ROWS 7
#define COUNTR_DRAW_FONT_COLS 5
#define COUNTR_DRAW_RGB 0
#define COUNTR_DRAW_NV12 1
#define COUNTR_DRAW_NV21 2
#define COUNTR_DRAW_I420 3
#define COUNTR_DRAW_BT601 0
#define COUNTR_DRAW_BT709 1
#define COUNTR_DRAW_LIMITED 0
#define COUNTR_DRAW_FULL 1
int countr_draw_version(void);               /* COUNTR_DRAW_ABI_VERSION */
const char* countr_draw_last_error(void);    /* thread-local message of the last failing call of THIS library */

/* The font: out receives COUNTR_DRAW_FONT_GLYPHS x COUNTR_DRAW_FONT_ROWS bytes on the HOST.  Needs no device. */
int countr_draw_font(void* out);

/* One frame of a call.  rgb, owner and yuv are device pointers: rgb the frame uint8 [H, W, 3], drawn in place; owner its plane
 * uint32 [H, W], 4-byte aligned, all zero before the call and all zero after it; yuv the packed 4:2:0 buffer, required when the call's
 * format is not COUNTR_DRAW_RGB and NULL otherwise.  No two frames of a call share a buffer. */
typedef struct countr_draw_frame {
  void* rgb;
  void* owner;
  void* yuv;
  int n_segments, segments_off;
  int n_discs, discs_off;
  int n_texts, texts_off;
} countr_draw_frame;

/*
 * countr_draw_paint: n (1 .. COUNTR_DRAW_MAX_FRAMES) frames of ONE shape, by the rule above, on `stream`: the claim launch and the paint
 * launch (neither when no frame of the call has a mark), each with a wave per segment, a wave per disc and a block per text, and the
 * RGB -> 4:2:0 conversion when format is not COUNTR_DRAW_RGB.  host_pack: the packed upload on the HOST, read during the call; pack:
 * its copy on the device, 16-byte aligned; both pack_bytes long.  The conversion uses 16-byte loads and stores when every rgb and yuv
 * pointer is 16-byte aligned and W is a multiple of 16, and is element-wise otherwise; the bytes written are the same.  A refused call
 * (n, H or W out of range, an unknown format, matrix or range, more marks than the limits, a half-width, radius, scale, length,
 * colour or coordinate out of range, an offset outside the pack or not a multiple of 4, a null pointer) launches nothing.
 */
int countr_draw_paint(const countr_draw_frame* frames, int n, int H, int W, const void* host_pack, const void* pack, int pack_bytes,
                      int format, int matrix, int range, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* COUNTR_HIP_DRAW_H */
