/*
 * countr_hip_yuv.h -- C ABI of libcountr_hip_yuv.so: the 4:2:0 surfaces a video decoder writes (NV12, NV21, I420, P010), converted to the
 * packed 8-bit RGB [H, W, 3] every raw-frame entry point takes.  countr_hip.h, countr_hip_ext.h, countr_hip_classes.h and
 * countr_hip_tiles.h are closed; this header is the one statement of a library of its own, in the same dialect
 * (countr_amd/_lib.py::parse_header reads all five), with the same conventions: extern "C", plain pointers and sizes, 0 on success and
 * < 0 on error with the text in countr_yuv_last_error() (thread-local), no allocation and no synchronisation inside a call.  One build,
 * no fp16 twin: the conversion is integer arithmetic.  The library keeps no per-device state and needs no init call.
 *
 * THE RULE (countr_amd/yuv.py::yuv_host restates it in numpy).
 *   Formats.  All are 4:2:0: a frame of H rows and W columns has Hc = (H + 1) / 2 chroma rows of Wc = (W + 1) / 2 chroma samples.  Odd W
 *     and H are valid; the last chroma column or row then serves one luma column or row.
 *       NV12  8-bit Y [H, W]; c0 = one interleaved plane [Hc, 2 Wc] of (U, V) pairs
 *       NV21  as NV12 with the pairs in (V, U) order
 *       I420  8-bit Y; c0 = U [Hc, Wc], c1 = V [Hc, Wc] (YV12: the caller swaps the two planes)
 *       P010  as NV12 with 16-bit little-endian words; a sample is word >> 6 (10 bits)
 *     Every plane has a row pitch in bytes, at least the row's bytes: pitch_y for Y, pitch_c for the chroma plane(s).
 *   One pixel.  int32, arithmetic shift, clamp to 0 .. 255.  b = the sample bits (8 or 10), s = b - 8, C = cy (Y - (yoff << s)),
 *     D = U - (128 << s), E = V - (128 << s):
 *       R = clamp((C + rv E + (128 << s)) >> (8 + s))
 *       G = clamp((C + gu D + gv E + (128 << s)) >> (8 + s))
 *       B = clamp((C + bu D + (128 << s)) >> (8 + s))
 *                          cy  yoff   rv    gu    gv   bu
 *       BT601 full        256    0   359   -88  -183  454
 *       BT709 full        256    0   403   -48  -120  475
 *       BT601 limited     298   16   409  -100  -208  516
 *       BT709 limited     298   16   459   -55  -136  541
 *     (round(256 x the exact coefficient): every channel lies within 1 of the float matrix rounded half up.)  P010 is reduced to 8-bit
 *     RGB by this rule and nothing else: no tone mapping, no transfer function.
 *   Chroma.  NEAREST: luma (y, x) uses chroma (y >> 1, x >> 1).  LINEAR: the MPEG-2 / H.264 default siting -- a chroma sample is co-sited
 *     with the even luma column and lies midway between its two luma rows -- rounded once.  For luma row y: j = y >> 1,
 *     jn = min(j + 1, Hc - 1) if y is odd, else max(j - 1, 0), s[i] = 3 c[j][i] + c[jn][i].  For luma column x: i = x >> 1; the chroma is
 *     (s[i] + 2) >> 2 if x is even, (s[i] + s[min(i + 1, Wc - 1)] + 4) >> 3 if x is odd.  U and V separately, on 8- or 10-bit samples
 *     alike, then the pixel as above.
 */
#ifndef COUNTR_HIP_YUV_H
#define COUNTR_HIP_YUV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden: what this header declares is what it exports */

#define COUNTR_YUV_ABI_VERSION 1
#define COUNTR_YUV_MAX_FRAMES 16  /* frames of one countr_yuv_to_rgb call */
#define COUNTR_YUV_MAX_SIDE 16384 /* H and W are 1 .. this */
#define COUNTR_YUV_NV12 0
#define COUNTR_YUV_NV21 1
#define COUNTR_YUV_I420 2
#define COUNTR_YUV_P010 3
#define COUNTR_YUV_BT601 0
#define COUNTR_YUV_BT709 1
#define COUNTR_YUV_LIMITED 0
#define COUNTR_YUV_FULL 1
#define COUNTR_YUV_NEAREST 0
#define COUNTR_YUV_LINEAR 1
int countr_yuv_version(void);               /* COUNTR_YUV_ABI_VERSION */
const char* countr_yuv_last_error(void);    /* thread-local message of the last failing call of THIS library */

/*
 * countr_yuv_to_rgb: n (1 .. COUNTR_YUV_MAX_FRAMES) frames of ONE shape, one format and one pair of pitches -> rgb[j], a contiguous
 * uint8 [H, W, 3] on the device, by the rule above, in one launch on `stream`.  y, c0, c1 and rgb are HOST arrays of n device pointers,
 * read at call time; c1 is required for I420 and must be NULL otherwise.  pitch_y / pitch_c: bytes from one row of the Y plane / of a
 * chroma plane to the next.  P010 planes are 2-byte aligned and their pitches even.  16-byte loads when every plane is 16-byte aligned
 * and both pitches are multiples of 16; 16-byte stores when every rgb pointer is 16-byte aligned and W a multiple of 16, 4-byte stores
 * when they are 4-byte aligned and W a multiple of 4; element-wise otherwise.  The bytes written are the same.  A refused
 * call (a null pointer, n, H or W out of range, a pitch below the row's bytes, an unknown enum) launches nothing.
 */
int countr_yuv_to_rgb(const void* const* y, const void* const* c0, const void* const* c1, void* const* rgb, int n, int H, int W,
                      int pitch_y, int pitch_c, int format, int matrix, int range, int chroma, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* COUNTR_HIP_YUV_H */
