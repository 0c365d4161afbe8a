/*
 * countr_hip_cam.h -- C ABI of libcountr_hip_cam.so: the camera's own motion, estimated from the motion field the flow library computes,
 * and that field compensated for it -- on the device and on the caller's stream.  The eight older headers are closed; this header is the
 * one statement of a library of its own, in the same dialect (countr_amd/_lib.py::parse_header reads all nine), with the same
 * conventions: extern "C", plain pointers and sizes, 0 on success and < 0 on error with the text in countr_cam_last_error()
 * (thread-local), no allocation and no synchronisation inside a call.  One build, no fp16 twin.  The library keeps no state and needs no
 * init call.
 *
 * THE RULE (countr_amd/cam.py::camera_host restates it in numpy).  The camera's motion is the motion most of the textured background
 * agrees on.  The model is a translation in the image plane (a pan); rotation and zoom are not modelled.  All of it is integer arithmetic:
 * device bytes equal host bytes.
 *   Sizes.  A luma is uint8 [h, w] (countr_flow_luma's), a motion field int16 [h / 8, w / 8, 2] as (x, y) in 1/16 px
 *     (countr_flow_motion's: the backward offset of the current luma against an earlier one); h and w are multiples of COUNTR_CAM_CELL in
 *     COUNTR_CAM_CELL .. COUNTR_CAM_MAX_SIDE, as the flow library's.  A field handed in may hold ANY int16.
 *   Texture of cell (j, i) of the current luma L: over the cell's 64 pixels (y, x)
 *       T = sum of |L(y, min(x + 1, w - 1)) - L(y, x)| + |L(min(y + 1, h - 1), x) - L(y, x)|          (uint32; at most 64 * 2 * 255)
 *     The cell's flag is 1 iff T >= min_texture.  A flat cell is "at rest" by the flow rule's min_gain test whatever the camera does:
 *     it must not drag the estimate to zero, so it does not vote.
 *   Votes.  A cell votes iff its flag is 1 and both components of its offset (ox, oy) lie in [-R, R], R = COUNTR_CAM_RANGE =
 *     16 * COUNTR_FLOW_MAX_SEARCH + 8 = 264: what countr_flow_motion can write.  An offset outside never indexes a histogram.
 *   Estimate.  n = the number of voters.  Per axis, g = the lower median of the voters' offsets: the element of rank ceil(n / 2) in
 *     ascending order (0 when n = 0).  inliers = the number of voters with |ox - gx| <= tol and |oy - gy| <= tol, against that median.
 *     The estimate is valid iff n >= min_voters and 2 * inliers >= n; otherwise g = (0, 0) is written.
 *     The record is int32 [COUNTR_CAM_RECORD_INTS]: gx, gy, voters, inliers, valid, cells (= h / 8 * w / 8), 0, 0.
 *     With the flow library's sign, g = 16 * (cam_t - cam_earlier) when image pixel p shows scene point p + cam_t.
 *   Compensate.  V'(cell) = (0, 0) if V(cell) == (0, 0) and the cell's flag is 0: a flat, resting cell is taken to move with the scene.
 *     Otherwise V' = V - g per component, saturated to int16: a textured cell that rests in the image does move against the scene.
 *
 * The defaults the Python side passes (min_texture = 128, tol = 8, min_voters = 16) are unmeasured on real video.
 */
#ifndef COUNTR_HIP_CAM_H
#define COUNTR_HIP_CAM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden: what this header declares is what it exports */

#define COUNTR_CAM_ABI_VERSION 1
#define COUNTR_CAM_MAX_FRAMES 16      /* (field, luma) pairs of one call */
#define COUNTR_CAM_CELL 8             /* a motion cell is 8 x 8 pixels: COUNTR_FLOW_CELL */
#define COUNTR_CAM_MAX_SIDE 4096      /* h and w of a call: COUNTR_FLOW_MAX_SIDE */
#define COUNTR_CAM_RANGE 264          /* R: a voter's offset lies in [-R, R] per axis */
#define COUNTR_CAM_BINS 529           /* 2 R + 1 bins of an axis' histogram */
#define COUNTR_CAM_RECORD_INTS 8      /* gx, gy, voters, inliers, valid, cells, 0, 0 */
int countr_cam_version(void);                /* COUNTR_CAM_ABI_VERSION */
const char* countr_cam_last_error(void);     /* thread-local message of the last failing call of THIS library */

/* bytes of scratch a countr_cam_estimate call of n fields of h x w pixels needs (< 0: bad arguments): two histograms per field */
int countr_cam_workspace(int n, int h, int w);

/*
 * countr_cam_estimate: n (1 .. COUNTR_CAM_MAX_FRAMES) pairs (motion field, current luma) -> n records and the cells' flags, by the rule
 * above.  fields and lumas are HOST arrays of device pointers, read at call time (a field 4-byte aligned).  records is ONE device buffer
 * int32 [n, 8], flags ONE device buffer uint8 [n, h / 8 * w / 8], both 4-byte aligned.  min_texture >= 0, tol >= 0, min_voters >= 1.
 * workspace: 4-byte aligned device scratch of countr_cam_workspace(n, h, w) bytes; the call clears it on the stream first.  Two launches:
 * a block per cell row of a field forms the textures, writes the flags and adds the voters into the block's two histograms in LDS, then
 * into the field's with integer atomics (integer sums do not depend on the order: two runs give the same bytes); a block per field then
 * scans the histograms for the two medians, counts the inliers and writes the record.
 */
int countr_cam_estimate(const void* const* fields, const void* const* lumas, void* records, void* flags, int n, int h, int w,
                        int min_texture, int tol, int min_voters, void* workspace, void* stream);

/*
 * countr_cam_compensate: n fields, the records and flags of countr_cam_estimate over the same n -> n compensated fields, one launch.  g
 * is read from the device record, so no wait lies between the two calls.  fields and out_fields are HOST arrays of device pointers
 * (4-byte aligned); out_fields[k] may equal fields[k], and overlaps nothing else.
 *
 * A refused call (a count, a size or a setting out of range, a null or misaligned pointer) launches nothing.
 */
int countr_cam_compensate(const void* const* fields, const void* records, const void* flags, void* const* out_fields, int n, int h, int w,
                          void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* COUNTR_HIP_CAM_H */
