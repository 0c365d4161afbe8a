/*
 * countr_hip_classes.h -- C ABI of libcountr_hip_classes.so: the fold of several class density maps of a frame into one label map.
 * countr_hip.h and countr_hip_ext.h are closed; this header is the one statement of a library of its own, in the same dialect
 * (countr_amd/_lib.py::parse_header reads all three), with the same conventions: extern "C", plain pointers and sizes, 0 / a size on
 * success and < 0 on error with the text in countr_classes_last_error() (thread-local), no allocation and no synchronisation inside a
 * call.  One build, no fp16 twin: nothing here has a 16-bit operand.  The library keeps no per-device state and needs no init call.
 */
#ifndef COUNTR_HIP_CLASSES_H
#define COUNTR_HIP_CLASSES_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden: what this header declares is what it exports */

#define COUNTR_CLASSES_ABI_VERSION 1
int countr_classes_version(void);               /* COUNTR_CLASSES_ABI_VERSION */
const char* countr_classes_last_error(void);    /* thread-local message of the last failing call of THIS library */

/*
 * countr_class_fold: "which class owns this pixel, and how much of each class's count lies on pixels it owns".
 *
 * A SET is one frame: nc class maps, each fp32 [h, w] and contiguous, and one fp32 scale per class.  With
 *     v_c(p) = scale[c] * map_c[p]                  one fp32 multiply, never contracted into the compare or the sums,
 *   label(p) = the smallest c that attains max_c v_c(p); 255 when that maximum is <= floor          (uint8 [h, w])
 *   won[c]   = the fp32 sum of v_c(p) over the pixels with label(p) == c
 *   total[c] = the fp32 sum of v_c(p) over all pixels
 *   area[c]  = the int32 number of pixels with label(p) == c.
 * Inputs are finite; negative values are compared and summed as they are.  Set s's results are won / total / area
 * [s * COUNTR_CLASSES_MAX + c]; the slots c >= nc are written as zeros.
 *
 * No floating-point atomics: a workgroup owns a strip of rows of one set and writes one partial per class; a second launch folds the
 * partials of a set in strip order.  Two runs give the same bytes.  Two launches on `stream` for up to COUNTR_CLASSES_MAX_SETS sets.
 *
 * sets is a HOST array read at call time (validated: a malformed set is refused, not computed); sets_dev is the DEVICE copy of the same
 * nsets structs (8-byte aligned), uploaded by the caller on `stream` -- the one packed upload of a call; the kernel reads the map
 * pointers, the scales and the label pointers there.  won, total [nsets * 16], area [nsets * 16] and the workspace (4-byte aligned,
 * countr_classes_workspace bytes) are device buffers.  Limits: 1 .. COUNTR_CLASSES_MAX classes a set, 1 .. COUNTR_CLASSES_MAX_SETS sets a
 * call, a map of at most 2^28 pixels.
 */
#define COUNTR_CLASSES_MAX_SETS 16
#define COUNTR_CLASSES_MAX 16
typedef struct countr_class_set {
  const float* map[16]; /* device, fp32 [h, w], contiguous; map[0 .. nc - 1] */
  void* labels;         /* device, uint8 [h, w] */
  float scale[16];
  int nc;               /* 1 .. 16 */
  int h, w;
} countr_class_set;
/* bytes of workspace of a call with these sets (host only; reads nc, h, w) */
int countr_classes_workspace(const countr_class_set* sets, int nsets);
int countr_class_fold(const countr_class_set* sets, int nsets, const void* sets_dev, float floor, float* won, float* total, int* area,
                      void* workspace, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* COUNTR_HIP_CLASSES_H */
