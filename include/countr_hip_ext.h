/*
 * countr_hip_ext.h -- C ABI of libcountr_hip_ext.so: exports that came after the ABI of countr_hip.h was closed.  The main header stays
 * the one statement of libcountr_hip.so / libcountr_hip_f16.so; this one is the one statement of the extension library, in the same
 * dialect (countr_amd/_lib.py::parse_header reads both), with the same conventions: extern "C", plain pointers and sizes, 0 / a size on
 * success and < 0 on error with the text in countr_ext_last_error() (thread-local), no allocation and no synchronisation inside a call.
 * One build, no fp16 twin: nothing here has a 16-bit operand.  The library keeps no per-device state and needs no init call.
 */
#ifndef COUNTR_HIP_EXT_H
#define COUNTR_HIP_EXT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden: what this header declares is what it exports */

#define COUNTR_EXT_ABI_VERSION 1
int countr_ext_version(void);               /* COUNTR_EXT_ABI_VERSION */
const char* countr_ext_last_error(void);    /* thread-local message of the last failing call of THIS library */

/*
 * countr_region_sums: sums of density maps over regions -- "how many in this part of the frame", and the per-cell counts of GAME.
 *
 * Coordinates are pixel-centre coordinates of the original frame (pixel i has centre i; a W x H frame covers [-0.5, W - 0.5) x
 * [-0.5, H - 0.5)), the ones countr_amd.frames.frame_points produces.  Map i carries an affine placement (ax, bx, ay, by) in fp64 at
 * data[place .. place + 3], ax > 0 and ay > 0: the centre of its pixel (cy, cx) lies at
 *     x = ax * cx + bx,   y = ay * cy + by          one fp64 multiply and one fp64 add per axis, never contracted.
 * Each map names the SET it adds to (a set is one frame: the nine crop maps of a 3 x 3 split share one set).  A set owns regions:
 *   polygon  nv vertices (x, y) at data[data .. data + 2 nv - 1], 3 <= nv <= COUNTR_REGIONS_MAX_VERTICES.  A centre is inside iff the
 *            number of edges (x0, y0) -> (x1, y1), the closing edge included, with
 *                (y0 <= y) != (y1 <= y)   and   x < x0 + (y - y0) * (x1 - x0) / (y1 - y0)
 *            is odd, in fp64, in exactly that operation order (subtract, subtract, multiply, subtract, divide, add), no contraction.
 *            Polygons that share an edge therefore share no pixel and leave none out.  Polygons may overlap, hang over the frame or
 *            miss it (mass 0, area 0).
 *   grid     nv = 0: boundaries ys[0 .. gy] at data[data ..] and xs[0 .. gx] behind them, strictly increasing, gy * gx <=
 *            COUNTR_REGIONS_MAX_CELLS.  A centre belongs to cell (i, j) iff ys[i] <= y < ys[i + 1] and xs[j] <= x < xs[j + 1]; outside
 *            all cells it belongs to none.  A grid owns gy * gx result slots, row-major.
 * The regions of a call are sorted by set; region r's first result slot is the number of slots of the regions in front of it.  Per
 * slot the call returns mass (fp32 sum of the member pixels' values over all maps of the set; negative values are summed as they are)
 * and area (int32 number of member pixels); per set, total = the fp32 sum of ALL pixels of its maps.  A set without maps gets zeros.
 *
 * No floating-point atomics: a workgroup owns a strip of rows of one map and writes one partial per slot; a second launch folds the
 * partials of a slot in (map, strip) order.  Two runs give the same bytes.  Two launches on `stream`, whatever the call holds.
 *
 * maps, regions and data_host are HOST arrays read at call time (data_host is validated: a malformed region is refused, not computed);
 * data is the DEVICE copy of data_host's ndata doubles (8-byte aligned), uploaded by the caller on `stream` -- the one packed upload of
 * a call.  mass [slots], area [slots], total [nsets] and the workspace (4-byte aligned, countr_regions_workspace bytes) are device
 * buffers.  Limits: n <= COUNTR_REGIONS_MAX_MAPS maps and sets, <= COUNTR_REGIONS_MAX_REGIONS polygons and <= COUNTR_REGIONS_MAX_MAPS
 * grids per call, a map of at most 2^28 pixels.
 */
#define COUNTR_REGIONS_MAX_MAPS 16
#define COUNTR_REGIONS_MAX_REGIONS 64 /* polygons per call */
#define COUNTR_REGIONS_MAX_VERTICES 64
#define COUNTR_REGIONS_MAX_CELLS 256 /* of one grid */
typedef struct countr_region_map {
  const float* map; /* device, fp32 [h, w], contiguous */
  int h, w;
  int set;          /* 0 .. nsets - 1 */
  int place;        /* index into data of (ax, bx, ay, by) */
} countr_region_map;
typedef struct countr_region {
  int set;
  int nv;           /* polygon: 3 .. 64 vertices; grid: 0 */
  int gy, gx;       /* grid: cells down and across (polygon: 0, 0) */
  int data;         /* index into data: polygon x0, y0, x1, y1, ...; grid ys[0 .. gy], xs[0 .. gx] */
} countr_region;
/* bytes of workspace of a call with these maps and regions (host only; reads h, w, set of the maps and set, nv, gy, gx of the regions) */
int countr_regions_workspace(const countr_region_map* maps, int n, const countr_region* regions, int nregions, int nsets);
int countr_region_sums(const countr_region_map* maps, int n, const countr_region* regions, int nregions, int nsets,
                       const double* data_host, const double* data, int ndata, float* mass, int* area, float* total, void* workspace,
                       void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* COUNTR_HIP_EXT_H */
