// Sums of density maps over regions (include/countr_hip_ext.h states the rule): polygons by the crossing number, grids by half-open
// cells, both decided in fp64 with the header's operation order; the sums are fp32.  Two launches, whatever the call holds.
//   countr_regions_workspace  (host only) bytes of scratch a call needs
//   countr_region_sums        n fp32 [h, w] maps with placements, regions per set -> mass[slot], area[slot], total[set]
// The launches:
//   1 regions_strip_kernel  a block per strip of rows of one map, a wave per 64-column chunk of the strip.  x depends on the column
//                           only and y on the row only, so an edge's crossing abscissa and a row's grid row are wave-uniform: per
//                           (row, edge) the lanes differ in one compare.  The set's polygons are staged in LDS (<= VCAP vertices at
//                           a time, with their bounding boxes: a chunk or a row outside the box skips the edge loop); a grid's
//                           boundaries likewise.  A lane adds up its member pixels over the strip's rows; one butterfly per (chunk,
//                           region) then adds the lanes, and lane 0 adds the result to its wave's accumulator in LDS -- a fixed
//                           order.  The block writes one partial {mass, area} per slot of its set, and the strip's sum of all pixels
//   2 regions_fold_kernel   a thread per slot: the partials of the set's maps in (map, strip) order -- no atomic decides a sum
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include "../csrc/common.hpp"
#include "../csrc/host_api.hpp"
#include "../../include/countr_hip_ext.h"

namespace {

constexpr int MAX_MAPS = COUNTR_REGIONS_MAX_MAPS, MAX_POLY = COUNTR_REGIONS_MAX_REGIONS;
constexpr int MAX_NV = COUNTR_REGIONS_MAX_VERTICES, MAX_CELLS = COUNTR_REGIONS_MAX_CELLS;
constexpr int MAX_REG = MAX_POLY + MAX_MAPS;     // regions of a call: <= 64 polygons + <= 16 grids
constexpr int MIN_ROWS = 4, MAX_STRIPS = 256;    // a strip is max(MIN_ROWS, ceil(h / MAX_STRIPS)) rows
constexpr int VCAP = 1024;                       // vertices staged at a time (16 KB of LDS)
constexpr int WAVES = 4;

struct RegionArgs {
  const float* map[MAX_MAPS];
  int h[MAX_MAPS], w[MAX_MAPS], set[MAX_MAPS], place[MAX_MAPS];
  int rows[MAX_MAPS];                            // rows of a strip of map i
  int blk_off[MAX_MAPS + 1];                     // first block of map i
  int part_off[MAX_MAPS];                        // first partial of map i: [strips][slots of its set + 1]
  int first[MAX_MAPS + 1];                       // regions of set s: first[s] .. first[s + 1] - 1
  int slot0[MAX_MAPS + 1];                       // first result slot of set s
  int nv[MAX_REG], gy[MAX_REG], gx[MAX_REG], data[MAX_REG], slot[MAX_REG];
};

// the header's two rules, fp64, one operation per statement and no contraction
#pragma clang fp contract(off)
__device__ __forceinline__ double place(double a, double c, double b) {
  const double m = a * c;
  return m + b;
}
__device__ __forceinline__ double crossing(double x0, double y0, double x1, double y1, double y) {
  const double dy = y - y0;
  const double dx = x1 - x0;
  const double ey = y1 - y0;
  const double p = dy * dx;
  const double q = p / ey;
  return x0 + q;
}

// number of boundaries b[0 .. n - 1] (strictly increasing) that are <= v
__device__ __forceinline__ int count_le(const double* b, int n, double v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (b[mid] <= v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the waves' accumulators of slots [0, cnt) -> the block's partials at pm / pa; every thread calls it
__device__ __forceinline__ void write_partials(const float* accm, const int* acca, int stride, int cnt, float* pm, int* pa) {
  __syncthreads();
  for (int k = threadIdx.x; k < cnt; k += 256) {
    float m = 0.f;
    int a = 0;
#pragma unroll
    for (int wv = 0; wv < WAVES; ++wv) { m += accm[wv * stride + k]; a += acca[wv * stride + k]; }
    pm[k] = m; pa[k] = a;
  }
  __syncthreads();
}

__global__ __launch_bounds__(256) void regions_strip_kernel(const RegionArgs a, const double* __restrict__ data, float* __restrict__ pmass,
                                                            int* __restrict__ parea, int n) {
  __shared__ double verts[2 * VCAP];             // polygons: x, y pairs; a grid: ys then xs
  __shared__ double box[MAX_POLY][4];            // min x, max x (widened), min y, max y
  __shared__ int vfirst[MAX_POLY + 1];
  __shared__ float accm[WAVES * MAX_CELLS];
  __shared__ int acca[WAVES * MAX_CELLS];
  int i = 0;
  while (i + 1 < n && (int)blockIdx.x >= a.blk_off[i + 1]) ++i;      // (block-uniform)
  const int strip = blockIdx.x - a.blk_off[i];
  const int h = a.h[i], w = a.w[i], s = a.set[i];
  const int r0 = strip * a.rows[i], r1 = min(r0 + a.rows[i], h);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int chunks = (w + 63) >> 6;
  const float* __restrict__ m = a.map[i];
  const double ax = data[a.place[i]], bx = data[a.place[i] + 1], ay = data[a.place[i] + 2], by = data[a.place[i] + 3];
  const int S = a.slot0[s + 1] - a.slot0[s] + 1;                     // the set's slots + its total
  float* pm = pmass + a.part_off[i] + (int64_t)strip * S;
  int* pa = parea + a.part_off[i] + (int64_t)strip * S;
  const double ylo = place(ay, (double)r0, by), yhi = place(ay, (double)(r1 - 1), by);      // ay > 0: the strip's y range

  // ---- the strip's sum of all pixels
  {
    float t = 0.f;
    for (int c = wave; c < chunks; c += WAVES) {
      const int cx = c * 64 + lane;
      if (cx < w)
        for (int y = r0; y < r1; ++y) t += m[(int64_t)y * w + cx];
    }
    t = wave_sum(t);
    if (lane == 0) { accm[wave] = t; acca[wave] = 0; }
    write_partials(accm, acca, 1, 1, pm + S - 1, pa + S - 1);
  }

  // ---- polygons, <= VCAP vertices and <= MAX_POLY polygons at a time (the set's regions are walked in order; grids in between are
  // taken by the loop below)
  const int e0 = a.first[s], e1 = a.first[s + 1];
  for (int p0 = e0; p0 < e1;) {
    int p1 = p0, nvt = 0, np = 0;                                    // (block-uniform: reads the arguments only)
    while (p1 < e1 && (a.nv[p1] == 0 || (nvt + a.nv[p1] <= VCAP && np < MAX_POLY))) {
      if (a.nv[p1]) { nvt += a.nv[p1]; ++np; }
      ++p1;
    }
    if (np) {
      // stage: vertex k of the group's j-th polygon at verts[2 (vfirst[j] + k)]
      if (threadIdx.x == 0) {
        int at = 0, j = 0;
        for (int e = p0; e < p1; ++e)
          if (a.nv[e]) { vfirst[j++] = at; at += a.nv[e]; }
        vfirst[j] = at;
      }
      for (int k = threadIdx.x; k < WAVES * MAX_POLY; k += 256) { accm[k] = 0.f; acca[k] = 0; }
      __syncthreads();
      {
        int j = 0;
        for (int e = p0; e < p1; ++e) {
          if (!a.nv[e]) continue;
          for (int k = threadIdx.x; k < 2 * a.nv[e]; k += 256) verts[2 * vfirst[j] + k] = data[a.data[e] + k];
          ++j;
        }
      }
      __syncthreads();
      if ((int)threadIdx.x < np) {
        const double* v = verts + 2 * vfirst[threadIdx.x];
        const int nv = vfirst[threadIdx.x + 1] - vfirst[threadIdx.x];
        double x0 = v[0], x1 = v[0], y0 = v[1], y1 = v[1];
        for (int k = 1; k < nv; ++k) {
          x0 = fmin(x0, v[2 * k]); x1 = fmax(x1, v[2 * k]);
          y0 = fmin(y0, v[2 * k + 1]); y1 = fmax(y1, v[2 * k + 1]);
        }
        // a crossing abscissa is rounded (four operations): it may leave [min x, max x] by a few ulps of the largest |x|.  The box
        // is widened by far more than that, so a pixel the box rejects is one the rule rejects.  The y test is exact.
        const double pad = 1e-9 * fmax(fmax(fabs(x0), fabs(x1)), 1.0);
        box[threadIdx.x][0] = x0 - pad; box[threadIdx.x][1] = x1 + pad; box[threadIdx.x][2] = y0; box[threadIdx.x][3] = y1;
      }
      __syncthreads();
      for (int c = wave; c < chunks; c += WAVES) {
        const int cx = c * 64 + lane;
        const bool valid = cx < w;
        const double x = place(ax, (double)cx, bx);
        const double xlo = place(ax, (double)(c * 64), bx), xhi = place(ax, (double)min(c * 64 + 63, w - 1), bx);      // ax > 0
        for (int j = 0; j < np; ++j) {
          if (xhi < box[j][0] || xlo > box[j][1] || yhi < box[j][2] || ylo >= box[j][3]) continue;      // (wave-uniform)
          const double* v = verts + 2 * vfirst[j];
          const int nv = vfirst[j + 1] - vfirst[j];
          float acc = 0.f;
          int cnt = 0;
          for (int yy = r0; yy < r1; ++yy) {
            const double y = place(ay, (double)yy, by);
            if (y < box[j][2] || y >= box[j][3]) continue;           // (wave-uniform)
            bool odd = false;
            double px = v[2 * nv - 2], py = v[2 * nv - 1];           // the closing edge first: a parity has no order
            for (int k = 0; k < nv; ++k) {
              const double qx = v[2 * k], qy = v[2 * k + 1];
              if ((py <= y) != (qy <= y)) odd ^= x < crossing(px, py, qx, qy, y);      // (wave-uniform condition)
              px = qx; py = qy;
            }
            if (odd && valid) { acc += m[(int64_t)yy * w + cx]; ++cnt; }
          }
          acc = wave_sum(acc);
          cnt = wave_sum_i(cnt);
          if (lane == 0) { accm[wave * MAX_POLY + j] += acc; acca[wave * MAX_POLY + j] += cnt; }
        }
      }
      // the group's polygons -> their slots (a polygon owns one)
      __syncthreads();
      if ((int)threadIdx.x < np) {
        int j = 0, e = p0;
        for (; e < p1; ++e)
          if (a.nv[e] && j++ == (int)threadIdx.x) break;
        float sm_ = 0.f;
        int sa = 0;
#pragma unroll
        for (int wv = 0; wv < WAVES; ++wv) { sm_ += accm[wv * MAX_POLY + threadIdx.x]; sa += acca[wv * MAX_POLY + threadIdx.x]; }
        const int k = a.slot[e] - a.slot0[s];
        pm[k] = sm_; pa[k] = sa;
      }
      __syncthreads();
    }
    if (p1 == p0) break;                                             // (cannot happen: a polygon has <= MAX_NV <= VCAP vertices)
    p0 = p1;
  }

  // ---- grids, one at a time
  for (int e = e0; e < e1; ++e) {
    if (a.nv[e]) continue;                                           // (block-uniform)
    const int gy = a.gy[e], gx = a.gx[e], cells = gy * gx;
    double* ys = verts;
    double* xs = verts + gy + 1;
    __syncthreads();
    for (int k = threadIdx.x; k < gy + gx + 2; k += 256) verts[k] = data[a.data[e] + k];
    for (int k = threadIdx.x; k < WAVES * MAX_CELLS; k += 256) { accm[k] = 0.f; acca[k] = 0; }
    __syncthreads();
    for (int c = wave; c < chunks; c += WAVES) {
      const int cx = c * 64 + lane;
      const bool valid = cx < w;
      const double x = place(ax, (double)cx, bx);
      int jl = count_le(xs, gx + 1, x) - 1;                          // xs[jl] <= x < xs[jl + 1]
      if (!valid || jl >= gx) jl = -1;
      const float ninf = -__builtin_inff();
      const int jmax = (int)wave_max(jl >= 0 ? (float)jl : -1.f);    // (a cell index is exact as a float)
      if (jmax < 0) continue;                                        // (wave-uniform)
      const int jmin = (int)(-wave_max(jl >= 0 ? -(float)jl : ninf));
      float acc = 0.f;
      int cnt = 0, cur = -1;
      for (int yy = r0; yy <= r1; ++yy) {                            // (yy == r1: the last flush)
        int il = -1;
        if (yy < r1) {
          il = count_le(ys, gy + 1, place(ay, (double)yy, by)) - 1;  // (wave-uniform)
          if (il >= gy) il = -1;
        }
        if (il != cur) {
          if (cur >= 0) {
            for (int j = jmin; j <= jmax; ++j) {
              const float sj = wave_sum(jl == j ? acc : 0.f);
              const int cj = wave_sum_i(jl == j ? cnt : 0);
              if (lane == 0) { accm[wave * MAX_CELLS + cur * gx + j] += sj; acca[wave * MAX_CELLS + cur * gx + j] += cj; }
            }
          }
          acc = 0.f; cnt = 0; cur = il;
        }
        if (il >= 0 && jl >= 0) { acc += m[(int64_t)yy * w + cx]; ++cnt; }
      }
    }
    const int k0 = a.slot[e] - a.slot0[s];
    write_partials(accm, acca, MAX_CELLS, cells, pm + k0, pa + k0);
  }
}

__global__ __launch_bounds__(256) void regions_fold_kernel(const RegionArgs a, const float* __restrict__ pmass, const int* __restrict__ parea,
                                                           float* __restrict__ mass, int* __restrict__ area, float* __restrict__ total, int n) {
  const int s = blockIdx.y;
  const int S = a.slot0[s + 1] - a.slot0[s] + 1;
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= S) return;
  float sm_ = 0.f;
  int sa = 0;
  for (int i = 0; i < n; ++i) {
    if (a.set[i] != s) continue;
    const int strips = a.blk_off[i + 1] - a.blk_off[i];
    const float* pm = pmass + a.part_off[i] + k;
    const int* pa = parea + a.part_off[i] + k;
    for (int b = 0; b < strips; ++b) { sm_ += pm[(int64_t)b * S]; sa += pa[(int64_t)b * S]; }
  }
  if (k == S - 1) total[s] = sm_;
  else { mass[a.slot0[s] + k] = sm_; area[a.slot0[s] + k] = sa; }
}

// the part of a call that its sizes decide: strips, partial offsets, slots.  -> the number of partials, or < 0
int64_t layout(const countr_region_map* maps, int n, const countr_region* regions, int nregions, int nsets, RegionArgs* a, const char* who) {
  if (!maps || n < 1 || n > MAX_MAPS || nsets < 1 || nsets > MAX_MAPS || nregions < 0 || nregions > MAX_REG || (nregions && !regions))
    return failf(-1, "%s: bad args (1..16 maps, 1..16 sets, at most 64 polygons and 16 grids)", who);
  int polys = 0, grids = 0, slots = 0, r = 0;
  for (int s = 0; s <= MAX_MAPS; ++s) {
    a->first[s] = r; a->slot0[s] = slots;
    if (s >= nsets) continue;
    for (; r < nregions && regions[r].set == s; ++r) {
      const countr_region& d = regions[r];
      a->nv[r] = d.nv; a->gy[r] = d.gy; a->gx[r] = d.gx; a->data[r] = d.data; a->slot[r] = slots;
      if (d.nv == 0) {
        if (d.gy < 1 || d.gx < 1 || (int64_t)d.gy * d.gx > MAX_CELLS)
          return failf(-1, "%s: region %d: a grid has gy, gx >= 1 and at most 256 cells", who, r);
        ++grids; slots += d.gy * d.gx;
      } else {
        if (d.nv < 3 || d.nv > MAX_NV) return failf(-1, "%s: region %d: a polygon has 3..64 vertices, got %d", who, r, d.nv);
        ++polys; slots += 1;
      }
    }
  }
  if (r != nregions) return failf(-1, "%s: region %d: the regions are sorted by set, sets are 0..%d", who, r, nsets - 1);
  if (polys > MAX_POLY || grids > MAX_MAPS)
    return failf(-1, "%s: %d polygons and %d grids: a call takes at most 64 and 16", who, polys, grids);
  for (int r2 = nregions; r2 < MAX_REG; ++r2) a->nv[r2] = a->gy[r2] = a->gx[r2] = a->data[r2] = a->slot[r2] = 0;
  int64_t parts = 0;
  int blocks = 0;
  for (int i = 0; i < MAX_MAPS; ++i) {
    if (i >= n) {
      a->map[i] = nullptr; a->h[i] = a->w[i] = a->set[i] = a->place[i] = a->rows[i] = a->part_off[i] = 0; a->blk_off[i + 1] = blocks;
      continue;
    }
    const countr_region_map& d = maps[i];
    if (d.h < 1 || d.w < 1 || (int64_t)d.h * d.w > (int64_t)1 << 28 || d.set < 0 || d.set >= nsets)
      return failf(-1, "%s: map %d: a map has 1 .. 2^28 pixels and a set in 0..%d", who, i, nsets - 1);
    const int per = (d.h + MAX_STRIPS - 1) / MAX_STRIPS;
    const int rows = per > MIN_ROWS ? per : MIN_ROWS;
    const int strips = (d.h + rows - 1) / rows;
    a->map[i] = d.map; a->h[i] = d.h; a->w[i] = d.w; a->set[i] = d.set; a->place[i] = d.place; a->rows[i] = rows;
    a->blk_off[i] = blocks; a->part_off[i] = (int)parts;
    blocks += strips;
    a->blk_off[i + 1] = blocks;
    parts += (int64_t)strips * (a->slot0[d.set + 1] - a->slot0[d.set] + 1);      // <= 16 * 256 * 4161: fits an int
  }
  return parts;
}

}  // namespace

extern "C" int countr_ext_version(void) { return COUNTR_EXT_ABI_VERSION; }

extern "C" const char* countr_ext_last_error(void) { return g_err; }

extern "C" int countr_regions_workspace(const countr_region_map* maps, int n, const countr_region* regions, int nregions, int nsets) {
  RegionArgs a;
  const int64_t parts = layout(maps, n, regions, nregions, nsets, &a, "countr_regions_workspace");
  if (parts < 0) return (int)parts;
  return (int)(parts * 8);                       // a float and an int per partial
}

extern "C" int countr_region_sums(const countr_region_map* maps, int n, const countr_region* regions, int nregions, int nsets,
                                  const double* data_host, const double* data, int ndata, float* mass, int* area, float* total,
                                  void* workspace, void* stream) {
  RegionArgs a;
  const int64_t parts = layout(maps, n, regions, nregions, nsets, &a, "countr_region_sums");
  if (parts < 0) return (int)parts;
  if (!data_host || !data || ndata < 4 || !mass || !area || !total || !workspace || (((uintptr_t)data) & 7) || (((uintptr_t)workspace) & 3) ||
      (((uintptr_t)mass) & 3) || (((uintptr_t)area) & 3) || (((uintptr_t)total) & 3))
    return fail(-1, "countr_region_sums: data_host, data (8-byte aligned), mass, area, total and a workspace are required");
  for (int i = 0; i < n; ++i) {
    const countr_region_map& d = maps[i];
    if (!d.map || (((uintptr_t)d.map) & 3)) return failf(-1, "countr_region_sums: map %d: null or misaligned", i);
    if (d.place < 0 || d.place > ndata - 4) return failf(-1, "countr_region_sums: map %d: its placement lies outside data", i);
    const double* p = data_host + d.place;
    if (!(p[0] > 0.0 && p[2] > 0.0 && __builtin_isfinite(p[0]) && __builtin_isfinite(p[1]) && __builtin_isfinite(p[2]) && __builtin_isfinite(p[3])))
      return failf(-1, "countr_region_sums: map %d: a placement is finite with ax > 0 and ay > 0", i);
  }
  for (int r = 0; r < nregions; ++r) {
    const countr_region& d = regions[r];
    const int len = d.nv ? 2 * d.nv : d.gy + d.gx + 2;
    if (d.data < 0 || d.data > ndata - len) return failf(-1, "countr_region_sums: region %d: its data lies outside data", r);
    const double* p = data_host + d.data;
    for (int k = 0; k < len; ++k)
      if (!__builtin_isfinite(p[k])) return failf(-1, "countr_region_sums: region %d: a coordinate is not finite", r);
    if (d.nv == 0) {
      for (int k = 0; k < len - 1; ++k)
        if (k != d.gy && !(p[k] < p[k + 1])) return failf(-1, "countr_region_sums: region %d: grid boundaries are strictly increasing", r);
    }
  }
  float* pmass = (float*)workspace;
  int* parea = (int*)workspace + parts;
  int maxS = 1;
  for (int s = 0; s < nsets; ++s)
    if (a.slot0[s + 1] - a.slot0[s] + 1 > maxS) maxS = a.slot0[s + 1] - a.slot0[s] + 1;
  hipLaunchKernelGGL(regions_strip_kernel, dim3((unsigned)a.blk_off[MAX_MAPS]), dim3(256), 0, STREAM(stream), a, data, pmass, parea, n);
  hipLaunchKernelGGL(regions_fold_kernel, dim3((maxS + 255) / 256, nsets), dim3(256), 0, STREAM(stream), a, pmass, parea, mass, area, total, n);
  return launched("countr_region_sums");
}
