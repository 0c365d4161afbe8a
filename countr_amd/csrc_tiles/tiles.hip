// A frame counted on a 2-D grid of 384 x 384 tiles (include/countr_hip_tiles.h states the rule): the tiles cut straight into the forward's
// input batch, and the per-tile density maps stitched in both directions with the map's sum and up to 8 rectangle sums.
//   countr_tiles_workspace  (host only) bytes of scratch a blend needs
//   countr_tile_gather      img [3, hk, wk] -> wins [nt, 3, 384, 384], one launch
//   countr_tile_blend       outs [nrows * ncols, 384, 384] -> dm [hk, wk], sums [1 + nrects], two launches
// The launches:
//   tile_gather_kernel  a thread per 16 bytes of the batch: consecutive threads read consecutive 16-byte groups of an image row and write
//                       consecutive groups of a tile row.  Both sides are aligned: wk and the column starts are multiples of 4
//   tile_blend_kernel   a block per 4 rows x 1024 columns of the map, a thread per four adjacent pixels of a row.  Tile edges lie on
//                       multiples of 4 columns, so the four pixels are covered by the same tiles.  Per row the bands that cover it are
//                       walked in band order; inside a band the tiles that cover the pixels in column order (the sequential blend, one
//                       16-byte load per covering tile), then the band's value enters the vertical blend.  The starts are kernel
//                       arguments, the walks are block-uniform.  A thread keeps the 9 sums in registers; one butterfly per sum adds the
//                       lanes, the waves' results go through LDS and are added in wave order: the block writes one partial per sum
//   tile_sums_kernel    a wave per sum: lane l adds the partials l, l + 64, ... in that order, one butterfly adds the lanes
#include <stdio.h>
#include <string.h>
#include "../csrc/common.hpp"
#include "../csrc/host_api.hpp"
#include "../../include/countr_hip_tiles.h"

namespace {

constexpr int T = COUNTR_TILES_SIZE, MAX_STARTS = COUNTR_TILES_MAX_STARTS, MAX_RECTS = COUNTR_TILES_MAX_RECTS;
constexpr int NSUMS = 1 + MAX_RECTS;
constexpr int BLOCK_ROWS = 4, BLOCK_COLS = 1024, WAVES = 4;      // a block of the blend: 256 threads x 4 pixels, 4 rows
constexpr int MAX_SIDE = MAX_STARTS * T;                         // 24576: hk * wk < 2^30
constexpr int GROUPS = 3 * T * (T / 4);                          // 16-byte groups of one tile of the batch
static_assert(GROUPS % 256 == 0, "the gather's grid is exact");

struct GatherArgs {
  int rows[MAX_STARTS], cols[MAX_STARTS];
};

struct BlendArgs {
  int rows[MAX_STARTS], cols[MAX_STARTS];
  int rect[MAX_RECTS][4];                                        // clipped to the map; y1 > y2 where the intersection is empty
  int nrows, ncols, nrects, hk, wk;
};

__global__ __launch_bounds__(256) void tile_gather_kernel(const GatherArgs a, const float* __restrict__ img, int hk, int wk,
                                                          float* __restrict__ wins) {
  const int j = blockIdx.y;
  const int g = blockIdx.x * 256 + threadIdx.x;                  // < GROUPS
  const int c = g / (T * (T / 4)), rem = g - c * (T * (T / 4));
  const int y = rem / (T / 4), x4 = rem - y * (T / 4);
  const int64_t src = ((int64_t)c * hk + a.rows[j] + y) * wk + a.cols[j] + 4 * x4;
  const float4 v = *reinterpret_cast<const float4*>(img + src);
  *reinterpret_cast<float4*>(wins + ((int64_t)j * GROUPS + g) * 4) = v;
}

// old / 2 + new / 2, one operation per statement and no contraction (the halves are exact, the sum is rounded once)
#pragma clang fp contract(off)
__device__ __forceinline__ float4 half_half(const float4 o, const float4 n) {
  float4 r;
  r.x = o.x * 0.5f + n.x * 0.5f;
  r.y = o.y * 0.5f + n.y * 0.5f;
  r.z = o.z * 0.5f + n.z * 0.5f;
  r.w = o.w * 0.5f + n.w * 0.5f;
  return r;
}

__global__ __launch_bounds__(256) void tile_blend_kernel(const BlendArgs a, const float* __restrict__ outs, float* __restrict__ dm,
                                                         float* __restrict__ part) {
  __shared__ float red[WAVES][NSUMS];
  const int x0 = blockIdx.x * BLOCK_COLS + 4 * threadIdx.x;
  const bool live = x0 < a.wk;                                   // (wk is a multiple of 4: a live thread owns four pixels of the map)
  float acc[NSUMS];
#pragma unroll
  for (int q = 0; q < NSUMS; ++q) acc[q] = 0.f;

  for (int r = 0; r < BLOCK_ROWS; ++r) {
    const int y = blockIdx.y * BLOCK_ROWS + r;
    if (y >= a.hk) break;                                        // (block-uniform)
    if (live) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      int prev_row_end = -1;
      for (int b = 0; b < a.nrows; ++b) {                        // (block-uniform walk: the starts increase)
        const int rb = a.rows[b];
        if (rb > y) break;
        if (y < rb + T) {
          float4 h = make_float4(0.f, 0.f, 0.f, 0.f);
          int prev_col_end = -1;
          const float* band = outs + ((int64_t)b * a.ncols * T + (y - rb)) * T;
          for (int k = 0; k < a.ncols; ++k) {
            const int s = a.cols[k];
            if (s > x0) break;
            if (x0 < s + T) {
              const float4 o = *reinterpret_cast<const float4*>(band + (int64_t)k * T * T + (x0 - s));
              h = x0 <= prev_col_end ? half_half(h, o) : o;
            }
            prev_col_end = s + T - 1;
          }
          v = y <= prev_row_end ? half_half(v, h) : h;
        }
        prev_row_end = rb + T - 1;
      }
      *reinterpret_cast<float4*>(dm + (int64_t)y * a.wk + x0) = v;
      acc[0] = acc[0] + v.x; acc[0] = acc[0] + v.y; acc[0] = acc[0] + v.z; acc[0] = acc[0] + v.w;
#pragma unroll
      for (int q = 0; q < MAX_RECTS; ++q) {
        if (q < a.nrects && y >= a.rect[q][0] && y <= a.rect[q][2]) {
          const int x1 = a.rect[q][1], x2 = a.rect[q][3];
          float t = acc[1 + q];
          if (x0 >= x1 && x0 <= x2) t = t + v.x;
          if (x0 + 1 >= x1 && x0 + 1 <= x2) t = t + v.y;
          if (x0 + 2 >= x1 && x0 + 2 <= x2) t = t + v.z;
          if (x0 + 3 >= x1 && x0 + 3 <= x2) t = t + v.w;
          acc[1 + q] = t;
        }
      }
    }
  }

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < NSUMS; ++q) {
    const float s = wave_sum(acc[q]);
    if (lane == 0) red[wave][q] = s;
  }
  __syncthreads();
  if (threadIdx.x < NSUMS) {
    float t = 0.f;
#pragma unroll
    for (int wv = 0; wv < WAVES; ++wv) t = t + red[wv][threadIdx.x];
    part[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * NSUMS + threadIdx.x] = t;
  }
}

__global__ __launch_bounds__(64) void tile_sums_kernel(const float* __restrict__ part, int nblocks, float* __restrict__ sums) {
  const int q = blockIdx.x;
  float t = 0.f;
  for (int i = threadIdx.x; i < nblocks; i += 64) t = t + part[(int64_t)i * NSUMS + q];
  t = wave_sum(t);
  if (threadIdx.x == 0) sums[q] = t;
}

// the number of workgroups (= partials) of a blend of an [hk, wk] map, or < 0
int blend_blocks(int hk, int wk, const char* who, int* gx, int* gy) {
  if (hk < T || wk < T || hk > MAX_SIDE || wk > MAX_SIDE || (wk & 3))
    return failf(-1, "%s: a map is 384 .. %d on a side and its width a multiple of 4, got %d x %d", who, MAX_SIDE, hk, wk);
  *gx = (wk + BLOCK_COLS - 1) / BLOCK_COLS;
  *gy = (hk + BLOCK_ROWS - 1) / BLOCK_ROWS;
  return *gx * *gy;                                              // <= 24 * 6144
}

// a list of starts is a full cover of [0, size): begins at 0, increases strictly, leaves no gap, ends at size - 384
int check_starts(const int* s, int n, int size, int mult, const char* who, const char* axis) {
  if (!s || n < 1 || n > MAX_STARTS) return failf(-1, "%s: 1..%d %s starts, got %d", who, MAX_STARTS, axis, n);
  for (int i = 0; i < n; ++i) {
    const int lo = i ? s[i - 1] + 1 : 0, hi = i ? s[i - 1] + T : 0;
    if (s[i] < lo || s[i] > hi || s[i] + T > size || (s[i] % mult))
      return failf(-1, "%s: %s start %d = %d: the starts begin at 0, increase, leave no gap, are multiples of %d and keep "
                   "their tiles inside %d", who, axis, i, s[i], mult, size);
  }
  if (s[n - 1] + T != size) return failf(-1, "%s: the last %s tile ends at %d, the map at %d", who, axis, s[n - 1] + T, size);
  return 0;
}

}  // namespace

extern "C" int countr_tiles_version(void) { return COUNTR_TILES_ABI_VERSION; }

extern "C" const char* countr_tiles_last_error(void) { return g_err; }

extern "C" int countr_tiles_workspace(int hk, int wk) {
  int gx, gy;
  const int blocks = blend_blocks(hk, wk, "countr_tiles_workspace", &gx, &gy);
  if (blocks < 0) return blocks;
  return blocks * NSUMS * 4;
}

extern "C" int countr_tile_gather(const float* img, int hk, int wk, const int* rows, const int* cols, int nt, float* wins,
                                  void* stream) {
  if (!rows || !cols || nt < 1 || nt > MAX_STARTS) return failf(-1, "countr_tile_gather: 1..%d tiles a call, got %d", MAX_STARTS, nt);
  if (!img || !wins || (((uintptr_t)img) & 15) || (((uintptr_t)wins) & 15))
    return fail(-1, "countr_tile_gather: img and wins are required, 16-byte aligned");
  if (hk < T || wk < T || hk > MAX_SIDE || wk > MAX_SIDE || (wk & 3))
    return failf(-1, "countr_tile_gather: an image is 384 .. %d on a side and its width a multiple of 4, got %d x %d", MAX_SIDE,
             hk, wk);
  GatherArgs a;
  memset(&a, 0, sizeof(a));
  for (int j = 0; j < nt; ++j) {
    if (rows[j] < 0 || rows[j] > hk - T || cols[j] < 0 || cols[j] > wk - T)
      return failf(-1, "countr_tile_gather: tile %d at (%d, %d) lies outside the %d x %d image", j, rows[j], cols[j], hk, wk);
    if (cols[j] & 3) return failf(-1, "countr_tile_gather: tile %d: column start %d is not a multiple of 4", j, cols[j]);
    a.rows[j] = rows[j];
    a.cols[j] = cols[j];
  }
  hipLaunchKernelGGL(tile_gather_kernel, dim3(GROUPS / 256, (unsigned)nt), dim3(256), 0, STREAM(stream), a, img, hk, wk, wins);
  return launched("countr_tile_gather");
}

extern "C" int countr_tile_blend(const float* outs, int nrows, int ncols, const int* row_starts, const int* col_starts, int hk, int wk,
                                 const int* rects, int nrects, float* dm, float* sums, void* workspace, void* stream) {
  int gx, gy;
  const int blocks = blend_blocks(hk, wk, "countr_tile_blend", &gx, &gy);
  if (blocks < 0) return blocks;
  if (check_starts(row_starts, nrows, hk, 1, "countr_tile_blend", "row")) return -1;
  if (check_starts(col_starts, ncols, wk, 4, "countr_tile_blend", "column")) return -1;
  if (nrects < 0 || nrects > MAX_RECTS || (nrects && !rects))
    return failf(-1, "countr_tile_blend: 0..%d rectangles, got %d", MAX_RECTS, nrects);
  if (!outs || !dm || !sums || !workspace || (((uintptr_t)outs) & 15) || (((uintptr_t)dm) & 15) || (((uintptr_t)sums) & 3) ||
      (((uintptr_t)workspace) & 3))
    return fail(-1, "countr_tile_blend: outs and dm (16-byte aligned), sums and a workspace are required");
  BlendArgs a;
  memset(&a, 0, sizeof(a));
  for (int i = 0; i < nrows; ++i) a.rows[i] = row_starts[i];
  for (int i = 0; i < ncols; ++i) a.cols[i] = col_starts[i];
  for (int q = 0; q < nrects; ++q) {
    const int y1 = rects[4 * q], x1 = rects[4 * q + 1], y2 = rects[4 * q + 2], x2 = rects[4 * q + 3];
    if (y2 < y1 || x2 < x1)
      return failf(-1, "countr_tile_blend: rectangle %d (%d, %d, %d, %d): corners are (y1, x1) <= (y2, x2)", q, y1, x1, y2, x2);
    a.rect[q][0] = y1 < 0 ? 0 : y1;
    a.rect[q][1] = x1 < 0 ? 0 : x1;
    a.rect[q][2] = y2 > hk - 1 ? hk - 1 : y2;
    a.rect[q][3] = x2 > wk - 1 ? wk - 1 : x2;
    if (a.rect[q][1] > a.rect[q][3]) { a.rect[q][0] = 1; a.rect[q][2] = 0; }      // no column left: no row matches
  }
  a.nrows = nrows; a.ncols = ncols; a.nrects = nrects; a.hk = hk; a.wk = wk;
  float* part = (float*)workspace;
  hipLaunchKernelGGL(tile_blend_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, STREAM(stream), a, outs, dm, part);
  hipLaunchKernelGGL(tile_sums_kernel, dim3((unsigned)(1 + nrects)), dim3(64), 0, STREAM(stream), part, blocks, sums);
  return launched("countr_tile_blend");
}
