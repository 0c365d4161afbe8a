// The fold of a frame's class density maps into a dominant-class label map (include/countr_hip_classes.h states the rule): per pixel
// v_c = scale[c] * map_c, the label is the smallest c with the largest v_c (255 when that is <= floor); per class the sums of v_c over
// the pixels it won and over all pixels, and the number of pixels it won.  Two launches for up to 16 sets.
//   countr_classes_workspace  (host only) bytes of scratch a call needs
//   countr_class_fold         nsets sets of nc fp32 [h, w] maps -> labels uint8 [h, w] per set, won / total / area [set][16]
// The launches:
//   1 class_fold_strip_kernel  a block per strip of rows of one set.  The maps are contiguous, so a strip is a run of h-major pixels and
//                              the threads walk it in order: every class map is read once, a wave reads consecutive addresses.  Where
//                              every pointer of the set is 16-byte aligned and a strip is a whole number of 4-pixel groups, a thread
//                              takes four pixels at a time (one 16-byte load per class, one 4-byte store of labels); else one.  A
//                              thread keeps the 3 x 16 sums in registers; one butterfly per sum adds the lanes, the waves' results go
//                              through LDS and are added in wave order: the block writes one partial per class
//   2 class_fold_sum_kernel    a block per set, a thread per sum: the strips' partials in strip order -- no atomic decides a sum
#include <stdio.h>
#include <string.h>
#include "../csrc/common.hpp"
#include "../csrc/host_api.hpp"
#include "../../include/countr_hip_classes.h"

namespace {

constexpr int MAX_SETS = COUNTR_CLASSES_MAX_SETS, NC = COUNTR_CLASSES_MAX;
constexpr int MIN_ROWS = 16, MAX_STRIPS = 256;   // a strip is max(MIN_ROWS, ceil(h / MAX_STRIPS)) rows
constexpr int WAVES = 4;
constexpr int SUMS = 3 * NC;                     // a partial: won[16] | total[16] (floats) | area[16] (ints)
static_assert(NC == 16 && sizeof(countr_class_set) == 216, "the kernels below unroll over the 16 classes of countr_class_set");

struct FoldArgs {
  int h[MAX_SETS], w[MAX_SETS], nc[MAX_SETS];
  int rows[MAX_SETS];                            // rows of a strip of set s
  int vec[MAX_SETS];                             // 1: the four-pixel path
  int blk_off[MAX_SETS + 1];                     // first block (= first partial) of set s
};

struct Sums {
  float won[NC], total[NC];
  int area[NC];
};

// the header's rule for one pixel, one operation per statement and no contraction: the product is rounded to fp32 before it is
// compared or added.  Every index below is a constant after unrolling: the arrays live in registers.
#pragma clang fp contract(off)
__device__ __forceinline__ unsigned fold_pixel(const float (&m)[NC], const float (&sc)[NC], int nc, float floor, Sums& a) {
  float v[NC];
  float best = 0.f;
  int label = 0;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    if (c < nc) {                                // (block-uniform)
      v[c] = sc[c] * m[c];
      a.total[c] = a.total[c] + v[c];
      if (c == 0) best = v[0];
      else if (v[c] > best) { best = v[c]; label = c; }      // strictly larger: a tie stays with the smaller index
    }
  }
  if (best <= floor) label = 255;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    if (c < nc) {
      const bool mine = label == c;
      a.won[c] = a.won[c] + (mine ? v[c] : 0.f);
      a.area[c] += mine ? 1 : 0;
    }
  }
  return (unsigned)label;
}

__global__ __launch_bounds__(256) void class_fold_strip_kernel(const FoldArgs a, const countr_class_set* __restrict__ sets, float floor,
                                                               float* __restrict__ part, int nsets) {
  __shared__ float redf[WAVES][2 * NC];
  __shared__ int redi[WAVES][NC];
  int s = 0;
  while (s + 1 < nsets && (int)blockIdx.x >= a.blk_off[s + 1]) ++s;      // (block-uniform)
  const int strip = blockIdx.x - a.blk_off[s];
  const int h = a.h[s], w = a.w[s], nc = a.nc[s], rows = a.rows[s];
  const int r0 = strip * rows, r1 = min(r0 + rows, h);
  const int64_t p0 = (int64_t)r0 * w, p1 = (int64_t)r1 * w;              // the strip's pixels: [p0, p1) of h * w <= 2^28
  const countr_class_set& d = sets[s];
  const float* m[NC];
  float sc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    m[c] = c < nc ? d.map[c] : nullptr;
    sc[c] = c < nc ? d.scale[c] : 0.f;
  }
  unsigned char* __restrict__ lab = (unsigned char*)d.labels;
  Sums acc;
#pragma unroll
  for (int c = 0; c < NC; ++c) { acc.won[c] = 0.f; acc.total[c] = 0.f; acc.area[c] = 0; }

  int64_t p = p0 + threadIdx.x;
  if (a.vec[s]) {                                // (block-uniform) p0 and every base are multiples of 4 pixels / 16 bytes
    const int64_t groups = (p1 - p0) >> 2;
    for (int64_t g = threadIdx.x; g < groups; g += 256) {
      const int64_t q = p0 + 4 * g;
      float x[4][NC];
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        if (c < nc) {
          const float4 t = *reinterpret_cast<const float4*>(m[c] + q);
          x[0][c] = t.x; x[1][c] = t.y; x[2][c] = t.z; x[3][c] = t.w;
        }
      }
      unsigned pack = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) pack |= fold_pixel(x[j], sc, nc, floor, acc) << (8 * j);
      *reinterpret_cast<unsigned*>(lab + q) = pack;
    }
    p = p0 + 4 * groups + threadIdx.x;           // (rows * w is a multiple of 4; the last strip of a set may still leave a tail)
  }
  for (; p < p1; p += 256) {
    float x[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (c < nc) x[c] = m[c][p];
    lab[p] = (unsigned char)fold_pixel(x, sc, nc, floor, acc);
  }

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const float sw = wave_sum(acc.won[c]), st = wave_sum(acc.total[c]);
    const int sa = wave_sum_i(acc.area[c]);
    if (lane == 0) { redf[wave][c] = sw; redf[wave][NC + c] = st; redi[wave][c] = sa; }
  }
  __syncthreads();
  float* out = part + (int64_t)blockIdx.x * SUMS;
  if (threadIdx.x < 2 * NC) {
    float t = 0.f;
#pragma unroll
    for (int wv = 0; wv < WAVES; ++wv) t = t + redf[wv][threadIdx.x];
    out[threadIdx.x] = t;
  } else if (threadIdx.x < SUMS) {
    int t = 0;
#pragma unroll
    for (int wv = 0; wv < WAVES; ++wv) t += redi[wv][threadIdx.x - 2 * NC];
    reinterpret_cast<int*>(out)[threadIdx.x] = t;
  }
}

__global__ __launch_bounds__(64) void class_fold_sum_kernel(const FoldArgs a, const float* __restrict__ part, float* __restrict__ won,
                                                            float* __restrict__ total, int* __restrict__ area) {
  const int s = blockIdx.x, k = threadIdx.x;
  if (k >= SUMS) return;
  const int b0 = a.blk_off[s], b1 = a.blk_off[s + 1];
  if (k < 2 * NC) {
    float t = 0.f;
    for (int b = b0; b < b1; ++b) t = t + part[(int64_t)b * SUMS + k];
    if (k < NC) won[s * NC + k] = t; else total[s * NC + k - NC] = t;
  } else {
    const int* pi = reinterpret_cast<const int*>(part);
    int t = 0;
    for (int b = b0; b < b1; ++b) t += pi[(int64_t)b * SUMS + k];
    area[s * NC + k - 2 * NC] = t;
  }
}

// the part of a call that its sizes decide: strips and the four-pixel path.  -> the number of blocks (= partials), or < 0
int layout(const countr_class_set* sets, int nsets, FoldArgs* a, const char* who) {
  if (!sets || nsets < 1 || nsets > MAX_SETS) return failf(-1, "%s: bad args (1..16 sets a call)", who);
  int blocks = 0;
  for (int s = 0; s < MAX_SETS; ++s) {
    if (s >= nsets) {
      a->h[s] = a->w[s] = a->nc[s] = a->rows[s] = a->vec[s] = 0; a->blk_off[s + 1] = blocks;
      continue;
    }
    const countr_class_set& d = sets[s];
    if (d.nc < 1 || d.nc > NC) return failf(-1, "%s: set %d: a set has 1..16 classes, got %d", who, s, d.nc);
    if (d.h < 1 || d.w < 1 || (int64_t)d.h * d.w > (int64_t)1 << 28)
      return failf(-1, "%s: set %d: a map has 1 .. 2^28 pixels, got %d x %d", who, s, d.h, d.w);
    const int per = (d.h + MAX_STRIPS - 1) / MAX_STRIPS;
    const int rows = per > MIN_ROWS ? per : MIN_ROWS;
    int vec = (((int64_t)rows * d.w) & 3) == 0 && (((uintptr_t)d.labels) & 3) == 0;
    for (int c = 0; c < d.nc; ++c) vec = vec && (((uintptr_t)d.map[c]) & 15) == 0;
    a->h[s] = d.h; a->w[s] = d.w; a->nc[s] = d.nc; a->rows[s] = rows; a->vec[s] = vec;
    a->blk_off[s] = blocks;
    blocks += (d.h + rows - 1) / rows;           // <= 16 * 256
    a->blk_off[s + 1] = blocks;
  }
  return blocks;
}

}  // namespace

extern "C" int countr_classes_version(void) { return COUNTR_CLASSES_ABI_VERSION; }

extern "C" const char* countr_classes_last_error(void) { return g_err; }

extern "C" int countr_classes_workspace(const countr_class_set* sets, int nsets) {
  FoldArgs a;
  const int blocks = layout(sets, nsets, &a, "countr_classes_workspace");
  if (blocks < 0) return blocks;
  return blocks * SUMS * 4;                      // 48 four-byte sums per strip
}

extern "C" int countr_class_fold(const countr_class_set* sets, int nsets, const void* sets_dev, float floor, float* won, float* total,
                                 int* area, void* workspace, void* stream) {
  FoldArgs a;
  const int blocks = layout(sets, nsets, &a, "countr_class_fold");
  if (blocks < 0) return blocks;
  if (!sets_dev || !won || !total || !area || !workspace || (((uintptr_t)sets_dev) & 7) || (((uintptr_t)workspace) & 3) ||
      (((uintptr_t)won) & 3) || (((uintptr_t)total) & 3) || (((uintptr_t)area) & 3))
    return fail(-1, "countr_class_fold: sets_dev (8-byte aligned), won, total, area and a workspace are required");
  if (!__builtin_isfinite(floor)) return fail(-1, "countr_class_fold: floor is finite");
  for (int s = 0; s < nsets; ++s) {
    const countr_class_set& d = sets[s];
    if (!d.labels) return failf(-1, "countr_class_fold: set %d: no label map", s);
    for (int c = 0; c < d.nc; ++c) {
      if (!d.map[c] || (((uintptr_t)d.map[c]) & 3)) return failf(-1, "countr_class_fold: set %d: map %d: null or misaligned", s, c);
      if (!__builtin_isfinite(d.scale[c])) return failf(-1, "countr_class_fold: set %d: scale %d is not finite", s, c);
    }
  }
  float* part = (float*)workspace;
  hipLaunchKernelGGL(class_fold_strip_kernel, dim3((unsigned)blocks), dim3(256), 0, STREAM(stream), a,
                     (const countr_class_set*)sets_dev, floor, part, nsets);
  hipLaunchKernelGGL(class_fold_sum_kernel, dim3((unsigned)nsets), dim3(64), 0, STREAM(stream), a, part, won, total, area);
  return launched("countr_class_fold");
}
