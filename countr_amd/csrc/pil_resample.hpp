// Pillow's 8-bit resample (Resample.c), the one copy: the tap tables (precompute_coeffs + normalize_coeffs_8bpc) for BILINEAR and
// BICUBIC, and the bodies of the two image passes.  frames.hip (frames of one size, uniform arguments) and pretrain_aug.hip (samples
// that all differ, per-sample descriptors) keep their own kernels: a kernel decodes its work item and calls the body here.
// Every pass goes into 8 bits before the next one, as Pillow's does, with int32 accumulators.  One table row is ONE function
// (table_row) for the host exports and the device kernel, compiled with fp contraction off: an fma in (xx + 0.5) * scale - support or
// in the cubic would change the last bit of a double and with it a rounded tap.
#pragma once
#include "common.hpp"

#include <math.h>

constexpr int PRECISION_BITS = 32 - 8 - 2;      // Pillow's fixed point: weights are int(+-0.5 + w * 2^22)
constexpr int STAGE_BYTES = 16384;              // LDS staging of one source row segment (horizontal passes)

struct Axis {
  double scale, support, ss;
  int ksize;
};

// precompute_coeffs' per-axis constants.  filter 0: bilinear (support 1), 1: bicubic (support 2)
__host__ __device__ inline Axis axis_of(int filter, int in_size, int out_size) {
#pragma clang fp contract(off)
  Axis a;
  a.scale = (double)in_size / (double)out_size;
  const double fs = a.scale < 1.0 ? 1.0 : a.scale;
  a.support = (filter == 1 ? 2.0 : 1.0) * fs;
  a.ss = 1.0 / fs;                              // (Pillow multiplies by this reciprocal; so does this file)
  const double k = ceil(a.support) * 2 + 1;
  a.ksize = k > (double)(1 << 30) ? 1 << 30 : (int)k;
  return a;
}
// (host) the constants of an axis whose whole table may be asked for: sizes >= 1 and in / out below 2^19
inline bool axis_ok(int filter, int in_size, int out_size, Axis* a) {
  if (in_size < 1 || out_size < 1) return false;
  *a = axis_of(filter, in_size, out_size);
  return a->ksize <= 1 << 20;
}

__host__ __device__ inline double filter_of(int filter, double x) {
#pragma clang fp contract(off)
  if (x < 0.0) x = -x;
  if (filter == 1) {                            // bicubic_filter, a = -0.5
    const double a = -0.5;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
  }
  return x < 1.0 ? 1.0 - x : 0.0;               // bilinear_filter
}

// Row xx of the tables of one axis: bounds[2 xx] = {first source index, tap count}, weights[xx * stride ..] = the taps in fixed point,
// zeros behind the tap count up to `stride` (>= the axis' ksize).  The weights are summed in a first loop and evaluated again in the
// second (the same operations give the same doubles), so that no per-row array of doubles is needed.
__host__ __device__ inline void table_row(int filter, const Axis& ax, int in_size, int xx, int stride, int* bounds, int* weights) {
#pragma clang fp contract(off)
  const double center = (xx + 0.5) * ax.scale;
  int xmin = (int)(center - ax.support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + ax.support + 0.5);
  if (xmax > in_size) xmax = in_size;
  xmax -= xmin;
  double ww = 0.0;
  for (int x = 0; x < xmax; ++x) ww += filter_of(filter, (x + xmin - center + 0.5) * ax.ss);
  int* k = weights + (int64_t)xx * stride;
  for (int x = 0; x < stride; ++x) {
    double w = 0.0;
    if (x < xmax) {
      w = filter_of(filter, (x + xmin - center + 0.5) * ax.ss);
      if (ww != 0.0) w /= ww;
    }
    k[x] = w < 0 ? (int)(-0.5 + w * (double)(1 << PRECISION_BITS)) : (int)(0.5 + w * (double)(1 << PRECISION_BITS));
  }
  bounds[2 * xx] = xmin;
  bounds[2 * xx + 1] = xmax;
}

// (host) output pixels per horizontal work item: the source bytes of a tile (+ alignment slack) must fit the LDS staging buffer.
// Below 1: the taps of one output pixel alone exceed it.
inline int tile_of(int in_size, int out_size, int filter) {
  const Axis ax = axis_of(filter, in_size, out_size);
  int tile = 256;
  while (tile >= 1 && ((int64_t)ceil(ax.scale * (tile - 1)) + ax.ksize + 1) * 3 + 48 > STAGE_BYTES) tile >>= 1;
  return tile;
}

__device__ __forceinline__ uint8_t clip8(int v) {      // (an arithmetic shift: a negative sum of the bicubic lobes clips to 0)
  v >>= PRECISION_BITS;
  return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// Horizontal pass, one work item of a 256-thread workgroup: source row `y` of src (uint8 interleaved, `pitch` pixels per row,
// `src_bytes` in the whole buffer), columns x0 .. x0 + in_w -> output pixels [t * tile, (t + 1) * tile) of orow (uint8 [out_w, 3]).
// Taps are relative to x0 and clamp at in_w.  The bytes of the row the tile's taps touch are staged in `stage` (LDS, STAGE_BYTES,
// 16-byte aligned) with 16-byte loads (vec: src 16-byte aligned; they stop at src_bytes) and every thread resamples one output pixel
// (3 channels) from there.  Table entries are clamped to the staged range, so a wrong table cannot make the kernel read outside the
// rectangle.  Ends with a barrier: the caller may stage the next item at once.
__device__ __forceinline__ void pil_hpass_item(const uint8_t* src, int64_t src_bytes, int pitch, int x0, int y, int in_w,
                                               const int* __restrict__ bounds, const int* __restrict__ weights, int stride, uint8_t* orow,
                                               int out_w, int tile, int t, bool vec, uint8_t* stage) {
  const int xo0 = t * tile, xo1 = min(out_w, xo0 + tile);
  int xs = bounds[2 * xo0], xe = bounds[2 * (xo1 - 1)] + bounds[2 * (xo1 - 1) + 1];
  xs = max(0, min(xs, in_w));
  xe = max(xs, min(xe, in_w));
  const int64_t b0 = ((int64_t)y * pitch + x0 + xs) * 3;                  // first byte of the segment in src
  const int64_t a0 = vec ? (b0 & ~(int64_t)15) : b0;
  const int head = (int)(b0 - a0);
  const int span = min((xe - xs) * 3, STAGE_BYTES - 16 - head);           // (the host sized `tile` so that this never cuts)
  if (vec) {
    const int nvec = (head + span + 15) >> 4;
    for (int v = threadIdx.x; v < nvec; v += 256) {
      const int64_t off = a0 + (int64_t)v * 16;
      if (off + 16 <= src_bytes) {
        *reinterpret_cast<uint4*>(stage + v * 16) = *reinterpret_cast<const uint4*>(src + off);
      } else {
        for (int b = 0; b < 16; ++b) stage[v * 16 + b] = off + b < src_bytes ? src[off + b] : (uint8_t)0;
      }
    }
  } else {
    for (int b = threadIdx.x; b < span; b += 256) stage[b] = src[a0 + b];
  }
  __syncthreads();
  const int xo = xo0 + threadIdx.x;
  if (xo < xo1) {
    int xmin = bounds[2 * xo], cnt = bounds[2 * xo + 1];
    xmin = max(xs, min(xmin, xe));
    cnt = max(0, min(min(cnt, stride), min(xe - xmin, (span - (xmin - xs) * 3) / 3)));
    const int* k = weights + (int64_t)xo * stride;
    const uint8_t* p = stage + head + (xmin - xs) * 3;
    int r = 1 << (PRECISION_BITS - 1), g = r, b = r;
    for (int j = 0; j < cnt; ++j) {
      const int w = k[j];
      r += (int)p[3 * j] * w; g += (int)p[3 * j + 1] * w; b += (int)p[3 * j + 2] * w;
    }
    uint8_t* o = orow + (int64_t)xo * 3;
    o[0] = clip8(r); o[1] = clip8(g); o[2] = clip8(b);
  }
  __syncthreads();
}

// Vertical passes: the taps of output row yo -- first source row and tap count, clamped to the in_h rows that are there -- and its weights
__device__ __forceinline__ const int* pil_vtaps(const int* __restrict__ bounds, const int* __restrict__ weights, int stride, int in_h, int yo,
                                                int* ymin, int* cnt) {
  const int y = max(0, min(bounds[2 * yo], in_h));
  *ymin = y;
  *cnt = max(0, min(min(bounds[2 * yo + 1], stride), in_h - y));
  return weights + (int64_t)yo * stride;
}
// acc[e] = the rounding half + sum over the cnt tap rows (p, p + row_bytes, ...) of byte e * tap.  N = 12: four neighbouring pixels x 3
// channels read as three words (p 4-byte aligned); N = 3: one pixel, byte loads -- for widths that are no multiple of 4
template <int N> __device__ __forceinline__ void pil_vacc(const uint8_t* p, int64_t row_bytes, const int* k, int cnt, int (&acc)[N]) {
  static_assert(N == 12 || N == 3, "pil_vacc");
#pragma unroll
  for (int e = 0; e < N; ++e) acc[e] = 1 << (PRECISION_BITS - 1);
  for (int j = 0; j < cnt; ++j, p += row_bytes) {
    const int w = k[j];
    if constexpr (N == 12) {
      const uint32_t* p4 = reinterpret_cast<const uint32_t*>(p);
      const uint32_t w0 = p4[0], w1 = p4[1], w2 = p4[2];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc[e] += (int)((w0 >> (8 * e)) & 255u) * w;
        acc[4 + e] += (int)((w1 >> (8 * e)) & 255u) * w;
        acc[8 + e] += (int)((w2 >> (8 * e)) & 255u) * w;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 3; ++e) acc[e] += (int)p[e] * w;
    }
  }
}
// ToTensor of such sums into the three planes at o: float(u8) / 255 is a correctly rounded division, not x * (1 / 255).  acc[e] is byte e
// of the run: source pixel e / 3, channel e % 3.  N = 12: one 16-byte store per plane (o 16-byte aligned), the four pixels in reverse
// order when `mirror`
template <int N> __device__ __forceinline__ void pil_store_planes(float* o, int64_t plane, const int (&acc)[N], bool mirror) {
  float v[N];
#pragma unroll
  for (int e = 0; e < N; ++e) v[e] = (float)clip8(acc[e]) / 255.0f;
  if constexpr (N == 12) {
    if (mirror) {
#pragma unroll
      for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(o + c * plane) = make_float4(v[9 + c], v[6 + c], v[3 + c], v[c]);
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(o + c * plane) = make_float4(v[c], v[3 + c], v[6 + c], v[9 + c]);
    }
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c * plane] = v[c];
  }
}
