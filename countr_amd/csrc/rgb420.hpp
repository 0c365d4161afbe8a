// What the libraries that draw on packed RGB frames share (csrc_overlay/overlay.hip, csrc_draw/draw.hip): the rounded division of the
// line rule, a thread's 16 pixels of a row, and the RGB -> 4:2:0 conversion, step 5 of include/countr_hip_overlay.h, stated once.
// Everything is in an anonymous namespace, so every library that includes this has kernels of its own.
#pragma once
#include "common.hpp"

namespace {

constexpr int PX = 16;                                            // columns of a thread
constexpr int BX = 64, BY = 4;                                    // a block: 64 threads along a row x 4 row pairs
constexpr int RGB420_NV12 = 1, RGB420_NV21 = 2, RGB420_I420 = 3;  // the 4:2:0 formats, the numbers of the headers that name them

// n <= 16 finished RGB frames uint8 [H, W, 3] and the packed 4:2:0 buffer of each; vec: every pointer 16-byte aligned and W a multiple of 16
struct Rgb420Args {
  const uint8_t* src[16];
  uint8_t* dst[16];
  int H, W, vec;
  int yr, yg, yb, yoff, ur, ug, ub, vr, vg, vb;
};

// yr, yg, yb, yoff, ur, ug, ub, vr, vg, vb of [matrix][range] (the table of include/countr_hip_overlay.h)
const int COEF[2][2][10] = {{{66, 129, 25, 16, -38, -74, 112, 112, -94, -18}, {77, 150, 29, 0, -43, -85, 128, 128, -107, -21}},
                            {{47, 157, 16, 16, -26, -86, 112, 112, -102, -10}, {54, 184, 18, 0, -29, -99, 128, 128, -116, -12}}};

inline void set_coefficients(Rgb420Args& a, int matrix, int range) {
  const int* k = COEF[matrix][range];
  a.yr = k[0]; a.yg = k[1]; a.yb = k[2]; a.yoff = k[3]; a.ur = k[4]; a.ug = k[5]; a.ub = k[6]; a.vr = k[7]; a.vg = k[8]; a.vb = k[9];
}

// floor((2 a + n) / (2 n)), n > 0
__device__ __forceinline__ int64_t rdiv(int64_t v, int64_t n) {
  const int64_t num = 2 * v + n, den = 2 * n;
  int64_t q = num / den;
  if (num % den < 0) --q;
  return q;
}

// 16 pixels of a row from column x0 as 12 words; element-wise the column is clamped to W - 1
__device__ __forceinline__ void load_px(const uint8_t* __restrict__ row, int x0, int W, bool vec, uint32_t (&o)[12]) {
  if (vec) {
    const uint4* p = reinterpret_cast<const uint4*>(row + 3 * x0);
    const uint4 u = p[0], v = p[1], w = p[2];
    o[0] = u.x; o[1] = u.y; o[2] = u.z; o[3] = u.w; o[4] = v.x; o[5] = v.y; o[6] = v.z; o[7] = v.w;
    o[8] = w.x; o[9] = w.y; o[10] = w.z; o[11] = w.w;
  } else {
#pragma unroll
    for (int q = 0; q < 12; ++q) o[q] = 0u;
#pragma unroll
    for (int k = 0; k < PX; ++k) {
      const uint8_t* p = row + 3 * (int64_t)min(x0 + k, W - 1);
#pragma unroll
      for (int t = 0; t < 3; ++t) o[(3 * k + t) >> 2] |= (uint32_t)p[t] << (8 * ((3 * k + t) & 3));
    }
  }
}

__device__ __forceinline__ uint32_t byte_of(const uint32_t (&o)[12], int b) { return (o[b >> 2] >> (8 * (b & 3))) & 255u; }

// step 5 from the finished RGB: a thread per 16 columns x 2 rows = 8 chroma samples; `vec`: 16-byte Y stores and 16-byte (NV12 / NV21)
// or two 8-byte (I420) chroma stores
template <int FMT>
__global__ __launch_bounds__(BX * BY) void yuv_kernel(const Rgb420Args a) {
  const int x0 = (blockIdx.x * BX + threadIdx.x) * PX;
  const int j = blockIdx.y * BY + threadIdx.y;                    // the chroma row; luma rows 2 j and 2 j + 1
  const int Hc = (a.H + 1) >> 1, Wc = (a.W + 1) >> 1;
  if (x0 >= a.W || j >= Hc) return;
  const int f = blockIdx.z;
  const bool vec = a.vec != 0;
  const uint8_t* __restrict__ src = a.src[f];
  uint8_t* __restrict__ dst = a.dst[f];
  uint32_t o[2][12];
  load_px(src + (int64_t)(2 * j) * a.W * 3, x0, a.W, vec, o[0]);
  load_px(src + (int64_t)min(2 * j + 1, a.H - 1) * a.W * 3, x0, a.W, vec, o[1]);   // (an odd H: the last row again)
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int y = 2 * j + r;
    if (y >= a.H) break;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < PX; ++k) {
      const int R = (int)byte_of(o[r], 3 * k), G = (int)byte_of(o[r], 3 * k + 1), B = (int)byte_of(o[r], 3 * k + 2);
      const uint32_t Y = (uint32_t)(((a.yr * R + a.yg * G + a.yb * B + 128) >> 8) + a.yoff);
      w[k >> 2] |= Y << (8 * (k & 3));
    }
    uint8_t* yrow = dst + (int64_t)y * a.W;
    if (vec) {
      *reinterpret_cast<uint4*>(yrow + x0) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
      for (int k = 0; k < PX; ++k)
        if (x0 + k < a.W) yrow[x0 + k] = (uint8_t)((w[k >> 2] >> (8 * (k & 3))) & 255u);
    }
  }
  uint32_t U[PX / 2], V[PX / 2];
#pragma unroll
  for (int i = 0; i < PX / 2; ++i) {
    int s[3];
#pragma unroll
    for (int t = 0; t < 3; ++t)
      s[t] = (int)((byte_of(o[0], 6 * i + t) + byte_of(o[0], 6 * i + 3 + t) + byte_of(o[1], 6 * i + t) + byte_of(o[1], 6 * i + 3 + t) + 2u) >> 2);
    U[i] = clamp255(((a.ur * s[0] + a.ug * s[1] + a.ub * s[2] + 128) >> 8) + 128);
    V[i] = clamp255(((a.vr * s[0] + a.vg * s[1] + a.vb * s[2] + 128) >> 8) + 128);
  }
  const int i0 = x0 >> 1;
  uint8_t* c = dst + (int64_t)a.H * a.W;
  if constexpr (FMT == RGB420_I420) {
    uint8_t* urow = c + (int64_t)j * Wc;
    uint8_t* vrow = urow + (int64_t)Hc * Wc;
    if (vec) {
      uint32_t wu[2] = {0u, 0u}, wv[2] = {0u, 0u};
#pragma unroll
      for (int i = 0; i < PX / 2; ++i) {
        wu[i >> 2] |= U[i] << (8 * (i & 3));
        wv[i >> 2] |= V[i] << (8 * (i & 3));
      }
      *reinterpret_cast<uint2*>(urow + i0) = make_uint2(wu[0], wu[1]);
      *reinterpret_cast<uint2*>(vrow + i0) = make_uint2(wv[0], wv[1]);
    } else {
#pragma unroll
      for (int i = 0; i < PX / 2; ++i)
        if (i0 + i < Wc) { urow[i0 + i] = (uint8_t)U[i]; vrow[i0 + i] = (uint8_t)V[i]; }
    }
  } else {
    uint8_t* crow = c + (int64_t)j * 2 * Wc;
    if (vec) {
      uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int i = 0; i < PX / 2; ++i) {
        const uint32_t lo = FMT == RGB420_NV12 ? U[i] : V[i], hi = FMT == RGB420_NV12 ? V[i] : U[i];
        w[i >> 1] |= (lo | (hi << 8)) << (16 * (i & 1));
      }
      *reinterpret_cast<uint4*>(crow + 2 * i0) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
      for (int i = 0; i < PX / 2; ++i)
        if (i0 + i < Wc) {
          crow[2 * (i0 + i)] = (uint8_t)(FMT == RGB420_NV12 ? U[i] : V[i]);
          crow[2 * (i0 + i) + 1] = (uint8_t)(FMT == RGB420_NV12 ? V[i] : U[i]);
        }
    }
  }
}

// the grid of a thread per 16 columns x 2 rows, a plane per frame: <= 16 x 2048 x 16 blocks
inline dim3 rgb_grid(int H, int W, int n) {
  const int tx = (W + PX - 1) / PX, Hc = (H + 1) / 2;
  return dim3((unsigned)((tx + BX - 1) / BX), (unsigned)((Hc + BY - 1) / BY), (unsigned)n);
}

// the conversion of `n` frames on `st`; format is one of RGB420_NV12 / NV21 / I420, anything else launches nothing
inline void launch_rgb420(int format, const Rgb420Args& a, int n, hipStream_t st) {
  const dim3 grid = rgb_grid(a.H, a.W, n);
  if (format == RGB420_NV12) hipLaunchKernelGGL((yuv_kernel<RGB420_NV12>), grid, dim3(BX, BY), 0, st, a);
  else if (format == RGB420_NV21) hipLaunchKernelGGL((yuv_kernel<RGB420_NV21>), grid, dim3(BX, BY), 0, st, a);
  else if (format == RGB420_I420) hipLaunchKernelGGL((yuv_kernel<RGB420_I420>), grid, dim3(BX, BY), 0, st, a);
}

}  // namespace
