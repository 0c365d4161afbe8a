// 4:2:0 decoder surfaces (NV12, NV21, I420, P010) -> packed 8-bit RGB [H, W, 3] (include/countr_hip_yuv.h states the rule).
//   countr_yuv_to_rgb   n <= 16 frames of one shape -> rgb[j], one launch
// The launch:
//   yuv_kernel<format, linear>  a thread per 16 luma columns x 2 luma rows (the two rows of one chroma row), a block of 64 x 4 threads, a
//                       grid plane per frame.  Bandwidth work: a thread reads its chroma row once for both luma rows (plus, under LINEAR,
//                       the row above for the even and the row below for the odd luma row, and one sample to the right), 16 bytes of Y
//                       per row (32 for P010) and writes 48 bytes of RGB per row.  `vin` (every plane 16-byte aligned, both pitches
//                       multiples of 16): 16-byte loads (8-byte for the two I420 chroma planes) for every thread whose 16 columns lie
//                       inside the frame; the last thread of a row whose width is no multiple of 16 loads element-wise, clamped to
//                       the last column.  `vout` = 2 (rgb 16-byte aligned, W a multiple of 16): three 16-byte stores per row; 1 (rgb
//                       4-byte aligned, W a multiple of 4, a 1080-wide portrait frame for one): 4-byte stores; 0: byte stores behind
//                       x < W.  Both flags are uniform over the launch.  No LDS, no atomics.
#include <stdio.h>
#include <string.h>
#include "../csrc/common.hpp"
#include "../csrc/host_api.hpp"
#include "../../include/countr_hip_yuv.h"

namespace {

constexpr int MAXF = COUNTR_YUV_MAX_FRAMES;
constexpr int PX = 16, NC = PX / 2;                              // luma columns / chroma samples of a thread
constexpr int BX = 64, BY = 4;                                   // a block: 64 threads along a row x 4 chroma rows

struct YuvArgs {
  const uint8_t* y[MAXF];
  const uint8_t* c0[MAXF];
  const uint8_t* c1[MAXF];
  uint8_t* rgb[MAXF];
  int H, W, Hc, Wc, pitch_y, pitch_c;
  int cy, yoff, rv, gu, gv, bu;
  int vin, vout;
};

// 16 luma samples of a row from column x0; element-wise the column is clamped to W - 1 (the clamped values are never stored)
template <int FMT>
__device__ __forceinline__ void load_y(const uint8_t* __restrict__ row, int x0, int W, bool vec, int (&Y)[PX]) {
  if (vec) {
    if constexpr (FMT == COUNTR_YUV_P010) {
      const uint4 a = *reinterpret_cast<const uint4*>(row + 2 * x0), b = *reinterpret_cast<const uint4*>(row + 2 * x0 + 16);
      const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        Y[2 * k] = (int)((w[k] & 0xffffu) >> 6);
        Y[2 * k + 1] = (int)(w[k] >> 22);
      }
    } else {
      const uint4 a = *reinterpret_cast<const uint4*>(row + x0);
      const uint32_t w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
      for (int k = 0; k < PX; ++k) Y[k] = (int)((w[k >> 2] >> (8 * (k & 3))) & 255u);
    }
  } else {
#pragma unroll
    for (int k = 0; k < PX; ++k) {
      const int x = min(x0 + k, W - 1);
      if constexpr (FMT == COUNTR_YUV_P010) Y[k] = (int)(*reinterpret_cast<const uint16_t*>(row + 2 * x) >> 6);
      else Y[k] = (int)row[x];
    }
  }
}

// chroma sample i of a chroma row (r0: the interleaved plane or U, r1: V of I420)
template <int FMT>
__device__ __forceinline__ void sample_c(const uint8_t* __restrict__ r0, const uint8_t* __restrict__ r1, int i, int& u, int& v) {
  if constexpr (FMT == COUNTR_YUV_NV12) { u = r0[2 * i]; v = r0[2 * i + 1]; }
  else if constexpr (FMT == COUNTR_YUV_NV21) { v = r0[2 * i]; u = r0[2 * i + 1]; }
  else if constexpr (FMT == COUNTR_YUV_I420) { u = r0[i]; v = r1[i]; }
  else {
    const uint16_t* p = reinterpret_cast<const uint16_t*>(r0 + 4 * i);
    u = p[0] >> 6; v = p[1] >> 6;
  }
}

// chroma samples i0 .. i0 + 8 of a chroma row, each index clamped to Wc - 1; the ninth is read only when `ninth` (LINEAR needs it)
template <int FMT>
__device__ __forceinline__ void load_c(const uint8_t* __restrict__ r0, const uint8_t* __restrict__ r1, int i0, int Wc, bool vec, bool ninth,
                                       int (&U)[NC + 1], int (&V)[NC + 1]) {
  if (vec) {
    if constexpr (FMT == COUNTR_YUV_P010) {
      const uint4 a = *reinterpret_cast<const uint4*>(r0 + 4 * i0), b = *reinterpret_cast<const uint4*>(r0 + 4 * i0 + 16);
      const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        U[k] = (int)((w[k] & 0xffffu) >> 6);
        V[k] = (int)(w[k] >> 22);
      }
    } else if constexpr (FMT == COUNTR_YUV_I420) {
      const uint2 a = *reinterpret_cast<const uint2*>(r0 + i0), b = *reinterpret_cast<const uint2*>(r1 + i0);
      const uint32_t wu[2] = {a.x, a.y}, wv[2] = {b.x, b.y};
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        U[k] = (int)((wu[k >> 2] >> (8 * (k & 3))) & 255u);
        V[k] = (int)((wv[k >> 2] >> (8 * (k & 3))) & 255u);
      }
    } else {
      const uint4 a = *reinterpret_cast<const uint4*>(r0 + 2 * i0);
      const uint32_t w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        const int lo = (int)((w[k >> 1] >> (16 * (k & 1))) & 255u), hi = (int)((w[k >> 1] >> (16 * (k & 1) + 8)) & 255u);
        U[k] = FMT == COUNTR_YUV_NV12 ? lo : hi;
        V[k] = FMT == COUNTR_YUV_NV12 ? hi : lo;
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < NC; ++k) sample_c<FMT>(r0, r1, min(i0 + k, Wc - 1), U[k], V[k]);
  }
  U[NC] = V[NC] = 0;
  if (ninth) sample_c<FMT>(r0, r1, min(i0 + NC, Wc - 1), U[NC], V[NC]);
}

// one luma row of the thread: its 16 pixels from Y and the row's chroma (U, V: samples under NEAREST, the sums s[] of the rule under
// LINEAR), packed as 48 bytes and stored
template <int FMT, bool LINEAR>
__device__ __forceinline__ void emit_row(const YuvArgs& a, const int (&Y)[PX], const int (&U)[NC + 1], const int (&V)[NC + 1],
                                         uint8_t* __restrict__ dst, int x0) {
  constexpr int s = FMT == COUNTR_YUV_P010 ? 2 : 0;
  uint32_t o[12];
#pragma unroll
  for (int q = 0; q < 12; ++q) o[q] = 0u;
#pragma unroll
  for (int k = 0; k < PX; ++k) {
    const int i = k >> 1;
    int u, v;
    if constexpr (!LINEAR) { u = U[i]; v = V[i]; }
    else if ((k & 1) == 0) { u = (U[i] + 2) >> 2; v = (V[i] + 2) >> 2; }
    else { u = (U[i] + U[i + 1] + 4) >> 3; v = (V[i] + V[i + 1] + 4) >> 3; }
    const int c = a.cy * (Y[k] - (a.yoff << s)) + (128 << s), d = u - (128 << s), e = v - (128 << s);
    const uint32_t ch[3] = {clamp255((c + a.rv * e) >> (8 + s)), clamp255((c + a.gu * d + a.gv * e) >> (8 + s)),
                            clamp255((c + a.bu * d) >> (8 + s))};
#pragma unroll
    for (int t = 0; t < 3; ++t) o[(3 * k + t) >> 2] |= ch[t] << (8 * ((3 * k + t) & 3));
  }
  if (a.vout == 2) {
    uint4* p = reinterpret_cast<uint4*>(dst);
    p[0] = make_uint4(o[0], o[1], o[2], o[3]);
    p[1] = make_uint4(o[4], o[5], o[6], o[7]);
    p[2] = make_uint4(o[8], o[9], o[10], o[11]);
  } else if (a.vout == 1) {                                      // W % 4 == 0: the row's bytes from x0 on are whole 4-byte words
    uint32_t* p = reinterpret_cast<uint32_t*>(dst);
    const int nd = min(12, (3 * (a.W - x0)) >> 2);
#pragma unroll
    for (int q = 0; q < 12; ++q)
      if (q < nd) p[q] = o[q];
  } else {
#pragma unroll
    for (int k = 0; k < PX; ++k) {
      if (x0 + k < a.W) {
#pragma unroll
        for (int t = 0; t < 3; ++t) dst[3 * k + t] = (uint8_t)((o[(3 * k + t) >> 2] >> (8 * ((3 * k + t) & 3))) & 255u);
      }
    }
  }
}

template <int FMT, bool LINEAR>
__global__ __launch_bounds__(BX * BY) void yuv_kernel(const YuvArgs a) {
  const int x0 = (blockIdx.x * BX + threadIdx.x) * PX;
  const int j = blockIdx.y * BY + threadIdx.y;                   // the chroma row; luma rows 2 j and 2 j + 1
  if (x0 >= a.W || j >= a.Hc) return;
  const int f = blockIdx.z, i0 = x0 >> 1;
  const bool vec = a.vin && x0 + PX <= a.W;                      // (then i0 + 8 <= Wc: the chroma loads stay inside the row as well)
  const uint8_t* c0 = a.c0[f];
  const uint8_t* c1 = FMT == COUNTR_YUV_I420 ? a.c1[f] : a.c0[f];
  const int64_t cj = (int64_t)j * a.pitch_c;
  int U[NC + 1], V[NC + 1];
  load_c<FMT>(c0 + cj, c1 + cj, i0, a.Wc, vec, LINEAR, U, V);
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int y = 2 * j + r;
    if (y >= a.H) break;                                         // (an odd H: the last chroma row serves one luma row)
    int Y[PX];
    load_y<FMT>(a.y[f] + (int64_t)y * a.pitch_y, x0, a.W, vec, Y);
    uint8_t* dst = a.rgb[f] + ((int64_t)y * a.W + x0) * 3;
    if constexpr (LINEAR) {
      const int jn = r ? min(j + 1, a.Hc - 1) : max(j - 1, 0);
      const int64_t cn = (int64_t)jn * a.pitch_c;
      int Un[NC + 1], Vn[NC + 1];
      load_c<FMT>(c0 + cn, c1 + cn, i0, a.Wc, vec, true, Un, Vn);
#pragma unroll
      for (int k = 0; k <= NC; ++k) {
        Un[k] = 3 * U[k] + Un[k];
        Vn[k] = 3 * V[k] + Vn[k];
      }
      emit_row<FMT, true>(a, Y, Un, Vn, dst, x0);
    } else {
      emit_row<FMT, false>(a, Y, U, V, dst, x0);
    }
  }
}

// cy, yoff, rv, gu, gv, bu of [matrix][range] (the header's table)
const int COEF[2][2][6] = {{{298, 16, 409, -100, -208, 516}, {256, 0, 359, -88, -183, 454}},
                           {{298, 16, 459, -55, -136, 541}, {256, 0, 403, -48, -120, 475}}};

template <int FMT>
void launch(bool linear, dim3 grid, hipStream_t st, const YuvArgs& a) {
  if (linear) hipLaunchKernelGGL((yuv_kernel<FMT, true>), grid, dim3(BX, BY), 0, st, a);
  else hipLaunchKernelGGL((yuv_kernel<FMT, false>), grid, dim3(BX, BY), 0, st, a);
}

}  // namespace

extern "C" int countr_yuv_version(void) { return COUNTR_YUV_ABI_VERSION; }

extern "C" const char* countr_yuv_last_error(void) { return g_err; }

extern "C" int countr_yuv_to_rgb(const void* const* y, const void* const* c0, const void* const* c1, void* const* rgb, int n, int H, int W,
                                 int pitch_y, int pitch_c, int format, int matrix, int range, int chroma, void* stream) {
  if (n < 1 || n > MAXF) return failf(-1, "countr_yuv_to_rgb: 1..%d frames a call, got %d", MAXF, n);
  if (format < COUNTR_YUV_NV12 || format > COUNTR_YUV_P010) return failf(-1, "countr_yuv_to_rgb: unknown format %d", format);
  if (matrix != COUNTR_YUV_BT601 && matrix != COUNTR_YUV_BT709) return failf(-1, "countr_yuv_to_rgb: unknown matrix %d", matrix);
  if (range != COUNTR_YUV_LIMITED && range != COUNTR_YUV_FULL) return failf(-1, "countr_yuv_to_rgb: unknown range %d", range);
  if (chroma != COUNTR_YUV_NEAREST && chroma != COUNTR_YUV_LINEAR)
    return failf(-1, "countr_yuv_to_rgb: unknown chroma reconstruction %d", chroma);
  if (H < 1 || H > COUNTR_YUV_MAX_SIDE || W < 1 || W > COUNTR_YUV_MAX_SIDE)
    return failf(-1, "countr_yuv_to_rgb: H and W are 1..%d, got %d x %d", COUNTR_YUV_MAX_SIDE, H, W);
  const bool wide = format == COUNTR_YUV_P010;
  const int Hc = (H + 1) / 2, Wc = (W + 1) / 2;
  const int row_y = W * (wide ? 2 : 1);
  const int row_c = format == COUNTR_YUV_I420 ? Wc : 2 * Wc * (wide ? 2 : 1);
  if (pitch_y < row_y || (wide && (pitch_y & 1)))
    return failf(-1, "countr_yuv_to_rgb: pitch_y %d: a Y row has %d bytes%s", pitch_y, row_y, wide ? " and a P010 pitch is even" : "");
  if (pitch_c < row_c || (wide && (pitch_c & 1)))
    return failf(-1, "countr_yuv_to_rgb: pitch_c %d: a chroma row has %d bytes%s", pitch_c, row_c,
                 wide ? " and a P010 pitch is even" : "");
  if (!y || !c0 || !rgb) return fail(-1, "countr_yuv_to_rgb: the pointer arrays y, c0 and rgb are required");
  if (format == COUNTR_YUV_I420 && !c1) return fail(-1, "countr_yuv_to_rgb: c1 (the V planes) is required for I420");
  if (format != COUNTR_YUV_I420 && c1) return fail(-1, "countr_yuv_to_rgb: c1 must be NULL unless the format is I420");
  YuvArgs a;
  memset(&a, 0, sizeof(a));
  uintptr_t bits_in = (uintptr_t)pitch_y | (uintptr_t)pitch_c, bits_out = (uintptr_t)W;
  for (int j = 0; j < n; ++j) {
    if (!y[j] || !c0[j] || !rgb[j] || (c1 && !c1[j])) return failf(-1, "countr_yuv_to_rgb: frame %d has a null pointer", j);
    const uintptr_t in = (uintptr_t)y[j] | (uintptr_t)c0[j] | (c1 ? (uintptr_t)c1[j] : 0);
    if (wide && (in & 1)) return failf(-1, "countr_yuv_to_rgb: frame %d: a P010 plane is 2-byte aligned", j);
    bits_in |= in;
    bits_out |= (uintptr_t)rgb[j];
    a.y[j] = (const uint8_t*)y[j];
    a.c0[j] = (const uint8_t*)c0[j];
    a.c1[j] = c1 ? (const uint8_t*)c1[j] : nullptr;
    a.rgb[j] = (uint8_t*)rgb[j];
  }
  a.H = H; a.W = W; a.Hc = Hc; a.Wc = Wc; a.pitch_y = pitch_y; a.pitch_c = pitch_c;
  const int* k = COEF[matrix][range];
  a.cy = k[0]; a.yoff = k[1]; a.rv = k[2]; a.gu = k[3]; a.gv = k[4]; a.bu = k[5];
  a.vin = (bits_in & 15) == 0;
  a.vout = (bits_out & 15) == 0 ? 2 : (bits_out & 3) == 0 ? 1 : 0;
  const int tx = (W + PX - 1) / PX;
  const dim3 grid((unsigned)((tx + BX - 1) / BX), (unsigned)((Hc + BY - 1) / BY), (unsigned)n);      // <= 16 x 2048 x 16
  const bool linear = chroma == COUNTR_YUV_LINEAR;
  if (format == COUNTR_YUV_NV12) launch<COUNTR_YUV_NV12>(linear, grid, STREAM(stream), a);
  else if (format == COUNTR_YUV_NV21) launch<COUNTR_YUV_NV21>(linear, grid, STREAM(stream), a);
  else if (format == COUNTR_YUV_I420) launch<COUNTR_YUV_I420>(linear, grid, STREAM(stream), a);
  else launch<COUNTR_YUV_P010>(linear, grid, STREAM(stream), a);
  return launched("countr_yuv_to_rgb");
}
