// The camera's own motion from the flow library's motion field (include/countr_hip_cam.h states the rule).
//   countr_cam_workspace    (host only) bytes of scratch an estimate call needs
//   countr_cam_estimate     n <= 16 (motion field, current luma) pairs -> records int32 [n, 8] and the cells' texture flags
//   countr_cam_compensate   n <= 16 fields minus the records' g -> compensated fields (in place or not)
// The launches, all on the caller's stream (the estimate clears its histograms with a memset on the stream first):
//   cam_texture_kernel      a block per cell row of a field.  A thread takes a pixel column of the cell row: nine rows of bytes, the column's
//                           sum of the two absolute differences; eight neighbouring lanes are a cell and add up by three xor-shuffles.  The
//                           cell's first lane writes the flag and, if the cell votes, adds one to the block's two histograms in LDS; the
//                           block's non-empty bins then go to the field's histograms with integer atomics -- under a pan nearly all of a
//                           row's voters share a bin, so a block sends a handful of atomics, not one per cell.
//   cam_record_kernel       a block per field: per axis a thread takes three bins, a wave-level inclusive scan and the four waves' totals
//                           give every thread the rank range of its bins, and the one thread whose range holds rank ceil(n / 2) names the
//                           median.  The inliers are counted over the field's cells and the record is written by thread 0.
//   cam_compensate_kernel   a thread per cell; it reads its own cell before it writes it, so out may be the field itself
// Integer sums only: no result depends on the order the atomics land in.
#include <stdio.h>
#include <string.h>
#include "../csrc/common.hpp"
#include "../csrc/host_api.hpp"
#include "../../include/countr_hip_cam.h"

namespace {

constexpr int MAXF = COUNTR_CAM_MAX_FRAMES, CELL = COUNTR_CAM_CELL, MAX_SIDE = COUNTR_CAM_MAX_SIDE;
constexpr int R = COUNTR_CAM_RANGE, BINS = COUNTR_CAM_BINS, REC = COUNTR_CAM_RECORD_INTS;
constexpr int THREADS = 256, WAVES = THREADS / 64, PER = 3;      // a thread of the scan takes PER bins
static_assert(BINS == 2 * R + 1 && BINS <= THREADS * PER, "the scan covers every bin");
static_assert(CELL == 8, "a cell is eight lanes: three xor-shuffles");

struct EstimateArgs {
  const unsigned* mv[MAXF];                      // an int16 pair (x, y) as one word
  const unsigned char* luma[MAXF];
};

struct CompensateArgs {
  const unsigned* mv[MAXF];
  unsigned* out[MAXF];
};

__device__ __forceinline__ int lo16(unsigned v) { return (int)(short)(v & 0xFFFFu); }
__device__ __forceinline__ int hi16(unsigned v) { return (int)(short)(v >> 16); }
__device__ __forceinline__ int absdiff(int a, int b) { return a > b ? a - b : b - a; }
__device__ __forceinline__ bool in_range(int ox, int oy) { return ox >= -R && ox <= R && oy >= -R && oy <= R; }

__global__ __launch_bounds__(THREADS) void cam_texture_kernel(const EstimateArgs a, unsigned char* __restrict__ flags, int* __restrict__ hist,
                                                              int h, int w, unsigned min_texture) {
  __shared__ int s_hist[2 * BINS];
  const int j = blockIdx.x, f = blockIdx.y, Wc = w >> 3, Hc = h >> 3;
  const unsigned char* __restrict__ L = a.luma[f];
  const unsigned* __restrict__ mv = a.mv[f] + (int64_t)j * Wc;
  unsigned char* __restrict__ fl = flags + ((int64_t)f * Hc + j) * Wc;
  for (int b = threadIdx.x; b < 2 * BINS; b += THREADS) s_hist[b] = 0;
  __syncthreads();
  for (int c0 = 0; c0 < w; c0 += THREADS) {      // (block-uniform: every lane takes the shuffles)
    const int x = c0 + threadIdx.x;
    int col = 0;
    if (x < w) {
      const int xr = x + 1 < w ? x + 1 : w - 1;
      const unsigned char* p = L + (int64_t)CELL * j * w;
      int here = p[x];
#pragma unroll
      for (int row = 0; row < CELL; ++row) {
        const int y = CELL * j + row;
        const int right = p[xr];
        const unsigned char* q = y + 1 < h ? p + w : p;
        const int below = q[x];
        col += absdiff(right, here) + absdiff(below, here);
        here = below;
        p = q;
      }
    }
    // w is a multiple of 8 and so is c0: the eight lanes of a cell are all inside the image or all outside
    col += __shfl_xor(col, 1);
    col += __shfl_xor(col, 2);
    col += __shfl_xor(col, 4);
    if (x < w && (threadIdx.x & 7) == 0) {
      const int i = x >> 3;
      const bool textured = (unsigned)col >= min_texture;
      fl[i] = textured ? 1 : 0;
      const unsigned v = mv[i];
      const int ox = lo16(v), oy = hi16(v);
      if (textured && in_range(ox, oy)) {        // (an offset outside [-R, R] never indexes a histogram)
        atomicAdd(&s_hist[ox + R], 1);
        atomicAdd(&s_hist[BINS + oy + R], 1);
      }
    }
  }
  __syncthreads();
  int* __restrict__ H = hist + (int64_t)f * 2 * BINS;
  for (int b = threadIdx.x; b < 2 * BINS; b += THREADS) {
    const int c = s_hist[b];
    if (c) atomicAdd(&H[b], c);
  }
}

__global__ __launch_bounds__(THREADS) void cam_record_kernel(const EstimateArgs a, const unsigned char* __restrict__ flags,
                                                             const int* __restrict__ hist, int* __restrict__ records, int cells, int tol,
                                                             int min_voters) {
  __shared__ int s_wave[WAVES];
  __shared__ int s_g[2];
  __shared__ int s_in[WAVES];
  const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int* __restrict__ H = hist + (int64_t)f * 2 * BINS;
  int n = 0;
  for (int axis = 0; axis < 2; ++axis) {
    int c[PER], mine = 0;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int b = tid * PER + q;
      c[q] = b < BINS ? H[axis * BINS + b] : 0;
      mine += c[q];
    }
    int inc = wave_scan_incl_i(mine);
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int v = 0; v < WAVES; ++v) {
      if (v < wave) inc += s_wave[v];
      total += s_wave[v];
    }
    n = total;                                   // (both axes count the same voters)
    const int rank = (total + 1) >> 1, exc = inc - mine;
    if (total == 0) {
      if (tid == 0) s_g[axis] = 0;
    } else if (exc < rank && rank <= inc) {      // exactly one thread: the ranges (exc, inc] tile 1 .. total
      int left = rank - exc, q = 0;
      while (left > c[q]) left -= c[q++];        // (ends inside the thread's bins: left <= mine)
      s_g[axis] = tid * PER + q - R;
    }
    __syncthreads();                             // (s_g is written; s_wave may be written again)
  }
  const int gx = s_g[0], gy = s_g[1];
  const unsigned* __restrict__ mv = a.mv[f];
  const unsigned char* __restrict__ fl = flags + (int64_t)f * cells;
  int in = 0;
  for (int k = tid; k < cells; k += THREADS) {
    const unsigned v = mv[k];
    const int ox = lo16(v), oy = hi16(v);
    if (fl[k] && in_range(ox, oy) && absdiff(ox, gx) <= tol && absdiff(oy, gy) <= tol) ++in;
  }
  in = wave_sum_i(in);
  if (lane == 0) s_in[wave] = in;
  __syncthreads();
  if (tid == 0) {
    int inliers = 0;
#pragma unroll
    for (int v = 0; v < WAVES; ++v) inliers += s_in[v];
    const bool valid = n >= min_voters && 2 * (int64_t)inliers >= n;
    int* __restrict__ rec = records + (int64_t)f * REC;
    rec[0] = valid ? gx : 0;
    rec[1] = valid ? gy : 0;
    rec[2] = n;
    rec[3] = inliers;
    rec[4] = valid ? 1 : 0;
    rec[5] = cells;
    rec[6] = 0;
    rec[7] = 0;
  }
}

__device__ __forceinline__ int sat16(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

__global__ __launch_bounds__(THREADS) void cam_compensate_kernel(const CompensateArgs a, const int* __restrict__ records,
                                                                 const unsigned char* __restrict__ flags, int cells) {
  const int f = blockIdx.y;
  const int gx = records[(int64_t)f * REC], gy = records[(int64_t)f * REC + 1];
  const unsigned* mv = a.mv[f];                  // (no __restrict__: out may be the field)
  unsigned* out = a.out[f];
  const unsigned char* __restrict__ fl = flags + (int64_t)f * cells;
  for (int k = blockIdx.x * THREADS + threadIdx.x; k < cells; k += gridDim.x * THREADS) {
    const unsigned v = mv[k];
    unsigned o = 0u;
    if (v != 0u || fl[k]) {
      const int x = sat16(lo16(v) - gx), y = sat16(hi16(v) - gy);
      o = ((unsigned)x & 0xFFFFu) | ((unsigned)y << 16);
    }
    out[k] = o;
  }
}

inline bool bad_side(int v) { return v < CELL || v > MAX_SIDE || v % CELL != 0; }

// the checks every call shares: the count and the sizes
int check_sizes(const char* who, int n, int h, int w) {
  if (n < 1 || n > MAXF) return failf(-1, "%s: 1..%d frames a call, got %d", who, MAXF, n);
  if (bad_side(h) || bad_side(w))
    return failf(-3, "%s: h and w are multiples of %d in %d..%d, got %d x %d", who, CELL, CELL, MAX_SIDE, h, w);
  return 0;
}

}  // namespace

extern "C" int countr_cam_version(void) { return COUNTR_CAM_ABI_VERSION; }

extern "C" const char* countr_cam_last_error(void) { return g_err; }

extern "C" int countr_cam_workspace(int n, int h, int w) {
  const int rc = check_sizes("countr_cam_workspace", n, h, w);
  if (rc) return rc;
  return n * 2 * BINS * 4;
}

extern "C" int countr_cam_estimate(const void* const* fields, const void* const* lumas, void* records, void* flags, int n, int h, int w,
                                   int min_texture, int tol, int min_voters, void* workspace, void* stream) {
  const int rc = check_sizes("countr_cam_estimate", n, h, w);
  if (rc) return rc;
  if (min_texture < 0) return failf(-3, "countr_cam_estimate: min_texture is >= 0, got %d", min_texture);
  if (tol < 0) return failf(-3, "countr_cam_estimate: tol is >= 0, got %d", tol);
  if (min_voters < 1) return failf(-3, "countr_cam_estimate: min_voters is >= 1, got %d", min_voters);
  if (!fields || !lumas) return fail(-2, "countr_cam_estimate: the fields and lumas arrays are required");
  if (!records || misaligned(records, 4)) return fail(-2, "countr_cam_estimate: the records are required and 4-byte aligned");
  if (!flags) return fail(-2, "countr_cam_estimate: the flags are required");
  if (!workspace || misaligned(workspace, 4)) return fail(-2, "countr_cam_estimate: the workspace is required and 4-byte aligned");
  EstimateArgs a;
  memset(&a, 0, sizeof(a));
  for (int k = 0; k < n; ++k) {
    if (!fields[k] || !lumas[k]) return failf(-2, "countr_cam_estimate: pair %d has a null pointer", k);
    if (misaligned(fields[k], 4)) return failf(-5, "countr_cam_estimate: pair %d: the motion field is 4-byte aligned", k);
    a.mv[k] = (const unsigned*)fields[k];
    a.luma[k] = (const unsigned char*)lumas[k];
  }
  const int Hc = h / CELL, cells = Hc * (w / CELL);
  const hipError_t e = hipMemsetAsync(workspace, 0, (size_t)n * 2 * BINS * 4, STREAM(stream));
  if (e != hipSuccess) return failf(-10, "countr_cam_estimate: clearing the workspace failed: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(cam_texture_kernel, dim3(Hc, n), dim3(THREADS), 0, STREAM(stream), a, (unsigned char*)flags, (int*)workspace, h, w,
                     (unsigned)min_texture);
  hipLaunchKernelGGL(cam_record_kernel, dim3(n), dim3(THREADS), 0, STREAM(stream), a, (const unsigned char*)flags, (const int*)workspace,
                     (int*)records, cells, tol, min_voters);
  return launched("countr_cam_estimate");
}

extern "C" int countr_cam_compensate(const void* const* fields, const void* records, const void* flags, void* const* out_fields, int n,
                                     int h, int w, void* stream) {
  const int rc = check_sizes("countr_cam_compensate", n, h, w);
  if (rc) return rc;
  if (!fields || !out_fields) return fail(-2, "countr_cam_compensate: the fields and out_fields arrays are required");
  if (!records || misaligned(records, 4)) return fail(-2, "countr_cam_compensate: the records are required and 4-byte aligned");
  if (!flags) return fail(-2, "countr_cam_compensate: the flags are required");
  CompensateArgs a;
  memset(&a, 0, sizeof(a));
  for (int k = 0; k < n; ++k) {
    if (!fields[k] || !out_fields[k]) return failf(-2, "countr_cam_compensate: field %d has a null pointer", k);
    if (misaligned(fields[k], 4) || misaligned(out_fields[k], 4))
      return failf(-5, "countr_cam_compensate: field %d: the field and its output are 4-byte aligned", k);
    a.mv[k] = (const unsigned*)fields[k];
    a.out[k] = (unsigned*)out_fields[k];
  }
  const int cells = (h / CELL) * (w / CELL);
  hipLaunchKernelGGL(cam_compensate_kernel, dim3(countr_blocks_for(cells, THREADS), n), dim3(THREADS), 0, STREAM(stream), a,
                     (const int*)records, (const unsigned char*)flags, cells);
  return launched("countr_cam_compensate");
}
