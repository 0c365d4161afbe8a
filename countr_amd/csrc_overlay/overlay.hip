// Annotated frames on the device (include/countr_hip_overlay.h states the rule).
//   countr_overlay_render   n <= 16 frames of one frame shape and one map shape -> out[j] (RGB) and, when asked for, yuv[j] (4:2:0)
// The launches, all on the caller's stream, each with a grid plane per frame:
//   max_kernel        only when a frame has gain_max: the largest value above 0 of its map as the bits of an fp32 (which order as
//                     unsigned integers do), one LDS atomicMax per thread and one global atomicMax per block into maxbits[j], zeroed by a
//                     memset node in front.  Integer atomics of a maximum: the result does not depend on the order.
//   compose_kernel    steps 1 to 3.  A thread per 16 columns x 2 rows, a block of 64 x 4 threads.  The block stages the colour table in LDS
//                     (256 threads, 256 entries) and the frame's gain (the division of gain_max is done once per block).  A thread works
//                     out the column index and weight of its 16 columns once, for both rows, and the row index and weight once per row.
//                     The block's 1024 columns x 8 rows read a rectangle of the map; when it has at most 8192 pixels (any upscale, and
//                     a downscale up to about 1 : 3) the block quantises it ONCE into LDS as bytes, with coalesced loads, and a pixel is
//                     four LDS byte reads, the integer interpolation, one LDS lookup and three blends.  A larger rectangle (a strong
//                     downscale) is not staged: a pixel is then four map loads and four quantisations.  The levels are the same.  `vec` (every rgb and out pointer 16-byte aligned, W a multiple of
//                     16): three 16-byte loads and three 16-byte stores per row; element-wise behind x < W otherwise.
//   label_kernel      a thread per patch pixel.   edge_kernel  a block per edge, a thread per pixel i of 0 .. n in strides of 256.
//   point_kernel      a block of 64 threads per point over the (2 r + 1)^2 box of its disc.
//                     Each kind is a launch of its own behind the composition, so a later kind overwrites an earlier one; within a kind
//                     every write carries the same bytes.
//   yuv_kernel<fmt>   step 5 from the finished RGB (csrc/rgb420.hpp, shared with csrc_draw/draw.hip): a thread per 16 columns x 2 rows =
//                     8 chroma samples; `vec` as above with the yuv pointers.
#include <stdio.h>
#include <string.h>
#include "../csrc/common.hpp"
#include "../csrc/host_api.hpp"
#include "../csrc/rgb420.hpp"
#include "../../include/countr_hip_overlay.h"

namespace {

constexpr int MAXF = COUNTR_OVERLAY_MAX_FRAMES;
static_assert(MAXF == 16 && COUNTR_OVERLAY_NV12 == RGB420_NV12 && COUNTR_OVERLAY_NV21 == RGB420_NV21 && COUNTR_OVERLAY_I420 == RGB420_I420,
              "csrc/rgb420.hpp converts up to 16 frames and names the formats by the header's numbers");
constexpr int STRIP = 8192;                                       // levels of the map a block of the composition stages in LDS
constexpr int COORD = 1 << 20;                                    // a mark's coordinates lie in -COORD .. COORD (the Python layer refuses others)

struct OvArgs {
  const uint8_t* rgb[MAXF];
  const float* map[MAXF];
  uint8_t* out[MAXF];
  int n_points[MAXF], points_off[MAXF], n_edges[MAXF], edges_off[MAXF];
  int lh[MAXF], lw[MAXF], lx[MAXF], ly[MAXF], patch_off[MAXF];
  const uint8_t* pack;
  uint32_t* maxbits;
  int H, W, mh, mw;
  uint32_t gain_max;                                              // bit j: frame j takes 255 / max(map)
  int vec;
  int radius, point_rgb, edge_rgb;
};

__device__ __forceinline__ uint32_t div255(uint32_t v) { return (v * 0x8081u) >> 23; }      // exact for v < 65536

__global__ __launch_bounds__(256) void max_kernel(const OvArgs a) {
  const int f = blockIdx.y;
  if (!((a.gain_max >> f) & 1u)) return;                          // (uniform over the block)
  __shared__ uint32_t s_max;
  if (threadIdx.x == 0) s_max = 0u;
  __syncthreads();
  const float* __restrict__ m = a.map[f];
  const int64_t total = (int64_t)a.mh * a.mw;
  uint32_t best = 0u;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const float v = m[i];
    if (v > 0.0f) best = max(best, __float_as_uint(v));           // (NaN fails the comparison; +inf is a value above 0)
  }
  if (best) atomicMax(&s_max, best);
  __syncthreads();
  if (threadIdx.x == 0 && s_max) atomicMax(&a.maxbits[f], s_max);
}

__device__ __forceinline__ void store_px(uint8_t* __restrict__ row, int x0, int W, bool vec, const uint32_t (&o)[12]) {
  if (vec) {
    uint4* p = reinterpret_cast<uint4*>(row + 3 * x0);
    p[0] = make_uint4(o[0], o[1], o[2], o[3]);
    p[1] = make_uint4(o[4], o[5], o[6], o[7]);
    p[2] = make_uint4(o[8], o[9], o[10], o[11]);
  } else {
#pragma unroll
    for (int k = 0; k < PX; ++k) {
      if (x0 + k < W) {
#pragma unroll
        for (int t = 0; t < 3; ++t) row[3 * (int64_t)(x0 + k) + t] = (uint8_t)byte_of(o, 3 * k + t);
      }
    }
  }
}

// step 2's index and weight of output coordinate c of `size` over a map side of `msize`
__device__ __forceinline__ void axis(int c, int size, int msize, int& i0, int& i1, int& fr) {
  const int n = (2 * c + 1) * msize - size;
  int i = 0;
  fr = 0;
  if (n >= 0) {
    const uint32_t d = 2u * (uint32_t)size;
    i = (int)((uint32_t)n / d);
    fr = (int)((((uint32_t)n % d) * 256u) / d);
  }
  i1 = min(i + 1, msize - 1);
  i0 = min(i, msize - 1);
}

// step 1
__device__ __forceinline__ int heat(float m, float gain) {
  const float t = __fadd_rn(__fmul_rn(m, gain), 0.5f);
  return t >= 0.0f ? (t >= 255.0f ? 255 : (int)t) : 0;            // (NaN fails the first comparison)
}

__global__ __launch_bounds__(BX * BY) void compose_kernel(const OvArgs a) {
  __shared__ uint32_t s_lut[256];
  __shared__ float s_gain;
  __shared__ uint8_t s_q[STRIP];
  const int f = blockIdx.z, tid = threadIdx.y * BX + threadIdx.x;
  s_lut[tid] = reinterpret_cast<const uint32_t*>(a.pack + COUNTR_OVERLAY_PACK_LUT)[tid];
  if (tid == 0) {
    float g = reinterpret_cast<const float*>(a.pack + COUNTR_OVERLAY_PACK_GAINS)[f];
    if ((a.gain_max >> f) & 1u) {
      const uint32_t bits = a.maxbits[f];
      g = bits ? __fdiv_rn(255.0f, __uint_as_float(bits)) : 0.0f;
    }
    s_gain = g;
  }
  __syncthreads();
  const float gain = s_gain;
  const float* __restrict__ m = a.map[f];
  // the block's 1024 columns x 8 rows read the map's columns c_lo .. c_hi of its rows r_lo .. r_hi (the indices grow with the coordinate)
  int c_lo, c_hi, r_lo, r_hi, unused0, unused1;
  axis(blockIdx.x * BX * PX, a.W, a.mw, c_lo, unused0, unused1);
  axis(min((int)(blockIdx.x + 1) * BX * PX, a.W) - 1, a.W, a.mw, unused0, c_hi, unused1);
  axis(blockIdx.y * BY * 2, a.H, a.mh, r_lo, unused0, unused1);
  axis(min((int)(blockIdx.y + 1) * BY * 2, a.H) - 1, a.H, a.mh, unused0, r_hi, unused1);
  const int nc = c_hi - c_lo + 1, nr = r_hi - r_lo + 1;
  const bool staged = (int64_t)nc * nr <= STRIP;                  // (uniform over the block)
  if (staged) {
    for (int i = tid; i < nc * nr; i += BX * BY) {
      const int r = i / nc, c = i - r * nc;
      s_q[i] = (uint8_t)heat(m[(int64_t)(r_lo + r) * a.mw + c_lo + c], gain);
    }
    __syncthreads();
  }
  const int x0 = (blockIdx.x * BX + threadIdx.x) * PX;
  const int j = blockIdx.y * BY + threadIdx.y;                    // rows 2 j and 2 j + 1
  if (x0 >= a.W || 2 * j >= a.H) return;
  const bool vec = a.vec != 0;
  int ix0[PX], fx[PX];                                             // (the right tap is min(ix0 + 1, mw - 1): not kept)
#pragma unroll
  for (int k = 0; k < PX; ++k) {
    int right;
    axis(min(x0 + k, a.W - 1), a.W, a.mw, ix0[k], right, fx[k]);
  }
  uint32_t px[2][12];                                             // both rows' pixels are on their way before the first is used
  load_px(a.rgb[f] + (int64_t)(2 * j) * a.W * 3, x0, a.W, vec, px[0]);
  load_px(a.rgb[f] + (int64_t)min(2 * j + 1, a.H - 1) * a.W * 3, x0, a.W, vec, px[1]);      // (an odd H: the last row again, not stored)
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int y = 2 * j + r;
    if (y >= a.H) break;
    int iy0, iy1, fy;
    axis(y, a.H, a.mh, iy0, iy1, fy);
    const float* __restrict__ m0 = m + (int64_t)iy0 * a.mw;
    const float* __restrict__ m1 = m + (int64_t)iy1 * a.mw;
    const int s0 = (iy0 - r_lo) * nc - c_lo, s1 = (iy1 - r_lo) * nc - c_lo;          // the same two rows in the staged strip
    const uint32_t (&o)[12] = px[r];
    uint32_t w[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) w[q] = 0u;
#pragma unroll
    for (int k = 0; k < PX; ++k) {
      const int ix1 = min(ix0[k] + 1, a.mw - 1);
      int q00, q01, q10, q11;
      if (staged) {
        q00 = s_q[s0 + ix0[k]]; q01 = s_q[s0 + ix1];
        q10 = s_q[s1 + ix0[k]]; q11 = s_q[s1 + ix1];
      } else {
        q00 = heat(m0[ix0[k]], gain); q01 = heat(m0[ix1], gain);
        q10 = heat(m1[ix0[k]], gain); q11 = heat(m1[ix1], gain);
      }
      const int top = q00 * (256 - fx[k]) + q01 * fx[k], bot = q10 * (256 - fx[k]) + q11 * fx[k];
      const int h = (top * (256 - fy) + bot * fy + 32768) >> 16;
      const uint32_t c = s_lut[h], al = c >> 24;
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        const uint32_t v = div255(byte_of(o, 3 * k + t) * (255u - al) + ((c >> (8 * t)) & 255u) * al + 127u);
        w[(3 * k + t) >> 2] |= v << (8 * ((3 * k + t) & 3));
      }
    }
    store_px(a.out[f] + (int64_t)y * a.W * 3, x0, a.W, vec, w);
  }
}

__global__ __launch_bounds__(256) void label_kernel(const OvArgs a) {
  const int f = blockIdx.y;
  const int lh = a.lh[f], lw = a.lw[f];
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= lh * lw) return;
  const int x = a.lx[f] + idx % lw, y = a.ly[f] + idx / lw;
  if (x < 0 || x >= a.W || y < 0 || y >= a.H) return;
  const uint32_t mk = a.pack[a.patch_off[f] + idx];
  uint8_t* p = a.out[f] + ((int64_t)y * a.W + x) * 3;
#pragma unroll
  for (int t = 0; t < 3; ++t) p[t] = (uint8_t)div255((uint32_t)p[t] * (255u - mk) + 255u * mk + 127u);
}

__device__ __forceinline__ bool in_range(int v) { return v >= -COORD && v <= COORD; }

__global__ __launch_bounds__(256) void edge_kernel(const OvArgs a) {
  const int f = blockIdx.y, e = blockIdx.x;
  if (e >= a.n_edges[f]) return;
  const int* v = reinterpret_cast<const int*>(a.pack + a.edges_off[f]) + 4 * (int64_t)e;
  const int x0 = v[0], y0 = v[1], x1 = v[2], y1 = v[3];
  if (!in_range(x0) || !in_range(y0) || !in_range(x1) || !in_range(y1)) return;
  const int dx = x1 - x0, dy = y1 - y0;
  const int n = max(abs(dx), abs(dy));
  const uint32_t r = (a.edge_rgb >> 16) & 255, g = (a.edge_rgb >> 8) & 255, b = a.edge_rgb & 255;
  for (int i = threadIdx.x; i <= n; i += 256) {
    const int x = n ? x0 + (int)rdiv((int64_t)i * dx, n) : x0;
    const int y = n ? y0 + (int)rdiv((int64_t)i * dy, n) : y0;
    if (x < 0 || x >= a.W || y < 0 || y >= a.H) continue;
    uint8_t* p = a.out[f] + ((int64_t)y * a.W + x) * 3;
    p[0] = (uint8_t)r; p[1] = (uint8_t)g; p[2] = (uint8_t)b;
  }
}

__global__ __launch_bounds__(64) void point_kernel(const OvArgs a) {
  const int f = blockIdx.y, pt = blockIdx.x;
  if (pt >= a.n_points[f]) return;
  const int* v = reinterpret_cast<const int*>(a.pack + a.points_off[f]) + 2 * (int64_t)pt;
  const int cx = v[0], cy = v[1];
  if (!in_range(cx) || !in_range(cy)) return;
  const int rad = a.radius, side = 2 * rad + 1;
  const uint32_t r = (a.point_rgb >> 16) & 255, g = (a.point_rgb >> 8) & 255, b = a.point_rgb & 255;
  for (int idx = threadIdx.x; idx < side * side; idx += 64) {
    const int dx = idx % side - rad, dy = idx / side - rad;
    if (dx * dx + dy * dy > rad * rad) continue;
    const int x = cx + dx, y = cy + dy;
    if (x < 0 || x >= a.W || y < 0 || y >= a.H) continue;
    uint8_t* p = a.out[f] + ((int64_t)y * a.W + x) * 3;
    p[0] = (uint8_t)r; p[1] = (uint8_t)g; p[2] = (uint8_t)b;
  }
}

// [off, off + bytes) inside the pack, behind its fixed part
bool inside(int off, int64_t bytes, int pack_bytes) { return off >= COUNTR_OVERLAY_PACK_HEAD && (int64_t)off + bytes <= (int64_t)pack_bytes; }

}  // namespace

extern "C" int countr_overlay_version(void) { return COUNTR_OVERLAY_ABI_VERSION; }

extern "C" const char* countr_overlay_last_error(void) { return g_err; }

extern "C" int countr_overlay_render(const countr_overlay_frame* frames, int n, int H, int W, int mh, int mw, const void* pack, int pack_bytes,
                                     int point_radius, int point_rgb, int edge_rgb, int format, int matrix, int range, void* maxbits,
                                     void* stream) {
  if (n < 1 || n > MAXF) return failf(-1, "countr_overlay_render: 1..%d frames a call, got %d", MAXF, n);
  if (format < COUNTR_OVERLAY_RGB || format > COUNTR_OVERLAY_I420) return failf(-1, "countr_overlay_render: unknown format %d", format);
  if (matrix != COUNTR_OVERLAY_BT601 && matrix != COUNTR_OVERLAY_BT709)
    return failf(-1, "countr_overlay_render: unknown matrix %d", matrix);
  if (range != COUNTR_OVERLAY_LIMITED && range != COUNTR_OVERLAY_FULL) return failf(-1, "countr_overlay_render: unknown range %d", range);
  if (H < 1 || H > COUNTR_OVERLAY_MAX_SIDE || W < 1 || W > COUNTR_OVERLAY_MAX_SIDE)
    return failf(-1, "countr_overlay_render: H and W are 1..%d, got %d x %d", COUNTR_OVERLAY_MAX_SIDE, H, W);
  if (mh < 1 || mh > COUNTR_OVERLAY_MAX_SIDE || mw < 1 || mw > COUNTR_OVERLAY_MAX_SIDE)
    return failf(-1, "countr_overlay_render: mh and mw are 1..%d, got %d x %d", COUNTR_OVERLAY_MAX_SIDE, mh, mw);
  if (point_radius < 0 || point_radius > COUNTR_OVERLAY_MAX_RADIUS)
    return failf(-1, "countr_overlay_render: point_radius is 0..%d, got %d", COUNTR_OVERLAY_MAX_RADIUS, point_radius);
  if (!frames) return fail(-1, "countr_overlay_render: the frames array is required");
  if (!pack || ((uintptr_t)pack & 15)) return fail(-1, "countr_overlay_render: the packed upload is required, 16-byte aligned");
  if (pack_bytes < COUNTR_OVERLAY_PACK_HEAD)
    return failf(-1, "countr_overlay_render: the packed upload has at least %d bytes, got %d", COUNTR_OVERLAY_PACK_HEAD, pack_bytes);
  OvArgs a;
  Rgb420Args y;
  memset(&a, 0, sizeof(a));
  memset(&y, 0, sizeof(y));
  uintptr_t bits = (uintptr_t)W;
  int max_points = 0, max_edges = 0, max_patch = 0;
  for (int j = 0; j < n; ++j) {
    const countr_overlay_frame& fr = frames[j];
    if (!fr.rgb || !fr.map || !fr.out || (format != COUNTR_OVERLAY_RGB && !fr.yuv))
      return failf(-1, "countr_overlay_render: frame %d has a null pointer", j);
    if (format == COUNTR_OVERLAY_RGB && fr.yuv)
      return failf(-1, "countr_overlay_render: frame %d: yuv must be NULL when the format is RGB", j);
    if ((uintptr_t)fr.map & 3) return failf(-1, "countr_overlay_render: frame %d: the map is 4-byte aligned", j);
    if (fr.n_points < 0 || fr.n_points > COUNTR_OVERLAY_MAX_POINTS)
      return failf(-1, "countr_overlay_render: frame %d: 0..%d points, got %d", j, COUNTR_OVERLAY_MAX_POINTS, fr.n_points);
    if (fr.n_polys < 0 || fr.n_polys > COUNTR_OVERLAY_MAX_POLYGONS)
      return failf(-1, "countr_overlay_render: frame %d: 0..%d polygons, got %d", j, COUNTR_OVERLAY_MAX_POLYGONS, fr.n_polys);
    if (fr.n_polys > 0 && !fr.poly_verts) return failf(-1, "countr_overlay_render: frame %d has polygons and no poly_verts", j);
    int edges = 0;
    for (int p = 0; p < fr.n_polys; ++p) {
      const int nv = static_cast<const int*>(fr.poly_verts)[p];
      if (nv < 1 || nv > COUNTR_OVERLAY_MAX_VERTICES)
        return failf(-1, "countr_overlay_render: frame %d polygon %d: 1..%d vertices, got %d", j, p, COUNTR_OVERLAY_MAX_VERTICES, nv);
      edges += nv;
    }
    if (fr.n_edges != edges)
      return failf(-1, "countr_overlay_render: frame %d: n_edges %d, its polygons have %d vertices", j, fr.n_edges, edges);
    if (fr.lh < 0 || fr.lh > COUNTR_OVERLAY_PATCH_H || fr.lw < 0 || fr.lw > COUNTR_OVERLAY_PATCH_W || (fr.lh == 0) != (fr.lw == 0))
      return failf(-1, "countr_overlay_render: frame %d: a label patch is at most %d x %d (0 x 0: none), got %d x %d", j,
                   COUNTR_OVERLAY_PATCH_H, COUNTR_OVERLAY_PATCH_W, fr.lh, fr.lw);
    if (fr.lh && (fr.lx < -COORD || fr.lx > COORD || fr.ly < -COORD || fr.ly > COORD))
      return failf(-1, "countr_overlay_render: frame %d: the label's position is within +-%d, got (%d, %d)", j, COORD, fr.lx, fr.ly);
    if ((fr.n_points && (!inside(fr.points_off, 8ll * fr.n_points, pack_bytes) || (fr.points_off & 3))) ||
        (fr.n_edges && (!inside(fr.edges_off, 16ll * fr.n_edges, pack_bytes) || (fr.edges_off & 3))) ||
        (fr.lh && !inside(fr.patch_off, (int64_t)fr.lh * fr.lw, pack_bytes)))
      return failf(-1, "countr_overlay_render: frame %d: an offset lies outside the packed upload of %d bytes (or is not 4-byte aligned)",
                   j, pack_bytes);
    if (fr.gain_max) {
      if (!maxbits || ((uintptr_t)maxbits & 3)) return fail(-1, "countr_overlay_render: maxbits (n device uint32) is required when a frame has gain_max");
      a.gain_max |= 1u << j;
    }
    bits |= (uintptr_t)fr.rgb | (uintptr_t)fr.out | (uintptr_t)fr.yuv;
    a.rgb[j] = (const uint8_t*)fr.rgb;
    a.map[j] = (const float*)fr.map;
    a.out[j] = (uint8_t*)fr.out;
    y.src[j] = (const uint8_t*)fr.out;
    y.dst[j] = (uint8_t*)fr.yuv;
    a.n_points[j] = fr.n_points; a.points_off[j] = fr.points_off;
    a.n_edges[j] = fr.n_edges; a.edges_off[j] = fr.edges_off;
    a.lh[j] = fr.lh; a.lw[j] = fr.lw; a.lx[j] = fr.lx; a.ly[j] = fr.ly; a.patch_off[j] = fr.patch_off;
    max_points = fr.n_points > max_points ? fr.n_points : max_points;
    max_edges = fr.n_edges > max_edges ? fr.n_edges : max_edges;
    max_patch = fr.lh * fr.lw > max_patch ? fr.lh * fr.lw : max_patch;
  }
  a.pack = (const uint8_t*)pack;
  a.maxbits = (uint32_t*)maxbits;
  a.H = H; a.W = W; a.mh = mh; a.mw = mw;
  a.vec = (bits & 15) == 0;
  a.radius = point_radius; a.point_rgb = point_rgb & 0xffffff; a.edge_rgb = edge_rgb & 0xffffff;
  y.H = H; y.W = W; y.vec = a.vec;
  set_coefficients(y, matrix, range);
  hipStream_t st = STREAM(stream);
  hipError_t e = hipSuccess;
  if (a.gain_max) {
    e = hipMemsetAsync(maxbits, 0, sizeof(uint32_t) * n, st);
    if (e != hipSuccess) return failf(-10, "countr_overlay_render: memset failed: %s", hipGetErrorString(e));
    const int64_t total = (int64_t)mh * mw;
    const unsigned blocks = (unsigned)(total / 1024 < 1 ? 1 : total / 1024 > 256 ? 256 : total / 1024);
    hipLaunchKernelGGL(max_kernel, dim3(blocks, (unsigned)n), dim3(256), 0, st, a);
  }
  const dim3 grid = rgb_grid(H, W, n);
  hipLaunchKernelGGL(compose_kernel, grid, dim3(BX, BY), 0, st, a);
  if (max_patch) hipLaunchKernelGGL(label_kernel, dim3((unsigned)((max_patch + 255) / 256), (unsigned)n), dim3(256), 0, st, a);
  if (max_edges) hipLaunchKernelGGL(edge_kernel, dim3((unsigned)max_edges, (unsigned)n), dim3(256), 0, st, a);
  if (max_points) hipLaunchKernelGGL(point_kernel, dim3((unsigned)max_points, (unsigned)n), dim3(64), 0, st, a);
  launch_rgb420(format, y, n, st);
  return launched("countr_overlay_render");
}
