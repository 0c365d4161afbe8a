// The front of the inference path: raw 8-bit RGB frames and pixel boxes -> the tensors SupervisedMAE's sliding-window path consumes.
//   countr_pil_bilinear_tables  (host only) the per-axis tap tables of Pillow's 8-bit BILINEAR resample (Resample.c: precompute_coeffs +
//                               normalize_coeffs_8bpc), i.e. what transforms.Resize does to a PIL image (reference demo_zero.py:23-38,
//                               demo.py:42-49)
//   countr_frame_resize_u8      uint8 [H, W, 3] frames -> fp32 planar [3, out_h, out_w] in [0, 1]: horizontal pass into a uint8
//                               intermediate, vertical pass + ToTensor's / 255 -- equal to PIL + ToTensor bit for bit
//   countr_crop_resize_f32      rectangles of an fp32 planar image -> [n, 3, oh, ow], bilinear, align_corners=False, no antialias:
//                               the 64x64 exemplar crops (demo.py:60-68) and the 3x3 crop-and-upscale of tiny exemplars (:84-99)
// uint8 / fp32 only: the bf16 and the fp16 build of the library export the same code.
#include "common.hpp"
#include "../../include/countr_hip.h"

#include <math.h>

#define STREAM(s) reinterpret_cast<hipStream_t>(s)

namespace {

constexpr int PRECISION_BITS = 32 - 8 - 2;      // Pillow's fixed point: weights are int(0.5 + w * 2^22)
constexpr int MAX_FRAMES = 16, MAX_RECTS = 16;
constexpr int STAGE_BYTES = 16384;              // LDS staging of one source row segment (horizontal pass)
constexpr int MAX_BLOCKS = 2048;

struct Axis {
  double scale, support, inv_fs;
  int ksize;
};

bool axis_of(int in_size, int out_size, Axis* a) {
  if (in_size < 1 || out_size < 1) return false;
  a->scale = (double)in_size / out_size;
  const double fs = a->scale < 1.0 ? 1.0 : a->scale;
  a->support = fs;                              // bilinear support 1.0 x the filter scale
  a->inv_fs = 1.0 / fs;                         // (Pillow multiplies by this reciprocal; so does this file)
  const double k = ceil(a->support) * 2 + 1;
  if (k > 1 << 20) return false;
  a->ksize = (int)k;
  return true;
}

struct FrameArgs {
  const uint8_t* src[MAX_FRAMES];   // uint8 [H, W, 3]
  float* dst[MAX_FRAMES];           // fp32 [3, out_h, out_w]
};

__device__ __forceinline__ uint8_t clip8(int v) {
  v >>= PRECISION_BITS;
  return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// Horizontal pass.  One work item = (frame, source row, tile of `tile` output pixels): the bytes of the row the tile's taps touch are
// staged in LDS with 16-byte loads (VEC: frame base 16-byte aligned) and every thread resamples one output pixel (3 channels) from
// there.  Table entries are clamped to the staged range, so a wrong table cannot make the kernel read outside the frame.
template <bool VEC>
__global__ __launch_bounds__(256) void resize_h_kernel(const FrameArgs a, uint8_t* __restrict__ tmp, const int* __restrict__ bounds,
                                                       const int* __restrict__ weights, int ksize, int n, int H, int W, int out_w, int tile) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[STAGE_BYTES];
  const int tiles = (out_w + tile - 1) / tile;
  const int64_t items = (int64_t)n * H * tiles;
  const int64_t frame_bytes = (int64_t)H * W * 3;
  for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
    const int t = (int)(it % tiles);
    const int64_t fy = it / tiles;
    const int y = (int)(fy % H), f = (int)(fy / H);
    const int xo0 = t * tile, xo1 = min(out_w, xo0 + tile);
    int xs = bounds[2 * xo0], xe = bounds[2 * (xo1 - 1)] + bounds[2 * (xo1 - 1) + 1];
    xs = max(0, min(xs, W));
    xe = max(xs, min(xe, W));
    const int64_t b0 = ((int64_t)y * W + xs) * 3;              // first byte of the segment in the frame
    const int64_t a0 = VEC ? (b0 & ~(int64_t)15) : b0;
    const int head = (int)(b0 - a0);
    const int span = min((xe - xs) * 3, STAGE_BYTES - 16 - head) ;      // (the host sized `tile` so that this never cuts)
    const uint8_t* src = a.src[f];
    if (VEC) {
      const int nvec = (head + span + 15) >> 4;
      for (int v = threadIdx.x; v < nvec; v += 256) {
        const int64_t off = a0 + (int64_t)v * 16;
        if (off + 16 <= frame_bytes) {
          *reinterpret_cast<uint4*>(stage + v * 16) = *reinterpret_cast<const uint4*>(src + off);
        } else {
          for (int b = 0; b < 16; ++b) stage[v * 16 + b] = off + b < frame_bytes ? src[off + b] : (uint8_t)0;
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
      cnt = max(0, min(min(cnt, ksize), min(xe - xmin, (span - (xmin - xs) * 3) / 3)));
      const int* k = weights + (int64_t)xo * ksize;
      const uint8_t* p = stage + head + (xmin - xs) * 3;
      int r = 1 << (PRECISION_BITS - 1), g = r, b = r;
      for (int j = 0; j < cnt; ++j) {
        const int w = k[j];
        r += (int)p[3 * j] * w; g += (int)p[3 * j + 1] * w; b += (int)p[3 * j + 2] * w;
      }
      uint8_t* o = tmp + (((int64_t)f * H + y) * out_w + xo) * 3;
      o[0] = clip8(r); o[1] = clip8(g); o[2] = clip8(b);
    }
    __syncthreads();
  }
}

// Vertical pass + ToTensor.  VEC: one thread = 4 neighbouring output pixels x 3 channels (12 contiguous bytes of every tap row of the
// interleaved intermediate, one 16-byte store per channel plane; needs out_w % 4 == 0); otherwise one pixel per thread.
template <bool VEC>
__global__ __launch_bounds__(256) void resize_v_kernel(const FrameArgs a, const uint8_t* __restrict__ tmp, const int* __restrict__ bounds,
                                                       const int* __restrict__ weights, int ksize, int n, int H, int out_h, int out_w) {
  constexpr int PX = VEC ? 4 : 1;
  const int per = out_w / PX;
  const int64_t total = (int64_t)n * out_h * per;
  const int64_t plane = (int64_t)out_h * out_w;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int q = (int)(i % per);
    const int64_t fy = i / per;
    const int yo = (int)(fy % out_h), f = (int)(fy / out_h);
    int ymin = bounds[2 * yo], cnt = bounds[2 * yo + 1];
    ymin = max(0, min(ymin, H));
    cnt = max(0, min(min(cnt, ksize), H - ymin));
    const int* k = weights + (int64_t)yo * ksize;
    const uint8_t* p = tmp + (((int64_t)f * H + ymin) * out_w + (int64_t)q * PX) * 3;
    int acc[3 * PX];
#pragma unroll
    for (int e = 0; e < 3 * PX; ++e) acc[e] = 1 << (PRECISION_BITS - 1);
    for (int j = 0; j < cnt; ++j, p += (int64_t)out_w * 3) {
      const int w = k[j];
      if (VEC) {
        const uint32_t* p4 = reinterpret_cast<const uint32_t*>(p);      // (12 q bytes into a row of 3 out_w bytes, out_w % 4 == 0: 4-byte aligned)
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
    float* o = a.dst[f] + (int64_t)yo * out_w + (int64_t)q * PX;
    if (VEC) {
      float v[12];
#pragma unroll
      for (int e = 0; e < 12; ++e) v[e] = (float)clip8(acc[e]) / 255.0f;      // ToTensor: a correctly rounded division, not x * (1 / 255)
      // acc[e] is byte e of the 12: pixel e / 3, channel e % 3
      *reinterpret_cast<float4*>(o) = make_float4(v[0], v[3], v[6], v[9]);
      *reinterpret_cast<float4*>(o + plane) = make_float4(v[1], v[4], v[7], v[10]);
      *reinterpret_cast<float4*>(o + 2 * plane) = make_float4(v[2], v[5], v[8], v[11]);
    } else {
#pragma unroll
      for (int e = 0; e < 3; ++e) o[e * plane] = (float)clip8(acc[e]) / 255.0f;
    }
  }
}

struct CropArgs {
  int y0[MAX_RECTS], x0[MAX_RECTS], ch[MAX_RECTS], cw[MAX_RECTS];   // first row / column and size of every (clipped) rectangle
};

// torch's upsample_bilinear2d (align_corners=False) on rectangle r of img: VEC = 4 neighbouring output columns per thread
template <bool VEC>
__global__ __launch_bounds__(256) void crop_resize_kernel(const float* __restrict__ img, const CropArgs a, float* __restrict__ out, int n, int h,
                                                          int w, int oh, int ow) {
  constexpr int PX = VEC ? 4 : 1;
  const int per = ow / PX;
  const int64_t total = (int64_t)n * 3 * oh * per;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int q = (int)(i % per);
    const int64_t row = i / per;                      // (rectangle, channel, output row)
    const int oy = (int)(row % oh);
    const int c = (int)((row / oh) % 3), r = (int)(row / ((int64_t)3 * oh));
    const int ch = a.ch[r], cw = a.cw[r];
    const float sy = (float)ch / (float)oh, sx = (float)cw / (float)ow;
    const float fy = fmaxf(sy * ((float)oy + 0.5f) - 0.5f, 0.f);
    const int y1 = min((int)fy, ch - 1), yp = y1 < ch - 1 ? 1 : 0;
    const float ly = fy - (float)y1, ly0 = 1.f - ly;
    const float* s0 = img + ((int64_t)c * h + a.y0[r] + y1) * w + a.x0[r];
    const float* s1 = s0 + (int64_t)yp * w;
    float v[PX];
#pragma unroll
    for (int e = 0; e < PX; ++e) {
      const float fx = fmaxf(sx * ((float)(q * PX + e) + 0.5f) - 0.5f, 0.f);
      const int x1 = min((int)fx, cw - 1), xp = x1 < cw - 1 ? 1 : 0;
      const float lx = fx - (float)x1, lx0 = 1.f - lx;
      v[e] = ly0 * (lx0 * s0[x1] + lx * s0[x1 + xp]) + ly * (lx0 * s1[x1] + lx * s1[x1 + xp]);
    }
    float* o = out + row * ow + (int64_t)q * PX;
    if (VEC) *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1 % PX], v[2 % PX], v[3 % PX]);
    else o[0] = v[0];
  }
}

int blocks_for(int64_t threads) { return (int)max((int64_t)1, min((int64_t)MAX_BLOCKS, (threads + 255) / 256)); }

}  // namespace

extern "C" int countr_pil_bilinear_tables(int in_size, int out_size, int* bounds, int* weights) {
  Axis ax;
  if (!axis_of(in_size, out_size, &ax)) { countr_set_error("countr_pil_bilinear_tables: sizes must be >= 1 (and in / out below 2^19)"); return -1; }
  if (!bounds && !weights) return ax.ksize;
  if (!bounds || !weights) { countr_set_error("countr_pil_bilinear_tables: pass both tables, or neither to ask for the tap stride"); return -1; }
  double* wd = new double[ax.ksize];
  for (int xx = 0; xx < out_size; ++xx) {
    const double center = (xx + 0.5) * ax.scale;
    int xmin = (int)(center - ax.support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + ax.support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) {
      double t = (x + xmin - center + 0.5) * ax.inv_fs;
      if (t < 0.0) t = -t;
      const double w = t < 1.0 ? 1.0 - t : 0.0;
      wd[x] = w;
      ww += w;
    }
    int* k = weights + (int64_t)xx * ax.ksize;
    for (int x = 0; x < ax.ksize; ++x) {
      double w = x < xmax ? wd[x] : 0.0;
      if (x < xmax && ww != 0.0) w /= ww;
      k[x] = (int)(0.5 + w * (double)(1 << PRECISION_BITS));
    }
    bounds[2 * xx] = xmin;
    bounds[2 * xx + 1] = xmax;
  }
  delete[] wd;
  return ax.ksize;
}

extern "C" int countr_frame_resize_u8(const void* const* frames, void* const* outs, int n, int H, int W, int out_h, int out_w,
                                      const int* hbounds, const int* hweights, const int* vbounds, const int* vweights, void* tmp,
                                      void* stream) {
  if (!frames || !outs || !hbounds || !hweights || !vbounds || !vweights || !tmp || n < 1 || n > MAX_FRAMES) {
    countr_set_error("countr_frame_resize_u8: bad args (1..16 frames, four tables and the intermediate are required)"); return -1;
  }
  Axis ah, av;
  if (!axis_of(W, out_w, &ah) || !axis_of(H, out_h, &av) || (int64_t)H * W * 3 > (int64_t)1 << 40 || (int64_t)H * out_w > (int64_t)1 << 38) {
    countr_set_error("countr_frame_resize_u8: frame or output size out of range"); return -1;
  }
  // output pixels per horizontal tile: the source bytes of a tile (+ alignment slack) must fit the LDS staging buffer
  int tile = 256;
  while (tile >= 1 && ((int64_t)ceil(ah.scale * (tile - 1)) + ah.ksize + 1) * 3 + 48 > STAGE_BYTES) tile >>= 1;
  if (tile < 1) { countr_set_error("countr_frame_resize_u8: frame too wide for this output width (the taps of one output pixel exceed the 16-KB row staging)"); return -1; }
  FrameArgs a;
  bool vec_in = true, vec_out = (out_w & 3) == 0 && (((uintptr_t)tmp) & 3) == 0;
  for (int j = 0; j < MAX_FRAMES; ++j) {
    const int s = j < n ? j : n - 1;
    if (!frames[s] || !outs[s]) { countr_set_error("countr_frame_resize_u8: null frame or output pointer"); return -1; }
    a.src[j] = (const uint8_t*)frames[s]; a.dst[j] = (float*)outs[s];
    if (((uintptr_t)frames[s]) & 15) vec_in = false;
    if (((uintptr_t)outs[s]) & 15) vec_out = false;
  }
  const int tiles = (out_w + tile - 1) / tile;
  const int hblocks = (int)min((int64_t)MAX_BLOCKS, (int64_t)n * H * tiles);
  uint8_t* t8 = (uint8_t*)tmp;
  if (vec_in) hipLaunchKernelGGL(resize_h_kernel<true>, dim3(hblocks), dim3(256), 0, STREAM(stream), a, t8, hbounds, hweights, ah.ksize, n, H, W, out_w, tile);
  else hipLaunchKernelGGL(resize_h_kernel<false>, dim3(hblocks), dim3(256), 0, STREAM(stream), a, t8, hbounds, hweights, ah.ksize, n, H, W, out_w, tile);
  const int64_t vthreads = (int64_t)n * out_h * (vec_out ? out_w / 4 : out_w);
  if (vec_out) hipLaunchKernelGGL(resize_v_kernel<true>, dim3(blocks_for(vthreads)), dim3(256), 0, STREAM(stream), a, t8, vbounds, vweights, av.ksize, n, H, out_h, out_w);
  else hipLaunchKernelGGL(resize_v_kernel<false>, dim3(blocks_for(vthreads)), dim3(256), 0, STREAM(stream), a, t8, vbounds, vweights, av.ksize, n, H, out_h, out_w);
  COUNTR_LAUNCH_CHECK("countr_frame_resize_u8");
}

extern "C" int countr_crop_resize_f32(const float* img, int h, int w, const int* rects, int n, int oh, int ow, float* out, void* stream) {
  if (!img || !rects || !out || h < 1 || w < 1 || oh < 1 || ow < 1 || n < 1 || n > MAX_RECTS) {
    countr_set_error("countr_crop_resize_f32: bad args (1..16 rectangles)"); return -1;
  }
  CropArgs a;
  for (int j = 0; j < MAX_RECTS; ++j) {
    const int* r = rects + 4 * (j < n ? j : n - 1);             // {y1, x1, y2, x2}, inclusive
    if (r[0] < 0 || r[1] < 0) { countr_set_error("countr_crop_resize_f32: negative rectangle corner"); return -1; }
    const int y0 = min(r[0], h), x0 = min(r[1], w);             // img[:, y1:y2 + 1, x1:x2 + 1]: slicing clips both ends to the image
    const int ch = min((int64_t)r[2] + 1, (int64_t)h) - y0, cw = min((int64_t)r[3] + 1, (int64_t)w) - x0;
    if (ch < 1 || cw < 1) { countr_set_error("countr_crop_resize_f32: a rectangle is empty after clipping to the image"); return -1; }
    a.y0[j] = y0; a.x0[j] = x0; a.ch[j] = ch; a.cw[j] = cw;
  }
  const bool vec = (ow & 3) == 0 && (((uintptr_t)out) & 15) == 0;
  const int64_t threads = (int64_t)n * 3 * oh * (vec ? ow / 4 : ow);
  if (vec) hipLaunchKernelGGL(crop_resize_kernel<true>, dim3(blocks_for(threads)), dim3(256), 0, STREAM(stream), img, a, out, n, h, w, oh, ow);
  else hipLaunchKernelGGL(crop_resize_kernel<false>, dim3(blocks_for(threads)), dim3(256), 0, STREAM(stream), img, a, out, n, h, w, oh, ow);
  COUNTR_LAUNCH_CHECK("countr_crop_resize_f32");
}
