// The front of the inference path: raw 8-bit RGB frames and pixel boxes -> the tensors SupervisedMAE's sliding-window path consumes.
//   countr_pil_bilinear_tables  (host only) the per-axis tap tables of Pillow's 8-bit BILINEAR resample (Resample.c: precompute_coeffs +
//                               normalize_coeffs_8bpc), i.e. what transforms.Resize does to a PIL image (reference demo_zero.py:23-38,
//                               demo.py:42-49)
//   countr_frame_resize_u8      uint8 [H, W, 3] frames -> fp32 planar [3, out_h, out_w] in [0, 1]: horizontal pass into a uint8
//                               intermediate, vertical pass + ToTensor's / 255 -- equal to PIL + ToTensor bit for bit
//   countr_crop_resize_f32      rectangles of an fp32 planar image -> [n, 3, oh, ow], bilinear, align_corners=False, no antialias:
//                               the 64x64 exemplar crops (demo.py:60-68) and the 3x3 crop-and-upscale of tiny exemplars (:84-99)
// The tables and the bodies of the two passes are pil_resample.hpp's (shared with pretrain_aug.hip), the bilinear sampler is
// bilinear.hpp's (shared with augment.hip, mosaic.hip, carpk.hip).
// uint8 / fp32 only: the bf16 and the fp16 build of the library export the same code.
#include "common.hpp"
#include "pil_resample.hpp"
#include "bilinear.hpp"      // contraction ON (no pragma in this file): crop_resize_kernel may fuse the index and the blend, as it always has
#include "../../include/countr_hip.h"

namespace {

constexpr int MAX_FRAMES = COUNTR_FRAMES_MAX, MAX_RECTS = COUNTR_FRAMES_MAX;
constexpr int MAX_BLOCKS = 2048;

struct FrameArgs {
  const uint8_t* src[MAX_FRAMES];   // uint8 [H, W, 3]
  float* dst[MAX_FRAMES];           // fp32 [3, out_h, out_w]
};

// Horizontal pass (pil_hpass_item).  One work item = (frame, source row, tile of `tile` output pixels); VEC: every frame base is
// 16-byte aligned.
template <bool VEC>
__global__ __launch_bounds__(256) void resize_h_kernel(const FrameArgs a, uint8_t* __restrict__ tmp, const int* __restrict__ bounds,
                                                       const int* __restrict__ weights, int ksize, int n, int H, int W, int out_w, int tile) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[STAGE_BYTES];
  const int tiles = (out_w + tile - 1) / tile;
  const int64_t items = (int64_t)n * H * tiles;
  for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
    const int t = (int)(it % tiles);
    const int64_t fy = it / tiles;               // (frame, row): the row's index in the intermediate [n, H, out_w, 3]
    const int y = (int)(fy % H), f = (int)(fy / H);
    pil_hpass_item(a.src[f], (int64_t)H * W * 3, W, 0, y, W, bounds, weights, ksize, tmp + fy * out_w * 3, out_w, tile, t, VEC, stage);
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
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int q = (int)(i % per);
    const int64_t fy = i / per;
    const int yo = (int)(fy % out_h), f = (int)(fy / out_h);
    int ymin, cnt;
    const int* k = pil_vtaps(bounds, weights, ksize, H, yo, &ymin, &cnt);
    int acc[3 * PX];
    // (12 q bytes into a row of 3 out_w bytes, out_w % 4 == 0: 4-byte aligned)
    pil_vacc<3 * PX>(tmp + (((int64_t)f * H + ymin) * out_w + (int64_t)q * PX) * 3, (int64_t)out_w * 3, k, cnt, acc);
    pil_store_planes<3 * PX>(a.dst[f] + (int64_t)yo * out_w + (int64_t)q * PX, (int64_t)out_h * out_w, acc, false);
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
    const float* org = img + ((int64_t)c * h + a.y0[r]) * w + a.x0[r];
    const BilinearRow t = bilinear_row(org, w, ch, cw, bilinear_scale(ch, oh), bilinear_scale(cw, ow), oy);
    float v[PX];
#pragma unroll
    for (int e = 0; e < PX; ++e) v[e] = bilinear_at(t, q * PX + e);
    float* o = out + row * ow + (int64_t)q * PX;
    if (VEC) *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1 % PX], v[2 % PX], v[3 % PX]);
    else o[0] = v[0];
  }
}

}  // namespace

extern "C" int countr_pil_bilinear_tables(int in_size, int out_size, int* bounds, int* weights) {
  Axis ax;
  if (!axis_ok(0, in_size, out_size, &ax)) { countr_set_error("countr_pil_bilinear_tables: sizes must be >= 1 (and in / out below 2^19)"); return -1; }
  if (!bounds && !weights) return ax.ksize;
  if (!bounds || !weights) { countr_set_error("countr_pil_bilinear_tables: pass both tables, or neither to ask for the tap stride"); return -1; }
  for (int xx = 0; xx < out_size; ++xx) table_row(0, ax, in_size, xx, ax.ksize, bounds, weights);
  return ax.ksize;
}

extern "C" int countr_frame_resize_u8(const void* const* frames, void* const* outs, int n, int H, int W, int out_h, int out_w,
                                      const int* hbounds, const int* hweights, const int* vbounds, const int* vweights, void* tmp,
                                      void* stream) {
  if (!frames || !outs || !hbounds || !hweights || !vbounds || !vweights || !tmp || n < 1 || n > MAX_FRAMES) {
    countr_set_error("countr_frame_resize_u8: bad args (1..16 frames, four tables and the intermediate are required)"); return -1;
  }
  Axis ah, av;
  if (!axis_ok(0, W, out_w, &ah) || !axis_ok(0, H, out_h, &av) || (int64_t)H * W * 3 > (int64_t)1 << 40 || (int64_t)H * out_w > (int64_t)1 << 38) {
    countr_set_error("countr_frame_resize_u8: frame or output size out of range"); return -1;
  }
  const int tile = tile_of(W, out_w, 0);
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
  if (vec_out) hipLaunchKernelGGL(resize_v_kernel<true>, dim3(countr_blocks_for(vthreads, MAX_BLOCKS)), dim3(256), 0, STREAM(stream), a, t8, vbounds, vweights, av.ksize, n, H, out_h, out_w);
  else hipLaunchKernelGGL(resize_v_kernel<false>, dim3(countr_blocks_for(vthreads, MAX_BLOCKS)), dim3(256), 0, STREAM(stream), a, t8, vbounds, vweights, av.ksize, n, H, out_h, out_w);
  return countr_check_launch("countr_frame_resize_u8");
}

extern "C" int countr_crop_resize_f32(const float* img, int h, int w, const int* rects, int n, int oh, int ow, float* out, void* stream) {
  if (!img || !rects || !out || h < 1 || w < 1 || oh < 1 || ow < 1 || n < 1 || n > MAX_RECTS) {
    countr_set_error("countr_crop_resize_f32: bad args (1..16 rectangles)"); return -1;
  }
  CropArgs a;
  for (int j = 0; j < MAX_RECTS; ++j) {
    const int* r = rects + 4 * (j < n ? j : n - 1);             // {y1, x1, y2, x2}, inclusive
    if (!clip_rect(r[0], r[1], r[2], r[3], h, w, &a.y0[j], &a.x0[j], &a.ch[j], &a.cw[j])) {
      countr_set_error(r[0] < 0 || r[1] < 0 ? "countr_crop_resize_f32: negative rectangle corner"
                                            : "countr_crop_resize_f32: a rectangle is empty after clipping to the image");
      return -1;
    }
  }
  const bool vec = (ow & 3) == 0 && (((uintptr_t)out) & 15) == 0;
  const int64_t threads = (int64_t)n * 3 * oh * (vec ? ow / 4 : ow);
  if (vec) hipLaunchKernelGGL(crop_resize_kernel<true>, dim3(countr_blocks_for(threads, MAX_BLOCKS)), dim3(256), 0, STREAM(stream), img, a, out, n, h, w, oh, ow);
  else hipLaunchKernelGGL(crop_resize_kernel<false>, dim3(countr_blocks_for(threads, MAX_BLOCKS)), dim3(256), 0, STREAM(stream), img, a, out, n, h, w, oh, ow);
  return countr_check_launch("countr_crop_resize_f32");
}
