// The mosaic branch of the train-time augmentation (countr_amd/data/fsc147.py::mosaic / _blend_pair) as one device kernel: four
// length x length crops of clean resized frames, each resized to resize_l = 192 + 2 bl, joined two by two along the rows and then along
// the columns with the reference's 2 bl-wide cross-fades.  The oracle is fsc147.mosaic(); the host keeps the draws and the dot cells
// (fsc147.mosaic_plan), the frames come from countr_frame_resize_u8 (countr_amd/device_aug.py::DeviceAug).
//   countr_aug_mosaic     out[row] [3, 384, 384] <- the mosaic of its four pieces.  Neither the four resized pieces nor the two 384-line
//                         halves are stored: every output pixel evaluates the one (quadrant interior), two (a seam band) or four (where
//                         the bands cross) bilinear piece samples (bilinear.hpp) it depends on and mixes them in the reference's order
// fp32 only: both library builds export the same code.
#include "common.hpp"
#include "../../include/countr_hip.h"

// torch's CPU kernels round every product and sum on its own: no fused multiply-adds here
#pragma clang fp contract(off)
#include "bilinear.hpp"      // contraction OFF (below the pragma): a piece sample rounds every product and sum on its own, as exemplar_kernel does

namespace {

constexpr int MAX_IMGS = COUNTR_AUG_MAX_IMAGES;   // descriptors travel as kernel arguments: 32 x 104 bytes
constexpr int OUT = 384, HALF = OUT / 2;          // the training crop and one quadrant's core
constexpr int QW = 32;                            // a workgroup owns 8 rows x 32 four-pixel chunks of one channel: the chunks of a third of a row

struct MosPiece {
  const float* org;                // channel 0 of the crop's first pixel
  int plane, w;                    // h * w and the row stride of the frame
  int length;                      // the crop's edge
  float scale;                     // fp32(length) / fp32(resize_l): the source step of upsample_bilinear2d, align_corners=False
};
struct MosImg {
  MosPiece p[4];                   // quadrant order of mosaic(): 0 top left, 1 bottom left, 2 top right, 3 bottom right
  int bl, row;
};
struct MosArgs { MosImg im[MAX_IMGS]; };

// line r of a resized piece, channel c
__device__ __forceinline__ BilinearRow row_tap(const MosPiece& p, int c, int r) {
  return bilinear_row(p.org + (int64_t)c * p.plane, p.w, p.length, p.length, p.scale, p.scale, r);
}

// output line y of one half (two pieces joined along the rows): the kept line of the piece y lies in, and inside the band of bl lines
// either side of the seam the neighbour's overhanging line it is mixed with (weights and line indices of _blend_pair)
struct HalfRow {
  BilinearRow kept, over;
  float w_kept, w_over;
  bool seam;
};
__device__ __forceinline__ HalfRow half_row(const MosImg& d, int half, int c, int y) {
  HalfRow h;
  const int bl = d.bl, top = y < HALF ? 1 : 0;
  const int i = top ? HALF - 1 - y : y - HALF;
  const MosPiece& a = d.p[2 * half];
  const MosPiece& b = d.p[2 * half + 1];
  h.seam = i < bl;
  h.kept = row_tap(top ? a : b, c, top ? bl + y : bl + i);
  h.w_kept = (float)(i + bl) / (float)(2 * bl);
  h.w_over = (float)(bl - i) / (float)(2 * bl);
  if (h.seam) h.over = row_tap(top ? b : a, c, top ? bl - i : HALF - 1 + bl + i);
  else h.over = h.kept;
  return h;
}
__device__ __forceinline__ float half_at(const HalfRow& h, int col) {
  float v = bilinear_at(h.kept, col);
  if (h.seam) v = v * h.w_kept + bilinear_at(h.over, col) * h.w_over;
  return clamp01(v);
}

// one thread = four neighbouring pixels of one channel row, one 16-byte store.  A wave is two rows of one third of the width, so the
// row band is decided per wave (up to its first and last line) and the column band only ever meets the waves of the middle third
__global__ __launch_bounds__(256) void mosaic_kernel(const MosArgs a, float* __restrict__ out, int n) {
  constexpr int thirds = OUT / 4 / QW, groups = OUT / 8, per_img = 3 * groups * thirds;      // 432 workgroups per image
  for (int blk = blockIdx.x; blk < n * per_img; blk += gridDim.x) {
    const int b = blk / per_img, rest = blk % per_img;
    const int c = rest / (groups * thirds), third = rest % thirds;
    const int y = ((rest / thirds) % groups) * 8 + (int)threadIdx.x / QW;
    const int x0 = 4 * (third * QW + (int)threadIdx.x % QW);
    const MosImg& d = a.im[b];
    const int bl = d.bl, right = x0 >= HALF ? 1 : 0;               // (192 is a multiple of 4: a chunk lies in one half)
    const bool cseam = right ? x0 - HALF < bl : x0 + 3 >= HALF - bl;
    const HalfRow own = half_row(d, right, c, y);
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = half_at(own, bl + x0 + e - right * HALF);
    if (cseam) {
      const HalfRow oth = half_row(d, 1 - right, c, y);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int x = x0 + e;
        const int i = right ? x - HALF : HALF - 1 - x;
        if (i < bl) {
          const float w_kept = (float)(i + bl) / (float)(2 * bl), w_over = (float)(bl - i) / (float)(2 * bl);
          v[e] = clamp01(v[e] * w_kept + half_at(oth, right ? HALF - 1 + bl + i : bl - i) * w_over);
        }
      }
    }
    *reinterpret_cast<float4*>(out + (((int64_t)d.row * 3 + c) * OUT + y) * OUT + x0) = make_float4(v[0], v[1], v[2], v[3]);
  }
}

}  // namespace

extern "C" int countr_aug_mosaic(const countr_mosaic_image* imgs, int n, float* out, int out_rows, void* stream) {
  static thread_local char msg[200];
  if (!imgs || n < 1 || n > MAX_IMGS) {
    snprintf(msg, sizeof msg, "countr_aug_mosaic: 1..%d images per call", MAX_IMGS);
    countr_set_error(msg); return -1;
  }
  if (!out || (((uintptr_t)out) & 15) || out_rows < 1) {
    countr_set_error("countr_aug_mosaic: out must be a 16-byte aligned [out_rows, 3, 384, 384] tensor, out_rows >= 1"); return -1;
  }
  MosArgs a;
  for (int j = 0; j < MAX_IMGS; ++j) {
    const countr_mosaic_image& s = imgs[j < n ? j : n - 1];
    MosImg& d = a.im[j];
    if (s.bl < 10 || s.bl > 20) { countr_set_error("countr_aug_mosaic: bl lies in 10..20"); return -1; }
    if (s.row < 0 || s.row >= out_rows) { countr_set_error("countr_aug_mosaic: an image's row lies outside 0..out_rows - 1"); return -1; }
    const int resize_l = OUT / 2 + 2 * s.bl;
    for (int k = 0; k < 4; ++k) {
      const countr_mosaic_piece& q = s.piece[k];
      if (!q.src || q.h < 1 || q.w < 1 || (int64_t)q.h * q.w > (int64_t)1 << 26) {
        countr_set_error("countr_aug_mosaic: a piece lacks src or has a bad frame size"); return -1;
      }
      if (q.length < 1 || q.length > (q.h < q.w ? q.h : q.w)) { countr_set_error("countr_aug_mosaic: length lies in 1..min(h, w)"); return -1; }
      if (q.start_h < 0 || q.start_w < 0 || q.start_h > q.h - q.length || q.start_w > q.w - q.length) {
        countr_set_error("countr_aug_mosaic: a piece's length x length crop does not lie inside its frame"); return -1;
      }
      d.p[k].org = q.src + (int64_t)q.start_h * q.w + q.start_w;
      d.p[k].plane = q.h * q.w; d.p[k].w = q.w; d.p[k].length = q.length;
      d.p[k].scale = (float)q.length / (float)resize_l;
    }
    d.bl = s.bl; d.row = s.row;
  }
  const int blocks = n * 3 * (OUT / 8) * (OUT / 4 / QW);
  hipLaunchKernelGGL(mosaic_kernel, dim3(blocks < 2048 ? blocks : 2048), dim3(256), 0, STREAM(stream), a, out, n);
  return countr_check_launch("countr_aug_mosaic");
}
