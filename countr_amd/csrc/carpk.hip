// The CARPK pair of the reference (FSC_test_CARPK.py, FSC_finetune_CARPK.py): what those scripts do around SupervisedMAE.forward.
//   countr_carpk_prep_u8  uint8 [H, W, 3] frames -> the fp32 planar image of torchvision's TENSOR Resize (0.14.1: plain
//                         F.interpolate(frame / 255, bilinear, align_corners=False), no antialias -- not Pillow's resample of
//                         frames.hip) and the 64 x 64 exemplars cut from the ORIGINAL-resolution frame (FSC_test_CARPK.py:154-172,
//                         :191), both in one launch; the source index is bilinear.hpp's, the blend on uint8 / 255 is this file's
//   countr_carpk_count    the script's count rule on stitched maps (:220-243): 16 x 16 cell sums / 60, minus one per cell above
//                         1.224, plus 2 when the two exemplar rectangles hold at most half an object each
// uint8 / fp32 only: the bf16 and the fp16 build of the library export the same code.
#include "common.hpp"
#include "bilinear.hpp"      // contraction ON (above the pragma below): the source index of carpk_prep_kernel may be fused, as it always has been
#include "../../include/countr_hip.h"

namespace {

constexpr int MAX_FRAMES = COUNTR_CARPK_MAX_FRAMES, MAX_RECTS = 2 * MAX_FRAMES;
constexpr int BOX = 64;                          // exemplar crops are 64 x 64 (FSC_test_CARPK.py:171)
constexpr int MAX_BLOCKS = 4096;
constexpr int CELL = 16;                         // the count rule's Conv2d(1, 1, 16, stride 16)
constexpr int MAX_COUNT_BLOCKS = 32;

struct PrepArgs {
  const uint8_t* src[MAX_FRAMES];                // uint8 [H, W, 3]
  int H[MAX_FRAMES], W[MAX_FRAMES];
  int rf[MAX_RECTS];                             // frame of rectangle r
  int y0[MAX_RECTS], x0[MAX_RECTS], ch[MAX_RECTS], cw[MAX_RECTS];   // first row / column and size after clipping to the frame
};

// No fused multiply-adds in the blend of the kernel below: its vector and its scalar form must give the same bits (the training crop
// equals the test image's left columns), and torch's CPU kernel rounds every product.  The source index (bilinear_src, parsed above
// this pragma) may be contracted; it is one function for both forms.
#pragma clang fp contract(off)

// One work item = PX neighbouring output pixels of one row, all three channels: the 2 x 2 source neighbourhood of a pixel (12 bytes of
// the interleaved frame) is read once and feeds the three planes.  Items [0, frame_items) are the resized frames, the rest the
// exemplars; consecutive threads take consecutive x, so every plane is written in runs along x.  VEC: PX = 4 and one 16-byte store per
// plane (out_cols % 4 == 0, aligned outputs); otherwise one pixel per thread.
template <bool VEC>
__global__ __launch_bounds__(256) void carpk_prep_kernel(const PrepArgs a, float* __restrict__ img, float* __restrict__ ex, int n, int nrects,
                                                         int out_h, int out_w, int out_cols) {
  constexpr int PX = VEC ? 4 : 1;
  const int per = out_cols / PX, per_box = BOX / PX;
  const int64_t frame_items = (int64_t)n * out_h * per;
  const int64_t total = frame_items + (int64_t)nrects * BOX * per_box;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const uint8_t* src;
    float* o;
    int64_t plane;
    int W, ch, cw, oh, ow, oy, ox0;
    if (i < frame_items) {
      const int q = (int)(i % per);
      const int64_t fy = i / per;
      const int f = (int)(fy / out_h);
      oy = (int)(fy % out_h); ox0 = q * PX;
      W = a.W[f]; ch = a.H[f]; cw = W; oh = out_h; ow = out_w;
      src = a.src[f];
      plane = (int64_t)out_h * out_cols;
      o = img + (int64_t)f * 3 * plane + (int64_t)oy * out_cols + ox0;
    } else {
      const int64_t j = i - frame_items;
      const int q = (int)(j % per_box);
      const int64_t ry = j / per_box;
      const int r = (int)(ry / BOX);
      oy = (int)(ry % BOX); ox0 = q * PX;
      const int f = a.rf[r];
      W = a.W[f]; ch = a.ch[r]; cw = a.cw[r]; oh = BOX; ow = BOX;
      src = a.src[f] + ((int64_t)a.y0[r] * W + a.x0[r]) * 3;
      plane = BOX * BOX;
      o = ex + (int64_t)r * 3 * plane + oy * BOX + ox0;
    }
    int y1, yp, x1, xp;
    float ly, lx;
    bilinear_src(ch, bilinear_scale(ch, oh), oy, &y1, &yp, &ly);
    const float ly0 = 1.f - ly;
    const uint8_t* r0 = src + (int64_t)y1 * W * 3;
    const uint8_t* r1 = r0 + (int64_t)yp * W * 3;
    float v[3][PX];
#pragma unroll
    for (int e = 0; e < PX; ++e) {
      bilinear_src(cw, bilinear_scale(cw, ow), ox0 + e, &x1, &xp, &lx);
      const float lx0 = 1.f - lx;
      const uint8_t* p00 = r0 + x1 * 3;
      const uint8_t* p01 = p00 + xp * 3;
      const uint8_t* p10 = r1 + x1 * 3;
      const uint8_t* p11 = p10 + xp * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        // frame / 255 is a correctly rounded division in the reference (:154), not x * (1 / 255)
        const float t00 = (float)p00[c] / 255.0f, t01 = (float)p01[c] / 255.0f, t10 = (float)p10[c] / 255.0f, t11 = (float)p11[c] / 255.0f;
        v[c][e] = ly0 * (lx0 * t00 + lx * t01) + ly * (lx0 * t10 + lx * t11);
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (VEC) *reinterpret_cast<float4*>(o + c * plane) = make_float4(v[c][0], v[c][1 % PX], v[c][2 % PX], v[c][3 % PX]);
      else o[c * plane] = v[c][0];
    }
  }
}

struct CountArgs {
  int r0[2 * MAX_FRAMES], r1[2 * MAX_FRAMES], c0[2 * MAX_FRAMES], c1[2 * MAX_FRAMES];   // rows [r0, r1) x columns [c0, c1) of the map, clipped
};

// Block (b, image i): wave w sums the cells b * 4 + w, + 4 * blocks, ... (one 16 x 16 cell = 4 values per lane, then the wave's
// butterfly) and keeps {sum of cell values, cells above the threshold}; the block then walks the rows r0 + b, + blocks, ... of the two
// rectangles.  partial[i][b] = {total, n_over, rect 0, rect 1}.  Every sum has a fixed order: no atomics, two runs give the same bits.
__global__ __launch_bounds__(256) void carpk_count_kernel(const float* __restrict__ maps, const CountArgs a, int H, int W, float* __restrict__ partial,
                                                          int blocks) {
  __shared__ float sm[4][4];
  const int i = blockIdx.y, b = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* m = maps + (int64_t)i * H * W;
  const int cw = W / CELL, cells = (H / CELL) * cw;
  float total = 0.f, over = 0.f;
  for (int c = b * 4 + wave; c < cells; c += 4 * blocks) {
    const int cy = c / cw, cx = c - cy * cw;
    const float* p = m + (int64_t)(cy * CELL + (lane >> 2)) * W + cx * CELL + (lane & 3) * 4;
    const float s = wave_sum((p[0] + p[1]) + (p[2] + p[3]));
    const float cell = s / 60.f;
    total += cell;
    over += cell > 1.224f ? 1.f : 0.f;
  }
  float e[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int r0 = a.r0[2 * i + k], r1 = a.r1[2 * i + k], c0 = a.c0[2 * i + k], c1 = a.c1[2 * i + k];
    float acc = 0.f;
    for (int y = r0 + b; y < r1; y += blocks)
      for (int x = c0 + threadIdx.x; x < c1; x += 256) acc += m[(int64_t)y * W + x];
    e[k] = wave_sum(acc);
  }
  if (lane == 0) { sm[wave][0] = total; sm[wave][1] = over; sm[wave][2] = e[0]; sm[wave][3] = e[1]; }
  __syncthreads();
  if (threadIdx.x < 4) {
    const int k = threadIdx.x;
    partial[((int64_t)i * blocks + b) * 4 + k] = (sm[0][k] + sm[1][k]) + (sm[2][k] + sm[3][k]);
  }
}

// out[i] = {pred, total, n_over, e_cnt} from the image's block partials, in block order
__global__ __launch_bounds__(64) void carpk_fold_kernel(const float* __restrict__ partial, float* __restrict__ out, int blocks) {
  const int i = blockIdx.x, k = threadIdx.x;
  __shared__ float r[4];
  if (k < 4) {
    float acc = 0.f;
    for (int b = 0; b < blocks; ++b) acc += partial[((int64_t)i * blocks + b) * 4 + k];
    r[k] = acc;
  }
  __syncthreads();
  if (k == 0) {
    const float e_cnt = (r[2] / 60.f + r[3] / 60.f) / 2.f;
    out[4 * i] = r[0] - r[1] + (e_cnt <= 0.5f ? 2.f : 0.f);
    out[4 * i + 1] = r[0]; out[4 * i + 2] = r[1]; out[4 * i + 3] = e_cnt;
  }
}

}  // namespace

extern "C" int countr_carpk_prep_u8(const void* const* frames, const int* shapes, int n, const int* rects, int nrects, int out_h, int out_w,
                                    int out_cols, float* img, float* ex, void* stream) {
  if (!frames || !shapes || !img || n < 1 || n > MAX_FRAMES || nrects < 0 || nrects > MAX_RECTS || (nrects > 0 && (!rects || !ex)) ||
      out_h < 1 || out_w < 1 || out_cols < 1 || out_cols > out_w || (int64_t)out_h * out_w > (int64_t)1 << 28) {
    countr_set_error("countr_carpk_prep_u8: bad args (1..16 frames, 0..32 rectangles, 1 <= out_cols <= out_w)"); return -1;
  }
  PrepArgs a;
  for (int j = 0; j < MAX_FRAMES; ++j) {
    const int s = j < n ? j : n - 1;
    const int H = shapes[2 * s], W = shapes[2 * s + 1];
    if (!frames[s] || H < 1 || W < 1 || (int64_t)H * W > (int64_t)1 << 28) { countr_set_error("countr_carpk_prep_u8: null frame or frame size out of range"); return -1; }
    a.src[j] = (const uint8_t*)frames[s]; a.H[j] = H; a.W[j] = W;
  }
  for (int j = 0; j < MAX_RECTS; ++j) {
    if (nrects == 0) { a.rf[j] = 0; a.y0[j] = a.x0[j] = 0; a.ch[j] = a.cw[j] = 1; continue; }
    const int* r = rects + 5 * (j < nrects ? j : nrects - 1);      // {frame, y1, x1, y2, x2}, corners inclusive
    const char* bad = "countr_carpk_prep_u8: rectangle of a frame that is not there, or negative corner";
    if (r[0] < 0 || r[0] >= n) { countr_set_error(bad); return -1; }
    a.rf[j] = r[0];
    if (!clip_rect(r[1], r[2], r[3], r[4], a.H[r[0]], a.W[r[0]], &a.y0[j], &a.x0[j], &a.ch[j], &a.cw[j])) {      // corners inclusive
      countr_set_error(r[1] < 0 || r[2] < 0 ? bad : "countr_carpk_prep_u8: a rectangle is empty after clipping to its frame"); return -1;
    }
  }
  const bool vec = (out_cols & 3) == 0 && (((uintptr_t)img) & 15) == 0 && (nrects == 0 || (((uintptr_t)ex) & 15) == 0);
  const int px = vec ? 4 : 1;
  const int64_t threads = (int64_t)n * out_h * (out_cols / px) + (int64_t)nrects * BOX * (BOX / px);
  const int blocks = countr_blocks_for(threads, MAX_BLOCKS);
  if (vec) hipLaunchKernelGGL(carpk_prep_kernel<true>, dim3(blocks), dim3(256), 0, STREAM(stream), a, img, ex, n, nrects, out_h, out_w, out_cols);
  else hipLaunchKernelGGL(carpk_prep_kernel<false>, dim3(blocks), dim3(256), 0, STREAM(stream), a, img, ex, n, nrects, out_h, out_w, out_cols);
  return countr_check_launch("countr_carpk_prep_u8");
}

extern "C" int countr_carpk_count_blocks(int H, int W) {
  const int cells = (H / CELL) * (W / CELL);
  return max(1, min(MAX_COUNT_BLOCKS, cells / 16));
}

extern "C" int countr_carpk_count(const float* maps, int n, int H, int W, const int* rects, float* out, float* workspace, void* stream) {
  if (!maps || !rects || !out || !workspace || n < 1 || n > MAX_FRAMES || H < 1 || W < 1 || (int64_t)H * W > (int64_t)1 << 28) {
    countr_set_error("countr_carpk_count: bad args (1..16 maps, two rectangles each, out [n, 4] and the workspace are required)"); return -1;
  }
  CountArgs a;
  for (int j = 0; j < 2 * MAX_FRAMES; ++j) {
    const int* r = rects + 4 * (j < 2 * n ? j : 2 * n - 1);        // (a, b, c, d): map[a : a + c + 1, b : b + d + 1]
    if (r[0] < 0 || r[1] < 0 || r[2] < 0 || r[3] < 0) { countr_set_error("countr_carpk_count: negative rectangle entry"); return -1; }
    a.r0[j] = min(r[0], H); a.r1[j] = (int)min((int64_t)r[0] + r[2] + 1, (int64_t)H);
    a.c0[j] = min(r[1], W); a.c1[j] = (int)min((int64_t)r[1] + r[3] + 1, (int64_t)W);
    if (a.r1[j] < a.r0[j]) a.r1[j] = a.r0[j];
    if (a.c1[j] < a.c0[j]) a.c1[j] = a.c0[j];
  }
  const int blocks = countr_carpk_count_blocks(H, W);
  hipLaunchKernelGGL(carpk_count_kernel, dim3(blocks, n), dim3(256), 0, STREAM(stream), maps, a, H, W, workspace, blocks);
  hipLaunchKernelGGL(carpk_fold_kernel, dim3(n), dim3(64), 0, STREAM(stream), workspace, out, blocks);
  return countr_check_launch("countr_carpk_count");
}
