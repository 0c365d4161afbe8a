// The pictures of the reference's evaluation report (FSC_test_cross(few-shot).py:379-425), composed on the device as the bytes PIL encodes.
//   countr_report_panels      `full_*.png` of a group of <= 16 images of one height, widths free: error / exemplar / true-positive panels
//                             (or exemplar / density panels of an image without objects) from the sample, the stitched map (or the nine
//                             maps of the 3 x 3 path), the ground-truth map, the exemplar rectangles and the host-rasterised label patch;
//                             one launch, uint8 [h, P w, 3] per image at its offset of one packed buffer
//   countr_report_strip_shape (host only) the size of an exemplar picture
//   countr_report_quantize    `boxes_*.png` of the group: torchvision's make_grid of each image's exemplars, quantised; one launch
// Every value is computed per pixel in fp32 in the script's operation order, every product and sum rounded on its own (no fused
// multiply-adds in this file), and quantised as torchvision's save_image does -- the host statement countr_amd/report.py::compose_host
// gives the same bytes.  A bandwidth kernel: every input is read once, 16-byte loads and 4-byte stores where the width allows.
// uint8 / fp32 only: the bf16 and the fp16 build of the library export the same code.
#include "common.hpp"
#include "../../include/countr_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int MAX_IMAGES = COUNTR_REPORT_MAX_IMAGES;
constexpr int MAX_BLOCKS = 4096;
constexpr int PX = 4;                            // pixels of a row per work item
constexpr int GRID_ROW = 8, GRID_PAD = 2;        // torchvision.utils.make_grid defaults (save_image passes them on)

struct PanelImage {
  countr_report_image d;
  int per;                                       // work items per row: ceil(w / PX)
  int vec;                                       // w % 4 == 0 and 16-byte aligned inputs, 4-byte aligned panel
  int64_t first;                                 // index of the image's first work item among the group's
};
struct PanelArgs {
  PanelImage im[MAX_IMAGES];
  int n, h;
  int64_t items;
};

// save_image: mul(255).add_(0.5).clamp_(0, 255).to(uint8)
__device__ __forceinline__ uint32_t quant(float x) {
  const float v = x * 255.f + 0.5f;
  return (uint32_t)(int)fminf(fmaxf(v, 0.f), 255.f);
}

__device__ __forceinline__ void patch_at(const uint8_t* __restrict__ blob, const countr_report_patch& pt, int x, int y, float v[3]) {
  const int u = x - pt.px, t = y - pt.py;
  v[0] = v[1] = v[2] = 0.f;
  if (u >= 0 && u < pt.pw && t >= 0 && t < pt.ph) {
    const uint8_t* q = blob + pt.off + ((int64_t)t * pt.pw + u) * 3;
    v[0] = (float)q[0]; v[1] = (float)q[1]; v[2] = (float)q[2];
  }
}

// The three channels of panel k at one pixel.  s: sample, p: pred, g: gt, box: 0 or 255, add: the label (layout 3) or text (layout 2) raster.
__device__ __forceinline__ void panel_pixel(int layout, int k, const float s[3], float p, float g, float box, const float add[3], float o[3]) {
  if (layout == 3) {
    if (k == 0) {                                // mix2 = sam * 0.6 + (pred_img.clamp(0, 1) - gt_img.clamp(0, 1)).abs()
      o[0] = s[0] * 0.6f + fabsf(clamp01(p) - clamp01(g));
      o[1] = s[1] * 0.6f + fabsf(clamp01(p) - 0.f);
      o[2] = s[2] * 0.6f + 0.f;
    } else if (k == 1) {                         // sam_box = clamp(sam + box_map + labels, 0, 1)
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c] = clamp01((s[c] + box) + add[c]);
    } else {                                     // tp_img = sam * 0.6 + (pred_img - fp_img)[[1, 0, 2]], fp_img = pred_img where gt_img - pred_img < -0.01
      const float fp0 = (g - p) < -0.01f ? p : 0.f;
      const float fp1 = (0.f - p) < -0.01f ? p : 0.f;
      o[0] = s[0] * 0.6f + (p - fp1);
      o[1] = s[1] * 0.6f + (p - fp0);
      o[2] = s[2] * 0.6f + 0.f;
    }
  } else {
    if (k == 0) {                                // sam_box = clamp(sam + box_map, 0, 1)
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c] = clamp01(s[c] + box);
    } else {                                     // den_pr = clamp(sam * 0.6 + text + pred_img, 0, 1)
      o[0] = clamp01((s[0] * 0.6f + add[0]) + p);
      o[1] = clamp01((s[1] * 0.6f + add[1]) + p);
      o[2] = clamp01((s[2] * 0.6f + add[2]) + 0.f);
    }
  }
}

// One work item = PX neighbouring pixels of one row of one image, all its panels: the sample, pred and gt are read once.
__global__ __launch_bounds__(256) void panels_kernel(const PanelArgs a, const uint8_t* __restrict__ blob, const int* __restrict__ rects,
                                                     uint8_t* __restrict__ out) {
  for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < a.items; it += (int64_t)gridDim.x * 256) {
    int f = 0;
    while (f + 1 < a.n && a.im[f + 1].first <= it) ++f;
    const PanelImage& im = a.im[f];
    const countr_report_image& d = im.d;
    const int h = a.h, w = d.w;
    const int64_t local = it - im.first;
    const int y = (int)(local / im.per), x0 = (int)(local % im.per) * PX;
    const int npx = min(PX, w - x0);
    const int64_t plane = (int64_t)h * w, at = (int64_t)y * w + x0;
    float s[3][PX], p[PX], g[PX], box[PX];
    if (im.vec) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float4 v = *reinterpret_cast<const float4*>(d.sam + c * plane + at);
        s[c][0] = v.x; s[c][1] = v.y; s[c][2] = v.z; s[c][3] = v.w;
      }
      const float4 v = *reinterpret_cast<const float4*>(d.gt + at);
      g[0] = v.x; g[1] = v.y; g[2] = v.z; g[3] = v.w;
      if (!d.grid) {
        const float4 q = *reinterpret_cast<const float4*>(d.maps[0] + at);
        p[0] = q.x; p[1] = q.y; p[2] = q.z; p[3] = q.w;
      }
    } else {
#pragma unroll
      for (int e = 0; e < PX; ++e) {
        const bool in = e < npx;
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c][e] = in ? d.sam[c * plane + at + e] : 0.f;
        g[e] = in ? d.gt[at + e] : 0.f;
        if (!d.grid) p[e] = in ? d.maps[0][at + e] : 0.f;
      }
    }
    if (d.grid) {
      // misc.make_grid: the nine maps tiled 3 x 3 (row-major, list order), then the tensor Resize [3 h, 3 w] -> [h, w] (bilinear,
      // align_corners=False, no antialias).  Its source coordinate (d + 0.5) * 3 - 0.5 = 3 d + 1 is an integer, so the second tap of
      // each axis has weight 0 and the first weight 1: the resize is this point sample, exactly (tests/test_report_cpu.py checks it
      // against F.interpolate).
      const int Y = 3 * y + 1;
      const int ty = Y / h, yy = Y - ty * h;
#pragma unroll
      for (int e = 0; e < PX; ++e) {
        const int X = 3 * min(x0 + e, w - 1) + 1;
        const int tx = X / w, xx = X - tx * w;
        p[e] = d.maps[3 * ty + tx][(int64_t)yy * w + xx];
      }
    }
#pragma unroll
    for (int e = 0; e < PX; ++e) box[e] = 0.f;
    for (int r = 0; r < d.rect_cnt; ++r) {
      const int4 q = *reinterpret_cast<const int4*>(rects + 4 * (int64_t)(d.rect_off + r));      // {y1, x1, y2, x2}
      const int y1 = min(q.x, q.z), y2 = max(q.x, q.z), x1 = min(q.y, q.w), x2 = max(q.y, q.w);
      const bool on_row = y == y1 || y == y2, in_rows = y >= y1 && y <= y2;
#pragma unroll
      for (int e = 0; e < PX; ++e) {
        const int x = x0 + e;
        if ((on_row && x >= x1 && x <= x2) || (in_rows && (x == x1 || x == x2))) box[e] = 255.f;
      }
    }
    const countr_report_patch& pt = d.layout == 3 ? d.labels : d.text;
    float add[PX][3];
#pragma unroll
    for (int e = 0; e < PX; ++e) patch_at(blob, pt, x0 + e, y, add[e]);
    uint8_t* row = out + d.out_off + (int64_t)y * d.layout * w * 3;
    for (int k = 0; k < d.layout; ++k) {
      uint32_t b[PX * 3];
#pragma unroll
      for (int e = 0; e < PX; ++e) {
        const float sp[3] = {s[0][e], s[1][e], s[2][e]};
        float o[3];
        panel_pixel(d.layout, k, sp, p[e], g[e], box[e], add[e], o);
#pragma unroll
        for (int c = 0; c < 3; ++c) b[3 * e + c] = quant(o[c]);
      }
      uint8_t* o8 = row + ((int64_t)k * w + x0) * 3;
      if (im.vec) {
        uint32_t* o32 = reinterpret_cast<uint32_t*>(o8);
#pragma unroll
        for (int j = 0; j < 3; ++j) o32[j] = b[4 * j] | (b[4 * j + 1] << 8) | (b[4 * j + 2] << 16) | (b[4 * j + 3] << 24);
      } else {
#pragma unroll
        for (int j = 0; j < PX * 3; ++j)
          if (j < npx * 3) o8[j] = (uint8_t)b[j];
      }
    }
  }
}

struct Strip {
  const float* ex;
  int64_t out_off, first;                        // first: index of the strip's first output pixel among the group's
  int S, gh, gw;
};
struct StripArgs {
  Strip s[MAX_IMAGES];
  int n, eh, ew;
  int64_t items;
};

// One thread = one pixel of one strip's picture: an exemplar's pixel or the padding (value 0).
__global__ __launch_bounds__(256) void strips_kernel(const StripArgs a, uint8_t* __restrict__ out) {
  for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < a.items; it += (int64_t)gridDim.x * 256) {
    int f = 0;
    while (f + 1 < a.n && a.s[f + 1].first <= it) ++f;
    const Strip& t = a.s[f];
    const int64_t local = it - t.first;
    const int gy = (int)(local / t.gw), gx = (int)(local % t.gw);
    int k = -1, yy = 0, xx = 0;
    if (t.S == 1) { k = 0; yy = gy; xx = gx; }   // make_grid hands a single image back as it is
    else {
      const int cy = gy - GRID_PAD, cx = gx - GRID_PAD, ch = a.eh + GRID_PAD, cw = a.ew + GRID_PAD;
      if (cy >= 0 && cx >= 0) {
        const int r = cy / ch, c = cx / cw;
        yy = cy - r * ch; xx = cx - c * cw;
        const int cols = min(GRID_ROW, t.S);
        if (yy < a.eh && xx < a.ew && c < cols && r * cols + c < t.S) k = r * cols + c;
      }
    }
    uint8_t* o = out + t.out_off + local * 3;
    const int64_t plane = (int64_t)a.eh * a.ew;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = (uint8_t)quant(k < 0 ? 0.f : t.ex[((int64_t)k * 3 + c) * plane + (int64_t)yy * a.ew + xx]);
  }
}

bool patch_ok(const countr_report_patch& p, int64_t blob_bytes) {
  if (p.pw < 0 || p.ph < 0) return false;
  if (p.pw == 0 || p.ph == 0) return true;
  return p.off >= 0 && (int64_t)p.pw * p.ph * 3 <= blob_bytes - p.off && p.off <= blob_bytes;
}

}  // namespace

extern "C" int countr_report_panels(const countr_report_image* imgs, int n, int h, const void* blob, int64_t blob_bytes, int64_t rects_off,
                                    int nrects, void* out, int64_t out_bytes, void* stream) {
  if (!imgs || !out || n < 1 || n > MAX_IMAGES || h < 1 || h > 1 << 14 || blob_bytes < 0 || out_bytes < 1 || nrects < 0 || rects_off < 0 ||
      (rects_off & 15) != 0 || (nrects > 0 && (!blob || (int64_t)nrects * 16 > blob_bytes - rects_off))) {
    countr_set_error("countr_report_panels: bad args (1..16 images, h >= 1, rectangles 16-byte aligned inside the blob)"); return -1;
  }
  if (blob && (((uintptr_t)blob) & 15) != 0) { countr_set_error("countr_report_panels: the blob must be 16-byte aligned"); return -1; }
  PanelArgs a;
  a.n = n; a.h = h;
  int64_t items = 0;
  for (int j = 0; j < MAX_IMAGES; ++j) {
    const countr_report_image& d = imgs[j < n ? j : n - 1];
    PanelImage& im = a.im[j];
    im.d = d;
    if (j >= n) { im.per = 1; im.vec = 0; im.first = items; continue; }
    if (!d.sam || !d.gt || !d.maps[0] || d.w < 1 || d.w > 1 << 20 || (d.layout != 2 && d.layout != 3)) {
      countr_set_error("countr_report_panels: an image needs sam, maps[0], gt, w >= 1 and layout 2 or 3"); return -1;
    }
    if (d.grid) {
      for (int k = 0; k < 9; ++k)
        if (!d.maps[k]) { countr_set_error("countr_report_panels: the 3 x 3 layout needs nine maps"); return -1; }
    }
    if (d.rect_cnt < 0 || d.rect_off < 0 || (int64_t)d.rect_off + d.rect_cnt > nrects) {
      countr_set_error("countr_report_panels: an image's rectangles lie outside the group's list"); return -1;
    }
    const countr_report_patch& pt = d.layout == 3 ? d.labels : d.text;
    if (!patch_ok(pt, blob_bytes) || (pt.pw > 0 && pt.ph > 0 && !blob)) {
      countr_set_error("countr_report_panels: a label / text raster lies outside the blob"); return -1;
    }
    const int64_t bytes = (int64_t)h * d.layout * d.w * 3;
    if (d.out_off < 0 || bytes > out_bytes - d.out_off || d.out_off > out_bytes) {
      countr_set_error("countr_report_panels: a panel lies outside the output buffer"); return -1;
    }
    for (int k = 0; k < j; ++k) {
      const int64_t o = imgs[k].out_off, b = (int64_t)h * imgs[k].layout * imgs[k].w * 3;
      if (d.out_off < o + b && o < d.out_off + bytes) { countr_set_error("countr_report_panels: two panels overlap"); return -1; }
    }
    im.per = (d.w + PX - 1) / PX;
    bool vec = (d.w & 3) == 0 && (((uintptr_t)d.sam | (uintptr_t)d.gt) & 15) == 0 && (((uintptr_t)out + (uintptr_t)d.out_off) & 3) == 0;
    if (!d.grid) vec = vec && (((uintptr_t)d.maps[0]) & 15) == 0;
    im.vec = vec ? 1 : 0;
    im.first = items;
    items += (int64_t)h * im.per;
  }
  a.items = items;
  const int blocks = countr_blocks_for(items, MAX_BLOCKS);
  const uint8_t* b8 = (const uint8_t*)blob;
  hipLaunchKernelGGL(panels_kernel, dim3(blocks), dim3(256), 0, STREAM(stream), a, b8, (const int*)(b8 ? b8 + rects_off : nullptr), (uint8_t*)out);
  return countr_check_launch("countr_report_panels");
}

extern "C" int countr_report_strip_shape(int S, int eh, int ew, int* shape) {
  if (!shape || S < 1 || eh < 1 || ew < 1 || S > 1 << 16 || eh > 1 << 12 || ew > 1 << 12) {
    countr_set_error("countr_report_strip_shape: bad args"); return -1;
  }
  if (S == 1) { shape[0] = eh; shape[1] = ew; return 0; }
  const int cols = S < GRID_ROW ? S : GRID_ROW, rows = (S + cols - 1) / cols;
  shape[0] = (eh + GRID_PAD) * rows + GRID_PAD;
  shape[1] = (ew + GRID_PAD) * cols + GRID_PAD;
  return 0;
}

extern "C" int countr_report_quantize(const countr_report_strip* strips, int n, int eh, int ew, void* out, int64_t out_bytes, void* stream) {
  if (!strips || !out || n < 1 || n > MAX_IMAGES || out_bytes < 1) { countr_set_error("countr_report_quantize: bad args (1..16 strips)"); return -1; }
  StripArgs a;
  a.n = n; a.eh = eh; a.ew = ew;
  int64_t items = 0;
  for (int j = 0; j < MAX_IMAGES; ++j) {
    const countr_report_strip& d = strips[j < n ? j : n - 1];
    Strip& t = a.s[j];
    int shape[2];
    if (!d.ex || countr_report_strip_shape(d.S, eh, ew, shape) != 0) { countr_set_error("countr_report_quantize: a strip needs exemplars [S >= 1, 3, eh, ew]"); return -1; }
    t.ex = d.ex; t.out_off = d.out_off; t.S = d.S; t.gh = shape[0]; t.gw = shape[1]; t.first = items;
    if (j >= n) continue;
    const int64_t bytes = (int64_t)shape[0] * shape[1] * 3;
    if (d.out_off < 0 || d.out_off > out_bytes || bytes > out_bytes - d.out_off) { countr_set_error("countr_report_quantize: a picture lies outside the output buffer"); return -1; }
    for (int k = 0; k < j; ++k)
      if (d.out_off < a.s[k].out_off + (int64_t)a.s[k].gh * a.s[k].gw * 3 && a.s[k].out_off < d.out_off + bytes) {
        countr_set_error("countr_report_quantize: two pictures overlap"); return -1;
      }
    items += (int64_t)shape[0] * shape[1];
  }
  a.items = items;
  hipLaunchKernelGGL(strips_kernel, dim3(countr_blocks_for(items, MAX_BLOCKS)), dim3(256), 0, STREAM(stream), a, (uint8_t*)out);
  return countr_check_launch("countr_report_quantize");
}
