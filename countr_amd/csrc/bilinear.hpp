// torch's upsample_bilinear2d (align_corners=False, no antialias), the one copy of its source index and of the 2 x 2 blend on fp32
// planes, and the host's clipping of an inclusive rectangle as Python slicing clips it.
// ROUNDING RULE: this header carries NO fp-contract pragma.  Every expression below takes the contraction state in force where the
// header is parsed, i.e. at the #include line of the including file (the state travels with the inlined instructions): a file that wants
// each product and sum rounded on its own includes it BELOW its `#pragma clang fp contract(off)`, a file that lets the compiler fuse
// includes it above any such pragma.  Every #include of this header says which of the two it selects.  The choices differ between
// files and are kept as they are: changing one changes output bits.
#pragma once
#include "common.hpp"

__device__ __forceinline__ float bilinear_scale(int in_size, int out_size) { return (float)in_size / (float)out_size; }

// area_pixel_compute_source_index: src = scale * (dst + 0.5) - 0.5 clamped at 0 -> the first of the two samples, the step to its
// neighbour (0 at the last sample) and the neighbour's weight
__device__ __forceinline__ void bilinear_src(int in_size, float scale, int dst, int* i0, int* step, float* lambda) {
  const float s = fmaxf(scale * ((float)dst + 0.5f) - 0.5f, 0.f);
  const int i = min((int)s, in_size - 1);
  *i0 = i; *step = i < in_size - 1 ? 1 : 0; *lambda = s - (float)i;
}

// Output row oy of a ch x cw rectangle of an fp32 plane resized with the steps (sy, sx): its two source rows and their weights.  org:
// the rectangle's first pixel, pitch: the plane's row stride
struct BilinearRow {
  const float* s0;
  const float* s1;
  float ly, ly0, sx;
  int cw;
};
__device__ __forceinline__ BilinearRow bilinear_row(const float* org, int pitch, int ch, int cw, float sy, float sx, int oy) {
  BilinearRow t;
  int y1, yp;
  bilinear_src(ch, sy, oy, &y1, &yp, &t.ly);
  t.ly0 = 1.f - t.ly;
  t.s0 = org + (int64_t)y1 * pitch;
  t.s1 = t.s0 + (int64_t)yp * pitch;
  t.sx = sx; t.cw = cw;
  return t;
}
// ... and its pixel ox
__device__ __forceinline__ float bilinear_at(const BilinearRow& t, int ox) {
  int x1, xp;
  float lx;
  bilinear_src(t.cw, t.sx, ox, &x1, &xp, &lx);
  const float lx0 = 1.f - lx;
  return t.ly0 * (lx0 * t.s0[x1] + lx * t.s0[x1 + xp]) + t.ly * (lx0 * t.s1[x1] + lx * t.s1[x1 + xp]);
}

// (host) img[y1:y2 + 1, x1:x2 + 1] of an h x w image, corners inclusive: slicing clips both ends to the image.  False for a negative
// corner (slicing would count it from the far end) and for a rectangle that is empty after clipping
inline bool clip_rect(int y1, int x1, int y2, int x2, int h, int w, int* y0, int* x0, int* ch, int* cw) {
  if (y1 < 0 || x1 < 0) return false;
  *y0 = y1 < h ? y1 : h; *x0 = x1 < w ? x1 : w;
  *ch = (y2 < h ? y2 + 1 : h) - *y0; *cw = (x2 < w ? x2 + 1 : w) - *x0;
  return *ch >= 1 && *cw >= 1;
}
