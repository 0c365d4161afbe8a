// Line counts from density flux (include/countr_hip_flow.h states the rule).
//   countr_flow_workspace   (host only) bytes of scratch a flux call needs
//   countr_flow_luma        n <= 16 prepared images fp32 [3, h, w] -> lumas uint8 [h, w]
//   countr_flow_motion      n <= 16 (current, earlier) luma pairs -> motion fields int16 [h / 8, w / 8, 2]
//   countr_flow_flux        n <= 16 (map, motion, placement) triples against <= 16 lines -> flux[16][2] and total per map
// The launches, all on the caller's stream:
//   flow_luma_kernel     a thread per four pixels: three 16-byte loads, one 4-byte store
//   flow_motion_kernel   the hot one: cells x (2 r + 1)^2 candidates x 256 pixels.  A block of four waves takes four neighbouring cells of a
//                        cell row, a wave per cell.  The wave stages its 16 x 16 window and the (16 + 2 r)^2 search area in LDS as bytes
//                        (clamped coordinates, so the edge needs no special case afterwards).  A lane takes a candidate: per window row it
//                        reads the row (one 16-byte read, the same address in every lane: a broadcast) and five aligned words of the
//                        area, shifts them to the candidate's byte offset (v_alignbyte_b32) and adds four byte-SADs (v_sad_u8).  Every
//                        S(o) goes to LDS as 16 bits (S <= 256 * 255) for the sub-pixel step.  The first minimum in the rule's order is
//                        two butterflies over the wave: the smallest S, then the smallest order key (d2, oy, ox) that has it -- both are
//                        exact as floats -- so no execution order decides a tie.
//   flow_flux_kernel     a block per cell row of a map; the lines are walked one after the other (wave-uniform), membership and vn in
//                        fp64 with one operation per statement; lane, wave and block sums in the header's order
//   flow_fold_kernel     a thread per result of a map: the cell rows' partials in ascending order -- no atomic decides a sum
#include <math.h>
#include <stdio.h>
#include <string.h>
#include "../csrc/common.hpp"
#include "../csrc/host_api.hpp"
#include "../../include/countr_hip_flow.h"

#pragma clang fp contract(off)

namespace {

constexpr int MAXF = COUNTR_FLOW_MAX_FRAMES, MAXL = COUNTR_FLOW_MAX_LINES, MAXR = COUNTR_FLOW_MAX_SEARCH;
constexpr int CELL = COUNTR_FLOW_CELL, MAX_SIDE = COUNTR_FLOW_MAX_SIDE, OUTF = COUNTR_FLOW_OUT_FLOATS;
constexpr int WIN = 2 * CELL;                    // the window's side
constexpr int AROWS = WIN + 2 * MAXR;            // rows of the largest search area
constexpr int ASTRIDE = AROWS + 4;               // bytes of an area row in LDS: a candidate reads five aligned words from (2 r) & ~3 on
constexpr int MAXC = (2 * MAXR + 1) * (2 * MAXR + 1);
constexpr int WAVES = 4;
static_assert(WIN == 16 && ASTRIDE % 4 == 0 && ((2 * MAXR) & ~3) + 20 <= ASTRIDE, "five words from the candidate's aligned offset stay in the row");
static_assert(OUTF == 2 * MAXL + 1, "flux[16][2] and the total");

struct LumaArgs {
  const float* img[MAXF];
  unsigned char* luma[MAXF];
};

struct MotionArgs {
  const unsigned char* cur[MAXF];
  const unsigned char* old[MAXF];
  unsigned* mv[MAXF];                            // an int16 pair (x, y) as one word
};

struct FluxArgs {
  const float* map[MAXF];
  const short2* mv[MAXF];
  float* out[MAXF];
  double sx[MAXF], tx[MAXF], sy[MAXF], ty[MAXF];
  double ax[MAXL], ay[MAXL], ex[MAXL], ey[MAXL], len[MAXL], len2[MAXL], hw[MAXL];      // len, len2 and hw are formed on the host, in fp64
  double band, step;                             // step = 16 * interval
  int L;
};

__device__ __forceinline__ int byte_of(float v) {
  const int q = (int)__fadd_rn(__fmul_rn(v, 255.f), 0.5f);
  return q < 0 ? 0 : (q > 255 ? 255 : q);
}
__device__ __forceinline__ unsigned luma_of(float r, float g, float b) {
  return (unsigned)(77 * byte_of(r) + 150 * byte_of(g) + 29 * byte_of(b) + 128) >> 8;
}

__global__ __launch_bounds__(256) void flow_luma_kernel(const LumaArgs a, int quads) {      // quads = h * w / 4
  const int f = blockIdx.y;
  const float4* __restrict__ R = reinterpret_cast<const float4*>(a.img[f]);
  const float4* __restrict__ G = R + quads;
  const float4* __restrict__ B = G + quads;
  unsigned* __restrict__ out = reinterpret_cast<unsigned*>(a.luma[f]);
  for (int k = blockIdx.x * 256 + threadIdx.x; k < quads; k += gridDim.x * 256) {
    const float4 r = R[k], g = G[k], b = B[k];
    out[k] = luma_of(r.x, g.x, b.x) | (luma_of(r.y, g.y, b.y) << 8) | (luma_of(r.z, g.z, b.z) << 16) | (luma_of(r.w, g.w, b.w) << 24);
  }
}

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// the header's f: floor((16 (S- - S+) + den) / (2 den)) with den = max(S-, S+) - S0, or 0
__device__ __forceinline__ int subpel(int sm, int s0, int sp) {
  const int den = (sm > sp ? sm : sp) - s0;
  if (den <= 0) return 0;
  const int num = 16 * (sm - sp) + den, d = 2 * den;
  int q = num / d;
  if (num % d != 0 && num < 0) --q;
  return q;
}

__global__ __launch_bounds__(256) void flow_motion_kernel(const MotionArgs a, int h, int w, int r, int min_gain) {
  __shared__ __attribute__((aligned(16))) unsigned char s_win[WAVES][WIN * WIN];
  __shared__ __attribute__((aligned(16))) unsigned char s_area[WAVES][AROWS * ASTRIDE];
  __shared__ unsigned short s_S[WAVES][MAXC];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int f = blockIdx.z, j = blockIdx.y, Wc = w >> 3;
  const int i = blockIdx.x * WAVES + wave;
  const bool valid = i < Wc;                     // (wave-uniform; a wave without a cell still takes the barriers)
  const int D = 2 * r + 1, side = WIN + 2 * r, nc = D * D;
  const int y0 = CELL * j - CELL / 2, x0 = CELL * i - CELL / 2;
  if (valid) {
    const unsigned char* __restrict__ C = a.cur[f];
    const unsigned char* __restrict__ E = a.old[f];
    for (int k = lane; k < WIN * WIN; k += 64)
      s_win[wave][k] = C[(int64_t)clampi(y0 + (k >> 4), h - 1) * w + clampi(x0 + (k & 15), w - 1)];
    for (int k = lane; k < side * side; k += 64) {
      const int py = k / side, px = k - py * side;
      s_area[wave][py * ASTRIDE + px] = E[(int64_t)clampi(y0 - r + py, h - 1) * w + clampi(x0 - r + px, w - 1)];
    }
  }
  __syncthreads();
  unsigned bestS = 0xFFFFFFFFu, bestK = 0u;
  if (valid) {
    const uint4* __restrict__ win = reinterpret_cast<const uint4*>(s_win[wave]);
    for (int c0 = 0; c0 < nc; c0 += 64) {
      const int c = c0 + lane;
      if (c >= nc) continue;
      const int oyi = c / D, oxi = c - oyi * D;  // (oy + r, ox + r)
      const unsigned sh = (unsigned)oxi & 3u;
      const unsigned char* base = s_area[wave] + oyi * ASTRIDE + (oxi & ~3);
      unsigned S = 0u;
#pragma unroll 4
      for (int row = 0; row < WIN; ++row) {
        const unsigned* __restrict__ p = reinterpret_cast<const unsigned*>(base + row * ASTRIDE);
        const unsigned d0 = p[0], d1 = p[1], d2 = p[2], d3 = p[3], d4 = p[4];
        const uint4 wv = win[row];
        S = __builtin_amdgcn_sad_u8(wv.x, __builtin_amdgcn_alignbyte(d1, d0, sh), S);
        S = __builtin_amdgcn_sad_u8(wv.y, __builtin_amdgcn_alignbyte(d2, d1, sh), S);
        S = __builtin_amdgcn_sad_u8(wv.z, __builtin_amdgcn_alignbyte(d3, d2, sh), S);
        S = __builtin_amdgcn_sad_u8(wv.w, __builtin_amdgcn_alignbyte(d4, d3, sh), S);
      }
      s_S[wave][c] = (unsigned short)S;
      const int oy = oyi - r, ox = oxi - r;
      const unsigned key = (unsigned)(oy * oy + ox * ox) * 4096u + (unsigned)oyi * 64u + (unsigned)oxi;      // < 2^22: exact as a float
      if (S < bestS || (S == bestS && key < bestK)) { bestS = S; bestK = key; }
    }
  }
  __syncthreads();                               // (the sub-pixel step reads other lanes' S)
  if (valid) {
    const float ninf = -__builtin_inff();
    const float mine = bestS == 0xFFFFFFFFu ? ninf : -(float)bestS;      // (a lane without a candidate: r = 1 has 9)
    const float low = wave_max(mine);
    const float key = wave_max((mine == low && mine != ninf) ? -(float)bestK : ninf);
    const int k = (int)(-key);
    const int oyi = (k >> 6) & 63, oxi = k & 63;
    const unsigned short* S = s_S[wave];
    const int at = oyi * D + oxi;
    const int s0 = S[at], sz = S[r * D + r];
    int mx = 0, my = 0;
    if ((oyi == r && oxi == r) || sz - s0 >= min_gain) {
      const int fx = (oxi > 0 && oxi < 2 * r) ? subpel(S[at - 1], s0, S[at + 1]) : 0;
      const int fy = (oyi > 0 && oyi < 2 * r) ? subpel(S[at - D], s0, S[at + D]) : 0;
      mx = 16 * (oxi - r) + fx;
      my = 16 * (oyi - r) + fy;
    }
    if (lane == 0) a.mv[f][j * Wc + i] = ((unsigned)mx & 0xFFFFu) | ((unsigned)my << 16);
  }
}

__global__ __launch_bounds__(256) void flow_flux_kernel(const FluxArgs a, float* __restrict__ part, int h, int w) {
  __shared__ float s_part[WAVES][OUTF];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = blockIdx.x, f = blockIdx.y, Hc = h >> 3, Wc = w >> 3;
  const int chunks = (w + 63) >> 6;
  const float* __restrict__ m = a.map[f] + (int64_t)CELL * j * w;
  const short2* __restrict__ mv = a.mv[f] + (int64_t)j * Wc;
  const double sx = a.sx[f], tx = a.tx[f], sy = a.sy[f], ty = a.ty[f];

  // ---- the cell row's sum of all pixels
  {
    float t = 0.f;
    for (int c = wave; c < chunks; c += WAVES) {
      const int cx = c * 64 + lane;
      if (cx < w)
        for (int row = 0; row < CELL; ++row) t += m[row * w + cx];
    }
    t = wave_sum(t);
    if (lane == 0) s_part[wave][OUTF - 1] = t;
  }
  // ---- the lines, one after the other
  for (int k = 0; k < MAXL; ++k) {               // (wave-uniform)
    float fw = 0.f, bw = 0.f;
    if (k < a.L && a.len2[k] != 0.0) {
      const double ax = a.ax[k], ay = a.ay[k], ex = a.ex[k], ey = a.ey[k], len = a.len[k], len2 = a.len2[k], hw = a.hw[k];
      const double nhw = -hw;
      for (int c = wave; c < chunks; c += WAVES) {
        const int cx = c * 64 + lane;
        if (cx >= w) continue;
        const short2 o = mv[cx >> 3];
        if (o.x == 0 && o.y == 0) continue;      // (vn is +-0: the pixel adds nothing)
        const double mx = sx * (double)o.x, my = sy * (double)o.y;
        const double dx = -(mx / a.step), dy = -(my / a.step);
        const double v1 = dy * ex, v2 = dx * ey;
        const double v3 = v1 - v2;
        const double vn = v3 / len;
        if (!(vn > 0.0) && !(vn < 0.0)) continue;
        const double g0 = vn / a.band;
        const double g = g0 / 60.0;
        const double px = sx * (double)cx;
        const double Px = px + tx;
        const double ux = Px - ax;
        const double c1 = ey * ux, t1 = ex * ux;
        for (int row = 0; row < CELL; ++row) {
          const double py = sy * (double)(CELL * j + row);
          const double Py = py + ty;
          const double uy = Py - ay;
          const double c0 = ex * uy, t2 = ey * uy;
          const double cr = c0 - c1;
          const double t = t1 + t2;
          if (nhw <= cr && cr < hw && 0.0 <= t && t < len2) {
            const double mass = (double)m[row * w + cx];
            if (vn > 0.0) fw += (float)(mass * g);
            else bw += (float)(mass * -g);
          }
        }
      }
    }
    fw = wave_sum(fw);
    bw = wave_sum(bw);
    if (lane == 0) { s_part[wave][2 * k] = fw; s_part[wave][2 * k + 1] = bw; }
  }
  __syncthreads();
  if (threadIdx.x < OUTF) {
    float s = 0.f;
#pragma unroll
    for (int wv = 0; wv < WAVES; ++wv) s += s_part[wv][threadIdx.x];
    part[((int64_t)f * Hc + j) * OUTF + threadIdx.x] = s;
  }
}

__global__ __launch_bounds__(64) void flow_fold_kernel(const FluxArgs a, const float* __restrict__ part, int Hc) {
  const int f = blockIdx.x, k = threadIdx.x;
  if (k >= OUTF) return;
  const float* __restrict__ p = part + (int64_t)f * Hc * OUTF + k;
  float s = 0.f;
  for (int j0 = 0; j0 < Hc; j0 += 8) {           // eight independent loads at a time; the additions stay in ascending order
    float v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = j0 + q < Hc ? p[(int64_t)(j0 + q) * OUTF] : 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q)
      if (j0 + q < Hc) s += v[q];
  }
  a.out[f][k] = s;
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

extern "C" int countr_flow_version(void) { return COUNTR_FLOW_ABI_VERSION; }

extern "C" const char* countr_flow_last_error(void) { return g_err; }

extern "C" int countr_flow_workspace(int n, int h) {
  if (n < 1 || n > MAXF || bad_side(h))
    return failf(-1, "countr_flow_workspace: 1..%d maps of a height that is a multiple of %d in %d..%d, got %d of %d", MAXF, CELL, CELL,
                 MAX_SIDE, n, h);
  return n * (h / CELL) * OUTF * 4;
}

extern "C" int countr_flow_luma(const void* const* images, void* const* lumas, int n, int h, int w, void* stream) {
  const int rc = check_sizes("countr_flow_luma", n, h, w);
  if (rc) return rc;
  if (!images || !lumas) return fail(-2, "countr_flow_luma: the images and lumas arrays are required");
  LumaArgs a;
  memset(&a, 0, sizeof(a));
  for (int k = 0; k < n; ++k) {
    if (!images[k] || !lumas[k]) return failf(-2, "countr_flow_luma: frame %d has a null pointer", k);
    if (misaligned(images[k], 16) || misaligned(lumas[k], 4))
      return failf(-5, "countr_flow_luma: frame %d: the image is 16-byte aligned, the luma 4-byte aligned", k);
    a.img[k] = (const float*)images[k];
    a.luma[k] = (unsigned char*)lumas[k];
  }
  const int quads = h * w / 4;
  hipLaunchKernelGGL(flow_luma_kernel, dim3(countr_blocks_for(quads, 256), n), dim3(256), 0, STREAM(stream), a, quads);
  return launched("countr_flow_luma");
}

extern "C" int countr_flow_motion(const void* const* current, const void* const* earlier, void* const* motion, int n, int h, int w,
                                  int search, int min_gain, void* stream) {
  const int rc = check_sizes("countr_flow_motion", n, h, w);
  if (rc) return rc;
  if (search < 1 || search > MAXR) return failf(-3, "countr_flow_motion: search is 1..%d, got %d", MAXR, search);
  if (min_gain < 0) return failf(-3, "countr_flow_motion: min_gain is >= 0, got %d", min_gain);
  if (!current || !earlier || !motion) return fail(-2, "countr_flow_motion: the current, earlier and motion arrays are required");
  MotionArgs a;
  memset(&a, 0, sizeof(a));
  for (int k = 0; k < n; ++k) {
    if (!current[k] || !earlier[k] || !motion[k]) return failf(-2, "countr_flow_motion: pair %d has a null pointer", k);
    if (misaligned(motion[k], 4)) return failf(-5, "countr_flow_motion: pair %d: the motion field is 4-byte aligned", k);
    a.cur[k] = (const unsigned char*)current[k];
    a.old[k] = (const unsigned char*)earlier[k];
    a.mv[k] = (unsigned*)motion[k];
  }
  const int Wc = w / CELL, Hc = h / CELL;
  hipLaunchKernelGGL(flow_motion_kernel, dim3((Wc + WAVES - 1) / WAVES, Hc, n), dim3(256), 0, STREAM(stream), a, h, w, search, min_gain);
  return launched("countr_flow_motion");
}

extern "C" int countr_flow_flux(const countr_flow_map* maps, int n, int h, int w, const double* lines, int L, double band, int interval,
                                void* workspace, void* stream) {
  const int rc = check_sizes("countr_flow_flux", n, h, w);
  if (rc) return rc;
  if (L < 0 || L > MAXL) return failf(-3, "countr_flow_flux: 0..%d lines, got %d", MAXL, L);
  if (interval < 1 || interval > COUNTR_FLOW_MAX_INTERVAL)
    return failf(-3, "countr_flow_flux: interval is 1..%d, got %d", COUNTR_FLOW_MAX_INTERVAL, interval);
  if (!(band > 0.0) || !__builtin_isfinite(band)) return fail(-4, "countr_flow_flux: band is finite and > 0");
  if (!maps) return fail(-2, "countr_flow_flux: the maps array is required");
  if (L > 0 && !lines) return fail(-2, "countr_flow_flux: the lines array is required");
  if (!workspace || misaligned(workspace, 4)) return fail(-2, "countr_flow_flux: the workspace is required and 4-byte aligned");
  FluxArgs a;
  memset(&a, 0, sizeof(a));
  for (int k = 0; k < n; ++k) {
    const countr_flow_map& d = maps[k];
    if (!d.map || !d.motion || !d.out) return failf(-2, "countr_flow_flux: map %d has a null pointer", k);
    if (misaligned(d.map, 4) || misaligned(d.motion, 4) || misaligned(d.out, 4))
      return failf(-5, "countr_flow_flux: map %d: map, motion and out are 4-byte aligned", k);
    if (!(d.sx > 0.0 && d.sy > 0.0 && __builtin_isfinite(d.sx) && __builtin_isfinite(d.tx) && __builtin_isfinite(d.sy) && __builtin_isfinite(d.ty)))
      return failf(-4, "countr_flow_flux: map %d: a placement is finite with sx > 0 and sy > 0", k);
    a.map[k] = (const float*)d.map; a.mv[k] = (const short2*)d.motion; a.out[k] = (float*)d.out;
    a.sx[k] = d.sx; a.tx[k] = d.tx; a.sy[k] = d.sy; a.ty[k] = d.ty;
  }
  for (int k = 0; k < L; ++k) {
    const double* p = lines + 4 * k;
    if (!(__builtin_isfinite(p[0]) && __builtin_isfinite(p[1]) && __builtin_isfinite(p[2]) && __builtin_isfinite(p[3])))
      return failf(-4, "countr_flow_flux: line %d: a coordinate is not finite", k);
    // the header's e, len2, len and hw: fp64, one operation per statement
    const double ex = p[2] - p[0], ey = p[3] - p[1];
    const double xx = ex * ex, yy = ey * ey;
    const double len2 = xx + yy;
    const double len = sqrt(len2);
    const double half = band / 2.0;
    const double hw = half * len;
    if (!__builtin_isfinite(len2) || !__builtin_isfinite(hw))
      return failf(-4, "countr_flow_flux: line %d: its squared length and band are finite", k);
    a.ax[k] = p[0]; a.ay[k] = p[1]; a.ex[k] = ex; a.ey[k] = ey; a.len[k] = len; a.len2[k] = len2; a.hw[k] = hw;
  }
  a.band = band;
  a.step = 16.0 * (double)interval;
  a.L = L;
  float* part = (float*)workspace;
  hipLaunchKernelGGL(flow_flux_kernel, dim3(h / CELL, n), dim3(256), 0, STREAM(stream), a, part, h, w);
  hipLaunchKernelGGL(flow_fold_kernel, dim3(n), dim3(64), 0, STREAM(stream), a, (const float*)part, h / CELL);
  return launched("countr_flow_flux");
}
