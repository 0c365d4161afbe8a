// Train-time augmentation of the finetuning loader (countr_amd/data/fsc147.py::transform_train_aug) as device kernels: the pixel-rate
// work a DataLoader worker does per sample in ~0.2-0.4 s, on the step's stream.  The oracle of every kernel is the named host function
// of fsc147.py; the host keeps decoding, the random draws and the dot coordinates (countr_amd/device_aug.py::DeviceAug).
//   countr_aug_normal     out[e] = scale * z[e], z standard normal from Philox4x32-10 + Box-Muller (the stream is defined in the header)
//   countr_aug_jitter     clamp(x + noise, 0, 1) -> color_jitter: the four ops in the drawn order; the contrast op blends with the mean
//                         of the grey image AT THAT POINT of the chain, so the chain is cut there: pass A (noise + the ops before it)
//                         leaves fixed-order partial sums, pass B adds them up in one order and runs the rest -- two launches, no atomics
//   countr_aug_blur       gaussian_blur(img, (7, 9), sigma): 7 taps along x, 9 along y, reflect padding (edge pixel not repeated)
//   countr_aug_window     warp_affine (= scipy affine_transform order 1, constant 0) + horizontal flip + the 384 x 384 crop in one store
//                         pass -- the full warp is never materialised; copy mode cuts the same window out of an unwarped image
//   countr_aug_density    60 * scipy gaussian_filter(dot map, sigma 1) on 384 x 384 straight from the list of dot cells
//   countr_aug_exemplars  the formula of countr_crop_resize_f32 (frames.hip; bilinear.hpp) for the three exemplars of every image of a
//                         batch: the same formula, contraction off here, on there
// Every kernel serves a whole batch of differently sized images from a table of per-image descriptors passed by value (built here from
// the caller's HOST array of countr_aug_image), so launches per batch do not grow with the batch.  fp32 only: both library builds
// export the same code.
#include "common.hpp"
#include "../../include/countr_hip.h"

#include <math.h>

// the host functions round every product and sum on its own (torch CPU kernels, scipy's C loops): no fused multiply-adds here
#pragma clang fp contract(off)
#include "bilinear.hpp"      // contraction OFF (below the pragma): exemplar_kernel rounds every product and sum on its own, as torch's CPU kernel does

namespace {

constexpr int MAX_IMGS = COUNTR_AUG_MAX_IMAGES;   // descriptors travel as kernel arguments (4 KB): 32 x <= 104 bytes
constexpr int OUT = 384;                          // the training crop (util/FSC147.py MAX_HW)
constexpr int PARTS = 128;                        // workgroups (= partial grey sums) per image in the jitter passes
constexpr int BOX = 64, NBOX = 3;                 // exemplars: three 64 x 64 crops per image
constexpr int BT_W = 64, BT_H = 32;               // blur: outputs per workgroup
constexpr int BL_W = BT_W + 8, BL_H = BT_H + 8;   // ... and the staged input (4 columns either side keep the rows 16-byte aligned)
constexpr int DT = 32, DH = DT + 8;               // density: outputs per workgroup edge, and with the radius-4 halo

__device__ __forceinline__ void philox(unsigned int c0, unsigned int c1, unsigned int c2, unsigned int c3, unsigned int k0, unsigned int k1,
                                       unsigned int out[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned int n0 = (unsigned int)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned int)(p0 >> 32) ^ c3 ^ k1;
    c1 = (unsigned int)p1; c3 = (unsigned int)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// Box-Muller on two 32-bit words: u1 = ((a >> 9) + 1) 2^-23 in (0, 1], u2 = (b >> 8) 2^-24 in [0, 1) -- both exact in fp32 --
// z0 = sqrt(-2 ln u1) cos(2 pi u2), z1 = ... sin(2 pi u2)
__device__ __forceinline__ void box_muller(unsigned int a, unsigned int b, float& z0, float& z1) {
  const float u1 = (float)((a >> 9) + 1u) * 0x1p-23f;
  const float t = (float)(b >> 8) * 0x1p-23f;            // 2 u2, exact
  const float rad = sqrtf(-2.f * logf(u1));
  float s, c;
  sincospif(t, &s, &c);
  z0 = rad * c; z1 = rad * s;
}
// the four normals of group g of stream (key, ctr): elements 4 g .. 4 g + 3
__device__ __forceinline__ void normal4(unsigned int g, unsigned int k0, unsigned int k1, unsigned int t0, unsigned int t1, float z[4]) {
  unsigned int r[4];
  philox(g, 1u, t0, t1, k0, k1, r);      // counter word 1 = 1: the loss mask of countr_step_prologue draws with word 1 = 0
  box_muller(r[0], r[1], z[0], z[1]);
  box_muller(r[2], r[3], z[2], z[3]);
}

__global__ __launch_bounds__(256) void normal_kernel(float* __restrict__ out, long long n, float scale, unsigned int k0, unsigned int k1,
                                                     unsigned int t0, unsigned int t1) {
  const long long groups = (n + 3) >> 2;
  for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long long)gridDim.x * 256) {
    float z[4];
    normal4((unsigned int)g, k0, k1, t0, t1, z);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (4 * g + j < n) out[4 * g + j] = scale * z[j];
  }
}

// ---- colour jitter ------------------------------------------------------------------------------------------------------------
struct JitImg {
  const float* src;
  float* dst;
  const float* noise;
  int plane;                       // h * w
  unsigned int ctr[2];
  float f[4], g[4];                // blend factor of op k (brightness, contrast, saturation; f[3] = the hue shift) and fp32(1 - factor)
  unsigned char ops[4];
  signed char nops, cut;           // cut: position of the contrast op in ops, or nops when there is none
  signed char noise_mode, vec;     // vec: plane % 4 == 0 and 16-byte aligned pointers
};
struct JitArgs { JitImg im[MAX_IMGS]; };

__device__ __forceinline__ float gray_of(float r, float g, float b) { return (0.2989f * r + 0.587f * g) + 0.114f * b; }

// _rgb2hsv -> remainder(h + shift, 1) -> _hsv2rgb of fsc147.py, operation for operation
__device__ __forceinline__ void hue_op(float& r, float& g, float& b, float shift) {
  const float maxc = fmaxf(fmaxf(r, g), b), minc = fminf(fminf(r, g), b);
  const bool eqc = maxc == minc;
  const float cr = maxc - minc;
  const float s = cr / (eqc ? 1.f : maxc);
  const float crd = eqc ? 1.f : cr;
  const float rc = (maxc - r) / crd, gc = (maxc - g) / crd, bc = (maxc - b) / crd;
  const float hr = maxc == r ? bc - gc : 0.f;
  const float hg = (maxc == g && maxc != r) ? (2.f + rc) - bc : 0.f;
  const float hb = (maxc != g && maxc != r) ? (4.f + gc) - rc : 0.f;
  float h = fmodf(((hr + hg) + hb) / 6.f + 1.f, 1.f);
  h = h + shift;
  float m = fmodf(h, 1.f);                       // torch.remainder: the result takes the divisor's sign
  if (m != 0.f && m < 0.f) m += 1.f;
  h = m;
  const float v = maxc;
  const float h6 = h * 6.f;
  const float fl = floorf(h6);
  const float f = h6 - fl;
  const int i = ((int)fl) % 6;
  const float p = clamp01(v * (1.f - s));
  const float q = clamp01(v * (1.f - s * f));
  const float t = clamp01(v * (1.f - s * (1.f - f)));
  switch (i) {
    case 0: r = v; g = t; b = p; break;
    case 1: r = q; g = v; b = p; break;
    case 2: r = p; g = v; b = t; break;
    case 3: r = p; g = q; b = v; break;
    case 4: r = t; g = p; b = v; break;
    default: r = v; g = p; b = q; break;
  }
}

// ops[k0, k1) on one pixel; the contrast op (1) takes its blend value gm = fp32(1 - factor) * mean from the caller
__device__ __forceinline__ void apply_ops(const JitImg& d, int k0, int k1, float gm, float& r, float& g, float& b) {
  for (int k = k0; k < k1; ++k) {
    const int op = d.ops[k];
    if (op == 0) {
      r = clamp01(d.f[0] * r); g = clamp01(d.f[0] * g); b = clamp01(d.f[0] * b);
    } else if (op == 1) {
      r = clamp01(d.f[1] * r + gm); g = clamp01(d.f[1] * g + gm); b = clamp01(d.f[1] * b + gm);
    } else if (op == 2) {
      const float y = d.g[2] * gray_of(r, g, b);
      r = clamp01(d.f[2] * r + y); g = clamp01(d.f[2] * g + y); b = clamp01(d.f[2] * b + y);
    } else {
      hue_op(r, g, b, d.f[3]);
    }
  }
}

// PX pixels of a plane: one 16-byte access (PX = 4) or one element
template <int PX> __device__ __forceinline__ void ldpx(const float* p, float (&v)[PX]) {
  if constexpr (PX == 4) ld4<float>(p, v); else v[0] = p[0];
}
template <int PX> __device__ __forceinline__ void stpx(float* p, const float (&v)[PX]) {
  if constexpr (PX == 4) st4<float>(p, v); else p[0] = v[0];
}

// pass A of image d for workgroup `part`: noise, the ops in front of the contrast op, the workgroup's grey sum
template <int PX> __device__ __forceinline__ float jitter_a_body(const JitImg& d, int part, unsigned int k0, unsigned int k1) {
  const int per = d.plane / PX;
  float gsum = 0.f;
  for (int q = part * 256 + threadIdx.x; q < per; q += PARTS * 256) {
    const int p0 = q * PX;
    float c[3][PX];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) ldpx<PX>(d.src + (int64_t)ch * d.plane + p0, c[ch]);
    if (d.noise_mode == 2) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        float nz[PX];
        ldpx<PX>(d.noise + (int64_t)ch * d.plane + p0, nz);
#pragma unroll
        for (int e = 0; e < PX; ++e) c[ch][e] = clamp01(c[ch][e] + nz[e]);
      }
    } else if (d.noise_mode == 1) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const int64_t e0 = (int64_t)ch * d.plane + p0;      // element index in the [3, h, w] image
        float z[4];
        normal4((unsigned int)(e0 >> 2), k0, k1, d.ctr[0], d.ctr[1], z);
        if constexpr (PX == 4) {
#pragma unroll
          for (int e = 0; e < 4; ++e) c[ch][e] = clamp01(c[ch][e] + 0.1f * z[e]);
        } else {
          const int j = (int)(e0 & 3);
          c[ch][0] = clamp01(c[ch][0] + 0.1f * (j == 0 ? z[0] : j == 1 ? z[1] : j == 2 ? z[2] : z[3]));
        }
      }
    }
#pragma unroll
    for (int e = 0; e < PX; ++e) {
      apply_ops(d, 0, d.cut, 0.f, c[0][e], c[1][e], c[2][e]);
      gsum += gray_of(c[0][e], c[1][e], c[2][e]);
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) stpx<PX>(d.dst + (int64_t)ch * d.plane + p0, c[ch]);
  }
  return gsum;
}

__global__ __launch_bounds__(256) void jitter_a_kernel(const JitArgs a, unsigned int k0, unsigned int k1, float* __restrict__ partials) {
  __shared__ float sm[4];
  const int i = blockIdx.x / PARTS, part = blockIdx.x % PARTS;
  const JitImg& d = a.im[i];
  const float s = d.vec ? jitter_a_body<4>(d, part, k0, k1) : jitter_a_body<1>(d, part, k0, k1);
  const float t = block_sum<4>(s, sm);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

template <int PX> __device__ __forceinline__ void jitter_b_body(const JitImg& d, int part, float gm) {
  const int per = d.plane / PX;
  for (int q = part * 256 + threadIdx.x; q < per; q += PARTS * 256) {
    const int p0 = q * PX;
    float c[3][PX];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) ldpx<PX>(d.dst + (int64_t)ch * d.plane + p0, c[ch]);
#pragma unroll
    for (int e = 0; e < PX; ++e) apply_ops(d, d.cut, d.nops, gm, c[0][e], c[1][e], c[2][e]);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) stpx<PX>(d.dst + (int64_t)ch * d.plane + p0, c[ch]);
  }
}

// pass B: the image's grey mean from its PARTS partial sums (every workgroup adds them in the same order), then the contrast op and
// whatever follows it, in place
__global__ __launch_bounds__(256) void jitter_b_kernel(const JitArgs a, const float* __restrict__ partials) {
  __shared__ float mean;
  const int i = blockIdx.x / PARTS, part = blockIdx.x % PARTS;
  const JitImg& d = a.im[i];
  if (d.cut >= d.nops) return;       // (uniform) no contrast op: pass A did everything
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int k = 0; k < PARTS; ++k) s += (double)partials[i * PARTS + k];
    mean = (float)(s / (double)d.plane);
  }
  __syncthreads();
  const float gm = d.g[1] * mean;
  if (d.vec) jitter_b_body<4>(d, part, gm); else jitter_b_body<1>(d, part, gm);
}

// ---- blur ---------------------------------------------------------------------------------------------------------------------
struct BlurImg {
  const float* src;
  float* dst;
  int h, w, first, tx;             // first: this image's first work item; tx: tiles per row of tiles
  float kx[7], ky[9];
  int vec;
};
struct BlurArgs { BlurImg im[MAX_IMGS]; };

__device__ __forceinline__ int reflect_idx(int i, int n) {      // F.pad(mode="reflect"): -1 -> 1, n -> n - 2
  i = i < 0 ? -i : i;
  i = i >= n ? 2 * n - 2 - i : i;
  return max(0, min(i, n - 1));
}

__global__ __launch_bounds__(256) void blur_kernel(const BlurArgs a, int n) {
  __shared__ __attribute__((aligned(16))) float in[BL_H][BL_W];
  __shared__ __attribute__((aligned(16))) float mid[BL_H][BT_W];
  int i = 0;
  for (int k = 1; k < n; ++k) i += (int)blockIdx.x >= a.im[k].first ? 1 : 0;
  const BlurImg& d = a.im[i];
  const int item = blockIdx.x - d.first;
  const int ch = item % 3, tile = item / 3;
  const int x0 = (tile % d.tx) * BT_W, y0 = (tile / d.tx) * BT_H;
  const float* src = d.src + (int64_t)ch * d.h * d.w;
  for (int v = threadIdx.x; v < BL_H * (BL_W / 4); v += 256) {
    const int ry = v / (BL_W / 4), c4 = v % (BL_W / 4);
    const int gy = reflect_idx(y0 - 4 + ry, d.h), gx = x0 - 4 + 4 * c4;
    const float* row = src + (int64_t)gy * d.w;
    float4 t;
    if (d.vec && gx >= 0 && gx + 3 < d.w) {
      t = *reinterpret_cast<const float4*>(row + gx);
    } else {
      t.x = row[reflect_idx(gx, d.w)]; t.y = row[reflect_idx(gx + 1, d.w)];
      t.z = row[reflect_idx(gx + 2, d.w)]; t.w = row[reflect_idx(gx + 3, d.w)];
    }
    *reinterpret_cast<float4*>(&in[ry][4 * c4]) = t;
  }
  __syncthreads();
  for (int v = threadIdx.x; v < BL_H * BT_W; v += 256) {
    const int ry = v / BT_W, cx = v % BT_W;
    float s = d.kx[0] * in[ry][cx + 1];
#pragma unroll
    for (int k = 1; k < 7; ++k) s += d.kx[k] * in[ry][cx + 1 + k];
    mid[ry][cx] = s;
  }
  __syncthreads();
  float* dst = d.dst + (int64_t)ch * d.h * d.w;
  for (int v = threadIdx.x; v < BT_H * (BT_W / 4); v += 256) {
    const int ry = v / (BT_W / 4), c4 = v % (BT_W / 4);
    const int gy = y0 + ry, gx = x0 + 4 * c4;
    if (gy >= d.h || gx >= d.w) continue;
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float s = d.ky[0] * mid[ry][4 * c4 + e];
#pragma unroll
      for (int k = 1; k < 9; ++k) s += d.ky[k] * mid[ry + k][4 * c4 + e];
      o[e] = s;
    }
    float* p = dst + (int64_t)gy * d.w + gx;
    if (d.vec && gx + 3 < d.w) {
      *reinterpret_cast<float4*>(p) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) if (gx + e < d.w) p[e] = o[e];
    }
  }
}

// ---- affine warp + flip + crop ------------------------------------------------------------------------------------------------
struct WinImg {
  const float* src;                // fp32 [3, h, w]
  double m[6];                     // source (row, col) = (m[2] + y m[0] + x m[1], m[5] + y m[3] + x m[4]) of output pixel (y, x)
  int h, w, start_h, start_w;
  int mode, flip;
};
struct WinArgs { WinImg im[MAX_IMGS]; };

// one thread = four neighbouring pixels of one output row, three channels: 16-byte stores into row b of the batch tensor
__global__ __launch_bounds__(256) void window_kernel(const WinArgs a, float* __restrict__ out, int n) {
  constexpr int per = OUT / 4, chunks = OUT * per / 256;      // 144 workgroup-sized chunks per image: the image index is wave-uniform
  for (int blk = blockIdx.x; blk < n * chunks; blk += gridDim.x) {
    const int b = blk / chunks, t = (blk % chunks) * 256 + threadIdx.x;
    const int q = t % per, y = t / per;
    const WinImg& d = a.im[b];
    const int64_t plane = (int64_t)d.h * d.w;
    const int oy = d.start_h + y;
    float v[3][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int wx = d.start_w + 4 * q + e;              // column of the (flipped) full-size image
      const int ox = d.flip ? d.w - 1 - wx : wx;
      if (d.mode == 0) {
        const float* p = d.src + (int64_t)oy * d.w + ox;
        v[0][e] = p[0]; v[1][e] = p[plane]; v[2][e] = p[2 * plane];
      } else {
        // scipy's NI_GeometricTransform: shift first, then one product per output axis, all in double
        double sy = d.m[2]; sy += (double)oy * d.m[0]; sy += (double)ox * d.m[1];
        double sx = d.m[5]; sx += (double)oy * d.m[3]; sx += (double)ox * d.m[4];
        if (sy < 0.0 || sy > (double)(d.h - 1) || sx < 0.0 || sx > (double)(d.w - 1)) {
          v[0][e] = 0.f; v[1][e] = 0.f; v[2][e] = 0.f;
        } else {
          const double fy = floor(sy), fx = floor(sx);
          const double wy1 = sy - fy, wx1 = sx - fx, wy0 = 1.0 - wy1, wx0 = 1.0 - wx1;
          const int iy = (int)fy, ix = (int)fx;
          const int iy1 = min(iy + 1, d.h - 1), ix1 = min(ix + 1, d.w - 1);     // (the neighbour behind the last sample has weight 0)
          const float* r0 = d.src + (int64_t)iy * d.w;
          const float* r1 = d.src + (int64_t)iy1 * d.w;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            double s = (double)r0[c * plane + ix] * (wy0 * wx0);
            s += (double)r0[c * plane + ix1] * (wy0 * wx1);
            s += (double)r1[c * plane + ix] * (wy1 * wx0);
            s += (double)r1[c * plane + ix1] * (wy1 * wx1);
            v[c][e] = (float)s;
          }
        }
      }
    }
    float* o = out + (((int64_t)b * 3) * OUT + y) * OUT + 4 * q;
#pragma unroll
    for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(o + (int64_t)c * OUT * OUT) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
  }
}

// ---- density target -----------------------------------------------------------------------------------------------------------
struct DensArgs {
  int off[MAX_IMGS], cnt[MAX_IMGS];
  double w[9];
};

// scipy.ndimage.gaussian_filter(sigma 1, radius 4, mode "reflect": ... b a | a b ...): axis 0 into an fp32 intermediate, then axis 1, sums
// in double as correlate1d keeps them.  A workgroup owns a 32 x 32 tile: it walks the image's cell list, marks the cells that fall
// into the tile's halo (through the reflection too) in LDS and filters from there -- no dot map in memory, no atomics.
__global__ __launch_bounds__(256) void density_kernel(const DensArgs a, const int* __restrict__ cells, float* __restrict__ out) {
  __shared__ float dot[DH][DH + 1];
  __shared__ float tmp[DT][DH + 1];
  constexpr int tiles = OUT / DT;
  const int b = blockIdx.x / (tiles * tiles), tile = blockIdx.x % (tiles * tiles);
  const int y0 = (tile / tiles) * DT, x0 = (tile % tiles) * DT;
  for (int v = threadIdx.x; v < DH * (DH + 1); v += 256) (&dot[0][0])[v] = 0.f;
  __syncthreads();
  const int* cl = cells + a.off[b];
  for (int k = threadIdx.x; k < a.cnt[b]; k += 256) {
    const int packed = cl[k];
    const int r = packed >> 16, c = packed & 0xffff;
    if (r < 0 || r >= OUT || c >= OUT) continue;
    const int ry[3] = {r, -1 - r, 2 * OUT - 1 - r}, cx[3] = {c, -1 - c, 2 * OUT - 1 - c};
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      const int ly = ry[u] - (y0 - 4);
      if (ly < 0 || ly >= DH) continue;
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        const int lx = cx[s] - (x0 - 4);
        if (lx >= 0 && lx < DH) dot[ly][lx] = 1.f;
      }
    }
  }
  __syncthreads();
  for (int v = threadIdx.x; v < DT * DH; v += 256) {
    const int y = v / DH, x = v % DH;
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) s += a.w[k] * (double)dot[y + k][x];
    tmp[y][x] = (float)s;
  }
  __syncthreads();
  {
    const int y = threadIdx.x / (DT / 4), x4 = (threadIdx.x % (DT / 4)) * 4;
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 9; ++k) s += a.w[k] * (double)tmp[y][x4 + e + k];
      o[e] = (float)s * 60.f;
    }
    *reinterpret_cast<float4*>(out + ((int64_t)b * OUT + y0 + y) * OUT + x0 + x4) = make_float4(o[0], o[1], o[2], o[3]);
  }
}

// ---- exemplars ----------------------------------------------------------------------------------------------------------------
struct BoxImg {
  const float* src;
  int h, w;
  int y0[NBOX], x0[NBOX], ch[NBOX], cw[NBOX];
};
struct BoxArgs { BoxImg im[MAX_IMGS]; };

// crop_resize_kernel of frames.hip (torch's upsample_bilinear2d, align_corners=False) with the image taken from the table, contraction off
__global__ __launch_bounds__(256) void exemplar_kernel(const BoxArgs a, float* __restrict__ out, int n) {
  constexpr int per = BOX / 4, chunks = NBOX * 3 * BOX * per / 256;      // 36 workgroup-sized chunks per image
  for (int blk = blockIdx.x; blk < n * chunks; blk += gridDim.x) {
    const int b = blk / chunks;
    const int64_t i = (int64_t)blk * 256 + threadIdx.x;
    const int q = (int)(i % per);
    const int64_t row = i / per;                      // (image, rectangle, channel, output row)
    const int oy = (int)(row % BOX);
    const int c = (int)((row / BOX) % 3), r = (int)((row / (3 * BOX)) % NBOX);
    const BoxImg& d = a.im[b];
    const int ch = d.ch[r], cw = d.cw[r];
    const float* org = d.src + ((int64_t)c * d.h + d.y0[r]) * d.w + d.x0[r];
    const BilinearRow t = bilinear_row(org, d.w, ch, cw, bilinear_scale(ch, BOX), bilinear_scale(cw, BOX), oy);
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = bilinear_at(t, q * 4 + e);
    *reinterpret_cast<float4*>(out + row * BOX + (int64_t)q * 4) = make_float4(v[0], v[1], v[2], v[3]);
  }
}

bool table_ok(const countr_aug_image* imgs, int n, const char* who) {
  static thread_local char msg[160];
  if (!imgs || n < 1 || n > MAX_IMGS) {
    snprintf(msg, sizeof msg, "%s: 1..%d images per call", who, MAX_IMGS);
    countr_set_error(msg); return false;
  }
  return true;
}
bool size_ok(int h, int w) { return h >= 8 && w >= 8 && (int64_t)h * w <= (int64_t)1 << 26; }

}  // namespace

extern "C" int countr_aug_partials_floats(int n) { return (n < 1 ? 1 : n) * PARTS; }

extern "C" int countr_aug_normal(float* out, int64_t n, float scale, uint64_t seed, uint64_t counter, void* stream) {
  if (!out || n < 1 || n > ((int64_t)1 << 33)) { countr_set_error("countr_aug_normal: bad args (1 <= n <= 2^33)"); return -1; }
  hipLaunchKernelGGL(normal_kernel, dim3(countr_blocks_for((n + 3) / 4, 2048)), dim3(256), 0, STREAM(stream), out, (long long)n, scale,
                     (unsigned int)seed, (unsigned int)(seed >> 32), (unsigned int)counter, (unsigned int)(counter >> 32));
  return countr_check_launch("countr_aug_normal");
}

extern "C" int countr_aug_jitter(const countr_aug_image* imgs, int n, uint64_t seed, float* partials, void* stream) {
  if (!table_ok(imgs, n, "countr_aug_jitter")) return -1;
  if (!partials) { countr_set_error("countr_aug_jitter: the partial-sum workspace is required"); return -1; }
  JitArgs a;
  bool any_cut = false;
  for (int j = 0; j < MAX_IMGS; ++j) {
    const countr_aug_image& s = imgs[j < n ? j : n - 1];
    JitImg& d = a.im[j];
    if (!s.src || !s.jit || !size_ok(s.h, s.w) || s.nops < 0 || s.nops > 4 || s.noise_mode < 0 || s.noise_mode > 2 ||
        (s.noise_mode == 2 && !s.noise)) {
      countr_set_error("countr_aug_jitter: an image lacks src / jit (or its explicit noise), or has a bad size, op count or noise mode"); return -1;
    }
    d.src = s.src; d.dst = s.jit; d.noise = s.noise; d.plane = s.h * s.w;
    d.ctr[0] = (unsigned int)s.counter; d.ctr[1] = (unsigned int)(s.counter >> 32);
    const double fac[4] = {s.brightness, s.contrast, s.saturation, s.hue};
    for (int k = 0; k < 4; ++k) { d.f[k] = (float)fac[k]; d.g[k] = (float)(1.0 - fac[k]); }
    d.nops = (signed char)s.nops; d.cut = d.nops;
    unsigned seen = 0;
    for (int k = 0; k < 4; ++k) {
      const int op = k < s.nops ? s.order[k] : 0;
      if (op < 0 || op > 3 || (k < s.nops && (seen >> op & 1))) { countr_set_error("countr_aug_jitter: order holds each of the ops 0..3 at most once"); return -1; }
      if (k < s.nops) seen |= 1u << op;
      d.ops[k] = (unsigned char)op;
      if (k < s.nops && op == 1) d.cut = (signed char)k;
    }
    any_cut = any_cut || d.cut < d.nops;
    d.noise_mode = (signed char)s.noise_mode;
    d.vec = (d.plane & 3) == 0 && ((((uintptr_t)s.src) | ((uintptr_t)s.jit) | (s.noise_mode == 2 ? (uintptr_t)s.noise : 0)) & 15) == 0;
  }
  hipLaunchKernelGGL(jitter_a_kernel, dim3(n * PARTS), dim3(256), 0, STREAM(stream), a, (unsigned int)seed, (unsigned int)(seed >> 32), partials);
  if (any_cut) hipLaunchKernelGGL(jitter_b_kernel, dim3(n * PARTS), dim3(256), 0, STREAM(stream), a, partials);
  return countr_check_launch("countr_aug_jitter");
}

extern "C" int countr_aug_blur(const countr_aug_image* imgs, int n, void* stream) {
  if (!table_ok(imgs, n, "countr_aug_blur")) return -1;
  BlurArgs a;
  int items = 0;
  for (int j = 0; j < MAX_IMGS; ++j) {
    const countr_aug_image& s = imgs[j < n ? j : n - 1];
    BlurImg& d = a.im[j];
    if (!s.jit || !s.blr || s.jit == s.blr || !size_ok(s.h, s.w)) { countr_set_error("countr_aug_blur: an image lacks jit / blr (two buffers), or has a bad size"); return -1; }
    d.src = s.jit; d.dst = s.blr; d.h = s.h; d.w = s.w;
    d.tx = (s.w + BT_W - 1) / BT_W;
    d.first = items;
    if (j < n) items += d.tx * ((s.h + BT_H - 1) / BT_H) * 3;
    for (int k = 0; k < 7; ++k) d.kx[k] = s.kx[k];
    for (int k = 0; k < 9; ++k) d.ky[k] = s.ky[k];
    d.vec = (s.w & 3) == 0 && ((((uintptr_t)s.jit) | ((uintptr_t)s.blr)) & 15) == 0;
  }
  hipLaunchKernelGGL(blur_kernel, dim3(items), dim3(256), 0, STREAM(stream), a, n);
  return countr_check_launch("countr_aug_blur");
}

extern "C" int countr_aug_window(const countr_aug_image* imgs, int n, float* out, void* stream) {
  if (!table_ok(imgs, n, "countr_aug_window")) return -1;
  if (!out || (((uintptr_t)out) & 15)) { countr_set_error("countr_aug_window: out must be a 16-byte aligned [n, 3, 384, 384] tensor"); return -1; }
  WinArgs a;
  for (int j = 0; j < MAX_IMGS; ++j) {
    const countr_aug_image& s = imgs[j < n ? j : n - 1];
    WinImg& d = a.im[j];
    if (!s.win || !size_ok(s.win_h, s.win_w) || s.start_h < 0 || s.start_w < 0 || s.start_h > s.win_h - OUT || s.start_w > s.win_w - OUT ||
        s.win_mode < 0 || s.win_mode > 1) {
      countr_set_error("countr_aug_window: an image lacks win, or its 384 x 384 window does not lie inside win_h x win_w"); return -1;
    }
    d.src = s.win; d.h = s.win_h; d.w = s.win_w; d.start_h = s.start_h; d.start_w = s.start_w;
    d.mode = s.win_mode; d.flip = s.flip ? 1 : 0;
    for (int k = 0; k < 6; ++k) d.m[k] = s.affine[k];
  }
  hipLaunchKernelGGL(window_kernel, dim3(countr_blocks_for((int64_t)n * OUT * (OUT / 4), 2048)), dim3(256), 0, STREAM(stream), a, out, n);
  return countr_check_launch("countr_aug_window");
}

extern "C" int countr_aug_density(const countr_aug_image* imgs, int n, const int* cells, int ncells, float* out, void* stream) {
  if (!table_ok(imgs, n, "countr_aug_density")) return -1;
  if (!cells || ncells < 0 || !out || (((uintptr_t)out) & 15)) { countr_set_error("countr_aug_density: cells and a 16-byte aligned out [n, 384, 384] are required"); return -1; }
  DensArgs a;
  for (int j = 0; j < MAX_IMGS; ++j) {
    const countr_aug_image& s = imgs[j < n ? j : n - 1];
    if (s.cell_off < 0 || s.cell_cnt < 0 || (int64_t)s.cell_off + s.cell_cnt > ncells) { countr_set_error("countr_aug_density: a cell range lies outside the list"); return -1; }
    a.off[j] = s.cell_off; a.cnt[j] = s.cell_cnt;
  }
  double sum = 0.0;
  for (int k = 0; k < 9; ++k) { a.w[k] = exp(-0.5 * (double)((k - 4) * (k - 4))); sum += a.w[k]; }
  for (int k = 0; k < 9; ++k) a.w[k] /= sum;
  hipLaunchKernelGGL(density_kernel, dim3(n * (OUT / DT) * (OUT / DT)), dim3(256), 0, STREAM(stream), a, cells, out);
  return countr_check_launch("countr_aug_density");
}

extern "C" int countr_aug_exemplars(const countr_aug_image* imgs, int n, float* out, void* stream) {
  if (!table_ok(imgs, n, "countr_aug_exemplars")) return -1;
  if (!out || (((uintptr_t)out) & 15)) { countr_set_error("countr_aug_exemplars: out must be a 16-byte aligned [n, 3, 3, 64, 64] tensor"); return -1; }
  BoxArgs a;
  for (int j = 0; j < MAX_IMGS; ++j) {
    const countr_aug_image& s = imgs[j < n ? j : n - 1];
    BoxImg& d = a.im[j];
    if (!s.src || !size_ok(s.h, s.w)) { countr_set_error("countr_aug_exemplars: an image lacks src or has a bad size"); return -1; }
    d.src = s.src; d.h = s.h; d.w = s.w;
    for (int r = 0; r < NBOX; ++r) {
      const int* q = s.rects + 4 * r;                              // {y1, x1, y2, x2}, inclusive; clipped as img[:, y1:y2 + 1, x1:x2 + 1] clips
      if (!clip_rect(q[0], q[1], q[2], q[3], s.h, s.w, &d.y0[r], &d.x0[r], &d.ch[r], &d.cw[r])) {
        countr_set_error(q[0] < 0 || q[1] < 0 ? "countr_aug_exemplars: negative rectangle corner"
                                              : "countr_aug_exemplars: a rectangle is empty after clipping to the image");
        return -1;
      }
    }
  }
  hipLaunchKernelGGL(exemplar_kernel, dim3(countr_blocks_for((int64_t)n * NBOX * 3 * BOX * (BOX / 4), 2048)), dim3(256), 0, STREAM(stream), a, out, n);
  return countr_check_launch("countr_aug_exemplars");
}
