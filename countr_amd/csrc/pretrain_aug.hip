// The pretraining loader's transform on the device: fsc147.transform_pretrain = Pillow BILINEAR resize to multiples of 16 -> crop ->
// Pillow BICUBIC resize to 384 x 384 -> horizontal flip -> ToTensor, for a batch whose samples all differ in frame and crop size.
//   countr_pil_tables            (host only) the per-axis tap tables of Pillow's 8-bit resample for BILINEAR (0) and BICUBIC (1)
//                                (Resample.c: precompute_coeffs + normalize_coeffs_8bpc)
//   countr_pretrain_aug_layout   (host only) tap stride, table and workspace sizes of a group of <= 16 samples
//   countr_pretrain_aug_tables   one launch: the four tables of every sample, computed on the device in fp64 in Pillow's operation order
//   countr_pretrain_aug          four launches: stage 1 horizontal, stage 1 vertical (uint8 [H, W, 3] -> uint8 [H16, W16, 3]), the
//                                bicubic horizontal pass over the crop rectangle, the bicubic vertical pass + flip + ToTensor into the
//                                batch tensor
// Every pass goes into 8 bits before the next one, as Pillow's does, with int32 accumulators; the result equals PIL + ToTensor bit for bit.
// One table row is ONE function (table_row) for the host export and the device kernel, compiled with fp contraction off: an fma in
// (xx + 0.5) * scale - support or in the cubic would change the last bit of a double and with it a rounded tap.
// uint8 / fp32 only: the bf16 and the fp16 build of the library export the same code.
#include "common.hpp"
#include "../../include/countr_hip.h"

#include <math.h>

#define STREAM(s) reinterpret_cast<hipStream_t>(s)

namespace {

constexpr int PRECISION_BITS = 32 - 8 - 2;      // Pillow's fixed point: weights are int(+-0.5 + w * 2^22)
constexpr int MAX_IMAGES = COUNTR_PRETRAIN_MAX_IMAGES;
constexpr int OUT = 384;
constexpr int STAGE_BYTES = 16384;              // LDS staging of one source row segment (horizontal passes)
constexpr int MAX_BLOCKS = 2048;
constexpr int MAX_KSIZE = 1 << 12;

struct Axis {
  double scale, support, ss;
  int ksize;
};

// precompute_coeffs' per-axis constants.  filter 0: bilinear (support 1), 1: bicubic (support 2)
__host__ __device__ inline Axis axis_of(int filter, int in_size, int out_size) {
#pragma clang fp contract(off)
  Axis a;
  a.scale = (double)in_size / (double)out_size;
  const double fs = a.scale < 1.0 ? 1.0 : a.scale;
  a.support = (filter == 1 ? 2.0 : 1.0) * fs;
  a.ss = 1.0 / fs;                              // (Pillow multiplies by this reciprocal; so does this file)
  const double k = ceil(a.support) * 2 + 1;
  a.ksize = k > (double)(1 << 30) ? 1 << 30 : (int)k;
  return a;
}

__host__ __device__ inline double filter_of(int filter, double x) {
#pragma clang fp contract(off)
  if (x < 0.0) x = -x;
  if (filter == 1) {                            // bicubic_filter, a = -0.5
    const double a = -0.5;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
  }
  return x < 1.0 ? 1.0 - x : 0.0;               // bilinear_filter
}

// Row xx of the tables of one axis: bounds[2 xx] = {first source index, tap count}, weights[xx * stride ..] = the taps in fixed point,
// zeros behind the tap count up to `stride` (>= the axis' ksize).  The weights are summed in a first loop and evaluated again in the
// second (the same operations give the same doubles), so that no per-row array of doubles is needed.
__host__ __device__ inline void table_row(int filter, const Axis& ax, int in_size, int xx, int stride, int* bounds, int* weights) {
#pragma clang fp contract(off)
  const double center = (xx + 0.5) * ax.scale;
  int xmin = (int)(center - ax.support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + ax.support + 0.5);
  if (xmax > in_size) xmax = in_size;
  xmax -= xmin;
  double ww = 0.0;
  for (int x = 0; x < xmax; ++x) ww += filter_of(filter, (x + xmin - center + 0.5) * ax.ss);
  int* k = weights + (int64_t)xx * stride;
  for (int x = 0; x < stride; ++x) {
    double w = 0.0;
    if (x < xmax) {
      w = filter_of(filter, (x + xmin - center + 0.5) * ax.ss);
      if (ww != 0.0) w /= ww;
    }
    k[x] = w < 0 ? (int)(-0.5 + w * (double)(1 << PRECISION_BITS)) : (int)(0.5 + w * (double)(1 << PRECISION_BITS));
  }
  bounds[2 * xx] = xmin;
  bounds[2 * xx + 1] = xmax;
}

// ---- the tables of a group on the device
struct TableJob {
  int filter, in_size, out_size, off;           // off: first int of this table in the workspace (bounds, then weights)
  int first;                                    // index of its first row among the group's rows
};
struct TableArgs {
  TableJob job[4 * MAX_IMAGES];
  int njobs, rows, stride;
};

__global__ __launch_bounds__(256) void tables_kernel(const TableArgs a, int* __restrict__ ws) {
  for (int r = blockIdx.x * 256 + threadIdx.x; r < a.rows; r += gridDim.x * 256) {
    int j = 0;
    while (j + 1 < a.njobs && a.job[j + 1].first <= r) ++j;
    const TableJob& t = a.job[j];
    const Axis ax = axis_of(t.filter, t.in_size, t.out_size);
    table_row(t.filter, ax, t.in_size, r - t.first, a.stride, ws + t.off, ws + t.off + 2 * t.out_size);
  }
}

// ---- the image passes
__device__ __forceinline__ uint8_t clip8(int v) {      // (an arithmetic shift: a negative sum of the bicubic lobes clips to 0)
  v >>= PRECISION_BITS;
  return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// One sample of a horizontal pass: rows y0 .. y0 + rows of src (uint8 interleaved, `pitch` pixels per row), columns x0 .. x0 + in_w
// -> dst uint8 [rows, out_w, 3].  Taps are relative to x0 and clamp at in_w: Pillow crops first, so the filter sees the crop's edges.
struct HSample {
  const uint8_t* src;
  uint8_t* dst;
  int64_t src_bytes;                            // size of the buffer behind src: the 16-byte staging loads stop there
  int pitch, x0, y0, in_w, rows, out_w;
  int tab;                                      // the axis' table in the workspace
  int tile, tiles, vec;                         // output pixels per work item, items per row, src 16-byte aligned
  int first;                                    // index of the sample's first work item among the group's
};
struct HArgs {
  HSample s[MAX_IMAGES];
  int n, items, stride;
};

// Horizontal pass.  One work item = (sample, source row, tile of `tile` output pixels): the bytes of the row the tile's taps touch are
// staged in LDS with 16-byte loads and every thread resamples one output pixel (3 channels) from there.  Table entries are clamped to
// the staged range, so a wrong table cannot make the kernel read outside the rectangle.
__global__ __launch_bounds__(256) void hpass_kernel(const HArgs a, const int* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[STAGE_BYTES];
  for (int it = blockIdx.x; it < a.items; it += gridDim.x) {
    int f = 0;
    while (f + 1 < a.n && a.s[f + 1].first <= it) ++f;
    const HSample& s = a.s[f];
    const int local = it - s.first;
    const int t = local % s.tiles, y = local / s.tiles;
    const int* bounds = ws + s.tab;
    const int* weights = bounds + 2 * s.out_w;
    const int xo0 = t * s.tile, xo1 = min(s.out_w, xo0 + s.tile);
    int xs = bounds[2 * xo0], xe = bounds[2 * (xo1 - 1)] + bounds[2 * (xo1 - 1) + 1];
    xs = max(0, min(xs, s.in_w));
    xe = max(xs, min(xe, s.in_w));
    const int64_t b0 = ((int64_t)(s.y0 + y) * s.pitch + s.x0 + xs) * 3;      // first byte of the segment in src
    const int64_t a0 = s.vec ? (b0 & ~(int64_t)15) : b0;
    const int head = (int)(b0 - a0);
    const int span = min((xe - xs) * 3, STAGE_BYTES - 16 - head);           // (the host sized `tile` so that this never cuts)
    if (s.vec) {
      const int nvec = (head + span + 15) >> 4;
      for (int v = threadIdx.x; v < nvec; v += 256) {
        const int64_t off = a0 + (int64_t)v * 16;
        if (off + 16 <= s.src_bytes) {
          *reinterpret_cast<uint4*>(stage + v * 16) = *reinterpret_cast<const uint4*>(s.src + off);
        } else {
          for (int b = 0; b < 16; ++b) stage[v * 16 + b] = off + b < s.src_bytes ? s.src[off + b] : (uint8_t)0;
        }
      }
    } else {
      for (int b = threadIdx.x; b < span; b += 256) stage[b] = s.src[a0 + b];
    }
    __syncthreads();
    const int xo = xo0 + threadIdx.x;
    if (xo < xo1) {
      int xmin = bounds[2 * xo], cnt = bounds[2 * xo + 1];
      xmin = max(xs, min(xmin, xe));
      cnt = max(0, min(min(cnt, a.stride), min(xe - xmin, (span - (xmin - xs) * 3) / 3)));
      const int* k = weights + (int64_t)xo * a.stride;
      const uint8_t* p = stage + head + (xmin - xs) * 3;
      int r = 1 << (PRECISION_BITS - 1), g = r, b = r;
      for (int j = 0; j < cnt; ++j) {
        const int w = k[j];
        r += (int)p[3 * j] * w; g += (int)p[3 * j + 1] * w; b += (int)p[3 * j + 2] * w;
      }
      uint8_t* o = s.dst + ((int64_t)y * s.out_w + xo) * 3;
      o[0] = clip8(r); o[1] = clip8(g); o[2] = clip8(b);
    }
    __syncthreads();
  }
}

// One sample of the stage-1 vertical pass: src uint8 [in_h, row_bytes] -> dst uint8 [out_h, row_bytes], row_bytes = 3 W16 (a multiple
// of 48).  One thread = 4 neighbouring bytes of an output row.
struct VSample {
  const uint8_t* src;
  uint8_t* dst;
  int in_h, out_h, row_bytes, tab, vec;         // vec: src 4-byte aligned
  int first;                                    // index of the sample's first thread among the group's
};
struct VArgs {
  VSample s[MAX_IMAGES];
  int n, stride;
  int64_t total;
};

__global__ __launch_bounds__(256) void vpass_u8_kernel(const VArgs a, const int* __restrict__ ws) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.total; i += (int64_t)gridDim.x * 256) {
    int f = 0;
    while (f + 1 < a.n && a.s[f + 1].first <= i) ++f;
    const VSample& s = a.s[f];
    const int local = (int)(i - s.first);
    const int per = s.row_bytes >> 2;
    const int q = local % per, yo = local / per;
    const int* bounds = ws + s.tab;
    int ymin = bounds[2 * yo], cnt = bounds[2 * yo + 1];
    ymin = max(0, min(ymin, s.in_h));
    cnt = max(0, min(min(cnt, a.stride), s.in_h - ymin));
    const int* k = bounds + 2 * s.out_h + (int64_t)yo * a.stride;
    const uint8_t* p = s.src + (int64_t)ymin * s.row_bytes + 4 * q;
    int acc[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = 1 << (PRECISION_BITS - 1);
    for (int j = 0; j < cnt; ++j, p += s.row_bytes) {
      const int w = k[j];
      uint32_t v;
      if (s.vec) v = *reinterpret_cast<const uint32_t*>(p);
      else v = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] += (int)((v >> (8 * e)) & 255u) * w;
    }
    // four byte stores, not one packed word: for clip8(a) | clip8(b) << 8 | ... hipcc picks gfx950's packed shift-and-saturate
    // (v_ashr_pk_u8_i32), which leaves the upper half of its destination register as it was, and ORs that stale half into bytes 2 and 3
    uint8_t* o = s.dst + (int64_t)yo * s.row_bytes + 4 * q;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = clip8(acc[e]);
  }
}

// One sample of the last pass: src uint8 [in_h, 384, 3] (the bicubic horizontal pass' output) -> row `row` of the batch tensor
struct FSample {
  const uint8_t* src;
  int in_h, tab, flip, row;
};
struct FArgs {
  FSample s[MAX_IMAGES];
  int n, stride;
};

// Bicubic vertical pass + flip + ToTensor.  One thread = 4 neighbouring output pixels x 3 channels: 12 contiguous bytes of every tap
// row of the interleaved intermediate (the mirrored group when the sample flips), one 16-byte store per channel plane.
__global__ __launch_bounds__(256) void vpass_f32_kernel(const FArgs a, const int* __restrict__ ws, float* __restrict__ out) {
  constexpr int PER = OUT / 4;
  const int total = a.n * OUT * PER;
  constexpr int64_t plane = (int64_t)OUT * OUT;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int q = i % PER;
    const int fy = i / PER;
    const int yo = fy % OUT;
    const FSample& s = a.s[fy / OUT];
    const int* bounds = ws + s.tab;
    int ymin = bounds[2 * yo], cnt = bounds[2 * yo + 1];
    ymin = max(0, min(ymin, s.in_h));
    cnt = max(0, min(min(cnt, a.stride), s.in_h - ymin));
    const int* k = bounds + 2 * OUT + (int64_t)yo * a.stride;
    const int qs = s.flip ? PER - 1 - q : q;      // source group of this output group
    const uint8_t* p = s.src + ((int64_t)ymin * OUT + (int64_t)qs * 4) * 3;
    int acc[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) acc[e] = 1 << (PRECISION_BITS - 1);
    for (int j = 0; j < cnt; ++j, p += OUT * 3) {
      const int w = k[j];
      const uint32_t* p4 = reinterpret_cast<const uint32_t*>(p);      // (12 qs bytes into a row of 1152 bytes of a 16-byte aligned buffer)
      const uint32_t w0 = p4[0], w1 = p4[1], w2 = p4[2];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc[e] += (int)((w0 >> (8 * e)) & 255u) * w;
        acc[4 + e] += (int)((w1 >> (8 * e)) & 255u) * w;
        acc[8 + e] += (int)((w2 >> (8 * e)) & 255u) * w;
      }
    }
    float v[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) v[e] = (float)clip8(acc[e]) / 255.0f;      // ToTensor: a correctly rounded division, not x * (1 / 255)
    // acc[e] is byte e of the 12: source pixel e / 3, channel e % 3; a flipped sample stores the four pixels in reverse order
    float* o = out + (int64_t)s.row * 3 * plane + (int64_t)yo * OUT + (int64_t)q * 4;
    if (s.flip) {
      *reinterpret_cast<float4*>(o) = make_float4(v[9], v[6], v[3], v[0]);
      *reinterpret_cast<float4*>(o + plane) = make_float4(v[10], v[7], v[4], v[1]);
      *reinterpret_cast<float4*>(o + 2 * plane) = make_float4(v[11], v[8], v[5], v[2]);
    } else {
      *reinterpret_cast<float4*>(o) = make_float4(v[0], v[3], v[6], v[9]);
      *reinterpret_cast<float4*>(o + plane) = make_float4(v[1], v[4], v[7], v[10]);
      *reinterpret_cast<float4*>(o + 2 * plane) = make_float4(v[2], v[5], v[8], v[11]);
    }
  }
}

int blocks_for(int64_t threads) { return (int)max((int64_t)1, min((int64_t)MAX_BLOCKS, (threads + 255) / 256)); }
int64_t pad16(int64_t n) { return (n + 15) & ~(int64_t)15; }

// Where everything of a group lives: the four tables of every sample in the table workspace (ints), and in the byte workspace the
// horizontal intermediate of stage 1 [H, W16, 3], the 16-multiple frame [H16, W16, 3] and the bicubic intermediate [ch, 384, 3].
struct Layout {
  int stride;
  int64_t table_ints, ws_bytes;
  int tab[MAX_IMAGES][4];                       // 0: W -> W16, 1: H -> H16 (bilinear); 2: cw -> 384, 3: ch -> 384 (bicubic)
  int in_size[MAX_IMAGES][4], out_size[MAX_IMAGES][4];
  int64_t tmp1[MAX_IMAGES], f16[MAX_IMAGES], tmp2[MAX_IMAGES];
};

const char* layout_of(const countr_pretrain_image* imgs, int n, Layout* L) {
  if (!imgs || n < 1 || n > MAX_IMAGES) return "bad args (1..16 samples)";
  L->stride = 0;
  int64_t ints = 0, bytes = 0;
  for (int s = 0; s < n; ++s) {
    const countr_pretrain_image& d = imgs[s];
    if (d.H < 16 || d.W < 16 || d.H > 1 << 15 || d.W > 1 << 15) return "frame height and width must be 16..32768";
    const int H16 = d.H / 16 * 16, W16 = d.W / 16 * 16;
    if (d.ch < 1 || d.cw < 1 || d.i < 0 || d.j < 0 || (int64_t)d.i + d.ch > H16 || (int64_t)d.j + d.cw > W16) {
      return "the crop must lie inside the frame resized to multiples of 16";
    }
    const int in[4] = {d.W, d.H, d.cw, d.ch}, out[4] = {W16, H16, OUT, OUT};
    for (int x = 0; x < 4; ++x) {
      const Axis ax = axis_of(x >= 2, in[x], out[x]);
      if (ax.ksize > MAX_KSIZE) return "resize ratio out of range";
      L->stride = max(L->stride, ax.ksize);
      L->in_size[s][x] = in[x]; L->out_size[s][x] = out[x];
    }
    L->tmp1[s] = bytes; bytes += pad16((int64_t)d.H * W16 * 3);
    L->f16[s] = bytes; bytes += pad16((int64_t)H16 * W16 * 3);
    L->tmp2[s] = bytes; bytes += pad16((int64_t)d.ch * OUT * 3);
  }
  for (int s = 0; s < n; ++s) {
    for (int x = 0; x < 4; ++x) {
      L->tab[s][x] = (int)ints;
      ints += (int64_t)L->out_size[s][x] * (2 + L->stride);
      if (ints > (int64_t)1 << 30) return "tables out of range";
    }
  }
  L->table_ints = ints;
  L->ws_bytes = bytes;
  return nullptr;
}

bool fail(const char* fn, const char* why) {
  char msg[256];
  snprintf(msg, sizeof msg, "%s: %s", fn, why);
  countr_set_error(msg);
  return false;
}

// output pixels per horizontal work item: the source bytes of a tile (+ alignment slack) must fit the LDS staging buffer
int tile_of(int in_size, int out_size, int filter) {
  const Axis ax = axis_of(filter, in_size, out_size);
  int tile = 256;
  while (tile >= 1 && ((int64_t)ceil(ax.scale * (tile - 1)) + ax.ksize + 1) * 3 + 48 > STAGE_BYTES) tile >>= 1;
  return tile;
}

}  // namespace

extern "C" int countr_pil_tables(int filter, int in_size, int out_size, int* bounds, int* weights) {
  if (filter != 0 && filter != 1) { countr_set_error("countr_pil_tables: filter is 0 (bilinear) or 1 (bicubic)"); return -1; }
  if (in_size < 1 || out_size < 1) { countr_set_error("countr_pil_tables: sizes must be >= 1 (and in / out below 2^19)"); return -1; }
  const Axis ax = axis_of(filter, in_size, out_size);
  if (ax.ksize > 1 << 20) { countr_set_error("countr_pil_tables: sizes must be >= 1 (and in / out below 2^19)"); return -1; }
  if (!bounds && !weights) return ax.ksize;
  if (!bounds || !weights) { countr_set_error("countr_pil_tables: pass both tables, or neither to ask for the tap stride"); return -1; }
  for (int xx = 0; xx < out_size; ++xx) table_row(filter, ax, in_size, xx, ax.ksize, bounds, weights);
  return ax.ksize;
}

extern "C" int countr_pretrain_aug_layout(const countr_pretrain_image* imgs, int n, int64_t* sizes) {
  Layout L;
  const char* why = layout_of(imgs, n, &L);
  if (why || !sizes) { fail("countr_pretrain_aug_layout", why ? why : "sizes is required"); return -1; }
  sizes[0] = L.stride; sizes[1] = L.table_ints; sizes[2] = L.ws_bytes;
  for (int s = 0; s < n; ++s)
    for (int x = 0; x < 4; ++x) sizes[3 + 4 * s + x] = L.tab[s][x];
  return 0;
}

extern "C" int countr_pretrain_aug_tables(const countr_pretrain_image* imgs, int n, int* tables, void* stream) {
  Layout L;
  const char* why = layout_of(imgs, n, &L);
  if (why || !tables) { fail("countr_pretrain_aug_tables", why ? why : "the table workspace is required"); return -1; }
  TableArgs a;
  a.njobs = 4 * n; a.stride = L.stride; a.rows = 0;
  for (int s = 0; s < n; ++s) {
    for (int x = 0; x < 4; ++x) {
      TableJob& j = a.job[4 * s + x];
      j.filter = x >= 2; j.in_size = L.in_size[s][x]; j.out_size = L.out_size[s][x]; j.off = L.tab[s][x]; j.first = a.rows;
      a.rows += j.out_size;
    }
  }
  hipLaunchKernelGGL(tables_kernel, dim3(blocks_for(a.rows)), dim3(256), 0, STREAM(stream), a, tables);
  COUNTR_LAUNCH_CHECK("countr_pretrain_aug_tables");
}

extern "C" int countr_pretrain_aug(const countr_pretrain_image* imgs, int n, const int* tables, void* workspace, float* out, int out_rows,
                                   void* stream) {
  const char* fn = "countr_pretrain_aug";
  Layout L;
  const char* why = layout_of(imgs, n, &L);
  if (why) { fail(fn, why); return -1; }
  if (!tables || !workspace || !out || (((uintptr_t)workspace) & 15) || (((uintptr_t)out) & 15)) {
    fail(fn, "tables, workspace and out are required (workspace and out 16-byte aligned)"); return -1;
  }
  HArgs h1, h2;
  VArgs v1;
  FArgs f;
  h1.n = h2.n = v1.n = f.n = n;
  h1.stride = h2.stride = v1.stride = f.stride = L.stride;
  h1.items = h2.items = 0;
  v1.total = 0;
  uint8_t* ws = (uint8_t*)workspace;
  for (int s = 0; s < n; ++s) {
    const countr_pretrain_image& d = imgs[s];
    if (!d.frame) { fail(fn, "null frame pointer"); return -1; }
    if (d.row < 0 || d.row >= out_rows) { fail(fn, "destination row outside the batch tensor"); return -1; }
    for (int t = 0; t < s; ++t)
      if (imgs[t].row == d.row) { fail(fn, "two samples name one destination row"); return -1; }
    const int H16 = d.H / 16 * 16, W16 = d.W / 16 * 16;
    const uint8_t* frame = (const uint8_t*)d.frame;
    const int64_t frame_bytes = (int64_t)d.H * d.W * 3;
    // a pass whose sizes are equal is skipped (Pillow skips it too; its taps would be the identity): the next pass reads its input
    const bool hskip = d.W == W16, vskip = d.H == H16;
    uint8_t* f16 = ws + L.f16[s];
    uint8_t* tmp1 = vskip ? f16 : ws + L.tmp1[s];               // the horizontal pass' output IS the 16-multiple frame
    // stage 1, horizontal: frame [H, W] -> tmp1 [H, W16]
    HSample& a = h1.s[s];
    a.src = frame; a.dst = tmp1; a.src_bytes = frame_bytes;
    a.pitch = d.W; a.x0 = 0; a.y0 = 0; a.in_w = d.W; a.rows = hskip ? 0 : d.H; a.out_w = W16;
    a.tab = L.tab[s][0]; a.vec = (((uintptr_t)frame) & 15) == 0;
    a.tile = tile_of(d.W, W16, 0);
    // stage 1, vertical: [H, W16] -> f16 [H16, W16]
    VSample& b = v1.s[s];
    b.src = hskip ? frame : tmp1; b.dst = f16; b.in_h = d.H; b.out_h = H16; b.row_bytes = 3 * W16; b.tab = L.tab[s][1];
    b.vec = (((uintptr_t)b.src) & 3) == 0;
    b.first = (int)v1.total;
    v1.total += vskip ? 0 : (int64_t)H16 * (b.row_bytes >> 2);
    // stage 2: the crop of the 16-multiple frame -> tmp2 [ch, 384]
    const bool direct = hskip && vskip;
    HSample& c = h2.s[s];
    c.src = direct ? frame : f16; c.dst = ws + L.tmp2[s]; c.src_bytes = (int64_t)H16 * W16 * 3;
    c.pitch = W16; c.x0 = d.j; c.y0 = d.i; c.in_w = d.cw; c.rows = d.ch; c.out_w = OUT;
    c.tab = L.tab[s][2]; c.vec = (((uintptr_t)c.src) & 15) == 0;
    c.tile = tile_of(d.cw, OUT, 1);
    if (a.tile < 1 || c.tile < 1) { fail(fn, "frame too wide (the taps of one output pixel exceed the 16-KB row staging)"); return -1; }
    for (HArgs* g : {&h1, &h2}) {
      HSample& x = g->s[s];
      x.tiles = (x.out_w + x.tile - 1) / x.tile;
      x.first = g->items;
      if ((int64_t)g->items + (int64_t)x.rows * x.tiles > (int64_t)1 << 30 || v1.total > (int64_t)1 << 30) { fail(fn, "group too large"); return -1; }
      g->items += x.rows * x.tiles;
    }
    // stage 3: tmp2 -> out[row], flipped
    FSample& e = f.s[s];
    e.src = c.dst; e.in_h = d.ch; e.tab = L.tab[s][3]; e.flip = d.flip != 0; e.row = d.row;
  }
  // the launch count is fixed: a pass with no work in this group (every sample skips it) still launches one idle block
  hipLaunchKernelGGL(hpass_kernel, dim3(max(1, min(MAX_BLOCKS, h1.items))), dim3(256), 0, STREAM(stream), h1, tables);
  hipLaunchKernelGGL(vpass_u8_kernel, dim3(blocks_for(v1.total)), dim3(256), 0, STREAM(stream), v1, tables);
  hipLaunchKernelGGL(hpass_kernel, dim3(max(1, min(MAX_BLOCKS, h2.items))), dim3(256), 0, STREAM(stream), h2, tables);
  hipLaunchKernelGGL(vpass_f32_kernel, dim3(blocks_for((int64_t)n * OUT * (OUT / 4))), dim3(256), 0, STREAM(stream), f, tables, out);
  COUNTR_LAUNCH_CHECK(fn);
}
