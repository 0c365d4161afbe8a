// The pretraining loader's transform on the device: fsc147.transform_pretrain = Pillow BILINEAR resize to multiples of 16 -> crop ->
// Pillow BICUBIC resize to 384 x 384 -> horizontal flip -> ToTensor, for a batch whose samples all differ in frame and crop size.
//   countr_pil_tables            (host only) the per-axis tap tables of Pillow's 8-bit resample for BILINEAR (0) and BICUBIC (1)
//                                (Resample.c: precompute_coeffs + normalize_coeffs_8bpc)
//   countr_pretrain_aug_layout   (host only) tap stride, table and workspace sizes of a group of <= 16 samples
//   countr_pretrain_aug_tables   one launch: the four tables of every sample, computed on the device in fp64 in Pillow's operation order
//   countr_pretrain_aug          four launches: stage 1 horizontal, stage 1 vertical (uint8 [H, W, 3] -> uint8 [H16, W16, 3]), the
//                                bicubic horizontal pass over the crop rectangle, the bicubic vertical pass + flip + ToTensor into the
//                                batch tensor
// The tables and the bodies of the passes are pil_resample.hpp's (shared with frames.hip); the kernels here take every sample's sizes and
// buffers from a descriptor.  The result equals PIL + ToTensor bit for bit.
// uint8 / fp32 only: the bf16 and the fp16 build of the library export the same code.
#include "common.hpp"
#include "pil_resample.hpp"
#include "../../include/countr_hip.h"

namespace {

constexpr int MAX_IMAGES = COUNTR_PRETRAIN_MAX_IMAGES;
constexpr int OUT = 384;
constexpr int MAX_BLOCKS = 2048;
constexpr int MAX_KSIZE = 1 << 12;

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

// Horizontal pass (pil_hpass_item).  One work item = (sample, source row, tile of `tile` output pixels).
__global__ __launch_bounds__(256) void hpass_kernel(const HArgs a, const int* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[STAGE_BYTES];
  for (int it = blockIdx.x; it < a.items; it += gridDim.x) {
    int f = 0;
    while (f + 1 < a.n && a.s[f + 1].first <= it) ++f;
    const HSample& s = a.s[f];
    const int local = it - s.first;
    const int t = local % s.tiles, y = local / s.tiles;
    const int* bounds = ws + s.tab;
    pil_hpass_item(s.src, s.src_bytes, s.pitch, s.x0, s.y0 + y, s.in_w, bounds, bounds + 2 * s.out_w, a.stride,
                   s.dst + (int64_t)y * s.out_w * 3, s.out_w, s.tile, t, s.vec != 0, stage);
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
    int ymin, cnt;
    const int* k = pil_vtaps(bounds, bounds + 2 * s.out_h, a.stride, s.in_h, yo, &ymin, &cnt);
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
    int ymin, cnt;
    const int* k = pil_vtaps(bounds, bounds + 2 * OUT, a.stride, s.in_h, yo, &ymin, &cnt);
    const int qs = s.flip ? PER - 1 - q : q;      // source group of this output group
    int acc[12];
    // (12 qs bytes into a row of 1152 bytes of a 16-byte aligned buffer)
    pil_vacc<12>(s.src + ((int64_t)ymin * OUT + (int64_t)qs * 4) * 3, OUT * 3, k, cnt, acc);
    pil_store_planes<12>(out + (int64_t)s.row * 3 * plane + (int64_t)yo * OUT + (int64_t)q * 4, plane, acc, s.flip != 0);
  }
}

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

}  // namespace

extern "C" int countr_pil_tables(int filter, int in_size, int out_size, int* bounds, int* weights) {
  if (filter != 0 && filter != 1) { countr_set_error("countr_pil_tables: filter is 0 (bilinear) or 1 (bicubic)"); return -1; }
  Axis ax;
  if (!axis_ok(filter, in_size, out_size, &ax)) { countr_set_error("countr_pil_tables: sizes must be >= 1 (and in / out below 2^19)"); return -1; }
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
  hipLaunchKernelGGL(tables_kernel, dim3(countr_blocks_for(a.rows, MAX_BLOCKS)), dim3(256), 0, STREAM(stream), a, tables);
  return countr_check_launch("countr_pretrain_aug_tables");
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
  hipLaunchKernelGGL(vpass_u8_kernel, dim3(countr_blocks_for(v1.total, MAX_BLOCKS)), dim3(256), 0, STREAM(stream), v1, tables);
  hipLaunchKernelGGL(hpass_kernel, dim3(max(1, min(MAX_BLOCKS, h2.items))), dim3(256), 0, STREAM(stream), h2, tables);
  hipLaunchKernelGGL(vpass_f32_kernel, dim3(countr_blocks_for((int64_t)n * OUT * (OUT / 4), MAX_BLOCKS)), dim3(256), 0, STREAM(stream), f, tables, out);
  return countr_check_launch(fn);
}
