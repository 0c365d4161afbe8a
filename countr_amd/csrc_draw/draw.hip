// Marks drawn in place onto packed RGB frames on the device (include/countr_hip_draw.h states the rule).
//   countr_draw_paint   n <= 16 frames of one shape: segments, discs and texts in colours of their own, then the 4:2:0 buffer when asked for
//   countr_draw_font    the font, copied to the host
// The launches, all on the caller's stream, each with a grid plane per frame:
//   marks_kernel<false>  the claim.  blockIdx.x runs over the kinds: first the segments, four to a block (a wave each), then the discs, four
//                        to a block (a wave each), then the texts, one to a block.  A wave walks its segment's centres x brush in
//                        strides of 64 -- only the centres whose brush can reach the frame: on the segment's major axis the centre's
//                        coordinate is x0 +- i, so that range is two subtractions; when the call's longest segment has more than 128
//                        centres the segment blocks come in seg_parts copies, each walking its share of that range (a counting line
//                        across a 1080p frame is sixteen waves' work, not one's); the minor axis takes one fp64 division and an exact
//                        correction instead of int64 divisions -- and its disc's (2 r + 1)^2 box likewise; a block
//                        stages its text's glyph rows in LDS and walks the part of the text's box that lies inside the frame in strides
//                        of 256.  Every covered pixel of the frame gets atomicMax(owner, 1 + key).  Integer atomics of a maximum: the
//                        result does not depend on the order.
//   marks_kernel<true>   the paint.  The same walk; where owner == 1 + key the pixel takes the mark's colour and owner goes back to 0.
//                        Lanes of one mark that meet on a pixel write the same bytes.  Afterwards every plane is all zero again.
//   yuv_kernel<fmt>      step 5 of include/countr_hip_overlay.h from the finished RGB (csrc/rgb420.hpp, shared with csrc_overlay/overlay.hip).
// No kernel uses scratch (-Rpass-analysis=kernel-resource-usage).
#include <stdio.h>
#include <string.h>
#include "../csrc/common.hpp"
#include "../csrc/host_api.hpp"
#include "../csrc/rgb420.hpp"
#include "../../include/countr_hip_draw.h"

namespace {

constexpr int MAXF = COUNTR_DRAW_MAX_FRAMES;
constexpr int COORD = COUNTR_DRAW_MAX_COORD;
constexpr int PART = 128;                                         // centres of a segment a wave walks: a longer segment is shared by several waves
constexpr int SEGW = COUNTR_DRAW_SEGMENT_WORDS, DISCW = COUNTR_DRAW_DISC_WORDS, TEXTW = COUNTR_DRAW_TEXT_WORDS;
constexpr int GLYPHS = COUNTR_DRAW_FONT_GLYPHS, ROWS = COUNTR_DRAW_FONT_ROWS, CHARS = COUNTR_DRAW_TEXT_BYTES;
static_assert(MAXF == 16 && COUNTR_DRAW_NV12 == RGB420_NV12 && COUNTR_DRAW_NV21 == RGB420_NV21 && COUNTR_DRAW_I420 == RGB420_I420,
              "csrc/rgb420.hpp converts up to 16 frames and names the formats by the header's numbers");
static_assert(TEXTW * 4 == 24 + CHARS && COUNTR_DRAW_FONT_COLS == 5 && ROWS == 7 && COUNTR_DRAW_FONT_FIRST == 32, "the header's record and font");

// ---- the font, drawn by hand: 5 x 7, '#' is a set bit.  One statement (GLYPH_TABLE), two copies: the host's and the device's.
constexpr uint8_t glyph_row(const char (&s)[6]) {
  return (uint8_t)((s[0] == '#') << 4 | (s[1] == '#') << 3 | (s[2] == '#') << 2 | (s[3] == '#') << 1 | (s[4] == '#'));
}
#define G(a, b, c, d, e, f, g) {glyph_row(a), glyph_row(b), glyph_row(c), glyph_row(d), glyph_row(e), glyph_row(f), glyph_row(g)},
#define GLYPH_TABLE \
  G(".....", ".....", ".....", ".....", ".....", ".....", ".....") /* ' ' */ \
  G("..#..", "..#..", "..#..", "..#..", "..#..", ".....", "..#..") /* ! */ \
  G(".#.#.", ".#.#.", ".#.#.", ".....", ".....", ".....", ".....") /* " */ \
  G(".#.#.", ".#.#.", "#####", ".#.#.", "#####", ".#.#.", ".#.#.") /* # */ \
  G("..#..", ".####", "#.#..", ".###.", "..#.#", "####.", "..#..") /* $ */ \
  G("##...", "##..#", "...#.", "..#..", ".#...", "#..##", "...##") /* % */ \
  G(".##..", "#..#.", "#.#..", ".#...", "#.#.#", "#..#.", ".##.#") /* & */ \
  G("..#..", "..#..", "..#..", ".....", ".....", ".....", ".....") /* ' */ \
  G("...#.", "..#..", ".#...", ".#...", ".#...", "..#..", "...#.") /* ( */ \
  G(".#...", "..#..", "...#.", "...#.", "...#.", "..#..", ".#...") /* ) */ \
  G(".....", "..#..", "#.#.#", ".###.", "#.#.#", "..#..", ".....") /* * */ \
  G(".....", "..#..", "..#..", "#####", "..#..", "..#..", ".....") /* + */ \
  G(".....", ".....", ".....", ".....", ".##..", "..#..", ".#...") /* , */ \
  G(".....", ".....", ".....", "#####", ".....", ".....", ".....") /* - */ \
  G(".....", ".....", ".....", ".....", ".....", ".##..", ".##..") /* . */ \
  G(".....", "....#", "...#.", "..#..", ".#...", "#....", ".....") /* / */ \
  G(".###.", "#...#", "#..##", "#.#.#", "##..#", "#...#", ".###.") /* 0 */ \
  G("..#..", ".##..", "..#..", "..#..", "..#..", "..#..", ".###.") /* 1 */ \
  G(".###.", "#...#", "....#", "...#.", "..#..", ".#...", "#####") /* 2 */ \
  G("#####", "...#.", "..#..", "...#.", "....#", "#...#", ".###.") /* 3 */ \
  G("...#.", "..##.", ".#.#.", "#..#.", "#####", "...#.", "...#.") /* 4 */ \
  G("#####", "#....", "####.", "....#", "....#", "#...#", ".###.") /* 5 */ \
  G("..##.", ".#...", "#....", "####.", "#...#", "#...#", ".###.") /* 6 */ \
  G("#####", "....#", "...#.", "..#..", ".#...", ".#...", ".#...") /* 7 */ \
  G(".###.", "#...#", "#...#", ".###.", "#...#", "#...#", ".###.") /* 8 */ \
  G(".###.", "#...#", "#...#", ".####", "....#", "...#.", ".##..") /* 9 */ \
  G(".....", ".##..", ".##..", ".....", ".##..", ".##..", ".....") /* : */ \
  G(".....", ".##..", ".##..", ".....", ".##..", "..#..", ".#...") /* ; */ \
  G("...#.", "..#..", ".#...", "#....", ".#...", "..#..", "...#.") /* < */ \
  G(".....", ".....", "#####", ".....", "#####", ".....", ".....") /* = */ \
  G(".#...", "..#..", "...#.", "....#", "...#.", "..#..", ".#...") /* > */ \
  G(".###.", "#...#", "....#", "...#.", "..#..", ".....", "..#..") /* ? */ \
  G(".###.", "#...#", "....#", ".##.#", "#.#.#", "#.#.#", ".###.") /* @ */ \
  G(".###.", "#...#", "#...#", "#...#", "#####", "#...#", "#...#") /* A */ \
  G("####.", "#...#", "#...#", "####.", "#...#", "#...#", "####.") /* B */ \
  G(".###.", "#...#", "#....", "#....", "#....", "#...#", ".###.") /* C */ \
  G("###..", "#..#.", "#...#", "#...#", "#...#", "#..#.", "###..") /* D */ \
  G("#####", "#....", "#....", "####.", "#....", "#....", "#####") /* E */ \
  G("#####", "#....", "#....", "####.", "#....", "#....", "#....") /* F */ \
  G(".###.", "#...#", "#....", "#.###", "#...#", "#...#", ".####") /* G */ \
  G("#...#", "#...#", "#...#", "#####", "#...#", "#...#", "#...#") /* H */ \
  G(".###.", "..#..", "..#..", "..#..", "..#..", "..#..", ".###.") /* I */ \
  G("..###", "...#.", "...#.", "...#.", "...#.", "#..#.", ".##..") /* J */ \
  G("#...#", "#..#.", "#.#..", "##...", "#.#..", "#..#.", "#...#") /* K */ \
  G("#....", "#....", "#....", "#....", "#....", "#....", "#####") /* L */ \
  G("#...#", "##.##", "#.#.#", "#.#.#", "#...#", "#...#", "#...#") /* M */ \
  G("#...#", "#...#", "##..#", "#.#.#", "#..##", "#...#", "#...#") /* N */ \
  G(".###.", "#...#", "#...#", "#...#", "#...#", "#...#", ".###.") /* O */ \
  G("####.", "#...#", "#...#", "####.", "#....", "#....", "#....") /* P */ \
  G(".###.", "#...#", "#...#", "#...#", "#.#.#", "#..#.", ".##.#") /* Q */ \
  G("####.", "#...#", "#...#", "####.", "#.#..", "#..#.", "#...#") /* R */ \
  G(".####", "#....", "#....", ".###.", "....#", "....#", "####.") /* S */ \
  G("#####", "..#..", "..#..", "..#..", "..#..", "..#..", "..#..") /* T */ \
  G("#...#", "#...#", "#...#", "#...#", "#...#", "#...#", ".###.") /* U */ \
  G("#...#", "#...#", "#...#", "#...#", "#...#", ".#.#.", "..#..") /* V */ \
  G("#...#", "#...#", "#...#", "#.#.#", "#.#.#", "#.#.#", ".#.#.") /* W */ \
  G("#...#", "#...#", ".#.#.", "..#..", ".#.#.", "#...#", "#...#") /* X */ \
  G("#...#", "#...#", "#...#", ".#.#.", "..#..", "..#..", "..#..") /* Y */ \
  G("#####", "....#", "...#.", "..#..", ".#...", "#....", "#####") /* Z */ \
  G(".###.", ".#...", ".#...", ".#...", ".#...", ".#...", ".###.") /* [ */ \
  G(".....", "#....", ".#...", "..#..", "...#.", "....#", ".....") /* \ */ \
  G(".###.", "...#.", "...#.", "...#.", "...#.", "...#.", ".###.") /* ] */ \
  G("..#..", ".#.#.", "#...#", ".....", ".....", ".....", ".....") /* ^ */ \
  G(".....", ".....", ".....", ".....", ".....", ".....", "#####") /* _ */ \
  G(".#...", "..#..", "...#.", ".....", ".....", ".....", ".....") /* ` */ \
  G(".....", ".....", ".###.", "....#", ".####", "#...#", ".####") /* a */ \
  G("#....", "#....", "#.##.", "##..#", "#...#", "#...#", "####.") /* b */ \
  G(".....", ".....", ".###.", "#....", "#....", "#...#", ".###.") /* c */ \
  G("....#", "....#", ".##.#", "#..##", "#...#", "#...#", ".####") /* d */ \
  G(".....", ".....", ".###.", "#...#", "#####", "#....", ".###.") /* e */ \
  G("..##.", ".#..#", ".#...", "###..", ".#...", ".#...", ".#...") /* f */ \
  G(".....", ".####", "#...#", "#...#", ".####", "....#", ".###.") /* g */ \
  G("#....", "#....", "#.##.", "##..#", "#...#", "#...#", "#...#") /* h */ \
  G("..#..", ".....", ".##..", "..#..", "..#..", "..#..", ".###.") /* i */ \
  G("...#.", ".....", "..##.", "...#.", "...#.", "#..#.", ".##..") /* j */ \
  G("#....", "#....", "#..#.", "#.#..", "##...", "#.#..", "#..#.") /* k */ \
  G(".##..", "..#..", "..#..", "..#..", "..#..", "..#..", ".###.") /* l */ \
  G(".....", ".....", "##.#.", "#.#.#", "#.#.#", "#...#", "#...#") /* m */ \
  G(".....", ".....", "#.##.", "##..#", "#...#", "#...#", "#...#") /* n */ \
  G(".....", ".....", ".###.", "#...#", "#...#", "#...#", ".###.") /* o */ \
  G(".....", ".....", "####.", "#...#", "####.", "#....", "#....") /* p */ \
  G(".....", ".....", ".##.#", "#..##", ".####", "....#", "....#") /* q */ \
  G(".....", ".....", "#.##.", "##..#", "#....", "#....", "#....") /* r */ \
  G(".....", ".....", ".###.", "#....", ".###.", "....#", "####.") /* s */ \
  G(".#...", ".#...", "###..", ".#...", ".#...", ".#..#", "..##.") /* t */ \
  G(".....", ".....", "#...#", "#...#", "#...#", "#..##", ".##.#") /* u */ \
  G(".....", ".....", "#...#", "#...#", "#...#", ".#.#.", "..#..") /* v */ \
  G(".....", ".....", "#...#", "#...#", "#.#.#", "#.#.#", ".#.#.") /* w */ \
  G(".....", ".....", "#...#", ".#.#.", "..#..", ".#.#.", "#...#") /* x */ \
  G(".....", ".....", "#...#", "#...#", ".####", "....#", ".###.") /* y */ \
  G(".....", ".....", "#####", "...#.", "..#..", ".#...", "#####") /* z */ \
  G("...#.", "..#..", "..#..", ".#...", "..#..", "..#..", "...#.") /* { */ \
  G("..#..", "..#..", "..#..", "..#..", "..#..", "..#..", "..#..") /* | */ \
  G(".#...", "..#..", "..#..", "...#.", "..#..", "..#..", ".#...") /* } */ \
  G(".....", ".....", ".#...", "#.#.#", "...#.", ".....", ".....") /* ~ */

const uint8_t FONT[GLYPHS][ROWS] = {GLYPH_TABLE};
__constant__ uint8_t d_font[GLYPHS][ROWS] = {GLYPH_TABLE};
#undef G

struct DrawArgs {
  uint8_t* rgb[MAXF];
  uint32_t* owner[MAXF];
  int n_segments[MAXF], segments_off[MAXF], n_discs[MAXF], discs_off[MAXF], n_texts[MAXF], texts_off[MAXF];
  const uint8_t* pack;
  int H, W;
  int seg_blocks, seg_parts, disc_blocks;                         // blocks of blockIdx.x: seg_blocks x seg_parts carry segments, then discs; texts behind
};

// 1 + key of mark i of its kind: segments below discs below texts
constexpr uint32_t SEG_KEY = 1u, DISC_KEY = SEG_KEY + COUNTR_DRAW_MAX_SEGMENTS, TEXT_KEY = DISC_KEY + COUNTR_DRAW_MAX_DISCS;

__device__ __forceinline__ bool in_range(int v) { return v >= -COORD && v <= COORD; }

// rdiv of csrc/rgb420.hpp for |v| <= 2^42 and 0 < n <= 2^21: one fp64 division (its operands are exact) and an exact correction
__device__ __forceinline__ int rdiv21(int64_t v, int n) {
  const int64_t num = 2 * v + n, den = 2 * (int64_t)n;
  int64_t q = (int64_t)floor((double)num / (double)den);
  const int64_t r = num - q * den;
  if (r < 0) --q;
  else if (r >= den) ++q;
  return (int)q;
}

// a pixel a mark covers: the claim, or the paint where the claim was won
template <bool PAINT>
__device__ __forceinline__ void touch(const DrawArgs& a, int f, int x, int y, uint32_t key, int rgb) {
  if (x < 0 || x >= a.W || y < 0 || y >= a.H) return;
  const int64_t i = (int64_t)y * a.W + x;
  uint32_t* o = a.owner[f] + i;
  if constexpr (!PAINT) {
    atomicMax(o, key);
  } else {
    if (*o != key) return;
    uint8_t* p = a.rgb[f] + 3 * i;
    p[0] = (uint8_t)(rgb >> 16); p[1] = (uint8_t)(rgb >> 8); p[2] = (uint8_t)rgb;
    *o = 0u;
  }
}

template <bool PAINT>
__global__ __launch_bounds__(256) void marks_kernel(const DrawArgs a) {
  __shared__ uint8_t s_rows[CHARS * 8];                           // a text's glyph rows, 8 bytes a character (the eighth is empty)
  const int f = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int b = blockIdx.x;
  if (b < a.seg_blocks * a.seg_parts) {                           // ---- a wave per segment and part of its centres
    const int part = b % a.seg_parts, s = (b / a.seg_parts) * 4 + wave;
    if (s >= a.n_segments[f]) return;
    const int* v = reinterpret_cast<const int*>(a.pack + a.segments_off[f]) + SEGW * (int64_t)s;
    const int x0 = v[0], y0 = v[1], x1 = v[2], y1 = v[3], w = v[4], rgb = v[5];
    if (!in_range(x0) || !in_range(y0) || !in_range(x1) || !in_range(y1) || w < 0 || w > COUNTR_DRAW_MAX_HALF_WIDTH) return;
    const int dx = x1 - x0, dy = y1 - y0;
    const int n = max(abs(dx), abs(dy));
    // the centres lo .. hi whose brush can reach the frame: on the major axis the centre's coordinate is c0 + sgn i
    int lo = 0, hi = n;
    if (n) {
      const bool xm = abs(dx) == n;
      const int c0 = xm ? x0 : y0, last = (xm ? a.W : a.H) - 1 + w;
      if ((xm ? dx : dy) > 0) { lo = max(0, -w - c0); hi = min(n, last - c0); }
      else { lo = max(0, c0 - last); hi = min(n, c0 + w); }
    }
    if (hi < lo) return;
    const int chunk = (hi - lo + a.seg_parts) / a.seg_parts;      // this wave's share of lo .. hi
    lo += part * chunk;
    hi = min(hi, lo + chunk - 1);
    if (hi < lo) return;
    const bool xm = abs(dx) == n;                                 // on the major axis rdiv(i d, n) is +-i
    const int side = 2 * w + 1, box = side * side, total = (hi - lo + 1) * box;       // <= (16384 + 16) * 289
    for (int idx = lane; idx < total; idx += 64) {
      const int c = idx / box, q = idx - c * box, i = lo + c;
      const int u = q % side - w, t = q / side - w;
      if (u * u + t * t > w * w) continue;
      const int cx = !n ? x0 : xm ? x0 + (dx > 0 ? i : -i) : x0 + rdiv21((int64_t)i * dx, n);
      const int cy = !n ? y0 : xm ? y0 + rdiv21((int64_t)i * dy, n) : y0 + (dy > 0 ? i : -i);
      touch<PAINT>(a, f, cx + u, cy + t, SEG_KEY + (uint32_t)s, rgb);
    }
    return;
  }
  b -= a.seg_blocks * a.seg_parts;
  if (b < a.disc_blocks) {                                        // ---- a wave per disc
    const int d = b * 4 + wave;
    if (d >= a.n_discs[f]) return;
    const int* v = reinterpret_cast<const int*>(a.pack + a.discs_off[f]) + DISCW * (int64_t)d;
    const int cx = v[0], cy = v[1], r = v[2], rgb = v[3];
    if (!in_range(cx) || !in_range(cy) || r < 0 || r > COUNTR_DRAW_MAX_RADIUS) return;
    const int side = 2 * r + 1;
    for (int idx = lane; idx < side * side; idx += 64) {
      const int u = idx % side - r, t = idx / side - r;
      if (u * u + t * t > r * r) continue;
      touch<PAINT>(a, f, cx + u, cy + t, DISC_KEY + (uint32_t)d, rgb);
    }
    return;
  }
  b -= a.disc_blocks;                                             // ---- a block per text (every exit below is uniform over the block)
  if (b >= a.n_texts[f]) return;
  const int* v = reinterpret_cast<const int*>(a.pack + a.texts_off[f]) + TEXTW * (int64_t)b;
  const int x = v[0], y = v[1], s = v[2], fg = v[3], bg = v[4], len = v[5];
  if (!in_range(x) || !in_range(y) || s < 1 || s > COUNTR_DRAW_MAX_SCALE || len < 0 || len > CHARS) return;
  const int xa = max(x, 0), xb = min(x + 6 * s * len, a.W), ya = max(y, 0), yb = min(y + 8 * s, a.H);
  if (xa >= xb || ya >= yb) return;
  {
    const int k = threadIdx.x >> 3, r = threadIdx.x & 7;
    uint8_t bits = 0;
    if (k < len && r < ROWS) {
      const int ch = reinterpret_cast<const uint8_t*>(v + 6)[k];
      bits = d_font[(ch >= 32 && ch <= 126 ? ch : '?') - 32][r];
    }
    s_rows[threadIdx.x] = bits;
  }
  __syncthreads();
  const int cw = xb - xa, total = cw * (yb - ya);                 // <= 1536 x 64
  for (int idx = threadIdx.x; idx < total; idx += 256) {
    const int py = idx / cw, px = idx - py * cw;
    const int u = xa + px - x, t = ya + py - y;                   // inside the text's box
    const int k = u / (6 * s), gu = (u - k * 6 * s) / s, gt = t / s;
    const bool on = gu < 5 && ((s_rows[k * 8 + gt] >> (4 - gu)) & 1);
    if (on) touch<PAINT>(a, f, xa + px, ya + py, TEXT_KEY + (uint32_t)b, fg);
    else if (bg >= 0) touch<PAINT>(a, f, xa + px, ya + py, TEXT_KEY + (uint32_t)b, bg);
  }
}

bool coord(int v) { return v >= -COORD && v <= COORD; }
bool colour(int v) { return v >= 0 && v <= 0xffffff; }

// n records of `words` int32 at `off` lie inside the pack, 4-byte aligned
bool inside(int off, int n, int words, int pack_bytes) { return off >= 0 && !(off & 3) && (int64_t)off + 4ll * words * n <= (int64_t)pack_bytes; }

}  // namespace

extern "C" int countr_draw_version(void) { return COUNTR_DRAW_ABI_VERSION; }

extern "C" const char* countr_draw_last_error(void) { return g_err; }

extern "C" int countr_draw_font(void* out) {
  if (!out) return fail(-1, "countr_draw_font: out is required");
  memcpy(out, FONT, sizeof(FONT));
  return 0;
}

extern "C" int countr_draw_paint(const countr_draw_frame* frames, int n, int H, int W, const void* host_pack, const void* pack, int pack_bytes,
                                 int format, int matrix, int range, void* stream) {
  if (n < 1 || n > MAXF) return failf(-1, "countr_draw_paint: 1..%d frames a call, got %d", MAXF, n);
  if (format < COUNTR_DRAW_RGB || format > COUNTR_DRAW_I420) return failf(-1, "countr_draw_paint: unknown format %d", format);
  if (matrix != COUNTR_DRAW_BT601 && matrix != COUNTR_DRAW_BT709) return failf(-1, "countr_draw_paint: unknown matrix %d", matrix);
  if (range != COUNTR_DRAW_LIMITED && range != COUNTR_DRAW_FULL) return failf(-1, "countr_draw_paint: unknown range %d", range);
  if (H < 1 || H > COUNTR_DRAW_MAX_SIDE || W < 1 || W > COUNTR_DRAW_MAX_SIDE)
    return failf(-1, "countr_draw_paint: H and W are 1..%d, got %d x %d", COUNTR_DRAW_MAX_SIDE, H, W);
  if (!frames) return fail(-1, "countr_draw_paint: the frames array is required");
  if (pack_bytes < 0) return failf(-1, "countr_draw_paint: pack_bytes is >= 0, got %d", pack_bytes);
  DrawArgs a;
  Rgb420Args y;
  memset(&a, 0, sizeof(a));
  memset(&y, 0, sizeof(y));
  uintptr_t bits = (uintptr_t)W;
  int max_segments = 0, max_discs = 0, max_texts = 0, longest = 1;
  for (int j = 0; j < n; ++j) {
    const countr_draw_frame& fr = frames[j];
    if (!fr.rgb || !fr.owner || (format != COUNTR_DRAW_RGB && !fr.yuv)) return failf(-1, "countr_draw_paint: frame %d has a null pointer", j);
    if (format == COUNTR_DRAW_RGB && fr.yuv) return failf(-1, "countr_draw_paint: frame %d: yuv must be NULL when the format is RGB", j);
    if (misaligned(fr.owner, 4)) return failf(-1, "countr_draw_paint: frame %d: the owner plane is 4-byte aligned", j);
    if (fr.n_segments < 0 || fr.n_segments > COUNTR_DRAW_MAX_SEGMENTS)
      return failf(-1, "countr_draw_paint: frame %d: 0..%d segments, got %d", j, COUNTR_DRAW_MAX_SEGMENTS, fr.n_segments);
    if (fr.n_discs < 0 || fr.n_discs > COUNTR_DRAW_MAX_DISCS)
      return failf(-1, "countr_draw_paint: frame %d: 0..%d discs, got %d", j, COUNTR_DRAW_MAX_DISCS, fr.n_discs);
    if (fr.n_texts < 0 || fr.n_texts > COUNTR_DRAW_MAX_TEXTS)
      return failf(-1, "countr_draw_paint: frame %d: 0..%d texts, got %d", j, COUNTR_DRAW_MAX_TEXTS, fr.n_texts);
    if (fr.n_segments + fr.n_discs + fr.n_texts) {
      if (!host_pack || !pack || misaligned(pack, 16))
        return fail(-1, "countr_draw_paint: a call with marks needs the packed upload on the host and, 16-byte aligned, on the device");
      if ((fr.n_segments && !inside(fr.segments_off, fr.n_segments, SEGW, pack_bytes)) ||
          (fr.n_discs && !inside(fr.discs_off, fr.n_discs, DISCW, pack_bytes)) ||
          (fr.n_texts && !inside(fr.texts_off, fr.n_texts, TEXTW, pack_bytes)))
        return failf(-1, "countr_draw_paint: frame %d: an offset lies outside the packed upload of %d bytes (or is not 4-byte aligned)", j,
                     pack_bytes);
    }
    const char* base = static_cast<const char*>(host_pack);
    const int* v = fr.n_segments ? reinterpret_cast<const int*>(base + fr.segments_off) : nullptr;
    for (int i = 0; i < fr.n_segments; ++i, v += SEGW) {
      if (!coord(v[0]) || !coord(v[1]) || !coord(v[2]) || !coord(v[3]))
        return failf(-1, "countr_draw_paint: frame %d segment %d: coordinates are within +-%d, got (%d, %d) (%d, %d)", j, i, COORD, v[0], v[1],
                     v[2], v[3]);
      if (v[4] < 0 || v[4] > COUNTR_DRAW_MAX_HALF_WIDTH)
        return failf(-1, "countr_draw_paint: frame %d segment %d: half_width is 0..%d, got %d", j, i, COUNTR_DRAW_MAX_HALF_WIDTH, v[4]);
      if (!colour(v[5])) return failf(-1, "countr_draw_paint: frame %d segment %d: a colour is 0..0xffffff, got %d", j, i, v[5]);
      const int dx = v[2] > v[0] ? v[2] - v[0] : v[0] - v[2], dy = v[3] > v[1] ? v[3] - v[1] : v[1] - v[3];
      const int len = (dx > dy ? dx : dy) + 1;
      longest = len > longest ? len : longest;
    }
    v = fr.n_discs ? reinterpret_cast<const int*>(base + fr.discs_off) : nullptr;
    for (int i = 0; i < fr.n_discs; ++i, v += DISCW) {
      if (!coord(v[0]) || !coord(v[1]))
        return failf(-1, "countr_draw_paint: frame %d disc %d: coordinates are within +-%d, got (%d, %d)", j, i, COORD, v[0], v[1]);
      if (v[2] < 0 || v[2] > COUNTR_DRAW_MAX_RADIUS)
        return failf(-1, "countr_draw_paint: frame %d disc %d: r is 0..%d, got %d", j, i, COUNTR_DRAW_MAX_RADIUS, v[2]);
      if (!colour(v[3])) return failf(-1, "countr_draw_paint: frame %d disc %d: a colour is 0..0xffffff, got %d", j, i, v[3]);
    }
    v = fr.n_texts ? reinterpret_cast<const int*>(base + fr.texts_off) : nullptr;
    for (int i = 0; i < fr.n_texts; ++i, v += TEXTW) {
      if (!coord(v[0]) || !coord(v[1]))
        return failf(-1, "countr_draw_paint: frame %d text %d: coordinates are within +-%d, got (%d, %d)", j, i, COORD, v[0], v[1]);
      if (v[2] < 1 || v[2] > COUNTR_DRAW_MAX_SCALE)
        return failf(-1, "countr_draw_paint: frame %d text %d: scale is 1..%d, got %d", j, i, COUNTR_DRAW_MAX_SCALE, v[2]);
      if (v[5] < 0 || v[5] > CHARS) return failf(-1, "countr_draw_paint: frame %d text %d: 0..%d bytes of text, got %d", j, i, CHARS, v[5]);
      if (!colour(v[3]) || (v[4] != -1 && !colour(v[4])))
        return failf(-1, "countr_draw_paint: frame %d text %d: a colour is 0..0xffffff (background -1: none), got %d and %d", j, i, v[3], v[4]);
    }
    bits |= (uintptr_t)fr.rgb | (uintptr_t)fr.yuv;
    a.rgb[j] = (uint8_t*)fr.rgb;
    a.owner[j] = (uint32_t*)fr.owner;
    a.n_segments[j] = fr.n_segments; a.segments_off[j] = fr.segments_off;
    a.n_discs[j] = fr.n_discs; a.discs_off[j] = fr.discs_off;
    a.n_texts[j] = fr.n_texts; a.texts_off[j] = fr.texts_off;
    y.src[j] = (const uint8_t*)fr.rgb;
    y.dst[j] = (uint8_t*)fr.yuv;
    max_segments = fr.n_segments > max_segments ? fr.n_segments : max_segments;
    max_discs = fr.n_discs > max_discs ? fr.n_discs : max_discs;
    max_texts = fr.n_texts > max_texts ? fr.n_texts : max_texts;
  }
  a.pack = (const uint8_t*)pack;
  a.H = H; a.W = W;
  a.seg_blocks = (max_segments + 3) / 4;
  const int reach = (H > W ? H : W) + 2 * COUNTR_DRAW_MAX_HALF_WIDTH;                      // no more centres of a segment can reach the frame
  a.seg_parts = ((longest < reach ? longest : reach) + PART - 1) / PART;                   // 1 .. 129
  a.disc_blocks = (max_discs + 3) / 4;
  y.H = H; y.W = W; y.vec = (bits & 15) == 0;
  set_coefficients(y, matrix, range);
  hipStream_t st = STREAM(stream);
  const unsigned blocks = (unsigned)(a.seg_blocks * a.seg_parts + a.disc_blocks + max_texts);      // <= 16400 * 129 + 1024 + 4160
  if (blocks) {
    hipLaunchKernelGGL((marks_kernel<false>), dim3(blocks, (unsigned)n), dim3(256), 0, st, a);
    hipLaunchKernelGGL((marks_kernel<true>), dim3(blocks, (unsigned)n), dim3(256), 0, st, a);
  }
  launch_rgb420(format, y, n, st);
  return launched("countr_draw_paint");
}
