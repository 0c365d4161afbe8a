// Object locations from density maps: the local maxima of n maps, one deterministic rule (include/countr_hip.h states it), four launches.
//   countr_peaks_workspace  (host only) bytes of scratch a call needs
//   countr_density_peaks    fp32 [h, w] maps, sizes free per map -> totals[n] and recs[n][cap][6] = {y, x, score, cy, cx, mass}
// The launches, whatever n is:
//   1 peaks_max_kernel     PARTS block maxima per map (fmaxf: a NaN never wins); 16-byte loads when the map's base is aligned
//   2 peaks_detect_kernel  one 32 x 64 tile + an r-wide halo in LDS per block; a wave owns a tile row, lane = column, so the ballot of
//                          "is a peak" IS the row segment's 64-bit mask: masks[y][tile column].  The window test runs only for pixels
//                          above both thresholds
//   3 peaks_write_kernel   raster order = (y, tile column, bit): a block sums the popcounts in front of its rows, scans its own
//                          segments, and its waves write one record per peak (window sums over the lanes, fixed butterfly) at the
//                          peak's raster rank -- counts + exclusive scan, no atomic decides a place or a sum
//   4 peaks_rank_kernel    rank by counting: place = |{j: score_j > score_k, or equal and j < k}| (raster order = idx order)
// fp32 only: the bf16 and the fp16 build of the library export the same code.
#include <limits.h>
#include <math.h>
#include "common.hpp"
#include "../../include/countr_hip.h"

namespace {

constexpr int MAX_MAPS = COUNTR_PEAKS_MAX_MAPS;
constexpr int MAX_R = COUNTR_PEAKS_MAX_RADIUS, MAX_CAP = COUNTR_PEAKS_MAX_POINTS;
constexpr int TILE_H = 32, TILE_W = 64;          // TILE_W = the wave: a tile row's ballot is its mask
constexpr int PARTS = 32;                        // block maxima per map (one half-wave folds them)
constexpr int WRITE_BLOCKS = 32;                 // blocks per map of the scan + write launch
constexpr int LIST = 2048;                       // peaks a write block lists in LDS per pass
constexpr int RANK_CHUNK = 1024;                 // scores a rank block stages per pass
constexpr int REC = 6;

struct PeakArgs {
  const float* map[MAX_MAPS];
  int h[MAX_MAPS], w[MAX_MAPS];
  int tile_off[MAX_MAPS + 1];                    // first tile of map i in the detect grid
  int seg_off[MAX_MAPS];                         // first row segment (mask) of map i
  int vec[MAX_MAPS];                             // base 16-byte aligned
};

__device__ __forceinline__ float neg_inf() { return -__builtin_inff(); }

__global__ __launch_bounds__(256) void peaks_max_kernel(const PeakArgs a, float* __restrict__ parts) {
  __shared__ float sm[4];
  const int i = blockIdx.y, b = blockIdx.x;
  const float* __restrict__ m = a.map[i];
  const int64_t total = (int64_t)a.h[i] * a.w[i];
  float best = neg_inf();
  if (a.vec[i]) {
    const int64_t n4 = total >> 2;
    for (int64_t q = (int64_t)b * 256 + threadIdx.x; q < n4; q += (int64_t)PARTS * 256) {
      const float4 v = reinterpret_cast<const float4*>(m)[q];
      best = fmaxf(best, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
    }
    if (b == 0 && (int64_t)threadIdx.x < (total & 3)) best = fmaxf(best, m[(n4 << 2) + threadIdx.x]);
  } else {
    for (int64_t q = (int64_t)b * 256 + threadIdx.x; q < total; q += (int64_t)PARTS * 256) best = fmaxf(best, m[q]);
  }
  best = wave_max(best);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) parts[i * PARTS + b] = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
}

__global__ __launch_bounds__(256) void peaks_detect_kernel(const PeakArgs a, const float* __restrict__ parts, unsigned long long* __restrict__ masks,
                                                           int n, int r, float threshold, float rel_threshold) {
  __shared__ float tile[(TILE_H + 2 * MAX_R) * (TILE_W + 2 * MAX_R)];
  int i = 0;
  while (i + 1 < n && (int)blockIdx.x >= a.tile_off[i + 1]) ++i;
  const int h = a.h[i], w = a.w[i];
  const int tiles_x = (w + TILE_W - 1) / TILE_W;
  const int t = blockIdx.x - a.tile_off[i];
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  const int y0 = ty * TILE_H, x0 = tx * TILE_W;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* __restrict__ m = a.map[i];
  const float top = wave_max(lane < PARTS ? parts[i * PARTS + lane] : neg_inf());
  const float rel = rel_threshold * top;                  // one fp32 multiply
  const int lw = TILE_W + 2 * r, lh = TILE_H + 2 * r;
  for (int ly = wave; ly < lh; ly += 4) {
    const int gy = y0 - r + ly;
    for (int lx = lane; lx < lw; lx += 64) {
      const int gx = x0 - r + lx;
      // outside the map: -inf, below every candidate (a candidate is > threshold >= 0), so the window is the clipped one
      tile[ly * lw + lx] = (gy >= 0 && gy < h && gx >= 0 && gx < w) ? m[(int64_t)gy * w + gx] : neg_inf();
    }
  }
  __syncthreads();
  for (int k = 0; k < TILE_H / 4; ++k) {
    const int rr = wave * (TILE_H / 4) + k;
    const int y = y0 + rr, x = x0 + lane;
    if (y >= h) break;                                    // (wave-uniform)
    const float* c = tile + (rr + r) * lw + lane + r;
    const float v = *c;
    bool ok = x < w && v > threshold && v >= rel;
    if (ok) {
      for (int dy = -r; dy <= r && ok; ++dy) {
        const float* row = c + dy * lw;
        for (int dx = -r; dx <= r; ++dx) {
          const float q = row[dx];
          // q in front of p in raster order must be strictly lower; q behind p may be equal
          const bool behind = dy > 0 || (dy == 0 && dx > 0);
          const bool self = dy == 0 && dx == 0;
          if (!(self || v > q || (behind && v == q))) { ok = false; break; }
        }
      }
    }
    const unsigned long long mask = __ballot(ok);
    if (lane == 0) masks[a.seg_off[i] + (int64_t)y * tiles_x + tx] = mask;
  }
}

__global__ __launch_bounds__(256) void peaks_write_kernel(const PeakArgs a, const unsigned long long* __restrict__ masks, int* __restrict__ totals,
                                                          float* __restrict__ raw, int r, int cap) {
  __shared__ int sm[4];                                  // the scans' wave totals
  __shared__ int list[LIST];
  const int i = blockIdx.y, b = blockIdx.x;
  const int h = a.h[i], w = a.w[i];
  const int tiles_x = (w + TILE_W - 1) / TILE_W;
  const int segs = h * tiles_x;
  const int rows = (h + WRITE_BLOCKS - 1) / WRITE_BLOCKS;
  const int s0 = (int)min((int64_t)b * rows * tiles_x, (int64_t)segs), s1 = (int)min((int64_t)(b + 1) * rows * tiles_x, (int64_t)segs);
  const unsigned long long* __restrict__ mk = masks + a.seg_off[i];
  const float* __restrict__ m = a.map[i];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int before = 0;
  for (int s = threadIdx.x; s < s0; s += 256) before += __popcll(mk[s]);
  int base;
  block_scan_i<4>(before, sm, base);                     // peaks in front of this block's rows
  for (int c0 = s0; c0 < s1; c0 += 256) {
    const int s = c0 + threadIdx.x;
    const unsigned long long mask = s < s1 ? mk[s] : 0ull;
    int chunk;
    const int first = block_scan_i<4>(__popcll(mask), sm, chunk);
    const int sy = s / tiles_x, sx = (s - sy * tiles_x) * TILE_W;
    for (int p0 = 0; p0 < chunk && base + p0 < cap; p0 += LIST) {
      unsigned long long bits = mask;
      for (int j = first; bits; ++j) {
        const int bit = __ffsll((long long)bits) - 1;
        bits &= bits - 1;
        if (j >= p0 && j < p0 + LIST) list[j - p0] = sy * w + sx + bit;
      }
      __syncthreads();
      const int cnt = min(LIST, chunk - p0);
      for (int k = wave; k < cnt; k += 4) {              // a wave per peak: the lanes share the window
        const int rank = base + p0 + k;
        if (rank >= cap) break;
        const int idx = list[k];
        const int y = idx / w, x = idx - y * w;
        const int ya = max(y - r, 0), yb = min(y + r, h - 1), xa = max(x - r, 0), xb = min(x + r, w - 1);
        const int ww = xb - xa + 1, cells = (yb - ya + 1) * ww;
        float sw = 0.f, swy = 0.f, swx = 0.f;
        for (int q0 = 0; q0 < cells; q0 += 64) {
          const int q = q0 + lane;
          if (q < cells) {
            const int qy = ya + q / ww, qx = xa + q % ww;
            const float d = m[(int64_t)qy * w + qx];
            const float wt = d > 0.f ? d : 0.f;
            sw += wt; swy += wt * (float)(qy - y); swx += wt * (float)(qx - x);
          }
        }
        sw = wave_sum(sw); swy = wave_sum(swy); swx = wave_sum(swx);
        if (lane == 0) {
          float* o = raw + ((int64_t)i * cap + rank) * REC;
          o[0] = (float)y; o[1] = (float)x; o[2] = m[idx];
          o[3] = (float)y + swy / sw; o[4] = (float)x + swx / sw; o[5] = sw / 60.f;
        }
      }
      __syncthreads();
    }
    base += chunk;
  }
  if (b == WRITE_BLOCKS - 1 && threadIdx.x == 0) totals[i] = base;      // (its rows are the map's last: base = every peak)
}

__global__ __launch_bounds__(256) void peaks_rank_kernel(const int* __restrict__ totals, const float* __restrict__ raw, float* __restrict__ recs, int cap) {
  __shared__ float score[RANK_CHUNK];
  const int i = blockIdx.y;
  const int kept = min(totals[i], cap);
  if ((int)blockIdx.x * 256 >= kept) return;             // (block-uniform)
  const float* __restrict__ src = raw + (int64_t)i * cap * REC;
  const int k = blockIdx.x * 256 + threadIdx.x;
  const float mine = k < kept ? src[(int64_t)k * REC + 2] : 0.f;
  int place = 0;
  for (int j0 = 0; j0 < kept; j0 += RANK_CHUNK) {
    const int cnt = min(RANK_CHUNK, kept - j0);
    __syncthreads();
    for (int j = threadIdx.x; j < cnt; j += 256) score[j] = src[(int64_t)(j0 + j) * REC + 2];
    __syncthreads();
    for (int j = 0; j < cnt; ++j) {
      const float s = score[j];
      place += (s > mine || (s == mine && j0 + j < k)) ? 1 : 0;
    }
  }
  if (k < kept) {
    float* o = recs + ((int64_t)i * cap + place) * REC;
#pragma unroll
    for (int e = 0; e < REC; ++e) o[e] = src[(int64_t)k * REC + e];
  }
}

// the scratch of a call whose maps have these sizes: masks (8 bytes per row segment), the raster-order records, the block maxima
bool layout(int64_t segs, int n, int cap, int64_t* raw_off, int64_t* parts_off, int64_t* bytes) {
  *raw_off = segs * 8;
  *parts_off = *raw_off + (int64_t)n * cap * REC * 4;
  *bytes = *parts_off + (int64_t)n * PARTS * 4;
  return *bytes <= INT_MAX;
}

}  // namespace

extern "C" int countr_peaks_workspace(int n, int max_h, int max_w, int cap) {
  if (n < 1 || n > MAX_MAPS || max_h < 1 || max_w < 1 || cap < 1 || cap > MAX_CAP || (int64_t)max_h * max_w > (int64_t)1 << 28) {
    countr_set_error("countr_peaks_workspace: bad args (1..16 maps of at most 2^28 pixels, cap 1..8192)"); return -1;
  }
  int64_t raw_off, parts_off, bytes;
  if (!layout((int64_t)n * max_h * ((max_w + TILE_W - 1) / TILE_W), n, cap, &raw_off, &parts_off, &bytes)) {
    countr_set_error("countr_peaks_workspace: the workspace of these sizes exceeds 2 GB"); return -2;
  }
  return (int)bytes;
}

extern "C" int countr_density_peaks(const countr_peak_map* maps, int n, int radius, float threshold, float rel_threshold, int cap,
                                    int* totals, float* recs, void* workspace, void* stream) {
  if (!maps || !totals || !recs || !workspace || n < 1 || n > MAX_MAPS || (((uintptr_t)workspace) & 7)) {
    countr_set_error("countr_density_peaks: bad args (1..16 maps, totals, recs and an 8-byte aligned workspace are required)"); return -1;
  }
  if (radius < 1 || radius > MAX_R || cap < 1 || cap > MAX_CAP || !(threshold >= 0.f) || !(rel_threshold >= 0.f && rel_threshold <= 1.f)) {
    countr_set_error("countr_density_peaks: radius is 1..8, cap 1..8192, threshold >= 0 and 0 <= rel_threshold <= 1"); return -1;
  }
  PeakArgs a;
  int64_t tiles = 0, segs = 0;
  for (int j = 0; j < MAX_MAPS; ++j) {
    const countr_peak_map& d = maps[j < n ? j : n - 1];
    if (!d.map || d.h < 1 || d.w < 1 || (int64_t)d.h * d.w > (int64_t)1 << 28 || (((uintptr_t)d.map) & 3)) {
      countr_set_error("countr_density_peaks: null or misaligned map, or a map size outside 1 .. 2^28 pixels"); return -1;
    }
    a.map[j] = d.map; a.h[j] = d.h; a.w[j] = d.w;
    a.vec[j] = (((uintptr_t)d.map) & 15) == 0;
    if (j < n) {
      const int tiles_x = (d.w + TILE_W - 1) / TILE_W;
      a.tile_off[j] = (int)tiles; a.seg_off[j] = (int)segs;
      tiles += (int64_t)tiles_x * ((d.h + TILE_H - 1) / TILE_H);
      segs += (int64_t)tiles_x * d.h;
      if (tiles > INT_MAX || segs > INT_MAX) { countr_set_error("countr_density_peaks: the maps of one call exceed 2^31 tiles"); return -1; }
    } else {
      a.tile_off[j] = (int)tiles; a.seg_off[j] = 0;
    }
  }
  a.tile_off[MAX_MAPS] = (int)tiles;
  int64_t raw_off, parts_off, bytes;
  if (!layout(segs, n, cap, &raw_off, &parts_off, &bytes)) { countr_set_error("countr_density_peaks: the workspace of these maps exceeds 2 GB"); return -2; }
  unsigned long long* masks = (unsigned long long*)workspace;
  float* raw = (float*)((char*)workspace + raw_off);
  float* parts = (float*)((char*)workspace + parts_off);
  hipLaunchKernelGGL(peaks_max_kernel, dim3(PARTS, n), dim3(256), 0, STREAM(stream), a, parts);
  hipLaunchKernelGGL(peaks_detect_kernel, dim3((unsigned)tiles), dim3(256), 0, STREAM(stream), a, parts, masks, n, radius, threshold, rel_threshold);
  hipLaunchKernelGGL(peaks_write_kernel, dim3(WRITE_BLOCKS, n), dim3(256), 0, STREAM(stream), a, masks, totals, raw, radius, cap);
  hipLaunchKernelGGL(peaks_rank_kernel, dim3((cap + 255) / 256, n), dim3(256), 0, STREAM(stream), totals, raw, recs, cap);
  return countr_check_launch("countr_density_peaks");
}
