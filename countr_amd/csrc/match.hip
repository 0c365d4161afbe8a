// One-to-one matching of predicted points to annotated dots: the greedy matching in ascending (d2, i, j) order (include/countr_hip.h
// states the rule), computed exactly as rounds of locally dominant pairs.  Two launches, whatever the sets hold.
//   countr_match_workspace  (host only) bytes of scratch a call needs
//   countr_match_points     n sets of pred fp32 [P, 2] / gt fp32 [G, 2] -> match[i] (gt index or -1), match_d2[i] (or +inf), counts[s]
// The launches:
//   1 match_init_kernel    every CU: a wave per point (pred or gt) scans the other side, lane = candidate, and keeps the point's smallest
//                          key -- best gt (d2, j) of a pred, best pred (d2, i) of a gt -- as a 16-bit index in the workspace; the preds'
//                          slices of match / match_d2 get -1 / +inf
//   2 match_rounds_kernel  a block per set, the bests and two "still free" bit masks in LDS.  A round: (A) pred i and gt j are matched
//                          when each is the other's best -- the pair is then the smallest remaining key of both, which is the greedy
//                          matching's own choice; (B) only a free point whose best has just been taken scans again, over the free points
//                          of the other side (a wave per such point).  A best stays valid while its target is free, because the free
//                          sets only shrink.  The loop ends with the first round that matches nothing: while an eligible free pair is
//                          left, the smallest one is locally dominant, so no round count is assumed (a ladder takes one round per pair).
// Determinism: a point's best is a minimum over a set (fixed DPP butterflies over the lanes), the masks change by atomic AND and the
// count by an integer atomic add in LDS -- none of them depends on an order, and two runs give the same bytes.
// d2 is written with __fsub_rn / __fmul_rn / __fadd_rn: no contraction can fuse it.  fl(a - b) = -fl(b - a), so the pred's and the
// gt's scan compute the same bits for a pair.  fp32 only: the bf16 and the fp16 build of the library export the same code.
#include <math.h>
#include "common.hpp"
#include "../../include/countr_hip.h"

namespace {

constexpr int MAX_SETS = COUNTR_MATCH_MAX_SETS, MAX_PTS = COUNTR_MATCH_MAX_POINTS;
constexpr int NONE = 0xFFFF;                     // "no eligible free partner" (an index is < 8192)
constexpr int INIT_BLOCKS = 128;                 // blocks per set of the first launch (4 waves each)
constexpr int ROUND_THREADS = 1024, ROUND_WAVES = ROUND_THREADS / 64;

struct MatchArgs {
  const float2* pred[MAX_SETS];
  const float2* gt[MAX_SETS];
  int P[MAX_SETS], G[MAX_SETS], off[MAX_SETS];
  int ws_p[MAX_SETS], ws_g[MAX_SETS];            // the set's best-of-pred / best-of-gt arrays in the workspace, in 16-bit units
  float md2[MAX_SETS];                           // fl(max_dist * max_dist)
};

__device__ __forceinline__ float pair_d2(const float2 p, const float2 g) {
  const float dx = __fsub_rn(p.x, g.x), dy = __fsub_rn(p.y, g.y);
  return __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy));
}

__device__ __forceinline__ unsigned mask_word(const unsigned* m, int w) {      // (other threads may clear bits of the word meanwhile)
  return __hip_atomic_load(m + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ bool mask_bit(const unsigned* m, int k) { return (mask_word(m, k >> 5) >> (k & 31)) & 1u; }
__device__ __forceinline__ void mask_clear(unsigned* m, int k) { atomicAnd(m + (k >> 5), ~(1u << (k & 31))); }

// The index of q's smallest key (d2, index) among the eligible (and, MASKED, still free) points of `others`, or NONE.  The whole wave
// calls it with the same arguments; every lane gets the result.  A lane walks its candidates in ascending index order and replaces its
// best only by a strictly smaller d2, so it holds the smallest index of its smallest d2; two butterflies then take the smallest d2 of
// the wave and the smallest index that has it (an index is exact as a float).  A NaN d2 fails `<= md2`: such a pair is never eligible.
template <bool MASKED>
__device__ __forceinline__ int wave_best(const float2 q, const float2* __restrict__ others, int n, const unsigned* free, float md2, int lane) {
  float best = 0.f;
  int at = NONE;
  for (int k0 = 0; k0 < n; k0 += 64) {
    if (MASKED && (mask_word(free, k0 >> 5) | mask_word(free, (k0 >> 5) + 1)) == 0u) continue;      // (wave-uniform: k0 is)
    const int k = k0 + lane;
    if (k < n && (!MASKED || mask_bit(free, k))) {
      const float d = pair_d2(q, others[k]);
      if (d <= md2 && (at == NONE || d < best)) { best = d; at = k; }
    }
  }
  const float ninf = -__builtin_inff();
  const float low = -wave_max(at != NONE ? -best : ninf);
  const float idx = wave_max((at != NONE && best == low) ? -(float)at : ninf);
  return idx == ninf ? NONE : (int)(-idx);
}

__global__ __launch_bounds__(256) void match_init_kernel(const MatchArgs a, unsigned short* __restrict__ ws, int* __restrict__ match,
                                                         float* __restrict__ match_d2) {
  const int s = blockIdx.y;
  const int P = a.P[s], G = a.G[s];
  const int lane = threadIdx.x & 63;
  const float2* __restrict__ pred = a.pred[s];
  const float2* __restrict__ gt = a.gt[s];
  for (int q = blockIdx.x * 4 + (threadIdx.x >> 6); q < P + G; q += INIT_BLOCKS * 4) {      // (wave-uniform)
    if (q < P) {
      const int j = wave_best<false>(pred[q], gt, G, nullptr, a.md2[s], lane);
      if (lane == 0) {
        ws[a.ws_p[s] + q] = (unsigned short)j;
        match[a.off[s] + q] = -1;
        match_d2[a.off[s] + q] = __builtin_inff();
      }
    } else {
      const int i = wave_best<false>(gt[q - P], pred, P, nullptr, a.md2[s], lane);
      if (lane == 0) ws[a.ws_g[s] + q - P] = (unsigned short)i;
    }
  }
}

__global__ __launch_bounds__(ROUND_THREADS) void match_rounds_kernel(const MatchArgs a, const unsigned short* __restrict__ ws,
                                                                     int* __restrict__ match, float* __restrict__ match_d2,
                                                                     int* __restrict__ counts) {
  __shared__ unsigned short best_p[MAX_PTS], best_g[MAX_PTS];      // pred -> its best free gt, gt -> its best free pred (or NONE)
  __shared__ unsigned free_p[MAX_PTS / 32 + 2], free_g[MAX_PTS / 32 + 2];      // (+2: wave_best reads the two words of a 64-chunk)
  __shared__ int matched;
  const int s = blockIdx.x, t = threadIdx.x;
  const int P = a.P[s], G = a.G[s];
  const int lane = t & 63, wave = t >> 6;
  const float md2 = a.md2[s];
  const float2* __restrict__ pred = a.pred[s];
  const float2* __restrict__ gt = a.gt[s];
  for (int i = t; i < P; i += ROUND_THREADS) best_p[i] = ws[a.ws_p[s] + i];
  for (int j = t; j < G; j += ROUND_THREADS) best_g[j] = ws[a.ws_g[s] + j];
  if (t == 0) matched = 0;
  __syncthreads();
  // free = has an eligible partner at all: a point without one never gets one, and nobody's best points at it
  for (int w = t; w < MAX_PTS / 32 + 2; w += ROUND_THREADS) {
    unsigned mp = 0u, mg = 0u;
    for (int b = 0; b < 32; ++b) {
      const int k = w * 32 + b;
      if (k < P && best_p[k] != NONE) mp |= 1u << b;
      if (k < G && best_g[k] != NONE) mg |= 1u << b;
    }
    free_p[w] = mp; free_g[w] = mg;
  }
  __syncthreads();
  int mine = 0;
  for (;;) {
    // (A) mutual bests.  Only the thread of pred i clears bit i and reads it; best_p / best_g do not change in this phase.
    int hit = 0;
    for (int i = t; i < P; i += ROUND_THREADS) {
      if (!mask_bit(free_p, i)) continue;
      const int j = best_p[i];
      if (j == NONE || best_g[j] != i) continue;
      match[a.off[s] + i] = j;
      match_d2[a.off[s] + i] = pair_d2(pred[i], gt[j]);
      mask_clear(free_p, i);
      mask_clear(free_g, j);
      hit = 1; ++mine;
    }
    if (!__syncthreads_or(hit)) break;             // every round that goes on has cleared a bit of free_p: at most P + 1 rounds
    // (B) a free point whose best was taken scans the free points of the other side again; one that finds none leaves for good.  A
    // point that leaves during this phase is eligible for no free point, so whether a concurrent scan still sees its bit changes nothing.
    for (int base = wave * 64; base < P; base += ROUND_WAVES * 64) {
      const int i = base + lane;
      bool stale = false;
      if (i < P && mask_bit(free_p, i)) { const int j = best_p[i]; stale = j != NONE && !mask_bit(free_g, j); }
      for (unsigned long long m = __ballot(stale); m; m &= m - 1) {
        const int q = base + __ffsll((long long)m) - 1;
        const int j = wave_best<true>(pred[q], gt, G, free_g, md2, lane);
        if (lane == 0) { best_p[q] = (unsigned short)j; if (j == NONE) mask_clear(free_p, q); }
      }
    }
    for (int base = wave * 64; base < G; base += ROUND_WAVES * 64) {
      const int j = base + lane;
      bool stale = false;
      if (j < G && mask_bit(free_g, j)) { const int i = best_g[j]; stale = i != NONE && !mask_bit(free_p, i); }
      for (unsigned long long m = __ballot(stale); m; m &= m - 1) {
        const int q = base + __ffsll((long long)m) - 1;
        const int i = wave_best<true>(gt[q], pred, P, free_p, md2, lane);
        if (lane == 0) { best_g[q] = (unsigned short)i; if (i == NONE) mask_clear(free_g, q); }
      }
    }
    __syncthreads();
  }
  if (mine) atomicAdd(&matched, mine);
  __syncthreads();
  if (t == 0) counts[s] = matched;
}

inline int round8(int v) { return (v + 7) & ~7; }

}  // namespace

extern "C" int countr_match_workspace(int n, int max_p, int max_g) {
  if (n < 1 || n > MAX_SETS || max_p < 0 || max_p > MAX_PTS || max_g < 0 || max_g > MAX_PTS) {
    countr_set_error("countr_match_workspace: bad args (1..16 sets of 0..8192 points a side)"); return -1;
  }
  const int bytes = n * (round8(max_p) + round8(max_g)) * 2;
  return bytes > 16 ? bytes : 16;
}

extern "C" int countr_match_points(const countr_match_set* sets, int n, int* match, float* match_d2, int* counts, void* workspace,
                                   void* stream) {
  if (!sets || !match || !match_d2 || !counts || !workspace || n < 1 || n > MAX_SETS || (((uintptr_t)workspace) & 15)) {
    countr_set_error("countr_match_points: bad args (1..16 sets, match, match_d2, counts and a 16-byte aligned workspace are required)");
    return -1;
  }
  MatchArgs a;
  int ws = 0;
  for (int k = 0; k < MAX_SETS; ++k) {
    if (k >= n) {
      a.pred[k] = a.gt[k] = nullptr; a.P[k] = a.G[k] = a.off[k] = a.ws_p[k] = a.ws_g[k] = 0; a.md2[k] = 0.f;
      continue;
    }
    const countr_match_set& d = sets[k];
    if (d.P < 0 || d.P > MAX_PTS || d.G < 0 || d.G > MAX_PTS || d.offset < 0) {
      countr_set_error("countr_match_points: a set holds 0..8192 points a side and its offset is >= 0"); return -1;
    }
    if (!(d.max_dist > 0.f) || !__builtin_isfinite(d.max_dist)) { countr_set_error("countr_match_points: max_dist is finite and > 0"); return -1; }
    if ((d.P > 0 && !d.pred) || (d.G > 0 && !d.gt) || (((uintptr_t)d.pred) & 7) || (((uintptr_t)d.gt) & 7)) {
      countr_set_error("countr_match_points: null or misaligned points (fp32 (x, y) pairs, 8-byte aligned)"); return -1;
    }
    a.pred[k] = reinterpret_cast<const float2*>(d.pred); a.gt[k] = reinterpret_cast<const float2*>(d.gt);
    a.P[k] = d.P; a.G[k] = d.G; a.off[k] = d.offset;
    a.md2[k] = d.max_dist * d.max_dist;          // one fp32 multiply (the host compiler contracts nothing here: no addition follows)
    a.ws_p[k] = ws; ws += round8(d.P);
    a.ws_g[k] = ws; ws += round8(d.G);
  }
  unsigned short* best = (unsigned short*)workspace;
  hipLaunchKernelGGL(match_init_kernel, dim3(INIT_BLOCKS, n), dim3(256), 0, STREAM(stream), a, best, match, match_d2);
  hipLaunchKernelGGL(match_rounds_kernel, dim3(n), dim3(ROUND_THREADS), 0, STREAM(stream), a, best, match, match_d2, counts);
  COUNTR_LAUNCH_CHECK("countr_match_points");
}
