// One-to-one matching of predicted points to annotated dots: the greedy matching in ascending (d2, i, j) order (include/countr_hip.h
// states the rule), computed exactly as rounds of locally dominant pairs.  Two launches, whatever the sets hold.
//   countr_match_workspace  (host only) bytes of scratch a call needs
//   countr_match_points     n sets of pred fp32 [P, 2] / gt fp32 [G, 2] -> match[i] (gt index or -1), match_d2[i] (or +inf), counts[s]
// The launches:
//   1 match_init_kernel    every CU: a wave per point (pred or gt) scans the other side, lane = candidate, and keeps the point's smallest
//                          key -- best gt (d2, j) of a pred, best pred (d2, i) of a gt -- as a 16-bit index in the workspace; the preds'
//                          slices of match / match_d2 get -1 / +inf
//   2 match_rounds_kernel  a block per set, the bests and two "still free" bit masks in LDS: the rounds of greedy_match.hpp (mutual bests
//                          are matched; only a free point whose best has just been taken scans again) until a round matches nothing.
// Determinism: greedy_match.hpp's, and the count is an integer atomic add in LDS: two runs give the same bytes.
// fp32 only: the bf16 and the fp16 build of the library export the same code.
#include <math.h>
#include "common.hpp"
#include "greedy_match.hpp"
#include "../../include/countr_hip.h"

namespace {

using namespace countr_greedy;
constexpr int MAX_SETS = COUNTR_MATCH_MAX_SETS, MAX_PTS = COUNTR_MATCH_MAX_POINTS;
constexpr int INIT_BLOCKS = 128;                 // blocks per set of the first launch (4 waves each)
constexpr int ROUND_THREADS = 1024;

struct MatchArgs {
  const float2* pred[MAX_SETS];
  const float2* gt[MAX_SETS];
  int P[MAX_SETS], G[MAX_SETS], off[MAX_SETS];
  int ws_p[MAX_SETS], ws_g[MAX_SETS];            // the set's best-of-pred / best-of-gt arrays in the workspace, in 16-bit units
  float md2[MAX_SETS];                           // fl(max_dist * max_dist)
};

__global__ __launch_bounds__(256) void match_init_kernel(const MatchArgs a, unsigned short* __restrict__ ws, int* __restrict__ match,
                                                         float* __restrict__ match_d2) {
  const int s = blockIdx.y;
  const int P = a.P[s], G = a.G[s];
  const int lane = threadIdx.x & 63;
  const float2* __restrict__ pred = a.pred[s];
  const float2* __restrict__ gt = a.gt[s];
  for (int q = blockIdx.x * 4 + (threadIdx.x >> 6); q < P + G; q += INIT_BLOCKS * 4) {      // (wave-uniform)
    if (q < P) {
      const int j = wave_best<false>(pred[q], FromArray{gt}, G, nullptr, a.md2[s], lane);
      if (lane == 0) {
        ws[a.ws_p[s] + q] = (unsigned short)j;
        match[a.off[s] + q] = -1;
        match_d2[a.off[s] + q] = __builtin_inff();
      }
    } else {
      const int i = wave_best<false>(gt[q - P], FromArray{pred}, P, nullptr, a.md2[s], lane);
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
  const float md2 = a.md2[s];
  const float2* __restrict__ pred = a.pred[s];
  const float2* __restrict__ gt = a.gt[s];
  for (int i = t; i < P; i += ROUND_THREADS) best_p[i] = ws[a.ws_p[s] + i];
  for (int j = t; j < G; j += ROUND_THREADS) best_g[j] = ws[a.ws_g[s] + j];
  if (t == 0) matched = 0;
  __syncthreads();
  greedy_free_masks<ROUND_THREADS>(best_p, P, best_g, G, free_p, free_g, MAX_PTS / 32 + 2);
  const int mine = greedy_rounds<ROUND_THREADS>(FromArray{pred}, P, FromArray{gt}, G, best_p, best_g, free_p, free_g, md2, [&](int i, int j) {
    match[a.off[s] + i] = j;                       // (a.off[s] is read at the store, as the loop always did)
    match_d2[a.off[s] + i] = pair_d2(pred[i], gt[j]);
  });
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
  return countr_check_launch("countr_match_points");
}
