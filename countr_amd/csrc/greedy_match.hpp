// The greedy one-to-one matching of two point sets in ascending (d2, i, j) order, computed exactly as rounds of locally dominant pairs:
// the device code that csrc/match.hip (predicted points against dots) and csrc_tracks/tracks.hip (detections against the tracks'
// predictions) share.  A caller's first launch takes every point's best partner with wave_best; its second launch keeps the bests and
// two "still free" bit masks in LDS (the arrays are the kernel's own: their sizes are part of its budget), builds the masks with
// greedy_free_masks and runs greedy_rounds.
// Determinism: a point's best is a minimum over a set (fixed DPP butterflies over the lanes) and the masks change by atomic AND -- neither
// depends on an order, and two runs give the same bytes.
#pragma once
#include "common.hpp"

namespace countr_greedy {

constexpr int NONE = 0xFFFF;                     // "no eligible free partner" (an index is < 8192)

// d2 is written with __fsub_rn / __fmul_rn / __fadd_rn: no contraction can fuse it.  fl(a - b) = -fl(b - a) and the square of a negated
// difference is the same fp32 value, so the scans of the two sides -- pair_d2(a, b) from a's, pair_d2(b, a) from b's -- compute the same
// bits for a pair.
__device__ __forceinline__ float pair_d2(const float2 p, const float2 g) {
  const float dx = __fsub_rn(p.x, g.x), dy = __fsub_rn(p.y, g.y);
  return __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy));
}

__device__ __forceinline__ unsigned mask_word(const unsigned* m, int w) {      // (other threads may clear bits of the word meanwhile)
  return __hip_atomic_load(m + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ bool mask_bit(const unsigned* m, int k) { return (mask_word(m, k >> 5) >> (k & 31)) & 1u; }
__device__ __forceinline__ void mask_clear(unsigned* m, int k) { atomicAnd(m + (k >> 5), ~(1u << (k & 31))); }

// A candidate source is anything with `float2 at(int k) const`: the k-th point of a side.
struct FromArray {                               // points read from an array
  const float2* p;
  __device__ __forceinline__ float2 at(int k) const { return p[k]; }
};

// The index of q's smallest key (d2, index) among the eligible (and, MASKED, still free) points of `others`, or NONE.  The whole wave
// calls it with the same arguments; every lane gets the result.  A lane walks its candidates in ascending index order and replaces its
// best only by a strictly smaller d2, so it holds the smallest index of its smallest d2; two butterflies then take the smallest d2 of
// the wave and the smallest index that has it (an index is exact as a float).  A NaN d2 fails `<= md2`: such a pair is never eligible.
// MASKED reads the two words of a 64-candidate chunk: `free` holds two words past the last candidate's.
template <bool MASKED, class Src>
__device__ __forceinline__ int wave_best(const float2 q, const Src others, int n, const unsigned* free, float md2, int lane) {
  float best = 0.f;
  int at = NONE;
  for (int k0 = 0; k0 < n; k0 += 64) {
    if (MASKED && (mask_word(free, k0 >> 5) | mask_word(free, (k0 >> 5) + 1)) == 0u) continue;      // (wave-uniform: k0 is)
    const int k = k0 + lane;
    if (k < n && (!MASKED || mask_bit(free, k))) {
      const float d = pair_d2(q, others.at(k));
      if (d <= md2 && (at == NONE || d < best)) { best = d; at = k; }
    }
  }
  const float ninf = -__builtin_inff();
  const float low = -wave_max(at != NONE ? -best : ninf);
  const float idx = wave_max((at != NONE && best == low) ? -(float)at : ninf);
  return idx == ninf ? NONE : (int)(-idx);
}

// free_a / free_b from the first launch's bests (LDS, complete before the call): free = has an eligible partner at all -- a point without
// one never gets one, and nobody's best points at it.  All `words` words of both masks are written, the slack of wave_best included.
// Every thread of the block calls it; it ends with a barrier.
template <int THREADS>
__device__ __forceinline__ void greedy_free_masks(const unsigned short* best_a, int nA, const unsigned short* best_b, int nB,
                                                  unsigned* free_a, unsigned* free_b, int words) {
  for (int w = threadIdx.x; w < words; w += THREADS) {
    unsigned ma = 0u, mb = 0u;
    for (int b = 0; b < 32; ++b) {
      const int k = w * 32 + b;
      if (k < nA && best_a[k] != NONE) ma |= 1u << b;
      if (k < nB && best_b[k] != NONE) mb |= 1u << b;
    }
    free_a[w] = ma; free_b[w] = mb;
  }
  __syncthreads();
}

// The rounds, by the block's THREADS threads (every one calls it, after greedy_free_masks): best_a[i] is the best free point of side b
// for point i of side a, or NONE, and best_b the reverse.  A round: (A) i and j are matched when each is the other's best -- the pair
// is then the smallest remaining key of both, which is the greedy matching's own choice -- and on_match(i, j) is called by the thread of
// i; (B) only a free point whose best has just been taken scans again, over the free points of the other side (a wave per such point).
// A best stays valid while its target is free, because the free sets only shrink.  The loop ends with the first round that matches
// nothing: while an eligible free pair is left, the smallest one is locally dominant, so no round count is assumed (a ladder takes one
// round per pair).  Returns the number of pairs this thread matched.
template <int THREADS, class SrcA, class SrcB, class OnMatch>
__device__ __forceinline__ int greedy_rounds(const SrcA a, int nA, const SrcB b, int nB, unsigned short* best_a, unsigned short* best_b,
                                             unsigned* free_a, unsigned* free_b, float md2, OnMatch on_match) {
  constexpr int WAVES = THREADS / 64;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  int mine = 0;
  for (;;) {
    // (A) mutual bests.  Only the thread of i clears bit i of free_a and reads it; best_a / best_b do not change in this phase.
    int hit = 0;
    for (int i = t; i < nA; i += THREADS) {
      if (!mask_bit(free_a, i)) continue;
      const int j = best_a[i];
      if (j == NONE || best_b[j] != i) continue;
      on_match(i, j);
      mask_clear(free_a, i);
      mask_clear(free_b, j);
      hit = 1; ++mine;
    }
    if (!__syncthreads_or(hit)) break;             // every round that goes on has cleared a bit of free_a: at most nA + 1 rounds
    // (B) a free point whose best was taken scans the free points of the other side again; one that finds none leaves for good.  A
    // point that leaves during this phase is eligible for no free point, so whether a concurrent scan still sees its bit changes nothing.
    for (int base = wave * 64; base < nA; base += WAVES * 64) {
      const int i = base + lane;
      bool stale = false;
      if (i < nA && mask_bit(free_a, i)) { const int j = best_a[i]; stale = j != NONE && !mask_bit(free_b, j); }
      for (unsigned long long m = __ballot(stale); m; m &= m - 1) {
        const int q = base + __ffsll((long long)m) - 1;
        const int j = wave_best<true>(a.at(q), b, nB, free_b, md2, lane);
        if (lane == 0) { best_a[q] = (unsigned short)j; if (j == NONE) mask_clear(free_a, q); }
      }
    }
    for (int base = wave * 64; base < nB; base += WAVES * 64) {
      const int j = base + lane;
      bool stale = false;
      if (j < nB && mask_bit(free_b, j)) { const int i = best_b[j]; stale = i != NONE && !mask_bit(free_a, i); }
      for (unsigned long long m = __ballot(stale); m; m &= m - 1) {
        const int q = base + __ffsll((long long)m) - 1;
        const int i = wave_best<true>(b.at(q), a, nA, free_a, md2, lane);
        if (lane == 0) { best_b[q] = (unsigned short)i; if (i == NONE) mask_clear(free_b, q); }
      }
    }
    __syncthreads();
  }
  return mine;
}

}  // namespace countr_greedy
