// The frames' points joined over time (include/countr_hip_tracks.h states the rule).
//   countr_tracks_state_bytes / countr_tracks_workspace   (host only) sizes
//   countr_tracks_reset     n states -> empty trackers (one memset node each)
//   countr_tracks_step      n <= 16 trackers advance by one step each
// A step is two launches on the caller's stream, whatever the trackers hold.  The number of live tracks T is read from the state on the
// device: no grid size depends on it.
//   1 tracks_init_kernel    every CU, a grid plane per tracker: a wave per point -- detection or track -- scans the other side, lane =
//                           candidate, and keeps the point's smallest key (d2, index) as a 16-bit index in the workspace.  A track's
//                           wave also writes its prediction p = (fl(x + vx), fl(y + vy)) to the workspace; a detection's wave forms the
//                           predictions it scans from the state (the same two additions, so the same bits).
//   2 tracks_step_kernel    a block of 1024 threads per tracker.
//       the rounds          the rounds of csrc/greedy_match.hpp -- the code csrc/match.hip runs -- with side a = the detections and side b =
//                           the predictions: bests and the two "still free" masks in LDS; the loop ends with the first round that matches
//                           nothing, so no round count is assumed.  The matching stays in LDS (det -> track, track -> det).
//       the update          a thread holds four consecutive tracks in registers (16-byte loads): a matched track runs the crossing test
//                           in fp64 (__dsub_rn / __dmul_rn), writes ids[i] / events[i] of its detection and takes the detection; an
//                           unmatched one coasts.  After a barrier -- every old value is in a register -- an integer scan of the
//                           survivors gives each its slot, and the tracks are written back in ascending id order.
//       the births          a thread holds four consecutive detections; an integer scan over the unmatched finite ones in index order
//                           gives each its rank r: slot S + r and id started + r while S + r < 4096, ids[i] = -1 beyond.
// Determinism: a best is a minimum over a set (fixed DPP butterflies), the masks change by atomic AND, the per-line counts and the
// confirmed count by integer atomic adds in LDS, the slots by integer scans: none depends on an order, two runs give the same bytes.
// No floating-point atomics.  fp32 arithmetic is written with __fadd_rn / __fsub_rn / __fmul_rn: nothing can be contracted.
#include <math.h>
#include <stdio.h>
#include <string.h>
#include "../csrc/common.hpp"
#include "../csrc/greedy_match.hpp"
#include "../csrc/host_api.hpp"
#include "../../include/countr_hip_tracks.h"

namespace {

using namespace countr_greedy;
constexpr int MAXS = COUNTR_TRACKS_MAX_STREAMS, MAXT = COUNTR_TRACKS_MAX_TRACKS, MAXP = COUNTR_TRACKS_MAX_POINTS;
constexpr int MAXL = COUNTR_TRACKS_MAX_LINES, HEAD = COUNTR_TRACKS_HEAD_INTS, SUMMARY = COUNTR_TRACKS_SUMMARY_INTS;
constexpr int INIT_BLOCKS = 256;                 // blocks per tracker of the first launch (4 waves each): one tracker alone fills every CU
constexpr int STEP_THREADS = 1024, STEP_WAVES = STEP_THREADS / 64;
constexpr int PER = 4;                           // tracks / detections of a thread in the update: 4 * 1024 = 4096
static_assert(PER * STEP_THREADS == MAXT && PER * STEP_THREADS == MAXP, "a thread holds 4 tracks and 4 detections");
static_assert(SUMMARY == 8 + 2 * MAXL && HEAD >= 8 + 2 * MAXL, "summary and header hold the counts");
constexpr int WS_PRED = 0, WS_BEST_T = MAXT * 8, WS_BEST_D = MAXT * 8 + MAXT * 2;      // byte offsets inside a tracker's scratch

struct TrArgs {
  int* state[MAXS];
  const float2* points[MAXS];
  int* ids[MAXS];
  unsigned* events[MAXS];
  int* summary[MAXS];
  const float4* lines[MAXS];
  int N[MAXS], L[MAXS], ws[MAXS];                // ws: the tracker's scratch, byte offset in the workspace (a multiple of 16)
  float md2[MAXS], beta[MAXS];
  int max_missed[MAXS], min_hits[MAXS];
};

// the arrays of a state
struct State {
  int* head;
  int* id;
  float *x, *y, *vx, *vy, *lx, *ly;
  int *hits, *missed;
  __device__ explicit State(int* s)
      : head(s), id(s + HEAD), x((float*)(s + HEAD + MAXT)), y((float*)(s + HEAD + 2 * MAXT)), vx((float*)(s + HEAD + 3 * MAXT)),
        vy((float*)(s + HEAD + 4 * MAXT)), lx((float*)(s + HEAD + 5 * MAXT)), ly((float*)(s + HEAD + 6 * MAXT)),
        hits(s + HEAD + 7 * MAXT), missed(s + HEAD + 8 * MAXT) {}
  __device__ __forceinline__ float2 predict(int j) const { return make_float2(__fadd_rn(x[j], vx[j]), __fadd_rn(y[j], vy[j])); }
};

__device__ __forceinline__ int live_of(const int* head) { const int T = head[0]; return T < 0 ? 0 : (T > MAXT ? MAXT : T); }

struct FromState {                               // candidates are the tracks' predictions, formed from the state
  const State* s;
  __device__ __forceinline__ float2 at(int k) const { return s->predict(k); }
};

__global__ __launch_bounds__(256) void tracks_init_kernel(const TrArgs a, unsigned char* __restrict__ ws) {
  const int s = blockIdx.y;
  const State st(a.state[s]);
  const int N = a.N[s], T = live_of(st.head);
  const int lane = threadIdx.x & 63;
  const float2* __restrict__ det = a.points[s];
  unsigned char* w = ws + a.ws[s];
  float2* pred = reinterpret_cast<float2*>(w + WS_PRED);
  unsigned short* best_t = reinterpret_cast<unsigned short*>(w + WS_BEST_T);
  unsigned short* best_d = reinterpret_cast<unsigned short*>(w + WS_BEST_D);
  for (int q = blockIdx.x * 4 + (threadIdx.x >> 6); q < N + T; q += INIT_BLOCKS * 4) {      // (wave-uniform)
    if (q < N) {
      const int j = wave_best<false>(det[q], FromState{&st}, T, nullptr, a.md2[s], lane);
      if (lane == 0) best_d[q] = (unsigned short)j;
    } else {
      const float2 p = st.predict(q - N);
      const int i = wave_best<false>(p, FromArray{det}, N, nullptr, a.md2[s], lane);
      if (lane == 0) { best_t[q - N] = (unsigned short)i; pred[q - N] = p; }
    }
  }
}

// side(a, b, p) of the header: fp64 from the fp32 values, in the written order, no fma
__device__ __forceinline__ bool side(float ax, float ay, float bx, float by, float px, float py) {
  const double l = __dmul_rn(__dsub_rn((double)bx, (double)ax), __dsub_rn((double)py, (double)ay));
  const double r = __dmul_rn(__dsub_rn((double)by, (double)ay), __dsub_rn((double)px, (double)ax));
  return __dsub_rn(l, r) >= 0.0;
}

__global__ __launch_bounds__(STEP_THREADS) void tracks_step_kernel(const TrArgs a, const unsigned char* __restrict__ ws) {
  __shared__ unsigned short best_d[MAXP], best_t[MAXT];      // detection -> its best free track, track -> its best free detection (or NONE)
  __shared__ unsigned short m_d[MAXP], m_t[MAXT];            // the matching: detection -> track, track -> detection (or NONE)
  __shared__ unsigned free_d[MAXP / 32 + 2], free_t[MAXT / 32 + 2];      // (+2: wave_best reads the two words of a 64-chunk)
  __shared__ float4 s_lines[MAXL];
  __shared__ int s_counts[2 * MAXL], s_scan[STEP_WAVES], s_conf, s_matched;
  const int s = blockIdx.x, t = threadIdx.x;
  const State st(a.state[s]);
  const int N = a.N[s], L = a.L[s], T = live_of(st.head);
  const int started = st.head[1];
  const float md2 = a.md2[s], beta = a.beta[s];
  const int max_missed = a.max_missed[s], min_hits = a.min_hits[s];
  const float2* __restrict__ det = a.points[s];
  const unsigned char* w = ws + a.ws[s];
  const float2* __restrict__ pred = reinterpret_cast<const float2*>(w + WS_PRED);
  const unsigned short* __restrict__ ws_t = reinterpret_cast<const unsigned short*>(w + WS_BEST_T);
  const unsigned short* __restrict__ ws_d = reinterpret_cast<const unsigned short*>(w + WS_BEST_D);
  int* __restrict__ ids = a.ids[s];
  unsigned* __restrict__ events = a.events[s];

  for (int i = t; i < MAXP; i += STEP_THREADS) { best_d[i] = i < N ? ws_d[i] : (unsigned short)NONE; m_d[i] = (unsigned short)NONE; }
  for (int j = t; j < MAXT; j += STEP_THREADS) { best_t[j] = j < T ? ws_t[j] : (unsigned short)NONE; m_t[j] = (unsigned short)NONE; }
  if (t < MAXL) s_lines[t] = t < L ? a.lines[s][t] : make_float4(0.f, 0.f, 0.f, 0.f);
  if (t < 2 * MAXL) s_counts[t] = 0;
  if (t == 0) { s_conf = 0; s_matched = 0; }
  __syncthreads();
  greedy_free_masks<STEP_THREADS>(best_d, N, best_t, T, free_d, free_t, MAXP / 32 + 2);
  const int mine = greedy_rounds<STEP_THREADS>(FromArray{det}, N, FromArray{pred}, T, best_d, best_t, free_d, free_t, md2, [&](int i, int j) {
    m_d[i] = (unsigned short)j;
    m_t[j] = (unsigned short)i;
  });
  if (mine) atomicAdd(&s_matched, mine);

  // ---- the update: tracks PER * t .. PER * t + PER - 1 of this thread, in registers
  int id[PER], hits[PER], missed[PER];
  float x[PER], y[PER], vx[PER], vy[PER], lx[PER], ly[PER];
  bool keep[PER];
  int nkeep = 0, conf = 0;
  const int j0 = PER * t;
  if (j0 < T) {                                    // (the arrays hold MAXT entries: a 16-byte load past T reads the state's own memory)
    const int4 vi = reinterpret_cast<const int4*>(st.id)[t], vh = reinterpret_cast<const int4*>(st.hits)[t],
               vm = reinterpret_cast<const int4*>(st.missed)[t];
    const float4 fx = reinterpret_cast<const float4*>(st.x)[t], fy = reinterpret_cast<const float4*>(st.y)[t],
                 fvx = reinterpret_cast<const float4*>(st.vx)[t], fvy = reinterpret_cast<const float4*>(st.vy)[t],
                 flx = reinterpret_cast<const float4*>(st.lx)[t], fly = reinterpret_cast<const float4*>(st.ly)[t];
    id[0] = vi.x; id[1] = vi.y; id[2] = vi.z; id[3] = vi.w;
    hits[0] = vh.x; hits[1] = vh.y; hits[2] = vh.z; hits[3] = vh.w;
    missed[0] = vm.x; missed[1] = vm.y; missed[2] = vm.z; missed[3] = vm.w;
    x[0] = fx.x; x[1] = fx.y; x[2] = fx.z; x[3] = fx.w;
    y[0] = fy.x; y[1] = fy.y; y[2] = fy.z; y[3] = fy.w;
    vx[0] = fvx.x; vx[1] = fvx.y; vx[2] = fvx.z; vx[3] = fvx.w;
    vy[0] = fvy.x; vy[1] = fvy.y; vy[2] = fvy.z; vy[3] = fvy.w;
    lx[0] = flx.x; lx[1] = flx.y; lx[2] = flx.z; lx[3] = flx.w;
    ly[0] = fly.x; ly[1] = fly.y; ly[2] = fly.z; ly[3] = fly.w;
  }
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int j = j0 + k;
    keep[k] = false;
    if (j >= T) continue;
    const float2 p = pred[j];
    const int i = m_t[j];
    if (i != NONE) {
      const float2 d = det[i];
      unsigned ev = 0u;
      for (int l = 0; l < L; ++l) {
        const float4 ln = s_lines[l];
        const bool s0 = side(ln.x, ln.y, ln.z, ln.w, lx[k], ly[k]), s1 = side(ln.x, ln.y, ln.z, ln.w, d.x, d.y);
        if (s0 != s1 && side(lx[k], ly[k], d.x, d.y, ln.x, ln.y) != side(lx[k], ly[k], d.x, d.y, ln.z, ln.w)) {
          ev |= 1u << (s1 ? l : 16 + l);
          atomicAdd(&s_counts[2 * l + (s1 ? 0 : 1)], 1);
        }
      }
      ids[i] = id[k];
      events[i] = ev;
      vx[k] = __fadd_rn(vx[k], __fmul_rn(beta, __fsub_rn(d.x, p.x)));
      vy[k] = __fadd_rn(vy[k], __fmul_rn(beta, __fsub_rn(d.y, p.y)));
      x[k] = lx[k] = d.x;
      y[k] = ly[k] = d.y;
      hits[k] += 1;
      missed[k] = 0;
      conf += hits[k] == min_hits;
      keep[k] = true;
    } else {
      x[k] = p.x; y[k] = p.y;
      missed[k] += 1;
      keep[k] = missed[k] <= max_missed;
    }
    nkeep += keep[k];
  }
  int S;                                           // the survivors
  int pos = block_scan_i<STEP_WAVES>(nkeep, s_scan, S);      // (its first barrier: every old value of the state is in a register from here on)
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    if (!keep[k]) continue;
    st.id[pos] = id[k]; st.x[pos] = x[k]; st.y[pos] = y[k]; st.vx[pos] = vx[k]; st.vy[pos] = vy[k];
    st.lx[pos] = lx[k]; st.ly[pos] = ly[k]; st.hits[pos] = hits[k]; st.missed[pos] = missed[k];
    ++pos;
  }

  // ---- the births: detections PER * t .. PER * t + PER - 1 of this thread
  bool cand[PER];
  int ncand = 0;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int i = j0 + k;
    cand[k] = false;
    if (i >= N || m_d[i] != NONE) continue;
    const float2 d = det[i];
    cand[k] = isfinite(d.x) && isfinite(d.y);
    if (!cand[k]) { ids[i] = -1; events[i] = 0u; }
    ncand += cand[k];
  }
  int U;                                           // the unmatched finite detections
  int r = block_scan_i<STEP_WAVES>(ncand, s_scan, U);
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    if (!cand[k]) continue;
    const int i = j0 + k, at = S + r;
    if (at < MAXT) {
      const float2 d = det[i];
      st.id[at] = started + r; st.x[at] = d.x; st.y[at] = d.y; st.vx[at] = 0.f; st.vy[at] = 0.f;
      st.lx[at] = d.x; st.ly[at] = d.y; st.hits[at] = 1; st.missed[at] = 0;
      ids[i] = started + r;
    } else {
      ids[i] = -1;
    }
    events[i] = 0u;
    ++r;
  }
  if (conf) atomicAdd(&s_conf, conf);
  __syncthreads();
  const int born = U < MAXT - S ? U : MAXT - S;
  int* __restrict__ sum = a.summary[s];
  if (t < 2 * MAXL) {
    const int c = st.head[8 + t] + s_counts[t];
    st.head[8 + t] = c;
    sum[8 + t] = c;
  }
  if (t == 0) {
    const int confirmed = st.head[2] + s_conf + (min_hits == 1 ? born : 0), dropped = st.head[3] + (U - born), frame = st.head[4] + 1;
    st.head[0] = S + born; st.head[1] = started + born; st.head[2] = confirmed; st.head[3] = dropped; st.head[4] = frame;
    sum[0] = S + born; sum[1] = started + born; sum[2] = confirmed; sum[3] = s_matched; sum[4] = born; sum[5] = T - S;
    sum[6] = dropped; sum[7] = frame;
  }
}

inline int round8(int v) { return (v + 7) & ~7; }
inline int scratch_bytes(int N) { return WS_BEST_D + 2 * round8(N); }      // of one tracker: a multiple of 16

}  // namespace

extern "C" int countr_tracks_version(void) { return COUNTR_TRACKS_ABI_VERSION; }

extern "C" const char* countr_tracks_last_error(void) { return g_err; }

extern "C" int countr_tracks_state_bytes(void) { return 4 * (HEAD + COUNTR_TRACKS_FIELDS * MAXT); }

extern "C" int countr_tracks_workspace(int n, int max_points) {
  if (n < 1 || n > MAXS || max_points < 0 || max_points > MAXP)
    return failf(-1, "countr_tracks_workspace: 1..%d trackers of 0..%d points, got %d of %d", MAXS, MAXP, n, max_points);
  return n * scratch_bytes(max_points);
}

extern "C" int countr_tracks_reset(const void* const* states, int n, void* stream) {
  if (n < 1 || n > MAXS) return failf(-1, "countr_tracks_reset: 1..%d trackers a call, got %d", MAXS, n);
  if (!states) return fail(-2, "countr_tracks_reset: the states array is required");
  for (int k = 0; k < n; ++k)
    if (!states[k] || misaligned(states[k], 16))
      return failf(-2, "countr_tracks_reset: tracker %d: the state is required and 16-byte aligned", k);
  for (int k = 0; k < n; ++k) {
    const hipError_t e = hipMemsetAsync(const_cast<void*>(states[k]), 0, (size_t)countr_tracks_state_bytes(), STREAM(stream));
    if (e != hipSuccess) return failf(-10, "countr_tracks_reset: memset failed: %s", hipGetErrorString(e));
  }
  return 0;
}

extern "C" int countr_tracks_step(const countr_tracks_stream* streams, int n, void* workspace, void* stream) {
  if (n < 1 || n > MAXS) return failf(-1, "countr_tracks_step: 1..%d trackers a call, got %d", MAXS, n);
  if (!streams) return fail(-2, "countr_tracks_step: the streams array is required");
  if (!workspace || misaligned(workspace, 16)) return fail(-2, "countr_tracks_step: the workspace is required and 16-byte aligned");
  TrArgs a;
  memset(&a, 0, sizeof(a));
  int ws = 0;
  for (int k = 0; k < n; ++k) {
    const countr_tracks_stream& d = streams[k];
    if (d.N < 0 || d.N > MAXP) return failf(-3, "countr_tracks_step: tracker %d: 0..%d points, got %d", k, MAXP, d.N);
    if (d.L < 0 || d.L > MAXL) return failf(-3, "countr_tracks_step: tracker %d: 0..%d lines, got %d", k, MAXL, d.L);
    if (d.max_missed < 0 || d.max_missed > 255)
      return failf(-3, "countr_tracks_step: tracker %d: max_missed is 0..255, got %d", k, d.max_missed);
    if (d.min_hits < 1 || d.min_hits > 255) return failf(-3, "countr_tracks_step: tracker %d: min_hits is 1..255, got %d", k, d.min_hits);
    const float md2 = d.max_dist * d.max_dist;   // one fp32 multiply (the host compiler contracts nothing here: no addition follows)
    if (!(d.max_dist > 0.f) || !__builtin_isfinite(d.max_dist) || !__builtin_isfinite(md2))
      return failf(-4, "countr_tracks_step: tracker %d: max_dist is finite and > 0 and so is its fp32 square", k);
    if (!(d.beta >= 0.f && d.beta <= 1.f)) return failf(-4, "countr_tracks_step: tracker %d: beta is 0..1", k);
    if (!d.state || !d.summary || (d.N > 0 && (!d.points || !d.ids || !d.events)) || (d.L > 0 && !d.lines))
      return failf(-2, "countr_tracks_step: tracker %d has a null pointer", k);
    if (misaligned(d.state, 16) || misaligned(d.lines, 16))
      return failf(-5, "countr_tracks_step: tracker %d: the state and the lines are 16-byte aligned", k);
    if (misaligned(d.points, 8) || misaligned(d.ids, 4) || misaligned(d.events, 4) || misaligned(d.summary, 4))
      return failf(-5, "countr_tracks_step: tracker %d: the points are 8-byte aligned, ids, events and summary 4-byte aligned", k);
    for (int q = 0; q < k; ++q)
      if (streams[q].state == d.state) return failf(-6, "countr_tracks_step: trackers %d and %d share a state", q, k);
    a.state[k] = (int*)d.state; a.points[k] = (const float2*)d.points; a.ids[k] = (int*)d.ids; a.events[k] = (unsigned*)d.events;
    a.summary[k] = (int*)d.summary; a.lines[k] = (const float4*)d.lines;
    a.N[k] = d.N; a.L[k] = d.L; a.md2[k] = md2; a.beta[k] = d.beta; a.max_missed[k] = d.max_missed; a.min_hits[k] = d.min_hits;
    a.ws[k] = ws; ws += scratch_bytes(d.N);
  }
  unsigned char* w = (unsigned char*)workspace;
  hipLaunchKernelGGL(tracks_init_kernel, dim3(INIT_BLOCKS, n), dim3(256), 0, STREAM(stream), a, w);
  hipLaunchKernelGGL(tracks_step_kernel, dim3(n), dim3(STEP_THREADS), 0, STREAM(stream), a, (const unsigned char*)w);
  return launched("countr_tracks_step");
}
