/*
 * countr_hip_tracks.h -- C ABI of libcountr_hip_tracks.so: the frames' points joined over time -- detections associated to predicted
 * tracks, track birth and death, and crossings of counting lines -- on the device and on the caller's stream.  The six older headers
 * are closed; this header is the one statement of a library of its own, in the same dialect (countr_amd/_lib.py::parse_header reads all
 * seven), with the same conventions: extern "C", plain pointers and sizes, 0 on success and < 0 on error with the text in
 * countr_tracks_last_error() (thread-local), no allocation and no synchronisation inside a call.  One build, no fp16 twin.  The library
 * keeps no per-device state and needs no init call: a tracker IS its state buffer.
 *
 * THE RULE (countr_amd/tracks.py::tracks_host restates it in numpy).  Every fp32 operation is rounded once, nothing is contracted.
 *   A tracker holds at most COUNTR_TRACKS_MAX_TRACKS live tracks in ascending id order.  A track has: id; the estimate (x, y); the
 *   velocity (vx, vy); the last detection (lx, ly); hits; missed.  The tracker's counters: live; started (also the next id, from 0);
 *   confirmed; dropped; frame (the steps taken); counts[16][2] (forward, backward per line).
 *   One step takes the detections D, fp32 [N, 2] as (x, y), N in 0 .. COUNTR_TRACKS_MAX_POINTS:
 *   1 Predict.  For every live track p = (fl(x + vx), fl(y + vy)).
 *   2 Associate.  The matching rule of countr_match_points (include/countr_hip.h) with pred = the detections in their order, gt = the
 *     predictions in ascending id order, and max_dist: d2 = fl(fl(dx*dx) + fl(dy*dy)), a pair is eligible iff d2 <= fl(max_dist *
 *     max_dist), the matching is the greedy one over (d2, i, j).  A non-finite detection or prediction has no eligible pair.
 *   3 A matched track j with detection i: first the crossing test below on the move (lx, ly) -> D_i; then
 *     vx = fl(vx + fl(beta * fl(D_ix - p_x))), vy likewise; x = lx = D_ix, y = ly = D_iy; hits += 1; missed = 0; ids[i] = the track's id.
 *     When hits reaches min_hits (hits == min_hits after the increment), confirmed += 1.
 *   4 An unmatched track takes (x, y) = p and keeps v; missed += 1; it is removed when missed > max_missed.
 *   5 An unmatched finite detection, in ascending i, starts a track: id = started++, x = l = D_i, v = 0, hits = 1, missed = 0 (and
 *     confirmed += 1 if min_hits == 1) -- while fewer than COUNTR_TRACKS_MAX_TRACKS tracks are live after the survivors; beyond that
 *     ids[i] = -1 and dropped += 1.  A non-finite detection gets ids[i] = -1 and starts nothing.
 *   Crossings.  side(a, b, p) = ((bx - ax) * (py - ay) - (by - ay) * (px - ax) >= 0), in fp64 from the fp32 values, in that operation
 *     order, no fma.  A matched move l -> D crosses line k = (a, b) iff side(a, b, l) != side(a, b, D) and side(l, D, a) != side(l, D, b).
 *     It is forward when it ends on side 1 (bit k of events[i], counts[k][0] += 1) and backward otherwise (bit 16 + k, counts[k][1] += 1).
 *     A point exactly on the line is on side 1, so a track that lands on a line and moves on is counted once; a zero-length line, a
 *     zero-length move and a coasting step count nothing.
 *   Outputs of a step: ids int32 [N]; events uint32 [N]; summary int32 [COUNTR_TRACKS_SUMMARY_INTS] = live, started, confirmed, matched,
 *     born, died, dropped, frame, then counts[16][2].  live, started, confirmed, dropped, frame and counts are the tracker's counters
 *     after the step; matched, born and died are of this step.
 *
 * THE STATE.  countr_tracks_state_bytes() bytes per tracker, 16-byte aligned, all 32-bit words:
 *     int32 head[COUNTR_TRACKS_HEAD_INTS]: [0] live, [1] started, [2] confirmed, [3] dropped, [4] frame, [5 .. 7] 0,
 *                                          [8 .. 39] counts[16][2], the rest 0
 *     then nine arrays of COUNTR_TRACKS_MAX_TRACKS words in this order: id (int32), x, y, vx, vy, lx, ly (fp32), hits, missed (int32).
 *   Only the first `live` entries of an array mean anything.  A state of all zero bytes is an empty tracker at frame 0.
 */
#ifndef COUNTR_HIP_TRACKS_H
#define COUNTR_HIP_TRACKS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden: what this header declares is what it exports */

#define COUNTR_TRACKS_ABI_VERSION 1
#define COUNTR_TRACKS_MAX_STREAMS 16    /* trackers of one call */
#define COUNTR_TRACKS_MAX_TRACKS 4096   /* live tracks of a tracker */
#define COUNTR_TRACKS_MAX_POINTS 4096   /* detections of a step */
#define COUNTR_TRACKS_MAX_LINES 16      /* counting lines of a tracker */
#define COUNTR_TRACKS_HEAD_INTS 64      /* the state's header block, in 32-bit words */
#define COUNTR_TRACKS_FIELDS 9          /* arrays behind it: id x y vx vy lx ly hits missed */
#define COUNTR_TRACKS_SUMMARY_INTS 40   /* a step's summary */
int countr_tracks_version(void);               /* COUNTR_TRACKS_ABI_VERSION */
const char* countr_tracks_last_error(void);    /* thread-local message of the last failing call of THIS library */
int countr_tracks_state_bytes(void);           /* 4 * (COUNTR_TRACKS_HEAD_INTS + COUNTR_TRACKS_FIELDS * COUNTR_TRACKS_MAX_TRACKS) */

/* One tracker of a call.  state, points, ids, events, summary and lines are device pointers: state as above (16-byte aligned), points
 * fp32 [N, 2] (8-byte aligned; may be NULL when N = 0), ids int32 [N] and events uint32 [N] (may be NULL when N = 0), summary int32
 * [COUNTR_TRACKS_SUMMARY_INTS], lines fp32 [L, 4] as (ax, ay, bx, by) (16-byte aligned; NULL when L = 0).  max_dist is finite and > 0,
 * beta in 0 .. 1, max_missed in 0 .. 255, min_hits in 1 .. 255.  Two trackers of a call share no state and no output. */
typedef struct countr_tracks_stream {
  void* state;
  const void* points;
  void* ids;
  void* events;
  void* summary;
  const void* lines;
  int N, L;
  float max_dist, beta;
  int max_missed, min_hits;
} countr_tracks_stream;

/* bytes of scratch a countr_tracks_step call of n trackers with at most max_points detections each needs (< 0: bad arguments) */
int countr_tracks_workspace(int n, int max_points);

/* n (1 .. COUNTR_TRACKS_MAX_STREAMS) states (a HOST array of device pointers) become empty trackers at frame 0, on `stream`. */
int countr_tracks_reset(const void* const* states, int n, void* stream);

/*
 * countr_tracks_step: n (1 .. COUNTR_TRACKS_MAX_STREAMS) independent trackers advance by one step each, by the rule above, on `stream`.
 * `streams` is a HOST array read at call time.  Two launches whatever the trackers hold: (1) on every CU, a wave per detection or track
 * predicts and finds the point's first best partner; (2) a block per tracker runs the exact rounds of locally dominant pairs, then the
 * update, the crossings, the deaths and the compaction (an integer scan) and the births (an integer scan over the unmatched detections
 * in index order).  The number of live tracks is read on the device; nothing is read back, allocated or waited for.  Minima, integer
 * scans and integer atomics in LDS only: the bytes written do not depend on the execution order.  workspace: 16-byte aligned device
 * scratch of countr_tracks_workspace(n, max N) bytes.  A refused call (n out of range, a null or misaligned pointer, N, L, max_missed
 * or min_hits out of range, a max_dist that is not finite and > 0, a beta outside 0 .. 1) launches nothing.
 */
int countr_tracks_step(const countr_tracks_stream* streams, int n, void* workspace, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* COUNTR_HIP_TRACKS_H */
