"""The frames' points joined over time: track ids, crossings of counting lines, the number of distinct objects of a clip.

    tracks_host   the rule of countr_tracks_step (include/countr_hip_tracks.h) in numpy, fp32 arithmetic as the kernels' -- the yardstick
                  of the GPU tests, as match_host is for the matching it is built on
    Tracker       the same steps from csrc_tracks/tracks.hip on the stream the forward runs on: a whole list of frames is one packed
                  upload, the steps enqueued back to back (two launches each), one download and one synchronisation
    ClipCounts    what a clip adds up to: started, confirmed, dropped, line_counts [L, 2] (forward, backward), live
    lane_scene    a synthetic clip with a known answer (objects on lanes, drop-outs, shuffled detections): the tests' and the benchmark's

The rule in short (the header states it in full).  A step predicts every live track, p = (fl(x + vx), fl(y + vy)); associates the
detections to the predictions by the project's matching rule (match_host(D, p, max_dist): greedy over (d2, i, j)); a matched track tests
its move (last detection -> new detection) against every line in fp64, takes the detection and v = fl(v + fl(beta * fl(D - p))); an
unmatched track coasts on p and is removed when missed > max_missed; an unmatched finite detection starts a track in index order while
fewer than 4096 are live, and is dropped (ids -1) beyond.  A track counts as confirmed when its hits reach min_hits.

The defaults max_missed = 2, min_hits = 3 and beta = 0.5 are unmeasured: there is neither a checkpoint nor an annotated clip to tune them
on, and no accuracy figure exists.  What exists is the instrument, equal to this file's restatement byte for byte."""
import collections
import ctypes as C

import numpy as np

from . import _lib, _owned
from .match import match_host

_K = {k[len("COUNTR_TRACKS_"):]: v for k, v in _lib.TRACKS_CONSTS.items()}
MAX_STREAMS, MAX_TRACKS, MAX_POINTS, MAX_LINES = _K["MAX_STREAMS"], _K["MAX_TRACKS"], _K["MAX_POINTS"], _K["MAX_LINES"]
HEAD_INTS, SUMMARY_INTS = _K["HEAD_INTS"], _K["SUMMARY_INTS"]
FIELDS = ("id", "x", "y", "vx", "vy", "lx", "ly", "hits", "missed")                # the state's arrays, in the header's order
assert len(FIELDS) == _K["FIELDS"]
_INT_FIELDS = ("id", "hits", "missed")
STATE_BYTES = 4 * (HEAD_INTS + len(FIELDS) * MAX_TRACKS)

ClipCounts = collections.namedtuple("ClipCounts", "started confirmed dropped line_counts live")


def clip_counts(summary, L):
    """A step's summary int32 [40] and the number of lines -> ClipCounts (the counters after that step)."""
    s = np.asarray(summary).reshape(-1)
    return ClipCounts(int(s[1]), int(s[2]), int(s[6]), s[8:8 + 2 * L].astype(np.int64).reshape(L, 2), int(s[0]))


def _points(a):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float32))
    if a.size == 0:
        a = a.reshape(0, 2)
    if a.ndim != 2 or a.shape[1] != 2 or a.shape[0] > MAX_POINTS:
        raise ValueError("tracks: the detections of a frame are [N, 2] as (x, y), N <= %d" % MAX_POINTS)
    return a


def _lines(lines):
    a = np.ascontiguousarray(np.asarray(lines if lines is not None else (), dtype=np.float32))
    if a.size == 0:
        a = a.reshape(0, 4)
    if a.ndim != 2 or a.shape[1] != 4 or a.shape[0] > MAX_LINES or not np.isfinite(a).all():
        raise ValueError("tracks: lines are up to %d finite segments (ax, ay, bx, by)" % MAX_LINES)
    return a


def _params(max_dist, max_missed, min_hits, beta):
    md, b = np.float32(max_dist), np.float32(beta)
    with np.errstate(over="ignore"):
        if not (np.isfinite(md) and md > 0 and np.isfinite(md * md)):
            raise ValueError("max_dist is finite and > 0, and so is its fp32 square")
    if int(max_missed) != max_missed or not 0 <= max_missed <= 255:
        raise ValueError("max_missed is 0..255")
    if int(min_hits) != min_hits or not 1 <= min_hits <= 255:
        raise ValueError("min_hits is 1..255")
    if not 0 <= b <= 1:
        raise ValueError("beta is 0..1")
    return md, int(max_missed), int(min_hits), b


def empty_state():
    """An empty tracker at frame 0, in the form tracks_host and Tracker.state() return."""
    st = {f: np.zeros(0, np.int32 if f in _INT_FIELDS else np.float32) for f in FIELDS}
    st.update(started=0, confirmed=0, dropped=0, frame=0, counts=np.zeros((MAX_LINES, 2), np.int32))
    return st


def _side(ax, ay, bx, by, px, py):
    """The header's side(a, b, p): fp64 from the fp32 values, in the written order (numpy fuses nothing)."""
    ax, ay, bx, by, px, py = (np.asarray(v, np.float64) for v in (ax, ay, bx, by, px, py))
    with np.errstate(invalid="ignore", over="ignore"):
        return ((bx - ax) * (py - ay) - (by - ay) * (px - ax)) >= 0


def tracks_host(frames_points, *, max_dist, max_missed=2, min_hits=3, beta=0.5, lines=(), state=None, match=match_host):
    """frames_points: a list of detections [N, 2] as (x, y), one per frame -> ([(ids int32 [N], events uint32 [N], summary int32 [40]),
    ...] per frame, the final state).  `state` continues a tracker (the state of an earlier call, left unchanged); the state is a dict of
    the live tracks' arrays id, x, y, vx, vy, lx, ly, hits, missed in ascending id order and the counters started, confirmed, dropped,
    frame and counts int32 [16, 2].  match: the association, (D, p, max_dist) -> (match, d2) -- match_host by definition; tools/bench_tracks.py
    puts PointMatcher.match there to time the per-frame composition.  The defaults of max_missed, min_hits and beta are unmeasured."""
    md, max_missed, min_hits, beta = _params(max_dist, max_missed, min_hits, beta)
    lines = _lines(lines)
    st = empty_state() if state is None else {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in state.items()}
    out = []
    for D in frames_points:
        D = _points(D)
        N, T = D.shape[0], st["id"].shape[0]
        with np.errstate(invalid="ignore", over="ignore"):
            p = np.stack([st["x"] + st["vx"], st["y"] + st["vy"]], 1).astype(np.float32).reshape(T, 2)       # fp32 + fp32: rounded once
        match_, _d2 = match(D, p, md)
        ids, events = np.full(N, -1, np.int32), np.zeros(N, np.uint32)
        mi = np.nonzero(match_ >= 0)[0]
        mj = match_[mi]
        # matched tracks: crossings of (lx, ly) -> D_i first, then the update
        lx, ly, dx, dy = st["lx"][mj], st["ly"][mj], D[mi, 0], D[mi, 1]
        for k, (ax, ay, bx, by) in enumerate(lines):
            s0, s1 = _side(ax, ay, bx, by, lx, ly), _side(ax, ay, bx, by, dx, dy)
            cross = (s0 != s1) & (_side(lx, ly, dx, dy, ax, ay) != _side(lx, ly, dx, dy, bx, by))
            events[mi[cross & s1]] |= np.uint32(1 << k)
            events[mi[cross & ~s1]] |= np.uint32(1 << (16 + k))
            st["counts"][k, 0] += int((cross & s1).sum())
            st["counts"][k, 1] += int((cross & ~s1).sum())
        with np.errstate(invalid="ignore", over="ignore"):
            st["vx"][mj] = st["vx"][mj] + beta * (dx - p[mj, 0])
            st["vy"][mj] = st["vy"][mj] + beta * (dy - p[mj, 1])
        hit = np.zeros(T, bool)
        hit[mj] = True
        st["x"], st["y"] = p[:, 0].copy(), p[:, 1].copy()                              # a coasting track takes its prediction
        st["x"][mj] = st["lx"][mj] = dx
        st["y"][mj] = st["ly"][mj] = dy
        st["hits"][mj] += 1
        st["missed"] = np.where(hit, 0, st["missed"] + 1).astype(np.int32)
        ids[mi] = st["id"][mj]
        confirmed = int((st["hits"][mj] == min_hits).sum())
        keep = st["missed"] <= max_missed
        S = int(keep.sum())
        # births in ascending i, while fewer than MAX_TRACKS are live
        new = np.nonzero((match_ < 0) & np.isfinite(D).all(1))[0]
        born = min(new.shape[0], MAX_TRACKS - S)
        ids[new[:born]] = st["started"] + np.arange(born, dtype=np.int32)
        fresh = {"id": ids[new[:born]], "x": D[new[:born], 0], "y": D[new[:born], 1], "vx": np.zeros(born, np.float32),
                 "vy": np.zeros(born, np.float32), "lx": D[new[:born], 0], "ly": D[new[:born], 1], "hits": np.ones(born, np.int32),
                 "missed": np.zeros(born, np.int32)}
        for f in FIELDS:
            st[f] = np.concatenate([st[f][keep], fresh[f]]).astype(st[f].dtype)
        st["started"] += born
        st["confirmed"] += confirmed + (born if min_hits == 1 else 0)
        st["dropped"] += new.shape[0] - born
        st["frame"] += 1
        summary = np.zeros(SUMMARY_INTS, np.int32)
        summary[:8] = (S + born, st["started"], st["confirmed"], mi.shape[0], born, T - S, st["dropped"], st["frame"])
        summary[8:] = st["counts"].reshape(-1)
        out.append((ids, events, summary))
    return out, st


def lane_scene(K=70, frames=24, seed=0, lane=20.0, line_x=200.0):
    """A synthetic clip with a known answer: K objects, one per lane (lanes `lane` px apart), each at a constant speed of 2..6 px/frame
    to the left or to the right from a start within 100 px of the vertical line x = line_x, jitter under 0.5 px on both axes, the
    detections shuffled every frame, drop-outs of at most 2 consecutive frames and none in the first 3.  -> (frames_points, owners, line,
    truth): per frame the detections float32 [N, 2] and the object of each, the line (ax, ay, bx, by), and truth = (forward, backward)
    crossings read from every object's first and last detection with the rule's own side test."""
    rs = np.random.RandomState(seed)
    speed = rs.uniform(2.0, 6.0, K) * rs.choice([-1.0, 1.0], K)
    x0, y0 = line_x + rs.uniform(-100.0, 100.0, K), lane * np.arange(K) + lane / 2
    present = np.ones((frames, K), bool)
    for k in range(K):
        f = 3
        while f < frames:
            if rs.rand() < 0.15:
                n = int(rs.randint(1, 3))
                present[f:f + n, k] = False
                f += n + 1                                                         # a detection follows every drop-out
            else:
                f += 1
    out, owners = [], []
    for f in range(frames):
        who = rs.permutation(np.nonzero(present[f])[0])
        jit = rs.uniform(-0.49, 0.49, (who.shape[0], 2))
        out.append(np.stack([x0[who] + speed[who] * f + jit[:, 0], y0[who] + jit[:, 1]], 1).astype(np.float32))
        owners.append(who)
    line = (np.float32(line_x), np.float32(-lane), np.float32(line_x), np.float32(lane * (K + 1)))
    first, last = {}, {}
    for pts, who in zip(out, owners):
        for q, k in zip(pts, who.tolist()):
            first.setdefault(k, q)
            last[k] = q
    fwd = sum(1 for k in first if not _side(*line, *first[k]) and _side(*line, *last[k]))
    bwd = sum(1 for k in first if _side(*line, *first[k]) and not _side(*line, *last[k]))
    return out, owners, line, (fwd, bwd)


def state_from_bytes(raw):
    """The bytes of a device state (STATE_BYTES of them) -> the dict form of tracks_host."""
    w = np.frombuffer(bytes(raw), np.int32)
    live = int(w[0])
    st = {}
    for k, f in enumerate(FIELDS):
        a = w[HEAD_INTS + k * MAX_TRACKS:HEAD_INTS + k * MAX_TRACKS + live]
        st[f] = a.copy() if f in _INT_FIELDS else a.view(np.float32).copy()
    st.update(started=int(w[1]), confirmed=int(w[2]), dropped=int(w[3]), frame=int(w[4]),
              counts=w[8:8 + 2 * MAX_LINES].reshape(MAX_LINES, 2).copy())
    return st


def states_equal(a, b):
    """Two states in the dict form, bit for bit (a NaN equals itself)."""
    return (all(a[k] == b[k] for k in ("started", "confirmed", "dropped", "frame")) and np.array_equal(a["counts"], b["counts"])
            and all(a[f].dtype == b[f].dtype and a[f].tobytes() == b[f].tobytes() for f in FIELDS))


class Tracker:
    """countr_tracks_step on host point lists: `streams` independent trackers (one per camera) with the same parameters and lines.  Owns
    the states, the workspace, the packed point buffer, the packed result buffer and their pinned mirrors; they grow monotonically, so a
    steady stream of calls allocates nothing but its (host) results.  Calls follow each other on the current stream; a call on another
    stream waits for the previous call's event first.  The defaults of max_missed, min_hits and beta are unmeasured."""

    def __init__(self, device="cuda", *, streams=1, max_dist, max_missed=2, min_hits=3, beta=0.5, lines=()):
        self.device = _owned.resolve(device, "Tracker")
        if int(streams) != streams or streams < 1:
            raise ValueError("streams is >= 1")
        self.streams = int(streams)
        self.max_dist, self.max_missed, self.min_hits, self.beta = _params(max_dist, max_missed, min_hits, beta)
        self.lines = _lines(lines)
        self.L = _lib.tracks_lib()
        assert self.L.countr_tracks_state_bytes() == STATE_BYTES
        self._descs = (_lib.TracksStream * MAX_STREAMS)()
        self._ptrs = (C.c_void_p * MAX_STREAMS)()
        import torch
        with torch.cuda.device(self.device):
            self._states = torch.zeros(self.streams, STATE_BYTES, dtype=torch.uint8, device=self.device)
            self._lines = torch.zeros(MAX_LINES * 4, dtype=torch.float32, device=self.device)
            if self.lines.size:
                self._lines[:self.lines.size].copy_(torch.from_numpy(self.lines.reshape(-1)))
            self._guard = _owned.Guard(self.device, recorded=True)      # the first call on another stream waits for the fills above
        self._ws = None             # uint8, one call's scratch (the calls follow each other on one stream)
        self._pts = self._pts_host = None           # float32: every step's detections as (x, y) pairs
        self._out = self._out_host = None           # int32: ids [sum N] | events [sum N] | summaries [steps, 40]

    def _reserve(self, ws_bytes, floats, ints):
        import torch
        _owned.grow(self, "_ws", ws_bytes, torch.uint8)
        _owned.grow(self, "_pts", floats, torch.float32, pinned=True)
        _owned.grow(self, "_out", ints, torch.int32, pinned=True)

    def reset(self):
        """Every tracker becomes empty at frame 0 again (on the current stream; nothing is waited for)."""
        import torch
        with torch.cuda.device(self.device):
            cur = self._guard.enter()
            for c0 in range(0, self.streams, MAX_STREAMS):
                n = min(MAX_STREAMS, self.streams - c0)
                for k in range(n):
                    self._ptrs[k] = self._states[c0 + k].data_ptr()
                _lib.tracks_check(self.L.countr_tracks_reset(self._ptrs, n, C.c_void_p(cur.cuda_stream)), "countr_tracks_reset")
            self._guard.leave(cur)

    def state(self, stream=0):
        """The state of one tracker, downloaded (this synchronises), in the dict form of tracks_host."""
        import torch
        with torch.cuda.device(self.device):
            cur = self._guard.enter()
            raw = self._states[stream].cpu()
            self._guard.leave(cur)
        return state_from_bytes(raw.numpy().tobytes())

    def run(self, frames_points):
        """streams == 1: a list of detections [N, 2], one per frame -> [(ids, events, summary), ...] per frame.  streams > 1: one such
        list per stream (their lengths may differ) -> one list of results per stream.  One packed upload, the steps back to back (more
        than 16 streams in chunks of 16), one download, one synchronisation, on the current stream."""
        import torch
        per = [frames_points] if self.streams == 1 else list(frames_points)
        if len(per) != self.streams:
            raise ValueError("Tracker.run: %d streams, got %d lists of frames" % (self.streams, len(per)))
        per = [[_points(D) for D in frames] for frames in per]
        steps = [(s, f) for s, frames in enumerate(per) for f in range(len(frames))]
        if not steps:
            return [] if self.streams == 1 else [[] for _ in per]
        total = sum(per[s][f].shape[0] for s, f in steps)
        max_n = max(per[s][f].shape[0] for s, f in steps)
        ws_bytes = self.L.countr_tracks_workspace(min(self.streams, MAX_STREAMS), max_n)
        _lib.tracks_check(min(ws_bytes, 0), "countr_tracks_workspace")
        floats, ints = max(2 * total, 2), 2 * total + SUMMARY_INTS * len(steps)
        with torch.cuda.device(self.device):
            self._reserve(ws_bytes, floats, ints)
            cur = self._guard.enter()
            stage, at, where = self._pts_host.numpy(), 0, {}
            for k, (s, f) in enumerate(steps):
                D = per[s][f]
                where[s, f] = (at, k)
                stage[2 * at:2 * at + D.size] = D.reshape(-1)
                at += D.shape[0]
            self._pts[:floats].copy_(self._pts_host[:floats], non_blocking=True)          # the one upload
            pts, out, st = self._pts.data_ptr(), self._out.data_ptr(), C.c_void_p(cur.cuda_stream)
            lines = self._lines.data_ptr() if self.lines.shape[0] else None
            for c0 in range(0, self.streams, MAX_STREAMS):
                chunk = range(c0, min(c0 + MAX_STREAMS, self.streams))
                for f in range(max(len(per[s]) for s in chunk)):
                    n = 0
                    for s in chunk:
                        if f >= len(per[s]):
                            continue
                        off, k = where[s, f]
                        N, d = per[s][f].shape[0], self._descs[n]
                        d.state = self._states[s].data_ptr()
                        d.points, d.ids, d.events = (pts + 8 * off, out + 4 * off, out + 4 * (total + off)) if N else (None, None, None)
                        d.summary = out + 4 * (2 * total + SUMMARY_INTS * k)
                        d.lines, d.L, d.N = lines, self.lines.shape[0], N
                        d.max_dist, d.beta, d.max_missed, d.min_hits = float(self.max_dist), float(self.beta), self.max_missed, self.min_hits
                        n += 1
                    _lib.tracks_check(self.L.countr_tracks_step(self._descs, n, self._ws.data_ptr(), st), "countr_tracks_step")
            self._out_host[:ints].copy_(self._out[:ints], non_blocking=True)              # the one download
            self._guard.leave(cur)
        self._guard.event.synchronize()              # the one wait of the call
        got = self._out_host[:ints].numpy()
        res = [[] for _ in per]
        for s, f in steps:
            off, k = where[s, f]
            N = per[s][f].shape[0]
            res[s].append((got[off:off + N].copy(), got[total + off:total + off + N].view(np.uint32).copy(),
                           got[2 * total + SUMMARY_INTS * k:2 * total + SUMMARY_INTS * (k + 1)].copy()))
        return res[0] if self.streams == 1 else res
