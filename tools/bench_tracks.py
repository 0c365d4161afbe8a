"""Tracking: what joining the frames' points over time costs on the device, against the numpy rule and against the per-frame composition
that was available before the tracks library.

  (a) synthetic clips (countr_amd.tracks.lane_scene): eight trackers of 140 objects, then eight of 1000, then eight of 4000, 32 frames
      each, max_dist 8, one line:
        HIP       Tracker(streams=8).run: one packed upload, 32 steps of two launches, one download, one synchronisation
        HOST      tracks_host of the eight clips in numpy (the tests' yardstick)
        COMPOSED  per frame one PointMatcher.match of the eight trackers' (detections, predictions) -- an upload, two launches, a
                  download and a synchronisation per frame -- and the rest of the step in numpy (tracks_host(match=...))
      Before anything is timed the three agree on every id, event and summary.  The host forms take seconds at the larger sizes: they
      are timed over --host_calls calls (the first of them is the run that is compared), HIP over --calls, in --host_calls blocks
      that alternate with the host forms' calls.
  (b) eight 1920x1080 NV12 frames in HOST memory, ViT-B bf16, zero-shot: count_clip (one group of eight, a tracker kept across calls)
      against locate_frames alone on the same frames: what tracking adds to a group is CLIP - LOCATE.
Every call ends in a device synchronise; (b)'s forms are alternated call by call, (a)'s as said above; the figure is the median after
--warmup calls, with the quartiles and the extremes as the spread.  No threshold: whatever comes out is the record.
  --trace runs (a)'s HIP form alone, for a `rocprofv3 --kernel-trace --stats` run of its own; --kernels FILE appends the per-kernel
  averages of that run's kernel_stats.csv to --out.

    python tools/bench_tracks.py [--calls 30] [--warmup 5] [--host_calls 3] [--out profiles/tracks.txt] [--head <commit>]"""
import argparse
import csv
import os
import re
import socket
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from countr_amd import Tracker, tracks_host
from countr_amd import tracks as TR
from countr_amd.match import point_matcher

SIZES, TRACKERS, FRAMES = (140, 1000, 4000), 8, 32
H, W, N = 1080, 1920, 8


def head(root):
    try:
        return subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=root, stderr=subprocess.DEVNULL, text=True).strip()
    except Exception:
        return "unknown"


def spread(ms):
    q = np.percentile(ms, [0, 25, 50, 75, 100])
    return "median %10.3f ms  (quartiles %.3f .. %.3f, extremes %.3f .. %.3f, %d calls)" % (q[2], q[1], q[3], q[0], q[4], len(ms))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def composed(clips, kw):
    """The composition available before the library: the association of every frame through PointMatcher.match, the rest in numpy."""
    pm = point_matcher("cuda")
    states, outs = [None] * len(clips), [[] for _ in clips]
    for f in range(FRAMES):
        sets = []
        for s, clip in enumerate(clips):
            st = states[s] or TR.empty_state()
            p = np.stack([st["x"] + st["vx"], st["y"] + st["vy"]], 1).astype(np.float32).reshape(-1, 2)
            sets.append((clip[f], p, kw["max_dist"]))
        res = pm.match(sets)
        for s, clip in enumerate(clips):
            (r,), states[s] = tracks_host([clip[f]], state=states[s], match=lambda _D, _p, _md, m=res[s]: (m[0], m[1]), **kw)
            outs[s].append(r)
    return outs


def same(a, b):
    return all(np.array_equal(x[k], y[k]) for ca, cb in zip(a, b) for x, y in zip(ca, cb) for k in range(3))


def kernel_lines(path):
    rows = [r for r in csv.DictReader(open(path)) if "TrArgs" in r.get("Name", "")]          # the tracks library's launches
    lines = ["(c) the kernels' own times (a rocprofv3 --kernel-trace --stats run of its own over --trace: the three sizes of (a), eight trackers a launch)"]
    for r in rows:
        name = re.search(r"\w+_kernel", r["Name"]).group(0)
        lines.append("    %-24s %6s calls, average %9.1f us, min %9.1f us, max %9.1f us"
                     % (name, r["Calls"], float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host_calls", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--head", default="")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--kernels", default="")
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if args.kernels:
        text = "\n".join(kernel_lines(args.kernels))
        print(text)
        if args.out:
            with open(args.out, "a") as f:
                f.write(text + "\n")
        return
    lines = ["tracks: box %s, HEAD %s, %s" % (socket.gethostname(), args.head or head(root), torch.cuda.get_device_name(0)),
             "every call synchronised; (a) HIP: %d calls after %d warm-up calls, in %d blocks alternating with the host forms' %d calls; (b) forms "
             "alternated call by call, %d calls after %d" % (args.calls, args.warmup, args.host_calls, args.host_calls, args.calls, args.warmup),
             "(a) %d trackers x %d frames of a synthetic clip (lanes 20 px apart, 2..6 px/frame, drop-outs, shuffled), max_dist 8, one line; "
             "HIP, HOST and COMPOSED agree on every id, event and summary" % (TRACKERS, FRAMES)]
    for K in SIZES:
        scenes = [TR.lane_scene(K=K, frames=FRAMES, seed=s) for s in range(TRACKERS)]
        clips = [sc[0] for sc in scenes]
        kw = dict(max_dist=8.0, lines=[scenes[0][2]])
        tracker = Tracker("cuda", streams=TRACKERS, **kw)

        def hip():
            tracker.reset()
            return tracker.run(clips)

        if args.trace:
            for _ in range(10):
                hip()
            torch.cuda.synchronize()
            continue
        host = lambda: [tracks_host(c, **kw)[0] for c in clips]
        comp = lambda: composed(clips, kw)
        th, tc = [], []
        want, ms = timed(host)
        th.append(ms)
        got_c, ms = timed(comp)
        tc.append(ms)
        assert same(hip(), want), "Tracker.run and tracks_host disagree at %d objects" % K
        assert same(got_c, want), "the per-frame composition and tracks_host disagree at %d objects" % K
        last = want[0][-1][2]
        assert last[1] == last[2] == K and tuple(last[8:10]) == scenes[0][3], "the scene's known answer is not met"
        for _ in range(args.warmup):
            hip()
        tg = []
        for r in range(args.host_calls):
            if r:
                th.append(timed(host)[1])
                tc.append(timed(comp)[1])
            block = args.calls // args.host_calls + (r < args.calls % args.host_calls)
            tg += [timed(hip)[1] for _ in range(block)]
        lines.append("  %d objects a tracker (%d detections a call; tracker 0: started = confirmed = %d, crossings %d forward, %d backward = the truth)"
                     % (K, sum(len(f) for c in clips for f in c), K, last[8], last[9]))
        for name, t, note in (("HIP", tg, "Tracker.run"), ("HOST", th, "tracks_host in numpy"),
                              ("COMPOSED", tc, "PointMatcher.match per frame + the numpy update")):
            lines.append("    %-9s %s  %s" % (name, spread(t), note))
        g, c = float(np.median(tg)), float(np.median(tc))
        lines.append("    the library is %s the per-frame composition (%.3f ms against %.3f ms for %d steps of %d trackers)"
                     % ("faster than" if g < c else "NOT faster than", g, c, FRAMES, TRACKERS))
    if args.trace:
        return
    # (b) what tracking adds to a group
    import models_mae_cross
    from countr_amd import YuvFrame, count_clip, locate_frames
    rs = np.random.RandomState(0)
    torch.manual_seed(0)
    model = models_mae_cross.mae_vit_base_patch16(precision="bf16").to("cuda").eval()
    yy, xx = np.mgrid[0:H, 0:W]
    host8 = [YuvFrame((16 + 200 * ((yy / H + xx / W) / 2) + rs.randint(0, 20, (H, W))).astype(np.uint8),
                      rs.randint(64, 192, (H // 2, W)).astype(np.uint8)) for _ in range(N)]
    tracker = Tracker("cuda", max_dist=20.0, lines=[(W / 2, -1.0, W / 2, H + 1.0)])
    locate = lambda: locate_frames(model, host8, normalization=False)
    clip = lambda: count_clip(model, host8, max_dist=20.0, group=N, tracker=tracker, normalization=False)
    ref, (got, counts) = locate(), clip()
    for a, b in zip(got, ref):
        assert a[0] == b[0] and torch.equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]), "count_clip and locate_frames disagree"
    times = {"CLIP": [], "LOCATE": []}
    for it in range(args.warmup + args.calls):
        for k, fn in (("CLIP", clip), ("LOCATE", locate)):
            ms = timed(fn)[1]
            if it >= args.warmup:
                times[k].append(ms)
    lines.append("(b) eight 1920x1080 NV12 frames in host memory, ViT-B bf16, zero-shot, one group of eight (%s points a frame); count_clip's counts, maps "
                 "and points equal locate_frames'" % " ".join(str(len(r[2])) for r in ref))
    lines.append("    CLIP      %s  count_clip (a tracker kept across calls)" % spread(times["CLIP"]))
    lines.append("    LOCATE    %s  locate_frames alone" % spread(times["LOCATE"]))
    lines.append("    tracking adds CLIP - LOCATE = %+.3f ms per group of eight" % (float(np.median(times["CLIP"])) - float(np.median(times["LOCATE"]))))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
