"""An annotated tracked clip: what drawing ids, trails, lines and tallies on the device costs, against tracking alone and against the
existing annotated frames with their PIL label.

  Eight 1920x1080 NV12 frames in HOST memory, ViT-B bf16, zero-shot, two counting lines, trail 16.  The same eight frames are one group
  of a clip that goes on: tracker and trails are kept from call to call, so after the warm-up every track has its full trail.
  (1) CLIP+DRAW  annotate_clip(out="nv12") per group        CLIP   count_clip alone: the difference is what annotating a tracked clip costs
  (2) FRAMES+DRAW annotate_frames(out="nv12", points=True)   FRAMES count_frames + locate_maps: the existing composition with its PIL label,
      measured in the same run
  (3) Painter.paint alone on the eight composed device frames with the marks of (1), against draw_host of one frame; and the host's
      share of (1): Trails.update + clip_marks for the group
  Before anything is timed: annotate_clip's count .. events equal count_clip's bit for bit, and its NV12 frames equal
  draw_host(overlay_host(...), clip_marks(...)) byte for byte (frames 0 and 7 of the first group).
Every call ends in a device synchronise; the forms are alternated call by call; the figure is the median over --calls calls after
--warmup, with the quartiles and the extremes as the spread.  The aim -- difference (1) within the larger interquartile range of
difference (2) -- is reported, not asserted: whatever comes out is the record.
  --trace runs (3)'s paint calls alone, for a `rocprofv3 --kernel-trace --stats` run of its own; --kernels FILE appends the per-kernel
  averages of that run's kernel_stats.csv to --out.

    python tools/bench_draw.py [--calls 30] [--warmup 5] [--out profiles/draw.txt] [--head <commit>]"""
import argparse
import csv
import os
import re
import socket
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import models_mae_cross
from bench_overlay import H, N, W, alternated, head, nv12_frame, spread
from countr_amd import Tracker, YuvFrame, draw as D, frames as FR, overlay as O, overlay_host, yuv_host

LINES, NAMES = [(960.0, -1.0, 960.0, 1081.0), (-1.0, 540.0, 1921.0, 540.0)], ["gate", "mid"]
TRK = dict(max_dist=8.0, max_missed=2, min_hits=3)


def kernel_lines(path):
    rows = [r for r in csv.DictReader(open(path)) if "DrawArgs" in r.get("Name", "") or "Rgb420Args" in r.get("Name", "")]
    lines = ["(4) the kernels' own times (a rocprofv3 --kernel-trace --stats run of its own over --trace: paint of eight 1080p frames, NV12 out)"]
    for r in rows:
        name = re.search(r"\w+_kernel(<[^>]*>)?", r["Name"]).group(0)
        what = {"marks_kernel<false>": "claim", "marks_kernel<true>": "paint"}.get(name, "4:2:0")
        lines.append("    %-24s %-6s %5s calls, average %9.1f us" % (name, what, r["Calls"], float(r["AverageNs"]) / 1e3))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
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
    rs = np.random.RandomState(0)
    torch.manual_seed(0)
    model = models_mae_cross.mae_vit_base_patch16(precision="bf16").to("cuda").eval()
    host8 = [YuvFrame(*nv12_frame(rs)) for _ in range(N)]
    sizes = [(W, H)] * N
    # ---- the forms agree
    ref, _clip = FR.count_clip(model, host8, lines=LINES, summaries=True, normalization=False, **TRK)
    trails, marks8 = D.Trails(16), []
    (got, _so_far), = FR.annotate_clip(model, host8, lines=LINES, line_names=NAMES, out="nv12", normalization=False, **TRK)
    for k, (g, r) in enumerate(zip(got, ref)):
        assert g[0] == r[0] and torch.equal(g[1], r[1]) and all(np.array_equal(a, b) for a, b in zip(g[2:6], r[2:6])), "annotate_clip and count_clip disagree"
        marks8.append(D.clip_marks(r[2], r[4], r[5], r[6], NAMES, LINES, r[0], size=(W, H), trails=trails.update(r[2], r[4])))
        if k in (0, N - 1):
            want = D.draw_host(overlay_host(yuv_host(host8[k]), r[1].float().cpu().numpy()), marks8[k], "nv12")
            assert np.array_equal(g[6].cpu().numpy(), want), "the device bytes differ from draw_host"
    composed = [t.clone() for t in O.overlay_for("cuda").render(FR.frame_prep("cuda").device_frames(host8), [r[1] for r in ref])]
    painter = D.painter_for("cuda")
    paint = lambda: painter.paint(composed, marks8, out="nv12")
    if args.trace:
        for _ in range(20):
            paint()
        torch.cuda.synchronize()
        return
    lines = ["draw: box %s, HEAD %s, %s" % (socket.gethostname(), args.head or head(root), torch.cuda.get_device_name(0)),
             "every call synchronised, forms alternated call by call, %d calls after %d warm-up calls" % (args.calls, args.warmup),
             "eight 1920x1080 NV12 frames in host memory, ViT-B bf16, zero-shot, two lines, trail 16; the forms agree as the tool's docstring says "
             "(%s points; marks of frame 7 of the first group: %s segments, discs, texts)"
             % (" ".join(str(len(r[2])) for r in ref), " ".join(str(len(a)) for a in marks8[-1].arrays()))]
    ta, tb = Tracker("cuda", lines=LINES, **TRK), Tracker("cuda", lines=LINES, **TRK)
    kept = D.Trails(16)
    peak = dict(max_dist=TRK["max_dist"], normalization=False)
    clip_draw = lambda: list(FR.annotate_clip(model, host8, tracker=ta, trails=kept, line_names=NAMES, out="nv12", **peak))
    clip = lambda: FR.count_clip(model, host8, tracker=tb, **peak)
    frames_draw = lambda: FR.annotate_frames(model, host8, out="nv12", points=True, normalization=False)

    def frames_():
        res = FR.count_frames(model, host8, normalization=False)
        return res, FR.locate_maps(res, sizes)

    t = alternated({"CLIP+DRAW": clip_draw, "CLIP": clip, "FRAMES+DRAW": frames_draw, "FRAMES": frames_}, args.calls, args.warmup)
    for k, note in (("CLIP+DRAW", 'annotate_clip(out="nv12"), tracker and trails kept'), ("CLIP", "count_clip alone, tracker kept"),
                    ("FRAMES+DRAW", 'annotate_frames(out="nv12", points=True)'), ("FRAMES", "count_frames + locate_maps alone")):
        lines.append("    %-12s %s  %s" % (k, spread(t[k]), note))
    med = {k: float(np.median(v)) for k, v in t.items()}
    iqr = max(float(np.subtract(*np.percentile(t[k], [75, 25]))) for k in ("CLIP+DRAW", "FRAMES+DRAW"))
    d1, d2 = med["CLIP+DRAW"] - med["CLIP"], med["FRAMES+DRAW"] - med["FRAMES"]
    lines.append("(1) annotating a tracked clip adds CLIP+DRAW - CLIP = %+.3f ms per group of eight" % d1)
    lines.append("(2) the existing annotated frames add FRAMES+DRAW - FRAMES = %+.3f ms per group of eight" % d2)
    lines.append("    (1) - (2) = %+.3f ms; the larger interquartile range of the two drawing forms is %.3f ms: the aim (within it) is %s"
                 % (d1 - d2, iqr, "met" if d1 - d2 <= iqr else "NOT met"))
    # ---- (3) the parts
    last = clip_draw()[0][0]
    live = kept.update(last[-1][2], last[-1][4])
    full = D.clip_marks(last[-1][2], last[-1][4], last[-1][5], np.zeros(40, np.int32), NAMES, LINES, last[-1][0], size=(W, H), trails=live)
    marks8[:] = [full] * N                                          # the marks of a frame whose tracks have their full trails
    tp = alternated({"paint": paint}, args.calls, args.warmup)
    t0 = time.perf_counter()
    want = D.draw_host(composed[0].cpu().numpy(), full, "nv12")
    host_ms = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(paint()[0].cpu().numpy(), want), "the device bytes differ from draw_host"
    spare, times = D.Trails(16), []
    for it in range(args.warmup + args.calls):
        t0 = time.perf_counter()
        for r in last:
            D.clip_marks(r[2], r[4], r[5], np.zeros(40, np.int32), NAMES, LINES, r[0], size=(W, H), trails=spare.update(r[2], r[4]))
        if it >= args.warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    lines.append("(3) the parts, with every track's trail full (%s segments, discs, texts a frame)" % " ".join(str(len(a)) for a in full.arrays()))
    lines.append("    Painter.paint, eight composed device frames, NV12 out   %s" % spread(tp["paint"]))
    lines.append("    draw_host, ONE frame, NV12 out                         %9.3f ms (one call)" % host_ms)
    lines.append("    Trails.update + clip_marks on the host, eight frames    %s" % spread(times))
    part = "host mark building" if np.median(times) > np.median(tp["paint"]) else "upload and kernels"
    lines.append("    of what (1) adds over the Overlay's own render, the larger measured part is the %s" % part)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
