"""Decoder frames -> counts: what the colour conversion costs, and what the smaller upload saves.

  (a) YuvConverter alone on NV12 frames already on the device: eight 1920x1080 frames in one call (one launch) and one 3840x2160 frame,
      against the frames' own bytes -- 1.5 bytes a pixel read, 3 written.
  (b) count_frames (ViT-B, bf16, zero-shot, 32 windows in one forward) on eight 1920x1080 frames in HOST memory:
        YUV       the frames as NV12 YuvFrames: 1.5 bytes a pixel uploaded, converted on the device
        RGB       the same pictures as uint8 [H, W, 3] host arrays (yuv_host of the frames, made before the clock starts): the path
                  without this library, conversion time not counted
        HOST+RGB  yuv_host of every frame inside the timed call, then the RGB call: what a caller without the library pays in numpy
      The three give the same counts and maps bit for bit; that is asserted before anything is timed.
Every call ends in a device synchronise; the forms are alternated call by call; the figure is the median over --calls calls after
--warmup, with the quartiles and the extremes as the spread.  No threshold: whatever comes out is the record.

    python tools/bench_yuv.py [--calls 30] [--warmup 5] [--out profiles/yuv.txt] [--head <commit>]"""
import argparse
import os
import socket
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import models_mae_cross
from countr_amd import YuvConverter, YuvFrame, frames as FR, yuv_host


def head(root):
    try:
        return subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=root, stderr=subprocess.DEVNULL, text=True).strip()
    except Exception:
        return "unknown"


def nv12_frame(rs, H, W):
    """A picture with structure (smooth luma ramps + noise, smooth chroma), as NV12 planes."""
    yy, xx = np.mgrid[0:H, 0:W]
    y = (16 + 200 * ((yy / H + xx / W) / 2) + rs.randint(0, 20, (H, W))).astype(np.uint8)
    c = rs.randint(64, 192, (H // 2, W)).astype(np.uint8)
    return y, c


def alternated(fns, calls, warmup):
    """{name: [ms, ...]}: the forms called in turn, every call synchronised."""
    times = {k: [] for k in fns}
    for it in range(warmup + calls):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if it >= warmup:
                times[k].append((time.perf_counter() - t0) * 1e3)
    return times


def spread(ms):
    q = np.percentile(ms, [0, 25, 50, 75, 100])
    return "median %8.3f ms  (quartiles %.3f .. %.3f, extremes %.3f .. %.3f, %d calls)" % (q[2], q[1], q[3], q[0], q[4], len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--head", default="")
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rs = np.random.RandomState(0)
    lines = ["yuv: box %s, HEAD %s, %s" % (socket.gethostname(), args.head or head(root), torch.cuda.get_device_name(0)),
             "every call synchronised, forms alternated call by call, %d calls after %d warm-up calls" % (args.calls, args.warmup)]

    # (a) the converter alone, frames on the device
    conv = YuvConverter("cuda")
    planes = [nv12_frame(rs, 1080, 1920) for _ in range(8)]
    dev8 = [YuvFrame(torch.from_numpy(y).cuda(), torch.from_numpy(c).cuda()) for y, c in planes]
    y4, c4 = nv12_frame(rs, 2160, 3840)
    dev4k = [YuvFrame(torch.from_numpy(y4).cuda(), torch.from_numpy(c4).cuda(), chroma="linear")]
    dev8_lin = [YuvFrame(f.y, f.c0, chroma="linear") for f in dev8]
    for f, t in zip(dev8[:1] + dev4k, conv.convert(dev8[:1]) + conv.convert(dev4k)):
        assert np.array_equal(t.cpu().numpy(), yuv_host(f)), "the device bytes differ from yuv_host"
    ta = alternated({"8x1080p nearest": lambda: conv.convert(dev8), "8x1080p linear": lambda: conv.convert(dev8_lin),
                     "1x2160p nearest": lambda: conv.convert([YuvFrame(dev4k[0].y, dev4k[0].c0)]), "1x2160p linear": lambda: conv.convert(dev4k)},
                    args.calls, args.warmup)
    lines.append("(a) YuvConverter.convert on device NV12 frames (wall time of the call: grouping, one launch, synchronise); bytes = 1.5 read + 3 written per pixel")
    for k, ms in ta.items():
        px = 8 * 1080 * 1920 if k.startswith("8") else 2160 * 3840
        med = float(np.median(ms))
        lines.append("    %-16s %s  %.1f MB -> %.2f TB/s of the call" % (k, spread(ms), px * 4.5 / 1e6, px * 4.5 / 1e12 / (med / 1e3)))
    ev = []
    for name, fr in (("8x1080p nearest", dev8), ("1x2160p linear", dev4k)):          # the launch alone: events around 50 back-to-back calls
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        conv.convert(fr)
        a.record()
        for _ in range(50):
            conv.convert(fr)
        b.record()
        torch.cuda.synchronize()
        px = 8 * 1080 * 1920 if name.startswith("8") else 2160 * 3840
        us = a.elapsed_time(b) / 50 * 1e3
        ev.append("%s %.1f us per call = %.2f TB/s" % (name, us, px * 4.5 / 1e12 / (us / 1e6)))
    lines.append("    50 calls back to back between two events (enqueue-bound if the host is slower than the kernel): " + "; ".join(ev))

    # (b) count_frames from host frames
    torch.manual_seed(0)
    model = models_mae_cross.mae_vit_base_patch16(precision="bf16").to("cuda").eval()
    host8 = [YuvFrame(y, c) for y, c in planes]
    rgb8 = [yuv_host(f) for f in host8]
    forms = {"YUV": lambda: FR.count_frames(model, host8, normalization=False),
             "RGB": lambda: FR.count_frames(model, rgb8, normalization=False),
             "HOST+RGB": lambda: FR.count_frames(model, [yuv_host(f) for f in host8], normalization=False)}
    got = {k: fn() for k, fn in forms.items()}
    for k in ("RGB", "HOST+RGB"):
        for (c0, d0), (c1, d1) in zip(got["YUV"], got[k]):
            assert c0 == c1 and torch.equal(d0, d1), "YUV and %s disagree" % k
    lines.append("(b) count_frames, eight 1920x1080 host frames, ViT-B bf16, zero-shot; the three forms agree bit for bit (counts %s)"
                 % " ".join("%.2f" % c for c, _d in got["YUV"]))
    tb = alternated(forms, args.calls, args.warmup)
    for k, note in (("YUV", "NV12 YuvFrames, 24.9 MB uploaded, converted on the device"), ("RGB", "uint8 RGB arrays, 49.8 MB uploaded, conversion not counted"),
                    ("HOST+RGB", "yuv_host in numpy on the host, then the RGB call")):
        lines.append("    %-9s %s  %s" % (k, spread(tb[k]), note))
    y, r = float(np.median(tb["YUV"])), float(np.median(tb["RGB"]))
    iqr = max(np.percentile(tb["YUV"], 75) - np.percentile(tb["YUV"], 25), np.percentile(tb["RGB"], 75) - np.percentile(tb["RGB"], 25))
    lines.append("    YUV - RGB = %+.3f ms per group (the larger interquartile range of the two: %.3f ms): %s"
                 % (y - r, iqr, "YUV is the faster call" if y < r - iqr else "YUV is the SLOWER call" if y > r + iqr else "no difference beyond the spread"))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
