"""Line counts from density flux: what the motion field and the flux cost on the device, against the numpy rule and against the same SAD
search written with torch ops on the device.

  (a) a synthetic clip (countr_amd.flow.blob_scene at the size of a 1080p frame's map, 384 x 672, ten objects), nine frames = one frame of
      history and a group of eight, search 4, interval 1, three lines:
        HIP     FlowCounter.run of the group: luma, motion, flux and fold launches, one download, one synchronisation
        HOST    flow_host of the same frames in numpy (the tests' yardstick)
        TORCH   the same search as torch ops on the device (replicate padding, one |a - b| and an 8 x 8 block sum per candidate, argmin in
                the rule's order, the sub-pixel step), motion fields downloaded; the flux is not part of this form
      Before anything is timed the three agree on every motion byte, and HIP and HOST on the flux within the tests' bound.
  (b) eight 1920x1080 NV12 frames in HOST memory, ViT-B bf16, zero-shot: count_flow (one group of eight, a counter kept across calls)
      against count_frames alone on the same frames: what the flux adds to a group is FLOW - COUNT.
Every call ends in a device synchronise; the forms are alternated call by call (HOST, which takes seconds, over --host_calls calls); the
figure is the median after --warmup calls, with the quartiles and the extremes as the spread.  No threshold: whatever comes out is the
record.
  --trace runs (a)'s HIP form alone, for a `rocprofv3 --kernel-trace --stats` run of its own; --kernels FILE appends the per-kernel
  averages of that run's kernel_stats.csv to --out.

    python tools/bench_flow.py [--calls 30] [--warmup 5] [--host_calls 3] [--out profiles/flow.txt] [--head <commit>]"""
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

from countr_amd import FlowCounter, flow_host
from countr_amd import flow as FL

H, W, N = 1080, 1920, 8
MH, MW = 384, 672
SEARCH, INTERVAL, BAND = 4, 1, 8.0 * H / 384


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


def motion_torch(cur, old, r, min_gain):
    """flow.motion_host with torch ops on the device: cur, old uint8 [h, w] device tensors -> int16 [h / 8, w / 8, 2] on the device."""
    h, w = cur.shape
    Hc, Wc = h // 8, w // 8
    pad = lambda t, p: torch.nn.functional.pad(t.float()[None, None], (p, p, p, p), mode="replicate")[0, 0].to(torch.int32)
    a, b = pad(cur, 4), pad(old, 4 + r)
    order = FL.candidates(r)
    S = torch.empty(len(order), Hc, Wc, dtype=torch.int32, device=cur.device)
    for k, (oy, ox) in enumerate(order):
        d = (a - b[r + oy:r + oy + h + 8, r + ox:r + ox + w + 8]).abs()
        blk = d.reshape(Hc + 1, 8, Wc + 1, 8).sum((1, 3))
        S[k] = blk[:-1, :-1] + blk[1:, :-1] + blk[:-1, 1:] + blk[1:, 1:]
    # the first minimum in the rule's order: the smallest k among the minima
    low = S.min(0).values
    ks = torch.arange(len(order), device=cur.device).view(-1, 1, 1)
    pick = torch.where(S == low, ks, len(order)).min(0).values
    oys = torch.tensor([o[0] for o in order], device=cur.device)[pick]
    oxs = torch.tensor([o[1] for o in order], device=cur.device)[pick]
    index = {o: k for k, o in enumerate(order)}
    table = torch.tensor([[index[(oy, ox)] for ox in range(-r, r + 1)] for oy in range(-r, r + 1)], device=cur.device)
    at = lambda oy, ox: S.gather(0, table[oy.clamp(-r, r) + r, ox.clamp(-r, r) + r][None])[0]
    s0, sz = low, S[0]
    rest = ((oys != 0) | (oxs != 0)) & (sz - s0 < min_gain)

    def fit(sm, sp, inside):
        den = torch.maximum(sm, sp) - s0
        safe = torch.where(den > 0, den, torch.ones_like(den))
        f = torch.div(16 * (sm - sp) + safe, 2 * safe, rounding_mode="floor")
        return torch.where(inside & (den > 0), f, torch.zeros_like(f))

    fx = fit(at(oys, oxs - 1), at(oys, oxs + 1), oxs.abs() < r)
    fy = fit(at(oys - 1, oxs), at(oys + 1, oxs), oys.abs() < r)
    zero = torch.zeros_like(fx)
    return torch.stack([torch.where(rest, zero, 16 * oxs + fx), torch.where(rest, zero, 16 * oys + fy)], -1).to(torch.int16)


def kernel_lines(path):
    rows = [r for r in csv.DictReader(open(path)) if "flow_" in r.get("Name", "")]              # the flow library's launches
    lines = ["(c) the kernels' own times (a rocprofv3 --kernel-trace --stats run of its own over --trace: (a)'s group of eight 384 x 672 frames a launch)"]
    for r in rows:
        name = re.search(r"flow_\w+_kernel", r["Name"]).group(0)
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
    lumas, maps, lines3, _truth = FL.blob_scene(h=MH, w=MW, objects=10, frames=N + INTERVAL, speed=(1.0, 3.0), seed=0)
    placement = (W / MW, 0.5 * W / MW - 0.5, H / MH, 0.5 * H / MH - 0.5)
    lines3 = (np.asarray(lines3, np.float64) * (placement[0::2] * 2) + (placement[1::2] * 2)).astype(np.float32)      # map pixels -> frame pixels
    images = [torch.from_numpy(FL.image_of_luma(l)).cuda() for l in lumas]
    dmaps = [torch.from_numpy(m).cuda() for m in maps]
    dl = [torch.from_numpy(l).cuda() for l in lumas]
    kw = dict(lines=lines3, search=SEARCH, interval=INTERVAL, min_gain=256, band=BAND)
    fc = FlowCounter("cuda", **kw)
    fc.run(images[:INTERVAL], [None] * INTERVAL, [(W, H)] * INTERVAL)                            # the history
    hip = lambda: fc.run(images[INTERVAL:], dmaps[INTERVAL:], [(W, H)] * N, motion=True)
    if args.trace:
        for _ in range(10):
            hip()
        torch.cuda.synchronize()
        return
    host = lambda: flow_host(lumas, maps, placement=fc.placement, **kw)[0][INTERVAL:]
    tor = lambda: [motion_torch(dl[t], dl[t - INTERVAL], SEARCH, 256).cpu().numpy() for t in range(INTERVAL, N + INTERVAL)]
    want, got, gt = host(), hip(), tor()
    u, worst = 2.0 ** -24, 0.0
    for t, ((flux, mv, total), (wflux, wmv, wtotal), tmv) in enumerate(zip(got, want, gt)):
        assert np.array_equal(mv, wmv), "FlowCounter.run and flow_host disagree on a motion byte of frame %d" % t
        assert np.array_equal(tmv, wmv), "the torch form and flow_host disagree on a motion byte of frame %d" % t
        _f, _t, n, ab, tabs = FL.flux_host(maps[INTERVAL + t], wmv, fc.placement, lines3, BAND, INTERVAL, members=True)
        bound = n * u * ab + np.spacing(np.abs(wflux).astype(np.float32))
        err = np.abs(flux.astype(np.float64) - wflux)
        assert (err <= bound).all(), "the flux of frame %d is outside the fp32-sum bound" % t
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    lines = ["flow: box %s, HEAD %s, %s" % (socket.gethostname(), args.head or head(root), torch.cuda.get_device_name(0)),
             "every call synchronised; forms alternated call by call, %d calls after %d warm-up calls (HOST: %d calls)" % (args.calls, args.warmup, args.host_calls),
             "(a) a group of %d frames of a synthetic clip at %d x %d (ten objects, 1..3 px/frame), search %d, interval %d, %d lines; HIP, HOST and "
             "TORCH agree on every motion byte; HIP's flux within the fp32-sum bound of HOST's (worst error / bound %.3f)"
             % (N, MH, MW, SEARCH, INTERVAL, len(lines3), worst)]
    times = {"HIP": [], "TORCH": [], "HOST": []}
    for it in range(args.warmup + args.calls):
        for k, fn in (("HIP", hip), ("TORCH", tor)):
            ms = timed(fn)[1]
            if it >= args.warmup:
                times[k].append(ms)
        if it < args.host_calls:
            times["HOST"].append(timed(host)[1])
    for name, note in (("HIP", "FlowCounter.run (luma, motion, flux, fold, one download)"), ("TORCH", "the SAD search as torch ops, motion only"),
                       ("HOST", "flow_host in numpy (motion and flux)")):
        lines.append("    %-6s %s  %s" % (name, spread(times[name]), note))
    # (b) what the flux adds to a group
    import models_mae_cross
    from countr_amd import YuvFrame, count_flow, count_frames
    rs = np.random.RandomState(0)
    torch.manual_seed(0)
    model = models_mae_cross.mae_vit_base_patch16(precision="bf16").to("cuda").eval()
    yy, xx = np.mgrid[0:H, 0:W]
    host8 = [YuvFrame((16 + 200 * ((yy / H + (xx + 3 * t) / W) / 2) + rs.randint(0, 20, (H, W))).astype(np.uint8),
                      rs.randint(64, 192, (H // 2, W)).astype(np.uint8)) for t in range(N)]
    counter = FlowCounter("cuda", lines=[(W / 2, -1.0, W / 2, H + 1.0), (-1.0, H / 2, W + 1.0, H / 2)])
    count = lambda: count_frames(model, host8, normalization=False)
    flow = lambda: count_flow(model, host8, lines=None, group=N, counter=counter, normalization=False)
    ref, (got, _counts) = count(), flow()
    for a, b in zip(got, ref):
        assert a[0] == b[0] and torch.equal(a[1], b[1]), "count_flow and count_frames disagree"
    times = {"FLOW": [], "COUNT": []}
    for it in range(args.warmup + args.calls):
        for k, fn in (("FLOW", flow), ("COUNT", count)):
            ms = timed(fn)[1]
            if it >= args.warmup:
                times[k].append(ms)
    lines.append("(b) eight 1920x1080 NV12 frames in host memory, ViT-B bf16, zero-shot, one group of eight, two lines, search 4, interval 1; "
                 "count_flow's counts and maps equal count_frames'")
    lines.append("    FLOW      %s  count_flow (a counter kept across calls)" % spread(times["FLOW"]))
    lines.append("    COUNT     %s  count_frames alone" % spread(times["COUNT"]))
    lines.append("    the flux adds FLOW - COUNT = %+.3f ms per group of eight" % (float(np.median(times["FLOW"])) - float(np.median(times["COUNT"]))))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
