"""The camera's own motion (countr_amd/cam.py): what the estimate and the compensation cost on the device, what the second
synchronisation costs a chunk, and what camera="translation" adds to count_flow.

  (a) a synthetic panned clip (countr_amd.cam.pan_scene at the size of a 1080p frame's map, 384 x 672, six objects, pan (1.3, 0.4) +- 0.3),
      nine frames = one frame of history and a group of eight, search 6, interval 1, three lines:
        ON      FlowCounter(camera="translation").run of the group: luma, motion, estimate, a download and a wait, compensate, flux, fold,
                a download and a wait
        OFF     FlowCounter().run of the same group: the path without the feature, the baseline
  (b) the estimate alone on those eight (field, luma) pairs:
        HIP     countr_cam_estimate (a memset and two launches) and the download of the eight records
        TORCH   the same estimate as torch ops on the device (gradient sums, boolean masks, kthvalue), records downloaded
        HOST    camera_host's estimate in numpy
      Before anything is timed HIP, TORCH and HOST agree on every record.
  (c) eight 1920x1080 NV12 frames in HOST memory, ViT-B bf16, zero-shot: count_flow with the camera on against off (a counter kept across
      calls); counts and maps are equal.
Every call ends in a device synchronise; the forms are alternated call by call; the figure is the median after --warmup calls, with the
quartiles and the extremes as the spread.  No threshold: whatever comes out is the record.  The clips are synthetic: no figure on real
moving-camera video exists.

    python tools/bench_cam.py [--calls 30] [--warmup 5] [--out profiles/cam.txt] [--head <commit>]"""
import argparse
import ctypes as C
import os
import socket
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from countr_amd import CameraEstimator, FlowCounter
from countr_amd import cam as CM, flow as FL

H, W, N = 1080, 1920, 8
MH, MW = 384, 672
SEARCH, INTERVAL, BAND = 6, 1, 8.0 * H / 384
SET = (128, 8, 16)


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


def estimate_torch(V, L, min_texture, tol, min_voters):
    """cam.estimate_host with torch ops on the device: V int16 [h / 8, w / 8, 2], L uint8 [h, w] device tensors -> record (a list)."""
    h, w = L.shape
    v = L.to(torch.int32)
    right, below = torch.cat([v[:, 1:], v[:, -1:]], 1), torch.cat([v[1:], v[-1:]], 0)
    T = ((right - v).abs() + (below - v).abs()).reshape(h // 8, 8, w // 8, 8).sum((1, 3))
    Vi = V.to(torch.int32)
    votes = (T >= min_texture) & (Vi.abs() <= CM.RANGE).all(-1)
    ox, oy = Vi[..., 0][votes], Vi[..., 1][votes]
    n = int(ox.numel())
    gx = gy = inliers = 0
    if n:
        rank = (n + 1) // 2
        gx, gy = int(ox.kthvalue(rank).values), int(oy.kthvalue(rank).values)
        inliers = int((((ox - gx).abs() <= tol) & ((oy - gy).abs() <= tol)).sum())
    valid = n >= min_voters and 2 * inliers >= n
    return [gx if valid else 0, gy if valid else 0, n, inliers, int(valid), T.numel(), 0, 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--head", default="")
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lumas, maps, lines3, _truth, _c = CM.pan_scene(h=MH, w=MW, objects=6, frames=N + INTERVAL, seed=0, pan=(1.3, 0.4), jitter=0.3)
    placement = (W / MW, 0.5 * W / MW - 0.5, H / MH, 0.5 * H / MH - 0.5)
    lines3 = (np.asarray(lines3, np.float64) * (placement[0::2] * 2) + (placement[1::2] * 2)).astype(np.float32)      # map pixels -> frame pixels
    images = [torch.from_numpy(FL.image_of_luma(l)).cuda() for l in lumas]
    dmaps = [torch.from_numpy(m).cuda() for m in maps]
    kw = dict(lines=lines3, search=SEARCH, interval=INTERVAL, min_gain=256, band=BAND)
    counters = {"ON": FlowCounter("cuda", camera="translation", **kw), "OFF": FlowCounter("cuda", **kw)}
    for fc in counters.values():
        fc.run(images[:INTERVAL], [None] * INTERVAL, [(W, H)] * INTERVAL)                        # the history
    run = lambda k: counters[k].run(images[INTERVAL:], dmaps[INTERVAL:], [(W, H)] * N, motion=True)
    # ---- the three forms of the estimate agree before anything is timed
    fields = [mv for _f, mv, _t in run("OFF")]
    run("ON")
    want = np.stack([CM.estimate_host(V, L, *SET)[0] for V, L in zip(fields, lumas[INTERVAL:])])
    assert np.array_equal(counters["ON"].camera_path().records[INTERVAL:INTERVAL + N], want), "FlowCounter's records and the host rule disagree"
    dv, dl = [torch.from_numpy(V).cuda() for V in fields], [torch.from_numpy(L).cuda() for L in lumas[INTERVAL:]]
    est = CameraEstimator("cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    pv, pl = [t.data_ptr() for t in dv], [t.data_ptr() for t in dl]

    def hip():
        est.launch(pv, pl, MH, MW, st)
        return est.records[:N].cpu().numpy()

    tor = lambda: np.array([estimate_torch(V, L, *SET) for V, L in zip(dv, dl)], np.int32)
    host = lambda: np.stack([CM.estimate_host(V, L, *SET)[0] for V, L in zip(fields, lumas[INTERVAL:])])
    assert np.array_equal(hip(), want), "countr_cam_estimate and the host rule disagree on a record"
    assert np.array_equal(tor(), want), "the torch form and the host rule disagree on a record"
    lines = ["cam: box %s, HEAD %s, %s" % (socket.gethostname(), args.head or head(root), torch.cuda.get_device_name(0)),
             "every call synchronised; forms alternated call by call, %d calls after %d warm-up calls" % (args.calls, args.warmup),
             "(a) FlowCounter.run on a group of %d frames of a synthetic panned clip at %d x %d (six objects, pan (1.3, 0.4) +- 0.3 px/frame), "
             "search %d, interval %d, %d lines, motion fields downloaded; the records equal the host rule's; estimated g of the eight frames: %s"
             % (N, MH, MW, SEARCH, INTERVAL, len(lines3), want[:, :2].tolist())]

    def alternate(forms):
        times = {k: [] for k, _fn in forms}
        for it in range(args.warmup + args.calls):
            for k, fn in forms:
                ms = timed(fn)[1]
                if it >= args.warmup:
                    times[k].append(ms)
        return times

    times = alternate((("ON", lambda: run("ON")), ("OFF", lambda: run("OFF"))))
    lines.append("    ON     %s  camera=\"translation\": two downloads and two waits a chunk" % spread(times["ON"]))
    lines.append("    OFF    %s  camera=None: the path without the feature" % spread(times["OFF"]))
    lines.append("    the camera adds ON - OFF = %+.3f ms per group of eight: the estimate, the compensation and the second synchronisation"
                 % (float(np.median(times["ON"])) - float(np.median(times["OFF"]))))
    times = alternate((("HIP", hip), ("TORCH", tor), ("HOST", host)))
    lines.append("(b) the estimate of those eight (field, luma) pairs alone, eight records downloaded; HIP, TORCH and HOST agree on every record")
    for name, note in (("HIP", "countr_cam_estimate: a memset and two launches"), ("TORCH", "gradient sums, masks and kthvalue as torch ops"),
                       ("HOST", "estimate_host in numpy")):
        lines.append("    %-6s %s  %s" % (name, spread(times[name]), note))
    # ---- (c) what the camera adds to count_flow
    import models_mae_cross
    from countr_amd import YuvFrame, count_flow
    rs = np.random.RandomState(0)
    torch.manual_seed(0)
    model = models_mae_cross.mae_vit_base_patch16(precision="bf16").to("cuda").eval()
    yy, xx = np.mgrid[0:H, 0:W]
    tex = lambda X, Y: 128 + 40 * np.sin(X / 9.0) * np.cos(Y / 13.0) + 40 * np.sin((X + 2 * Y) / 31.0)
    host8 = [YuvFrame((tex(xx + 4 * t, yy + t) + rs.randint(0, 6, (H, W))).clip(0, 255).astype(np.uint8), np.full((H // 2, W), 128, np.uint8))
             for t in range(N)]
    two = [(W / 2, -1.0, W / 2, H + 1.0), (-1.0, H / 2, W + 1.0, H / 2)]
    con, coff = FlowCounter("cuda", lines=two, camera="translation"), FlowCounter("cuda", lines=two)
    on = lambda: count_flow(model, host8, lines=None, group=N, counter=con, normalization=False)
    off = lambda: count_flow(model, host8, lines=None, group=N, counter=coff, normalization=False)
    (a, _ca), (b, _cb) = on(), off()
    for x, y in zip(a, b):
        assert x[0] == y[0] and torch.equal(x[1], y[1]), "count_flow with and without the camera disagree on a count or a map"
    times = alternate((("ON", on), ("OFF", off)))
    lost = con.camera_path().lost
    lines.append("(c) count_flow on eight 1920x1080 NV12 frames in host memory (a texture panned by (4, 1) px a frame), ViT-B bf16, zero-shot, one "
                 "group of eight, two lines, search 4, interval 1; counts and maps equal with and without the camera; %d estimates lost" % lost)
    lines.append("    ON     %s  camera=\"translation\"" % spread(times["ON"]))
    lines.append("    OFF    %s  camera=None" % spread(times["OFF"]))
    lines.append("    the camera adds ON - OFF = %+.3f ms per group of eight" % (float(np.median(times["ON"])) - float(np.median(times["OFF"]))))
    lines.append("The clips are synthetic; no figure on real moving-camera video exists, and min_texture, tol and min_voters are unmeasured there.")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
