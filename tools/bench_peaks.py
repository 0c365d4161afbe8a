"""What locating the objects costs beside counting them: per call of eight synthetic 384 x 1360 density maps (sums of Gaussians + noise, on
the device), the median of --calls calls after --warmup warm-ups of

  a  PeakFinder.find (csrc/peaks.hip: four launches, one download, one synchronisation; radius 4, rel_threshold 0.1, 4096 points)
  b  the same peaks written as torch ops on the device: max_pool2d over the (2 r + 1)^2 window, compare, nonzero, download, host sort by
     (score descending, idx ascending).  No plateau rule (a plateau yields every pixel) and no centroid: it does less
  c  inference.count_images alone on eight 384 x 1360 images (zero-shot, bf16), for scale

Every call is synchronised before the next starts (tools/bench_report.py's median_ms).  Wall time on the host.

    python tools/bench_peaks.py [--calls 50] [--warmup 5] [--out profiles/peaks.txt] [--head <commit>]"""
import argparse
import os
import socket
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
import torch.nn.functional as F

import models_mae_cross
from bench_report import head, median_ms
from countr_amd import inference
from countr_amd.peaks import PeakFinder

H, W, N = 384, 1360, 8
RADIUS, REL, CAP = 4, 0.1, 4096


def synthetic_maps(seed=0, blobs=150):
    g = torch.Generator(device="cuda").manual_seed(seed)
    yy = torch.arange(H, device="cuda", dtype=torch.float32)[:, None]
    xx = torch.arange(W, device="cuda", dtype=torch.float32)[None, :]
    maps = []
    for _ in range(N):
        p = torch.rand(blobs, 4, device="cuda", generator=g)
        d = (torch.rand(H, W, device="cuda", generator=g) - 0.5) * 0.04
        for cy, cx, sg, amp in p.tolist():
            sg = 2 + 2 * sg
            d += (0.2 + 2.8 * amp) * torch.exp(-((yy - cy * H) ** 2 + (xx - cx * W) ** 2) / (2 * sg * sg))
        maps.append(d.contiguous())
    return maps


def torch_peaks(maps):
    d = torch.stack(maps).unsqueeze(1)
    top = d.amax(dim=(2, 3), keepdim=True)
    pooled = F.max_pool2d(d, 2 * RADIUS + 1, stride=1, padding=RADIUS)
    hit = (d == pooled) & (d > 0.0) & (d >= REL * top)
    idx = hit.nonzero()                                   # (the synchronisation the home-made path pays)
    score = d[hit]
    idx, score = idx.cpu().numpy(), score.cpu().numpy()
    out = []
    for i in range(len(maps)):
        sel = idx[:, 0] == i
        lin = idx[sel, 2] * W + idx[sel, 3]
        order = np.lexsort((lin, -score[sel]))[:CAP]
        out.append((lin[order], score[sel][order]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--head", default="")
    args = ap.parse_args()
    if args.calls < 50:
        raise SystemExit("bench_peaks: at least 50 calls per row")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    maps = synthetic_maps()
    pf = PeakFinder("cuda")
    found = pf.find(maps, RADIUS, 0.0, REL, CAP)
    ref = torch_peaks(maps)
    same = all(np.array_equal(pk.yx[:, 0].astype(np.int64) * W + pk.yx[:, 1], lin) for pk, (lin, _s) in zip(found, ref))
    torch.manual_seed(0)
    model = models_mae_cross.mae_vit_base_patch16(precision="bf16").to("cuda").eval()
    rs = np.random.RandomState(0)
    items = [(torch.from_numpy(rs.uniform(0, 1, size=(1, 3, H, W)).astype(np.float32)).cuda(), torch.zeros(1, 0, device="cuda"), None)
             for _ in range(N)]

    def count():
        inference.count_images(model, items, normalization=False)
        torch.cuda.synchronize()

    rows = [("a  PeakFinder.find", lambda: pf.find(maps, RADIUS, 0.0, REL, CAP)),
            ("b  torch ops: max_pool2d, compare, nonzero, host sort", lambda: torch_peaks(maps)),
            ("c  count_images alone (zero-shot, bf16)", count)]
    lines = ["peaks: box %s, HEAD %s, %s" % (socket.gethostname(), args.head or head(root), torch.cuda.get_device_name(0)),
             "%d synthetic %d x %d maps per call, radius %d, rel_threshold %g, max_points %d, %s peaks per map; ms per call, median (min .. max) of %d calls after %d warm-ups"
             % (N, H, W, RADIUS, REL, CAP, "/".join(str(pk.total) for pk in found), args.calls, args.warmup),
             "the torch formulation finds the same pixels: %s" % same]
    got = {}
    for label, fn in rows:
        med, lo, hi = median_ms(fn, args.calls, args.warmup)
        got[label[0]] = med
        lines.append("%-56s %9.3f  (%.3f .. %.3f)" % (label, med, lo, hi))
    lines.append("b / a = %.2f, a / c = %.2f %% of the forward" % (got["b"] / got["a"], 100 * got["a"] / got["c"]))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
