"""What summing density maps over regions costs: per call of eight synthetic 384 x 1360 maps (one set each, identity placement), every
call synchronised, in two forms -- (a) sixteen 8-vertex polygons per map, (b) the GAME(3) grid (8 x 8 cells) -- the median wall time of

  1  RegionSummer.sum (csrc_ext/regions.hip: one packed upload, two launches, one download, one synchronisation)
  2  regions_host on the downloaded maps (numpy: membership in float64, sums in float64); the download is inside the timed part
  3  torch on the device: einsum of the maps against boolean masks [regions, h, w] rasterised ONCE on the host by the same rule and
     uploaded before anything is timed -- mask building is NOT inside the timed part; the timed part is the einsum, the download of
     its [8, regions] result and the synchronisation

Before anything is timed the three must agree on every area exactly and on every mass within the bound of the tests
(n 2^-24 sum|v| over the n member pixels, plus one ulp).  Wall time on the host.

    python tools/bench_regions.py [--calls 50] [--host_calls 3] [--warmup 3] [--out profiles/regions.txt] [--head <commit>]"""
import argparse
import os
import socket
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from bench_report import head, median_ms
from countr_amd import regions
from countr_amd.regions import RegionSummer, regions_host

H, W, N = 384, 1360, 8
IDENT = (1.0, 0.0, 1.0, 0.0)


def octagons(seed):
    """Sixteen 8-vertex polygons spread over the frame, some hanging over its edges."""
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(16):
        cx, cy, r = rs.uniform(0, W), rs.uniform(0, H), rs.uniform(40, 200)
        ang = np.sort(rs.uniform(0, 2 * np.pi, 8))
        rad = r * rs.uniform(0.5, 1.0, 8)
        out.append(np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], 1))
    return out


def masks_of(regs):
    """bool [slots, H, W] by the rule, on the host."""
    x, y = regions.centres((H, W), IDENT)
    out = []
    for r in (regions.region(r) for r in regs):
        if isinstance(r, tuple):
            i, j = regions.grid_cells(x, y, r[1], r[2])
            for ci in range(r[1].size - 1):
                for cj in range(r[2].size - 1):
                    out.append((i == ci)[:, None] & (j == cj)[None, :])
        else:
            out.append(regions.inside_polygon(x, y, r))
    return np.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--host_calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--head", default="")
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rs = np.random.RandomState(0)
    maps_np = [(rs.uniform(0, 1, (H, W)) ** 8 * 0.5).astype(np.float32) for _ in range(N)]
    maps = [torch.from_numpy(m).cuda() for m in maps_np]
    stack = torch.stack(maps)
    summer = RegionSummer("cuda")
    lines = ["regions: box %s, HEAD %s, %s" % (socket.gethostname(), args.head or head(root), torch.cuda.get_device_name(0)),
             "%d maps of %d x %d per call, one set each; ms per call, median (min .. max) of %d calls (row 2: %d) after %d warm-ups (row 2: 1); "
             "row 3's masks are built and uploaded before the timed part" % (N, H, W, args.calls, args.host_calls, args.warmup)]
    for label, sets in (("(a) sixteen 8-vertex polygons per map", [octagons(k) for k in range(N)]),
                        ("(b) the GAME(3) grid, 8 x 8 cells per map", [[regions.game_grid(H, W, 3)] for _ in range(N)])):
        som = list(range(N))
        masks = torch.from_numpy(np.stack([masks_of(rs_) for rs_ in sets])).cuda()        # [N, slots, H, W]
        fmasks = masks.float()
        got = summer.sum(maps, [IDENT] * N, som, sets)
        host = regions_host(maps_np, [IDENT] * N, sets, som, members=True)
        dev = torch.einsum("nhw,nrhw->nr", stack, fmasks).cpu().numpy()
        dev_area = masks.sum(dim=(2, 3)).cpu().numpy()
        u = 2.0 ** -24
        for k in range(N):
            wm, wa, _wt, wabs, _tabs = host[k]
            bound = wa * u * wabs + np.spacing(np.abs(wm).astype(np.float32))
            if not (np.array_equal(got[k][1], wa) and np.array_equal(dev_area[k], wa)):
                raise SystemExit("bench_regions: the areas differ at %s, map %d" % (label, k))
            if not ((np.abs(got[k][0] - wm) <= bound).all() and (np.abs(dev[k] - wm) <= bound).all()):
                raise SystemExit("bench_regions: a mass is outside the bound at %s, map %d" % (label, k))
        lines.append("%s: %d slots per map, %d member pixels per map on average; the three agree on every area and on every mass within the bound"
                     % (label, len(host[0][0]), int(np.mean([h[1].sum() for h in host]))))
        ms = {}
        for key, what, fn, calls, warm in (
                ("1", "RegionSummer.sum", lambda: summer.sum(maps, [IDENT] * N, som, sets), args.calls, args.warmup),
                ("2", "download + regions_host (numpy)", lambda: regions_host([m.cpu().numpy() for m in maps], [IDENT] * N, sets, som), args.host_calls, 1),
                ("3", "torch einsum against prebuilt masks + download", lambda: torch.einsum("nhw,nrhw->nr", stack, fmasks).cpu(), args.calls, args.warmup)):
            med, lo, hi = median_ms(fn, calls, warm)
            ms[key] = med
            lines.append("  %s  %-48s %10.3f  (%.3f .. %.3f)" % (key, what, med, lo, hi))
        lines.append("  2 / 1 = %.1f, 3 / 1 = %.2f" % (ms["2"] / ms["1"], ms["3"] / ms["1"]))
        del masks, fmasks
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
