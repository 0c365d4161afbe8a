"""What matching predicted points to dots costs: per call of eight sets of uniform random points in a 384 x 1360 field (max_dist 16), the
median wall time of

  a  PointMatcher.match (csrc/match.hip: one upload, two launches, one download, one synchronisation)
  b  match_host: all pairs in numpy, one stable sort of the eligible ones, the sequential greedy pass
  c  scipy cKDTree candidate pairs (query_ball_tree), then the same fp32 keys, sort and greedy pass on the host

at ~140 x ~140 points (an FSC147 image), ~1000 x ~1000 and 4096 x 4096 per set, plus row a alone at 4096 x 4096 with every pair eligible
(max_dist 2000: the case the rounds structure likes least).  The three must agree on every match before anything is timed.  Every call is
synchronised before the next starts (tools/bench_report.py's median_ms).  Wall time on the host.

    python tools/bench_match.py [--calls 50] [--host_calls 5] [--warmup 3] [--out profiles/match.txt] [--head <commit>]"""
import argparse
import os
import socket
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from bench_report import head, median_ms
from countr_amd.match import PointMatcher, match_host

H, W, N = 384, 1360, 8
MAX_DIST = 16.0


def point_sets(p, g, spread, seed, max_dist=MAX_DIST):
    rs = np.random.RandomState(seed)
    sets = []
    for _ in range(N):
        P, G = p + int(rs.randint(-spread, spread + 1)), g + int(rs.randint(-spread, spread + 1))
        sets.append(((rs.uniform(0, 1, (P, 2)) * [W, H]).astype(np.float32), (rs.uniform(0, 1, (G, 2)) * [W, H]).astype(np.float32), max_dist))
    return sets


def match_kdtree(pred, gt, max_dist):
    """The rule with its candidate pairs from a k-d tree instead of all pairs: the tree's float64 radius is a hair wider than max_dist, the
    fp32 key then decides as the rule says."""
    from scipy.spatial import cKDTree
    md2 = np.float32(max_dist) * np.float32(max_dist)
    match, out = np.full(len(pred), -1, np.int32), np.full(len(pred), np.inf, np.float32)
    if not len(pred) or not len(gt):
        return match, out
    near = cKDTree(pred).query_ball_tree(cKDTree(gt), r=float(max_dist) * (1 + 1e-5))
    ii = np.repeat(np.arange(len(pred)), [len(c) for c in near])
    jj = np.fromiter((j for c in near for j in sorted(c)), np.int64, len(ii))
    dx, dy = pred[ii, 0] - gt[jj, 0], pred[ii, 1] - gt[jj, 1]
    d2 = dx * dx + dy * dy
    ok = d2 <= md2
    ii, jj, d2 = ii[ok], jj[ok], d2[ok]
    order = np.argsort(d2, kind="stable")
    taken = np.zeros(len(gt), bool)
    for i, j, d in zip(ii[order].tolist(), jj[order].tolist(), d2[order].tolist()):
        if match[i] < 0 and not taken[j]:
            match[i], out[i], taken[j] = j, d, True
    return match, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--host_calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--head", default="")
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pm = PointMatcher("cuda")
    lines = ["match: box %s, HEAD %s, %s" % (socket.gethostname(), args.head or head(root), torch.cuda.get_device_name(0)),
             "%d sets per call, uniform random points in a %d x %d field, max_dist %g; ms per call, median (min .. max) of %d calls (rows b, c: %d) "
             "after %d warm-ups (rows b, c: 1)" % (N, H, W, MAX_DIST, args.calls, args.host_calls, args.warmup)]
    for label, p, g, spread in (("~140 x ~140", 140, 140, 20), ("~1000 x ~1000", 1000, 1000, 100), ("4096 x 4096", 4096, 4096, 0)):
        sets = point_sets(p, g, spread, seed=p)
        got = pm.match(sets)
        host = [match_host(*s) for s in sets]
        tree = [match_kdtree(*s) for s in sets]
        same = all(np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes() and np.array_equal(a[0], c[0]) and a[1].tobytes() == c[1].tobytes()
                   for a, b, c in zip(got, host, tree))
        if not same:
            raise SystemExit("bench_match: the three matchings differ at %s" % label)
        lines.append("%s points per set, %s pairs matched per set; the three agree on every match and every d2 bit: %s"
                     % (label, "/".join(str(c) for _m, _d, c in got), same))
        ms = {}
        for key, what, fn, calls, warm in (("a", "PointMatcher.match", lambda: pm.match(sets), args.calls, args.warmup),
                                           ("b", "match_host (numpy all pairs + sort + greedy)", lambda: [match_host(*s) for s in sets], args.host_calls, 1),
                                           ("c", "cKDTree candidates + sort + greedy on the host", lambda: [match_kdtree(*s) for s in sets], args.host_calls, 1)):
            med, lo, hi = median_ms(fn, calls, warm)
            ms[key] = med
            lines.append("  %s  %-48s %10.3f  (%.3f .. %.3f)" % (key, what, med, lo, hi))
        lines.append("  b / a = %.1f, c / a = %.1f" % (ms["b"] / ms["a"], ms["c"] / ms["a"]))
    sets = point_sets(4096, 4096, 0, seed=7, max_dist=2000.0)
    got = pm.match(sets)
    med, lo, hi = median_ms(lambda: pm.match(sets), max(args.calls // 5, 5), 1)
    lines.append("4096 x 4096 points per set, max_dist 2000 (every pair eligible), %s pairs matched per set; rows b and c not run (16.8 M pairs per set to sort)"
                 % "/".join(str(c) for _m, _d, c in got))
    lines.append("  a  %-48s %10.3f  (%.3f .. %.3f)" % ("PointMatcher.match", med, lo, hi))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
