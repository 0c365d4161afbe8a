"""What FSC_test_cross.py --report costs beside the forward: per group of 8 synthetic 384 x 1360 images (3 exemplars each, fp32, 9 windows
per image), the median of --groups groups after --warmup warm-ups of

  a  inference.count_images alone (with return_crops=True, synchronised)
  b  a + ReportWriter.add_group up to the end of the download (the pictures are in pinned host memory); the encodes it submitted
     finish before the next timed group starts
  c  a + add_group + the PNG encodes (flush): end to end
  d  a + the same panels through compose_host on the device tensors (torch ops, one download per image), no encode

Each group is synchronised before the next starts, so c has nothing to overlap with: in the CLI the encodes run beside the next
group's forward.  Wall time on the host.

    python tools/bench_report.py [--groups 20] [--warmup 3] [--workers 4] [--out profiles/report.txt] [--head <commit>]"""
import argparse
import os
import shutil
import socket
import statistics
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import models_mae_cross
from countr_amd import inference, report


def head(root):
    try:
        return subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=root, stderr=subprocess.DEVNULL, text=True).strip()
    except Exception:
        return "unknown"


def median_ms(fn, groups, warmup, after=None):
    """Median / min / max wall time of fn over `groups` calls; `after` runs between the calls, outside the timed region."""
    times = []
    for k in range(warmup + groups):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if k >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
        if after is not None:
            after()
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--out", default="")
    ap.add_argument("--head", default="")
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    torch.manual_seed(0)
    model = models_mae_cross.mae_vit_base_patch16(precision="fp32").to("cuda").eval()
    rs = np.random.RandomState(0)
    h, w, n = 384, 1360, 8
    items, its = [], []
    for k in range(n):
        sam = torch.from_numpy(rs.uniform(0, 1, size=(1, 3, h, w)).astype(np.float32)).cuda()
        boxes = torch.from_numpy(rs.uniform(0, 1, size=(1, 3, 3, 64, 64)).astype(np.float32)).cuda()
        pos = [(10 * j, 10 * j, 10 * j + 40, 10 * j + 40) for j in range(3)]
        gt = torch.from_numpy(rs.uniform(0, 1, size=(h, w)).astype(np.float32))        # on the host, as the loader hands it over
        items.append(report.ReportItem("bench_%d" % k, sam, boxes, pos, 20 + k, gt))
        its.append((sam, boxes, pos))
    out_dir = tempfile.mkdtemp(prefix="countr_report_")
    wr = report.ReportWriter(out_dir, workers=args.workers)

    def count():
        res = inference.count_images(model, its, normalization=True, return_crops=True)
        torch.cuda.synchronize()
        return res

    def to_download():
        wr.add_group(items, count())
        wr.wait_download()

    def end_to_end():
        wr.add_group(items, count())
        wr.flush()

    def host_statement():
        for it, (pred, dm, _c) in zip(items, count()):
            report.compose_host(it.sample, dm, it.gt_map, it.pos, it.gt_cnt, pred)

    rows = [("a  count_images alone", count), ("b  + add_group up to the end of the download", to_download),
            ("c  + add_group + PNG encodes (flush)", end_to_end), ("d  + compose_host on the device tensors, no encode", host_statement)]
    lines = ["report: box %s, HEAD %s, %s" % (socket.gethostname(), args.head or head(root), torch.cuda.get_device_name(0)),
             "8 synthetic 384 x 1360 images per group (3 exemplars, fp32, %d windows), %d encode threads; ms per group, median (min .. max) of %d groups after %d warm-ups"
             % (n * len(inference.window_starts(w)), wr.pool._max_workers, args.groups, args.warmup)]
    got = {}
    for label, fn in rows:
        med, lo, hi = median_ms(fn, args.groups, args.warmup, after=wr.flush)      # (b: the encodes finish outside the timed region)
        got[label[0]] = med
        lines.append("%-52s %9.2f  (%.2f .. %.2f)" % (label, med, lo, hi))
    med, lo, hi = median_ms(lambda: [report.raster_patch(report.label_raster(w, h, it.gt_cnt, 12.345)) for it in items], args.groups, args.warmup)
    lines.append("%-52s %9.2f  (%.2f .. %.2f)" % ("-  the 8 label rasters alone (PIL, host; in b, c and d)", med, lo, hi))
    lines.append("b - a = %.2f ms, c - a = %.2f ms, d - a = %.2f ms per group of 8" % (got["b"] - got["a"], got["c"] - got["a"], got["d"] - got["a"]))
    wr.close()
    shutil.rmtree(out_dir, ignore_errors=True)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
