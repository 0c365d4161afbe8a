"""Raw frames -> counts: what the preparation costs in front of the forward (bf16, eight 1920x1080 frames = 32 windows per group).

  A  host preparation: PIL resize + ToTensor per frame on the host, .to(device), inference.count_images
  B  count_frames from host frames: pinned copy + device resize (countr_frame_resize_u8)
  C  count_frames from frames already on the device
plus the two kernels alone (events around 50 launches).  Wall time per group over --groups groups after warm-up, one
synchronisation at the end (the counts themselves are read back per image in all three forms, as the callers do).

    python tools/bench_frames.py [--groups 10] [--out profiles/frames_prep.txt] [--head <commit>]"""
import argparse
import os
import socket
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from PIL import Image

import models_mae_cross
from countr_amd import frames as FR, inference


def head(root):
    try:
        return subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=root, stderr=subprocess.DEVNULL, text=True).strip()
    except Exception:
        return "unknown"


def host_items(raw):
    items = []
    for f in raw:
        H, W = f.shape[:2]
        im = Image.fromarray(f).resize((FR.new_width(W, H), 384), Image.BILINEAR)
        t = torch.from_numpy(np.asarray(im, dtype=np.uint8).copy()).permute(2, 0, 1).float().div(255.0)
        items.append((t.unsqueeze(0).to("cuda", non_blocking=True), torch.Tensor([]).unsqueeze(0).to("cuda"), None))
    return items


def timed(fn, groups, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(groups):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / groups * 1e3


def kernel_ms(fn, n=50):
    for _ in range(5):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=10)
    ap.add_argument("--out", default="")
    ap.add_argument("--head", default="")
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    torch.manual_seed(0)
    model = models_mae_cross.mae_vit_base_patch16(precision="bf16").to("cuda").eval()
    rs = np.random.RandomState(0)
    raw = [rs.randint(0, 256, size=(1080, 1920, 3)).astype(np.uint8) for _ in range(8)]
    dev = [torch.from_numpy(f).cuda() for f in raw]
    lines = ["frames_prep: box %s, HEAD %s, %s" % (socket.gethostname(), args.head or head(root), torch.cuda.get_device_name(0)),
             "eight 1920x1080 uint8 frames -> 8 counts (zero-shot, bf16, 32 windows in one forward), ms per group over %d groups" % args.groups]
    t0 = time.perf_counter()
    for f in raw:
        Image.fromarray(f).resize((672, 384), Image.BILINEAR)
    lines.append("PIL resize alone on this box's host: %.2f ms per frame" % ((time.perf_counter() - t0) / 8 * 1e3))
    a = timed(lambda: inference.count_images(model, host_items(raw), normalization=False), args.groups)
    b = timed(lambda: FR.count_frames(model, raw, normalization=False), args.groups)
    c = timed(lambda: FR.count_frames(model, dev, normalization=False), args.groups)
    prepared = FR.frame_prep("cuda").prepare(dev)
    items = [(im, torch.zeros(1, 0, device="cuda"), None) for im in prepared]
    fwd = timed(lambda: inference.count_images(model, items, normalization=False), args.groups)
    lines += ["A  PIL on the host + count_images      %8.2f ms" % a,
              "B  count_frames, frames on the host     %8.2f ms" % b,
              "C  count_frames, frames on the device   %8.2f ms" % c,
              "-  count_images on prepared tensors     %8.2f ms  (no preparation at all)" % fwd]
    prep = FR.frame_prep("cuda")
    k8 = kernel_ms(lambda: prep.prepare(dev))
    k1 = kernel_ms(lambda: prep.prepare(dev[:1]))
    moved = 8 * (1080 * 1920 * 3 + 2 * 1080 * 672 * 3 + 384 * 672 * 3 * 4) / 1e6
    lines.append("countr_frame_resize_u8: 8 frames %.1f us (%.0f MB moved: %.2f TB/s), 1 frame %.1f us  (call included: output allocation + launch pair)"
                 % (k8 * 1e3, moved, moved / 1e6 / (k8 / 1e3), k1 * 1e3))
    im = prepared[0]
    rects = [[34, 47, 45, 60], [44, 73, 53, 84], [59, 74, 71, 90]]
    kc = kernel_ms(lambda: FR.crop_resize(im, rects, 64, 64))
    ks = kernel_ms(lambda: FR.crop_resize(im, FR.split_rects(384, 672), 384, 672))
    lines.append("countr_crop_resize_f32: 3 exemplars 64x64 %.1f us, nine 384x672 split crops %.1f us" % (kc * 1e3, ks * 1e3))
    lines.append("B %s A: %s" % ("<" if b < a else ">=", "the device preparation is the faster front end" if b < a else
                                   "the device preparation did NOT beat the host path in this run"))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
