"""What a second, fourth or eighth class per frame costs: mae_vit_base_patch16 in bf16 (randomly initialised), eight synthetic
1920 x 1080 frames on the device per call (32 windows, one forward batch), C classes of three exemplar boxes each, every call
synchronised; the median wall time per call of

  1  count_classes(fold=False)      one encoder forward, C class-dependent tails
  2  count_classes(fold=True)       the same plus the fold (csrc_classes/classes.hip)
  3  C successive count_frames      C full forwards

for C in {1, 2, 4, 8}, all in this process and this run.  At C = 1 rows 1 and 3 run the same launches: their difference is the noise
floor against which to read the other rows.  Before anything is timed, counts and maps of the two paths must be equal bit for bit.
Then, at C = 8, the fold alone for the call's eight frames: ClassFolder.fold (one upload, two launches, one download, one
synchronisation) against the same fold as torch ops on the device (stack, max, masked sums; the sums are downloaded and the labels stay
on the device, as ClassFolder leaves them).

    python tools/bench_classes.py [--calls 30] [--warmup 5] [--out profiles/classes.txt] [--head <commit>]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

import models_mae_cross
from bench_report import head, median_ms
from countr_amd import count_classes, count_frames
from countr_amd.classes import ClassFolder

FRAMES, H, W = 8, 1080, 1920


def boxes_of(c):
    """Three 150-px exemplar boxes per frame for class c (53 px after the resize: the plain path), shifted per class and per frame."""
    return [[(100 + 40 * c + 10 * f + 400 * k, 200 + 30 * c + 150 * k, 250 + 40 * c + 10 * f + 400 * k, 350 + 30 * c + 150 * k) for k in range(3)]
            for f in range(FRAMES)]


def torch_fold(maps, scale, floor):
    """The fold as torch ops: maps [[h, w] per class] per frame, scale [F, C] -> labels on the device, won, total, area on the host.
    (torch.max does not promise the lowest index on ties: this row is timed, not compared.)"""
    maps = torch.stack([torch.stack(m) for m in maps])
    v = maps * scale[:, :, None, None]
    best, lab = v.max(dim=1)
    lab = torch.where(best <= floor, torch.full_like(lab, 255), lab).to(torch.uint8)
    mine = lab[:, None] == torch.arange(maps.shape[1], device=maps.device, dtype=torch.uint8)[None, :, None, None]
    won = (v * mine).sum(dim=(2, 3))
    return lab, won.cpu(), v.sum(dim=(2, 3)).cpu(), mine.sum(dim=(2, 3)).cpu()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--head", default="")
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    torch.manual_seed(0)
    model = models_mae_cross.__dict__["mae_vit_base_patch16"](norm_pix_loss="store_true", precision="bf16").to("cuda").eval()
    frames = [torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(FRAMES)]
    lines = ["classes: HEAD %s, %s" % (args.head or head(root), torch.cuda.get_device_name(0)),
             "mae_vit_base_patch16 bf16, %d frames of %d x %d on the device per call (32 windows), 3-shot classes; ms per call, median (min .. max) "
             "of %d synchronised calls after %d warm-ups" % (FRAMES, W, H, args.calls, args.warmup)]

    def synced(fn):
        def run():
            fn()
            torch.cuda.synchronize()
        return run

    last = None
    for C_ in (1, 2, 4, 8):
        classes = {"class%d" % c: boxes_of(c) for c in range(C_)}
        shared = count_classes(model, frames, classes, fold=True)
        for c, name in enumerate(classes):
            for f, (cnt, dm) in enumerate(count_frames(model, frames, classes[name])):
                if not (shared[f].counts[c] == cnt and torch.equal(shared[f].maps[c], dm)):
                    raise SystemExit("bench_classes: count_classes and count_frames differ at C = %d, class %d, frame %d" % (C_, c, f))
        ms = {}
        for key, fn in (("1", lambda: count_classes(model, frames, classes, fold=False)),
                        ("2", lambda: count_classes(model, frames, classes, fold=True)),
                        ("3", lambda: [count_frames(model, frames, bx) for bx in classes.values()])):
            ms[key] = median_ms(synced(fn), args.calls, args.warmup)
        lines.append("C = %d (the two paths agree bit for bit on every count and map)" % C_)
        for key, what in (("1", "count_classes(fold=False)"), ("2", "count_classes(fold=True)"), ("3", "%d x count_frames" % C_)):
            lines.append("  %s  %-28s %9.3f  (%.3f .. %.3f)" % ((key, what) + ms[key]))
        lines.append("  3 / 1 = %.2f, 2 - 1 = %.3f ms, per further class: shared %.3f ms, separate %.3f ms"
                     % (ms["3"][0] / ms["1"][0], ms["2"][0] - ms["1"][0],
                        (ms["1"][0] - first[0]) / (C_ - 1) if C_ > 1 else 0.0, (ms["3"][0] - first[1]) / (C_ - 1) if C_ > 1 else 0.0))
        if C_ == 1:
            first = (ms["1"][0], ms["3"][0])
            lines[-1] = "  3 / 1 = %.2f (the same launches: the noise floor), 2 - 1 = %.3f ms" % (ms["3"][0] / ms["1"][0], ms["2"][0] - ms["1"][0])
        last = shared
    # the fold alone, C = 8, the call's eight frames
    folder = ClassFolder("cuda")
    sums = [[float(m.sum().item()) for m in r.maps] for r in last]
    sets = [(list(r.maps), [r.counts[c] / s[c] if s[c] != 0 else 1.0 / 60 for c in range(8)]) for r, s in zip(last, sums)]
    lists = [list(r.maps) for r in last]
    scale = torch.tensor([sc for _m, sc in sets], dtype=torch.float32, device="cuda")
    a = median_ms(synced(lambda: folder.fold(sets, 0.0)), args.calls, args.warmup)
    b = median_ms(synced(lambda: torch_fold(lists, scale, 0.0)), args.calls, args.warmup)
    lines.append("the fold alone, C = 8, eight frames of 384 x %d (sums on the host, labels on the device)" % lists[0][0].shape[-1])
    lines.append("  1  %-28s %9.3f  (%.3f .. %.3f)" % (("ClassFolder.fold",) + a))
    lines.append("  2  %-28s %9.3f  (%.3f .. %.3f)" % (("torch: stack, max, masked sums",) + b))
    lines.append("  2 / 1 = %.2f" % (b[0] / a[0]))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
