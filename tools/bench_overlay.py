"""Annotated frames: what composing them on the device costs, against counting alone, against today's host path and against torch ops.

  (a) eight 1920x1080 NV12 frames in HOST memory, ViT-B bf16, zero-shot:
        ANNOTATE  annotate_frames(out="nv12", points=True): count, locate, compose, convert -- one upload per frame
        COUNT     count_frames + locate_maps alone on the same frames: what annotating adds to a group is ANNOTATE - COUNT
        HOST      COUNT, then today's pictures: yuv_host of every frame in numpy, the frame resized to the model's height on the device,
                  save_visualisation's composition (sample / 2 + density / 2 + the label, downloaded, resized back by PIL, dots drawn
                  with ImageDraw), without the JPEG encode
      Before anything is timed: ANNOTATE's counts and maps equal COUNT's bit for bit and its points equal locate_maps'; its NV12 buffer
      equals overlay_host of the same inputs (frame 0, byte for byte), and rgb_to_yuv_host of its RGB output (the same rule).  HOST's
      pictures follow another rule (composed at the model's size and resized back): they are timed, not compared.
  (b) Overlay.render alone on the eight frames and maps already on the device (heat + label + points, RGB out and NV12 out), against the
      same composition written as torch ops on the device (the heat quantised, F.interpolate bilinear, a gather from the colour table,
      the blend in integers; the label and point masks rasterised on the host beforehand and not timed).  The torch form's levels differ
      from the rule's by the 8-bit weights only: the largest difference is asserted below 2.5 levels (the bound for a map whose
      neighbouring levels differ by up to 255: tests/test_overlay_cpu.py derives it) and reported.
Every call ends in a device synchronise; the forms are alternated call by call; the figure is the median over --calls calls after
--warmup, with the quartiles and the extremes as the spread.  No threshold: whatever comes out is the record.
  --trace runs (b)'s render calls alone, for a `rocprofv3 --kernel-trace --stats` run of its own; --kernels FILE appends the per-kernel
  averages of that run's kernel_stats.csv, and the composition kernel's distance from the bytes it has to move, to --out.

    python tools/bench_overlay.py [--calls 30] [--warmup 5] [--out profiles/overlay.txt] [--head <commit>]"""
import argparse
import csv
import re
import os
import socket
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from PIL import Image, ImageDraw

import models_mae_cross
from countr_amd import YuvFrame, frames as FR, overlay as O, overlay_host, yuv_host

H, W, N = 1080, 1920, 8


def head(root):
    try:
        return subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=root, stderr=subprocess.DEVNULL, text=True).strip()
    except Exception:
        return "unknown"


def nv12_frame(rs):
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


def host_picture(prep, frame, dm, count, pts):
    """Today's picture of a frame (demo_zero.py::run_yuv + save_visualisation), without the JPEG encode."""
    sample = prep.prepare([yuv_host(frame)])[0][0]
    _, h, w = sample.shape
    pred = torch.stack((dm, torch.zeros_like(dm), torch.zeros_like(dm)))
    label = Image.new(mode="RGB", size=(w, h), color=(0, 0, 0))
    ImageDraw.Draw(label).text((w - 70, h - 50), "%.3f" % count, (255, 255, 255))
    label = torch.from_numpy(np.array(label).transpose((2, 0, 1)).copy()).to(sample.device)
    fig = torch.clamp(sample / 2 + pred / 2 + label, 0, 1)
    arr = (fig.permute(1, 2, 0).cpu().numpy() * 255.0 + 0.5).astype(np.uint8)
    im = Image.fromarray(arr).resize((W, H), Image.BILINEAR)
    draw = ImageDraw.Draw(im)
    for x, y in pts:
        draw.ellipse((x + 0.5 - 2, y + 0.5 - 2, x + 0.5 + 2, y + 0.5 + 2), fill=(0, 255, 0))
    return im


def masks_on_host(labels, points, radius=2):
    """Per frame (label coverage [H, W] uint8, point mask [H, W] bool) on the device, rasterised with the host rule beforehand."""
    out = []
    for lab, pts in zip(labels, points):
        cover = np.zeros((H, W, 3), np.uint8)
        O.draw_label_host(cover, *O._check_label((np.full_like(lab[0], 255), lab[1], lab[2])))      # where the patch lies
        patch = np.zeros((H, W), np.uint8)
        ys, xs = np.nonzero(cover[..., 0])
        patch[ys, xs] = lab[0][ys - lab[2], xs - lab[1]]
        dots = np.zeros((H, W, 3), np.uint8)
        O.draw_points_host(dots, O._check_points(pts, radius), radius, (1, 1, 1))
        out.append((torch.from_numpy(patch).cuda(), torch.from_numpy(dots[..., 0] > 0).cuda()))
    return out


def torch_compose(frame, dm, gain, lut, mask):
    """The composition as torch ops: levels, bilinear to the frame, table, blend, label, points -> (uint8 [H, W, 3], levels [H, W])."""
    q = torch.clamp(torch.floor(dm * gain + 0.5), 0, 255).nan_to_num(0.0)
    h = torch.floor(torch.nn.functional.interpolate(q[None, None], size=(H, W), mode="bilinear", align_corners=False)[0, 0] + 0.5).long()
    c = lut[h]
    a = c[..., 3:4]
    out = torch.div(frame.int() * (255 - a) + c[..., :3] * a + 127, 255, rounding_mode="floor")
    m = mask[0].int()[..., None]
    out = torch.div(out * (255 - m) + 255 * m + 127, 255, rounding_mode="floor")
    out[mask[1]] = torch.tensor([0, 255, 0], dtype=out.dtype, device=out.device)
    return out.to(torch.uint8), h


def kernel_lines(path):
    rows = [r for r in csv.DictReader(open(path)) if "OvArgs" in r.get("Name", "")]          # the overlay library's launches
    lines = ["(c) the kernels' own times (a rocprofv3 --kernel-trace --stats run of its own over --trace: render of eight 1080p frames, NV12 out)"]
    for r in rows:
        avg = float(r["AverageNs"]) / 1e3
        name = re.search(r"\w+_kernel(<[^>]*>)?", r["Name"]).group(0)
        note = ""
        if "compose_kernel" in name:
            mb = N * H * W * 6 / 1e6
            note = "  %.1f MB read + written -> %.2f TB/s of the bytes it has to move" % (mb, mb / 1e6 / (avg / 1e6))
        elif "yuv_kernel" in name:
            mb = N * H * W * 4.5 / 1e6
            note = "  %.1f MB read + written -> %.2f TB/s" % (mb, mb / 1e6 / (avg / 1e6))
        lines.append("    %-40s %5s calls, average %9.1f us%s" % (name[-40:], r["Calls"], avg, note))
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
    prep, ov = FR.frame_prep("cuda"), O.overlay_for("cuda")

    def count():
        res = FR.count_frames(model, host8, normalization=False)
        return res, FR.locate_maps(res, sizes)

    annotate = lambda out="nv12": FR.annotate_frames(model, host8, out=out, points=True, normalization=False)
    res, loc = count()
    got = annotate()
    for (c0, d0), (p0, s0, _t), (c1, d1, _pic, p1, s1) in zip(res, loc, got):
        assert c0 == c1 and torch.equal(d0, d1) and np.array_equal(p0, p1) and np.array_equal(s0, s1), "annotate_frames and count_frames + locate_maps disagree"
    c, dm, pic, pts, _s = got[0]
    want = overlay_host(yuv_host(host8[0]), dm.float().cpu().numpy(), points=pts, label=O.count_label(c, W, H), out="nv12")
    assert np.array_equal(pic.cpu().numpy(), want), "the device bytes differ from overlay_host"
    nv12 = pic.cpu().numpy().copy()
    assert np.array_equal(O.rgb_to_yuv_host(annotate("rgb")[0][2].cpu().numpy()), nv12), "the RGB and the NV12 output are not the same picture"
    if not args.trace:
        lines = ["overlay: box %s, HEAD %s, %s" % (socket.gethostname(), args.head or head(root), torch.cuda.get_device_name(0)),
                 "every call synchronised, forms alternated call by call, %d calls after %d warm-up calls" % (args.calls, args.warmup),
                 "(a) eight 1920x1080 NV12 frames in host memory, ViT-B bf16, zero-shot; the forms agree as the tool's docstring says (counts %s; %s points)"
                 % (" ".join("%.2f" % r[0] for r in res), " ".join(str(len(p)) for p, _s, _t in loc))]

        def host():
            r, l = count()
            return [host_picture(prep, f, d.float(), cnt, p) for f, (cnt, d), (p, _s, _t) in zip(host8, r, l)]

        ta = alternated({"ANNOTATE": annotate, "COUNT": count, "HOST": host}, args.calls, args.warmup)
        for k, note in (("ANNOTATE", "annotate_frames(out=\"nv12\", points=True)"), ("COUNT", "count_frames + locate_maps alone"),
                        ("HOST", "COUNT + yuv_host + save_visualisation's composition, no JPEG encode")):
            lines.append("    %-9s %s  %s" % (k, spread(ta[k]), note))
        a, b, h = (float(np.median(ta[k])) for k in ("ANNOTATE", "COUNT", "HOST"))
        lines.append("    annotating adds ANNOTATE - COUNT = %+.3f ms per group of eight; today's host pictures add HOST - COUNT = %+.3f ms" % (a - b, h - b))
        t0 = time.perf_counter()
        for k in range(10):
            for r in res:
                O.count_label(r[0] + k, W, H)
        lines.append("    of which the eight labels rasterised with PIL on the host: %.3f ms per group" % ((time.perf_counter() - t0) / 10 * 1e3))
    # (b) the render alone, frames and maps on the device
    dev = [t.clone() for t in prep.device_frames(host8)]
    maps = [d.float().contiguous() for _c, d in res]
    points = [p for p, _s, _t in loc]
    labels = [O.count_label(r[0], W, H) for r in res]
    render = lambda out: ov.render(dev, maps, points=points, labels=labels, out=out)
    if args.trace:
        for _ in range(20):
            render("nv12")
        torch.cuda.synchronize()
        return
    lut = torch.from_numpy(O.colormap_table("red").astype(np.int32)).cuda()
    masks = masks_on_host(labels, points)
    torch_form = lambda: [torch_compose(f, m, 127.5, lut, k)[0] for f, m, k in zip(dev, maps, masks)]
    worst_level, worst_byte = 0, 0
    for f, m, k, pic in zip(dev, maps, masks, render("rgb")):
        t, h = torch_compose(f, m, 127.5, lut, k)
        rule = torch.from_numpy(O.upsample_host(O.heat_host(m.cpu().numpy(), np.float32(127.5)), H, W)).cuda()
        worst_level = max(worst_level, int((h - rule).abs().max()))
        worst_byte = max(worst_byte, int((t.int() - pic.int()).abs().max()))
    assert worst_level < 2.5, "the torch form's levels are %d from the rule's" % worst_level
    tb = alternated({"HIP rgb": lambda: render("rgb"), "HIP nv12": lambda: render("nv12"), "torch rgb": torch_form}, args.calls, args.warmup)
    lines.append("(b) Overlay.render on eight 1080p device frames with heat, label and points, against the same composition as torch ops (RGB out; "
                 "its levels are at most %d from the rule's, its bytes at most %d)" % (worst_level, worst_byte))
    for k, ms in tb.items():
        lines.append("    %-10s %s" % (k, spread(ms)))
    hip, tor = float(np.median(tb["HIP rgb"])), float(np.median(tb["torch rgb"]))
    lines.append("    the HIP composition is %s the torch-op form (%.3f ms against %.3f ms per eight frames)"
                 % ("faster than" if hip < tor else "NOT faster than", hip, tor))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
