#!/usr/bin/env python3
"""Few-shot counting demo: "this image, these boxes, how many?" on the MI355X engine.

    python demo.py --input_path <image or directory> --boxes "x1,y1,x2,y2;x1,y1,x2,y2;..." [--boxes_json FILE]
                   [--output_path results] [--model_path weights/FSC147.pth]

The boxes are exemplar rectangles in pixels of the ORIGINAL image (left upper and right lower corner, both inclusive).  --boxes
applies to every input image; --boxes_json names a JSON file {image file name: [[x1, y1, x2, y2], ...]} that takes precedence for
the images it lists.  An image without boxes is counted zero-shot.  The frame is handed to the device as decoded uint8 pixels:
the resize to height 384, the 64 x 64 exemplar crops and, for exemplars under 10 pixels, the 3 x 3 crop-and-upscale all run there
(countr_amd.frames).  The visualisation is image + exemplar outlines + density / 2, clamped to [0, 1], at the resized size.
`--model_path ""` runs the randomly initialised model (dry runs / tests).  `--points` also locates the objects (countr_amd.frames.locate_items):
points_<stem>.json = {"count", "total_peaks", "points": [[x, y, score], ...]} in pixel-centre coordinates of the input image is written
(with --no_viz too), and viz_<name>.jpg is resized back to the input size and gets a small dot per point.  `--regions_json FILE` counts
per region, as demo_zero.py does: {"name": [[x, y], ...], ...} in pixels of the original image -> one printed line per region,
regions_<stem>.json and the outlines in viz_<name>.jpg (then at the input size too); a frame that takes the 3 x 3 path is summed over
its nine crop maps.  It works together with --points.  `--classes_json FILE` counts several classes per image from one encoder pass
(countr_amd.frames.count_classes): {"name": [[x1, y1, x2, y2], ...], ...} exemplar boxes per class in pixels of the input image, applied
to every input image -> one printed line per class (count and won count), classes_<stem>.json = {"classes": {name: {"count", "won",
"area"}}} and viz_<name>.jpg tinted by the dominant class (won and area are null, and nothing is tinted, for an image on which a class
took the 3 x 3 path).  It replaces --boxes, --points and --regions_json for that run.  `--zoom {2,3,4,auto}` counts from the image's own
pixels, as demo_zero.py does: the image is resized on the device to height 384 k, the exemplars are cut from that image, and a 2-D grid
of tiles covers it (--band_stride, --zoom_max); "auto" takes the smallest k at which the exemplars are no longer under 10 pixels.
viz_<name>.jpg is then drawn from the zoomed image and map.  --regions_json and --classes_json are for --zoom 1."""
import json
import time
from argparse import ArgumentParser
from itertools import chain
from pathlib import Path

import numpy as np
import torch
from PIL import Image

import models_mae_cross
from countr_amd import frames
from demo_zero import (add_points_args, add_regions_args, add_zoom_args, count_zoomed, draw_points, draw_regions, load_regions, parse_zoom,
                       points_on, report_regions, write_points)


def parse_boxes(text):
    """ "x1,y1,x2,y2;x1,y1,x2,y2" -> [(x1, y1, x2, y2), ...]"""
    boxes = []
    for part in (text or "").split(";"):
        if not part.strip():
            continue
        v = [float(t) for t in part.split(",")]
        if len(v) != 4:
            raise ValueError("a box is x1,y1,x2,y2 -- got %r" % part)
        boxes.append(tuple(v))
    return boxes


def save_visualisation(sample, density_map, rects, path, points=None, size=None, regions=None):
    """sample [3, h, w] in [0, 1], density_map [h, w]: outlines are drawn at 10 (white after the clamp), the density is halved.
    points: [(x, y), ...] and regions: polygons of the input image of size (W, H): the picture is resized to that size, then outlined
    and dotted."""
    _, h, w = sample.shape
    box_map = torch.zeros(h, w, device=sample.device)
    for y1, x1, y2, x2 in rects or []:
        ya, yb, xa, xb = min(y1, h - 1), min(y2, h - 1), min(x1, w - 1), min(x2, w - 1)
        box_map[ya:yb + 1, xa] = 10
        box_map[ya:yb + 1, xb] = 10
        box_map[ya, xa:xb + 1] = 10
        box_map[yb, xa:xb + 1] = 10
    fig = torch.clamp(sample + box_map.unsqueeze(0) + density_map.unsqueeze(0) / 2, 0, 1)
    im = Image.fromarray((fig.permute(1, 2, 0).cpu().numpy() * 255.0 + 0.5).astype(np.uint8))
    if points is not None or regions is not None:
        im = im.resize(size, Image.BILINEAR)
    if regions is not None:
        draw_regions(im, regions)
    if points is not None:
        draw_points(im, points)
    im.save(path)


# the tint of class 0, 1, 2, ... in viz_<name>.jpg (repeats after sixteen)
PALETTE = [(230, 25, 75), (60, 180, 75), (0, 130, 200), (255, 225, 25), (245, 130, 48), (145, 30, 180), (70, 240, 240), (240, 50, 230),
           (210, 245, 60), (250, 190, 212), (0, 128, 128), (220, 190, 255), (170, 110, 40), (128, 0, 0), (170, 255, 195), (0, 0, 128)]


def save_class_visualisation(sample, labels, path):
    """sample [3, h, w] in [0, 1] on the device, labels uint8 [h, w] (255 = no class) or None: the picture with every labelled pixel
    mixed half and half with its class's colour, composed on the host."""
    fig = (sample.permute(1, 2, 0).cpu().numpy() * 255.0 + 0.5).astype(np.uint8)
    if labels is not None:
        lab = labels.cpu().numpy()
        tint = np.asarray(PALETTE, np.float32)[lab % len(PALETTE)]
        own = (lab != 255)[:, :, None]
        fig = np.where(own, (fig.astype(np.float32) + tint) / 2 + 0.5, fig).astype(np.uint8)
    Image.fromarray(fig).save(path)


def run_classes(args, model, device, inputs, named):
    """--classes_json: every group of images through frames.count_classes."""
    names = list(named)
    done = 0
    step = max(args.group_images, 1)
    for g0 in range(0, len(inputs), step):
        paths = inputs[g0:g0 + step]
        raw = [np.asarray(Image.open(pth).convert("RGB"), dtype=np.uint8) for pth in paths]
        t0 = time.perf_counter()
        res = frames.count_classes(model, raw, {n: [[tuple(b) for b in named[n]]] * len(raw) for n in names})
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / len(paths)
        samples = frames.frame_prep(device).prepare(raw) if not args.no_viz else [None] * len(raw)
        for pth, r, sample in zip(paths, res, samples):
            done += 1
            print("[%3d/%d] %s:\ttime = %5.2f" % (done, len(inputs), pth.name, dt))
            out = {}
            for c, n in enumerate(names):
                won = float(r.won[c]) if r.won is not None else None
                out[n] = {"count": float(r.counts[c]), "won": won, "area": int(r.area[c]) if r.area is not None else None}
                print("  class %s: count = %5.2f  won = %s" % (n, r.counts[c], "%5.2f" % won if won is not None else "n/a"))
            with open(args.output_path / ("classes_%s.json" % pth.stem), "w") as f:
                json.dump({"classes": out}, f)
            if not args.no_viz:
                save_class_visualisation(sample[0], r.labels, args.output_path / ("viz_%s.jpg" % pth.stem))


def main():
    p = ArgumentParser()
    p.add_argument("--input_path", type=Path, required=True)
    p.add_argument("--boxes", type=str, default="", help='exemplar boxes of every image: "x1,y1,x2,y2;..." in original pixels')
    p.add_argument("--boxes_json", type=Path, default=None, help="JSON {file name: [[x1, y1, x2, y2], ...]}")
    p.add_argument("--output_path", type=Path, default="results")
    p.add_argument("--model_path", type=str, default="weights/FSC147.pth")
    p.add_argument("--group_images", type=int, default=8, help="images prepared and counted per call")
    p.add_argument("--precision", default="bf16", choices=["bf16", "fp16", "fp32"])
    p.add_argument("--no_viz", action="store_true", help="counts only, no viz_*.jpg")
    p.add_argument("--classes_json", type=Path, default=None, help="JSON {class name: [[x1, y1, x2, y2], ...]}: several classes per image")
    add_points_args(p)
    add_regions_args(p)
    add_zoom_args(p)
    args = p.parse_args()
    zoom = parse_zoom(args)
    if zoom != 1 and (args.regions_json is not None or args.classes_json is not None):
        p.error("--regions_json and --classes_json are for --zoom 1")
    args.output_path.mkdir(exist_ok=True, parents=True)
    device = torch.device("cuda")
    region_names, polygons = load_regions(args.regions_json)

    if not args.model_path:
        torch.manual_seed(0)          # dry runs without a checkpoint: the same random model every time
    model = models_mae_cross.__dict__["mae_vit_base_patch16"](norm_pix_loss="store_true", precision=args.precision)
    if args.model_path:
        checkpoint = torch.load(args.model_path, map_location="cpu", weights_only=False)
        model.load_state_dict(checkpoint["model"], strict=False)
        print("Resume checkpoint %s" % args.model_path)
    model.to(device).eval()

    common = parse_boxes(args.boxes)
    named = json.load(open(args.boxes_json)) if args.boxes_json else {}
    if args.input_path.is_dir():
        inputs = sorted(chain(args.input_path.glob("*.jpg"), args.input_path.glob("*.png")))
    else:
        inputs = [args.input_path]
    if args.classes_json:
        run_classes(args, model, device, inputs, json.load(open(args.classes_json)))
        return
    done = 0
    step = max(args.group_images, 1)
    for g0 in range(0, len(inputs), step):
        paths = inputs[g0:g0 + step]
        raw = [np.asarray(Image.open(pth).convert("RGB"), dtype=np.uint8) for pth in paths]      # decoding stays on the host
        boxes = [[tuple(b) for b in named[pth.name]] if pth.name in named else common for pth in paths]
        t0 = time.perf_counter()
        if zoom != 1:
            got = count_zoomed(model, raw, boxes, zoom, args, True)
            dt = (time.perf_counter() - t0) / len(paths)
            for pth, r, bx, (pred_cnt, dm, pts, score, total, sample, k) in zip(paths, raw, boxes, got):
                done += 1
                if pts is not None:
                    write_points(args.output_path / ("points_%s.json" % pth.stem), pred_cnt, total, pts, score)
                if not args.no_viz:
                    old_w, old_h = r.shape[1], r.shape[0]
                    w, h = (sample.shape[2], sample.shape[1]) if k > 1 else (old_w, old_h)      # a zoomed picture stays at its size
                    save_visualisation(sample, dm.float(), frames.scale_boxes(bx, old_w, old_h, frames.NEW_H * k), args.output_path / ("viz_%s.jpg" % pth.stem),
                                       points_on(pts, old_w, old_h, w, h) if pts is not None else None, (w, h))
                if len(inputs) > 1:
                    print("[%3d/%d] %s:\tcount = %5.2f  -  time = %5.2f" % (done, len(inputs), pth.name, pred_cnt, dt))
                else:
                    print("Count:", pred_cnt, "- Time:", dt)
            continue
        items = frames.prepare_items(device, raw, boxes)
        sizes = [(r.shape[1], r.shape[0]) for r in raw]
        summed = [None] * len(paths)
        if args.points:
            results = frames.locate_items(model, items, sizes, radius=args.points_radius, rel_threshold=args.points_rel_threshold,
                                          keep=args.points_keep, crops=True)
        elif polygons is not None:
            results = [(c, dm, None, None, None, cr) for c, dm, cr in frames.count_items_crops(model, items)]
        else:
            results = [r + (None, None, None, None) for r in frames.count_items(model, items)]
        if polygons is not None:      # the nine crop maps of a frame that took the 3 x 3 path add into the frame's regions
            summed = frames.region_maps([r[:2] for r in results], sizes, [r[5] for r in results], polygons)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / len(paths)
        for pth, (sample, _ex, rects), (pred_cnt, dm, pts, score, total, _crops), size, reg in zip(paths, items, results, sizes, summed):
            done += 1
            if pts is not None:
                write_points(args.output_path / ("points_%s.json" % pth.stem), pred_cnt, total, pts, score)
            if not args.no_viz:
                save_visualisation(sample[0], dm.float(), rects, args.output_path / ("viz_%s.jpg" % pth.stem), pts, size, regions=polygons)
            if len(inputs) > 1:
                print("[%3d/%d] %s:\tcount = %5.2f  -  time = %5.2f" % (done, len(inputs), pth.name, pred_cnt, dt))
            else:
                print("Count:", pred_cnt, "- Time:", dt)
            if reg is not None:
                report_regions(args.output_path / ("regions_%s.json" % pth.stem), pred_cnt, region_names, reg[0], reg[1])


if __name__ == "__main__":
    main()
