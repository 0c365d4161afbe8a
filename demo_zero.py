#!/usr/bin/env python3
"""Zero-shot counting demo with the reference's flags (demo_zero.py:23-126), running the MI355X engine.

    python demo_zero.py --input_path <image or directory> [--output_path results] [--model_path weights/FSC147.pth]

Every image is resized to height 384 (width a multiple of 16, demo_zero.py:23-38), covered by 384-px windows with stride 128 and
counted with shot_num = 0 and an empty exemplar tensor (:41-74).  The reference runs one window per forward; here the windows of
--group_images images (default 8: eight 1920x1080 frames = 32 windows = BASELINE config 5) share ONE forward
(countr_amd.inference.count_images).  The visualisation (:77-90: image / 2 + density in the red channel / 2 + the count as text,
resized back to the input size) is written with PIL, since torchvision is not part of this build.
`--model_path ""` runs the randomly initialised model (dry runs / tests).  `--device_prep` moves the resize to the device: the frames
are decoded by PIL, handed over as uint8 pixels and resized by countr_frame_resize_u8 (same bits as the host resize, so same counts);
the printed time then includes the preparation.  `--points` also locates the objects (countr_amd.frames.locate_maps: the peaks of the
density map, found on the device): viz_<name>.jpg gets a small dot per point and points_<stem>.json = {"count", "total_peaks", "points":
[[x, y, score], ...]} (pixel-centre coordinates of the input image) is written, with --no_viz too.  `--regions_json FILE` counts per
region: FILE is {"name": [[x, y], ...], ...}, polygons in pixels of the original image (pixel-centre coordinates: pixel i has centre
i); the density map is summed over each polygon on the device (countr_amd.frames.region_maps), one line per region is printed,
regions_<stem>.json = {"count", "regions": {name: {"count", "area"}}} is written (area = map pixels inside) and viz_<name>.jpg gets the
outlines.  It works together with --points.  `--zoom {2,3,4,auto}` counts from the image's own pixels (countr_amd.frames.count_frames
with zoom=): the decoded image is resized on the device to height 384 k and covered by a 2-D grid of tiles (--band_stride: the row
stride of the grid, --zoom_max: the largest k "auto" takes; without exemplar boxes "auto" is 1).  Counts, --points and their JSON
work as before; viz_<name>.jpg is drawn from the zoomed image and map, at the zoomed size.  --regions_json is for --zoom 1.
`--yuv FORMAT:WxH[:MATRIX[:RANGE[:CHROMA]]]` counts a raw video clip: --input_path is then a file of consecutive packed frames (Y plane,
then the chroma plane(s), no padding) in nv12, nv21, i420 or p010, as a decoder or `ffmpeg -f rawvideo` writes them; MATRIX is bt709
(default) or bt601, RANGE limited (default) or full, CHROMA nearest (default) or linear.  The frames go to the device as they are --
1.5 bytes a pixel -- and are converted there (countr_amd/yuv.py, include/countr_hip_yuv.h); p010 is reduced to 8 bits by that rule alone,
without tone mapping.  --max_frames N reads the first N frames; an incomplete trailing frame is an error.  The frames are counted
--group_images at a time through countr_amd.frames.count_frames, each prints `<stem>#<index>: Count: ... - Time: ...`, and
viz_<stem>_<index>.jpg, points_<stem>_<index>.json and regions_<stem>_<index>.json are what they are for an image, the picture drawn
from countr_amd.yuv_host of the frame.  `--out_yuv FILE[:FORMAT]` (with --yuv) writes the annotated clip -- density overlay, count label, the
outlines of --regions_json and the dots of --points on the frame's own pixels -- as raw packed frames in nv12, nv21 or i420 (default: the
input's format, nv12 for p010; the input's matrix and range), composed on the device by countr_amd.frames.annotate_frames
(countr_amd/overlay.py states the rule).  `--device_viz`, for images and clips, writes viz_<name>.jpg from the device-composed RGB at the
input's size instead of the host composition (with --out_yuv the picture is decoded from the written frame).  Both are off by default.
`--track --track_dist D [--lines_json FILE] [--track_missed M] [--track_hits H]` (with --yuv, at --zoom 1) joins the frames' points over
time (countr_amd.frames.count_clip, include/countr_hip_tracks.h): --track implies --points, D is the largest move of an object between
two frames in pixels of the frame, --lines_json is {"name": [[ax, ay], [bx, by]], ...} (up to 16 counting lines in pixels of the frame).
Each frame's line gains ` - tracks: <live> - crossed: {name: [forward, backward]}` (the crossings of that frame), points_<stem>_<i>.json gains
"ids", viz_*.jpg gets the lines, and at the end {"clip": {"started", "confirmed", "lines": {name: [forward, backward]}}} is printed and
written to tracks_<stem>.json.  The defaults of --track_missed and --track_hits are unmeasured.  Without --track nothing changes.
With `--out_yuv` or `--device_viz`, --track goes through countr_amd.frames.annotate_clip instead: the written frames (and viz_*.jpg under
--device_viz) carry every track's id and trail in its colour, the counting lines with their running tallies, and count, live tracks and
confirmed total at the top left, drawn on the device (countr_amd/draw.py states the rule); `--trail N` (default 16, 0 = none) is the
trail's length in positions, `--no_tags` leaves the ids out, `--mark_scale S` sets the marks' size.  The printed lines and JSON files
are the same.
`--flow --lines_json FILE [--flow_search R] [--flow_interval S] [--flow_band W]` (with --yuv, at --zoom 1, without --track) counts the
crossings of the same lines from the flux of the density map instead (countr_amd.frames.count_flow, include/countr_hip_flow.h): no peaks
and no tracks.  Each frame's line gains ` - flux: {name: [forward, backward]}` (that frame's share; null for the first S frames) and at
the end {"clip": {"flux": {name: [forward, backward]}}} is printed and written to flow_<stem>.json.  The defaults of --flow_search and
--flow_band are unmeasured; slow motion needs --flow_interval.  Without --flow nothing changes.
`--camera translation` (with --flow or --track) counts in scene coordinates under a panning camera (countr_amd/cam.py,
include/countr_hip_cam.h): the lines, and --track_dist, are in pixels of the FIRST frame.  Each frame's line gains ` - cam: [x, y]`, the
camera's position in frame pixels, and the clip JSON gains "camera": {"end": [x, y], "lost": n} (n frames without a valid estimate).
Rotation and zoom are not modelled, and the estimate's settings are unmeasured on real video.  Without --camera nothing changes.
demo.py is the few-shot counterpart (exemplar boxes)."""
import json
import time
from argparse import ArgumentParser
from itertools import chain
from pathlib import Path

import numpy as np
import torch
from PIL import Image, ImageDraw

import models_mae_cross
from countr_amd import frames, inference, yuv

shot_num = 0


def load_image(img_path):
    """demo_zero.py:23-38 -> (image tensor [3, 384, new_W] in [0, 1], empty boxes, original W, H)."""
    image = Image.open(img_path).convert("RGB")
    image.load()
    W, H = image.size
    new_H = 384
    new_W = 16 * int((W / H * 384) / 16)
    image = image.resize((new_W, new_H), Image.BILINEAR)       # transforms.Resize on a PIL image
    t = torch.from_numpy(np.asarray(image, dtype=np.uint8).copy()).permute(2, 0, 1).float().div(255.0)
    return t, torch.Tensor([]), W, H


def draw_points(image, points, radius=2):
    """A small dot per (x, y) point (pixel-centre coordinates of `image`)."""
    draw = ImageDraw.Draw(image)
    for x, y in points:
        draw.ellipse((x + 0.5 - radius, y + 0.5 - radius, x + 0.5 + radius, y + 0.5 + radius), fill=(0, 255, 0))
    return image


def write_points(path, pred_cnt, total, points, score, ids=None):
    with open(path, "w") as f:
        doc = {"count": pred_cnt, "total_peaks": int(total),
               "points": [[float(x), float(y), float(s)] for (x, y), s in zip(points, score)]}
        if ids is not None:
            doc["ids"] = [int(i) for i in ids]
        json.dump(doc, f)


def add_points_args(p):
    p.add_argument("--points", action="store_true", help="locate the objects: dots in viz_*.jpg and points_<stem>.json")
    p.add_argument("--points_radius", type=int, default=4, help="half width of the peak window, 1..8 (the default is unmeasured)")
    p.add_argument("--points_rel_threshold", type=float, default=0.1, help="a peak is at least this share of the map's maximum (the default is unmeasured)")
    p.add_argument("--points_keep", default="all", choices=["all", "count"], help="count: keep the round(count) highest peaks")


def add_zoom_args(p):
    p.add_argument("--zoom", default="1", choices=["1", "2", "3", "4", "auto"],
                   help="count at k times the model's height, on a 2-D grid of tiles over the image's own pixels")
    p.add_argument("--zoom_max", type=int, default=3, choices=[1, 2, 3, 4], help="the largest zoom --zoom auto takes")
    p.add_argument("--band_stride", type=int, default=128, choices=[128, 192, 256, 384], help="row stride of the tile grid")


def parse_zoom(args):
    return "auto" if args.zoom == "auto" else int(args.zoom)


def count_zoomed(model, raw, boxes, zoom, args, normalization):
    """frames.count_frames(zoom=) for the demos -> per image (count, map, points or None, score, total peaks, zoomed image [3, Hk, Wk] or
    None with --no_viz, k).  The points are in pixel-centre coordinates of the input image."""
    ks = frames.frame_zooms(raw, boxes, zoom, args.zoom_max)
    res = frames.count_frames_zoomed(model, raw, boxes, ks, normalization, 1, 32, args.band_stride, crops=True)
    located = [(None, None, None)] * len(raw)
    if args.points:
        located = frames.locate_maps(res, [(r.shape[1], r.shape[0]) for r in raw], radius=args.points_radius,
                                     rel_threshold=args.points_rel_threshold, keep=args.points_keep, new_h=[frames.NEW_H * k for k in ks])
    torch.cuda.synchronize()
    prep = frames.frame_prep(next(model.parameters()).device)
    samples = [None if args.no_viz else prep.prepare([r], frames.NEW_H * k)[0][0] for r, k in zip(raw, ks)]
    return [(c, dm, pts, score, total, sample, k) for (c, dm, _cr), (pts, score, total), sample, k in zip(res, located, samples, ks)]


def points_on(points, old_w, old_h, w, h):
    """Points of the input image (old_w x old_h) in pixel-centre coordinates of its picture resized to w x h."""
    return [((x + 0.5) * w / old_w - 0.5, (y + 0.5) * h / old_h - 0.5) for x, y in points]


def add_regions_args(p):
    p.add_argument("--regions_json", type=Path, default=None,
                   help='count per region: JSON {"name": [[x, y], ...], ...}, polygons in pixels of the original image')


def load_regions(path):
    """--regions_json -> (names, polygons) or (None, None) without the flag."""
    if path is None:
        return None, None
    named = json.load(open(path))
    if not isinstance(named, dict) or not named:
        raise ValueError('--regions_json: a JSON object {"name": [[x, y], ...], ...}')
    return list(named), [[(float(x), float(y)) for x, y in poly] for poly in named.values()]


def draw_regions(image, polygons):
    """The outline of each polygon (pixel-centre coordinates of `image`)."""
    draw = ImageDraw.Draw(image)
    for poly in polygons:
        pts = [(x + 0.5, y + 0.5) for x, y in poly]
        draw.line(pts + pts[:1], fill=(255, 255, 0), width=1)
    return image


def report_regions(path, pred_cnt, names, counts, area):
    """One printed line per region and regions_<stem>.json."""
    for name, c, a in zip(names, counts, area):
        print("  region %s: count = %5.2f, area = %d" % (name, c, a))
    with open(path, "w") as f:
        json.dump({"count": pred_cnt, "regions": {name: {"count": float(c), "area": int(a)} for name, c, a in zip(names, counts, area)}}, f)


def save_visualisation(sample, density_map, pred_cnt, path, old_w, old_h, points=None, regions=None, lines=None):
    """demo_zero.py:77-90; points: [(x, y), ...], regions: polygons and lines: segments (ax, ay, bx, by) of the input image, drawn after
    the resize back to its size."""
    _, h, w = sample.shape
    pred_fig = torch.stack((density_map, torch.zeros_like(density_map), torch.zeros_like(density_map)))
    count_im = Image.new(mode="RGB", size=(w, h), color=(0, 0, 0))
    ImageDraw.Draw(count_im).text((w - 70, h - 50), "%.3f" % pred_cnt, (255, 255, 255))
    count_im = torch.from_numpy(np.array(count_im).transpose((2, 0, 1)).copy()).to(sample.device)   # 0 / 255, as in the reference
    fig = torch.clamp(sample / 2 + pred_fig / 2 + count_im, 0, 1)
    arr = (fig.permute(1, 2, 0).cpu().numpy() * 255.0 + 0.5).astype(np.uint8)
    im = Image.fromarray(arr).resize((old_w, old_h), Image.BILINEAR)
    if regions is not None:
        draw_regions(im, regions)
    if lines is not None:
        d = ImageDraw.Draw(im)
        for ax, ay, bx, by in lines:
            d.line([(ax, ay), (bx, by)], fill=(0, 255, 255), width=1)
    if points is not None:
        draw_points(im, points)
    im.save(path)


def parse_out_yuv(spec, input_format):
    """--out_yuv FILE[:FORMAT] -> (path, format); the format defaults to the input's own, nv12 for p010."""
    head, _, tail = spec.rpartition(":")
    if head and tail.lower() in ("nv12", "nv21", "i420"):
        return Path(head), tail.lower()
    return Path(spec), "nv12" if input_format == "p010" else input_format


def annotate_group(model, raw, args, zoom, polygons, out, **space):
    """frames.annotate_frames for the demos -> per frame (count, map, picture, points or None, score, total peaks, (region counts, areas) or
    None).  The counts are count_frames', the points locate_maps' with the demo's settings."""
    sizes = [(r.shape[1], r.shape[0]) for r in raw]
    res = frames.annotate_frames(model, raw, None, out=out, points=args.points, regions=polygons, normalization=False,
                                 radius=args.points_radius, rel_threshold=args.points_rel_threshold, keep=args.points_keep, zoom=zoom,
                                 zoom_max=args.zoom_max, band_stride=args.band_stride, **space)
    results = [(c, dm) for c, dm, _pic, _p, _s in res]
    totals = [None] * len(raw)
    if args.points:                     # the number of peaks found, for points_<stem>.json: the peak finder once more, no forward
        ks = frames.frame_zooms(raw, None, zoom, args.zoom_max) if zoom != 1 else [1] * len(raw)
        totals = [t for _p, _s, t in frames.locate_maps(results, sizes, radius=args.points_radius, rel_threshold=args.points_rel_threshold,
                                                        keep=args.points_keep, new_h=[frames.NEW_H * k for k in ks])]
    summed = [None] * len(raw)
    if polygons is not None:
        summed = frames.region_maps(results, sizes, None, polygons)
    torch.cuda.synchronize()
    return [(c, dm, pic, pts, score, total, reg) for (c, dm, pic, pts, score), total, reg in zip(res, totals, summed)]


def parse_yuv(spec):
    """--yuv FORMAT:WxH[:MATRIX[:RANGE[:CHROMA]]] -> (W, H, YuvFrame keywords)."""
    parts = spec.lower().split(":")
    names = ("format", "matrix", "range", "chroma")
    tables = (yuv.FORMATS, yuv.MATRICES, yuv.RANGES, yuv.CHROMAS)
    try:
        if not 2 <= len(parts) <= 5:
            raise ValueError("FORMAT:WxH[:MATRIX[:RANGE[:CHROMA]]]")
        w, h = (int(v) for v in parts[1].split("x"))
        kw = dict(zip(names, parts[:1] + parts[2:]))
        for (name, value), table in zip(kw.items(), tables):
            if value not in table:
                raise ValueError("%s is one of %s" % (name, ", ".join(table)))
        if not (1 <= w <= yuv.MAX_SIDE and 1 <= h <= yuv.MAX_SIDE):
            raise ValueError("W and H are 1..%d" % yuv.MAX_SIDE)
    except ValueError as e:
        raise SystemExit("--yuv %s: %s" % (spec, e))
    return w, h, kw


def read_clip(path, w, h, kw, max_frames=None):
    """The packed frames of a raw clip as YuvFrame views of one host array."""
    size = yuv.frame_bytes(kw["format"], w, h)
    total = path.stat().st_size
    if total == 0 or total % size:
        raise SystemExit("%s: %d bytes are %d frames of %d bytes (%s %dx%d) and an incomplete frame of %d bytes"
                         % (path, total, total // size, size, kw["format"], w, h, total % size))
    n = total // size if max_frames is None else min(total // size, max_frames)
    data = np.fromfile(path, dtype=np.uint8, count=n * size)
    return [yuv.YuvFrame.from_buffer(data[k * size:(k + 1) * size], w, h, **kw) for k in range(n)]


def run_yuv(args, model, device, zoom, region_names, polygons, clip):
    """--yuv: the clip's frames, --group_images at a time, through frames.count_frames on YuvFrame views."""
    h, w, _ = clip[0].shape
    stem = args.input_path.stem
    prep = frames.frame_prep(device)
    group = max(args.group_images, 1)
    out_file = None
    if args.out_yuv is not None:
        out_path, out_format = parse_out_yuv(args.out_yuv, clip[0].format)
        out_file = open(out_path, "wb")
    for g0 in range(0, len(clip), group):
        raw = clip[g0:g0 + group]
        t0 = time.perf_counter()
        if out_file is not None or args.device_viz:
            got = annotate_group(model, raw, args, zoom, polygons, out_format if out_file is not None else "rgb")
            dt = (time.perf_counter() - t0) / len(raw)
            for k, (f, (pred_cnt, dm, pic, pts, score, total, reg)) in enumerate(zip(raw, got)):
                name = "%s_%d" % (stem, g0 + k)
                pic = pic.cpu().numpy()
                if out_file is not None:
                    out_file.write(pic.tobytes())
                if pts is not None:
                    write_points(args.output_path / ("points_%s.json" % name), pred_cnt, total, pts, score)
                if args.device_viz and not args.no_viz:
                    if out_file is not None:
                        pic = yuv.yuv_host(yuv.YuvFrame.from_buffer(pic, w, h, format=out_format, matrix=f.matrix, range=f.range))
                    Image.fromarray(pic).save(args.output_path / ("viz_%s.jpg" % name))
                print("%s#%d: Count: %s - Time: %s" % (stem, g0 + k, pred_cnt, dt))
                if reg is not None:
                    report_regions(args.output_path / ("regions_%s.json" % name), pred_cnt, region_names, reg[0], reg[1])
            continue
        if zoom != 1:
            got = count_zoomed(model, raw, None, zoom, args, False)
        else:
            results = frames.count_frames(model, raw, normalization=False)
            located = [(None, None, None)] * len(raw)
            if args.points:
                located = frames.locate_maps(results, [(w, h)] * len(raw), radius=args.points_radius, rel_threshold=args.points_rel_threshold,
                                             keep=args.points_keep)
            summed = [None] * len(raw)
            if polygons is not None:
                summed = frames.region_maps(results, [(w, h)] * len(raw), None, polygons)
            torch.cuda.synchronize()
            got = [(c, dm, pts, score, total, None, 1) for (c, dm), (pts, score, total) in zip(results, located)]
        dt = (time.perf_counter() - t0) / len(raw)
        for k, (f, (pred_cnt, dm, pts, score, total, sample, zk)) in enumerate(zip(raw, got)):
            name = "%s_%d" % (stem, g0 + k)
            if pts is not None:
                write_points(args.output_path / ("points_%s.json" % name), pred_cnt, total, pts, score)
            if not args.no_viz:
                if zk == 1:                 # the picture of the frame: the rule on the host, resized as the model saw it
                    sample = prep.prepare([yuv.yuv_host(f)])[0][0]
                vw, vh = (sample.shape[2], sample.shape[1]) if zk > 1 else (w, h)
                save_visualisation(sample, dm.float(), pred_cnt, args.output_path / ("viz_%s.jpg" % name), vw, vh,
                                   points=points_on(pts, w, h, vw, vh) if pts is not None else None, regions=polygons if zk == 1 else None)
            print("%s#%d: Count: %s - Time: %s" % (stem, g0 + k, pred_cnt, dt))
            if zoom == 1 and polygons is not None:
                reg = summed[k]
                report_regions(args.output_path / ("regions_%s.json" % name), pred_cnt, region_names, reg[0], reg[1])
    if out_file is not None:
        out_file.close()


def load_lines(path):
    """--lines_json -> (names, [(ax, ay, bx, by), ...]); ([], []) without the flag."""
    if path is None:
        return [], []
    named = json.load(open(path))
    if not isinstance(named, dict) or not all(np.shape(v) == (2, 2) for v in named.values()):
        raise ValueError('--lines_json: a JSON object {"name": [[ax, ay], [bx, by]], ...}')
    return list(named), [(float(a[0]), float(a[1]), float(b[0]), float(b[1])) for a, b in named.values()]


def cam_text(where):
    """` - cam: [x, y]` of a frame counted with --camera, nothing without."""
    return " - cam: %s" % json.dumps([float(v) for v in where[0]]) if where else ""


def add_camera(doc, counter):
    """"camera": {"end": [x, y], "lost": n} of a clip counted with --camera."""
    if counter is not None and counter.camera is not None:
        path = counter.camera_path()
        end = path.position(-1, counter.placement) if len(path.path) else (0.0, 0.0)
        doc["camera"] = {"end": [float(v) for v in end], "lost": path.lost}


def run_track(args, model, device, clip):
    """--yuv --track: the clip's frames, --group_images at a time, through frames.count_clip with one tracker kept over the groups."""
    from countr_amd.tracks import Tracker
    h, w, _ = clip[0].shape
    stem = args.input_path.stem
    prep = frames.frame_prep(device)
    group = max(args.group_images, 1)
    names, lines = load_lines(args.lines_json)
    tracker = Tracker(device, max_dist=args.track_dist, max_missed=args.track_missed, min_hits=args.track_hits, lines=lines)
    peak = dict(radius=args.points_radius, rel_threshold=args.points_rel_threshold, keep=args.points_keep)
    clip_counts, counter = None, None
    if args.camera:
        from countr_amd.flow import FlowCounter
        counter = FlowCounter(device, lines=(), search=args.flow_search, interval=args.flow_interval, camera=args.camera)
    out_file, out_format, trails = None, "rgb", None
    if args.out_yuv is not None:
        out_path, out_format = parse_out_yuv(args.out_yuv, clip[0].format)
        out_file = open(out_path, "wb")
    drawn = out_file is not None or args.device_viz          # the annotated clip: ids, trails, lines and tallies composed on the device
    if drawn and args.trail:
        from countr_amd.draw import Trails
        trails = Trails(args.trail)
    for g0 in range(0, len(clip), group):
        raw = clip[g0:g0 + group]
        t0 = time.perf_counter()
        pics = [None] * len(raw)
        if drawn:
            (got, clip_counts), = frames.annotate_clip(model, raw, max_dist=args.track_dist, group=group, tracker=tracker, normalization=False,
                                                       summaries=True, counter=counter, line_names=names, out=out_format, trail=args.trail,
                                                       trails=trails, tags=not args.no_tags, scale=args.mark_scale, **peak)
            pics = [r[6].cpu().numpy() for r in got]
            got = [r[:6] + r[7:] for r in got]
        else:
            got, clip_counts = frames.count_clip(model, raw, max_dist=args.track_dist, group=group, tracker=tracker, normalization=False,
                                                 summaries=True, counter=counter, **peak)
        dt = (time.perf_counter() - t0) / len(raw)
        # the number of peaks found, for points_<stem>.json: the peak finder once more, no forward
        totals = [t for _p, _s, t in frames.locate_maps([(r[0], r[1]) for r in got], [(w, h)] * len(raw), **peak)]
        for k, (f, (pred_cnt, dm, pts, score, ids, events, summary, *where), total) in enumerate(zip(raw, got, totals)):
            name = "%s_%d" % (stem, g0 + k)
            write_points(args.output_path / ("points_%s.json" % name), pred_cnt, total, pts, score, ids)
            if out_file is not None:
                out_file.write(pics[k].tobytes())
            if args.device_viz:
                if not args.no_viz:
                    pic = pics[k]
                    if out_file is not None:
                        pic = yuv.yuv_host(yuv.YuvFrame.from_buffer(pic, w, h, format=out_format, matrix=f.matrix, range=f.range))
                    Image.fromarray(pic).save(args.output_path / ("viz_%s.jpg" % name))
            elif not args.no_viz:
                sample = prep.prepare([yuv.yuv_host(f)])[0][0]
                save_visualisation(sample, dm.float(), pred_cnt, args.output_path / ("viz_%s.jpg" % name), w, h, points=pts, lines=lines)
            crossed = {n: [int(((events >> j) & 1).sum()), int(((events >> (16 + j)) & 1).sum())] for j, n in enumerate(names)}
            print("%s#%d: Count: %s - Time: %s - tracks: %d - crossed: %s%s" % (stem, g0 + k, pred_cnt, dt, int(summary[0]), json.dumps(crossed),
                                                                               cam_text(where)))
    if out_file is not None:
        out_file.close()
    doc = {"clip": {"started": clip_counts.started, "confirmed": clip_counts.confirmed,
                    "lines": {n: [int(v) for v in clip_counts.line_counts[j]] for j, n in enumerate(names)}}}
    add_camera(doc, counter)
    print(json.dumps(doc))
    with open(args.output_path / ("tracks_%s.json" % stem), "w") as f:
        json.dump(doc, f)


def run_flow(args, model, device, clip):
    """--yuv --flow: the clip's frames, --group_images at a time, through frames.count_flow with one FlowCounter kept over the groups."""
    from countr_amd.flow import FlowCounter
    h, w, _ = clip[0].shape
    stem = args.input_path.stem
    prep = frames.frame_prep(device)
    group = max(args.group_images, 1)
    names, lines = load_lines(args.lines_json)
    counter = FlowCounter(device, lines=lines, search=args.flow_search, interval=args.flow_interval, band=args.flow_band, camera=args.camera)
    for g0 in range(0, len(clip), group):
        raw = clip[g0:g0 + group]
        t0 = time.perf_counter()
        got, _counts = frames.count_flow(model, raw, lines=None, group=group, counter=counter, normalization=False)
        dt = (time.perf_counter() - t0) / len(raw)
        for k, (f, (pred_cnt, dm, flux, *where)) in enumerate(zip(raw, got)):
            name = "%s_%d" % (stem, g0 + k)
            if not args.no_viz:
                sample = prep.prepare([yuv.yuv_host(f)])[0][0]
                save_visualisation(sample, dm.float(), pred_cnt, args.output_path / ("viz_%s.jpg" % name), w, h, lines=lines)
            share = None if flux is None else {n: [float(flux[j, 0]), float(flux[j, 1])] for j, n in enumerate(names)}
            print("%s#%d: Count: %s - Time: %s - flux: %s%s" % (stem, g0 + k, pred_cnt, dt, json.dumps(share), cam_text(where)))
    total = counter.counts().line_counts
    doc = {"clip": {"flux": {n: [float(total[j, 0]), float(total[j, 1])] for j, n in enumerate(names)}}}
    add_camera(doc, counter)
    print(json.dumps(doc))
    with open(args.output_path / ("flow_%s.json" % stem), "w") as f:
        json.dump(doc, f)


def main():
    p = ArgumentParser()
    p.add_argument("--input_path", type=Path, required=True)
    p.add_argument("--output_path", type=Path, default="results")
    p.add_argument("--model_path", type=str, default="weights/FSC147.pth")
    p.add_argument("--group_images", type=int, default=8, help="images whose windows share one forward (8 x 1920x1080 = 32 windows)")
    p.add_argument("--precision", default="bf16", choices=["bf16", "fp16", "fp32"])
    p.add_argument("--no_viz", action="store_true", help="counts only, no viz_*.jpg")
    p.add_argument("--device_prep", action="store_true",
                   help="hand the decoded uint8 frames to the device and resize them there (countr_amd.frames) instead of with PIL on the host")
    add_points_args(p)
    add_regions_args(p)
    add_zoom_args(p)
    p.add_argument("--yuv", default=None, metavar="FORMAT:WxH[:MATRIX[:RANGE[:CHROMA]]]",
                   help="--input_path is a raw clip of packed nv12 / nv21 / i420 / p010 frames, converted to RGB on the device")
    p.add_argument("--max_frames", type=int, default=None, help="with --yuv: read the first N frames of the clip")
    p.add_argument("--out_yuv", default=None, metavar="FILE[:FORMAT]",
                   help="with --yuv: write the annotated clip as raw nv12 / nv21 / i420 frames, composed on the device")
    p.add_argument("--device_viz", action="store_true", help="viz_*.jpg from the device-composed RGB at the input's size")
    p.add_argument("--track", action="store_true", help="with --yuv: join the frames' points over time (implies --points)")
    p.add_argument("--track_dist", type=float, default=None, help="with --track: the largest move between two frames, in pixels of the frame")
    p.add_argument("--lines_json", type=Path, default=None, help='with --track: counting lines {"name": [[ax, ay], [bx, by]], ...}, up to 16')
    p.add_argument("--track_missed", type=int, default=2, help="a track survives this many frames without a detection (the default is unmeasured)")
    p.add_argument("--track_hits", type=int, default=3, help="detections that confirm a track (the default is unmeasured)")
    p.add_argument("--trail", type=int, default=16, help="with --track and --out_yuv or --device_viz: positions of a track's drawn trail (0 = none)")
    p.add_argument("--no_tags", action="store_true", help="with --track and --out_yuv or --device_viz: no id beside the points")
    p.add_argument("--mark_scale", type=int, default=None, help="with --track and --out_yuv or --device_viz: the marks' size 1..8 (default by the height)")
    p.add_argument("--flow", action="store_true", help="with --yuv and --lines_json: line crossings from the flux of the density map")
    p.add_argument("--flow_search", type=int, default=4, help="with --flow: the motion search radius in map pixels (the default is unmeasured)")
    p.add_argument("--flow_interval", type=int, default=1, help="with --flow: match against the frame this many frames back (slow motion needs > 1)")
    p.add_argument("--flow_band", type=float, default=None, help="with --flow: the counting band in pixels of the frame (default 8 H / 384, unmeasured)")
    p.add_argument("--camera", default=None, choices=["translation"],
                   help="with --flow or --track: count in scene coordinates under a panning camera (the estimate's settings are unmeasured)")
    args = p.parse_args()
    if args.camera is not None and not (args.flow or args.track):
        p.error("--camera is for --flow or --track")
    if args.out_yuv is not None and not args.yuv:
        p.error("--out_yuv is for --yuv")
    zoom = parse_zoom(args)
    if args.track:
        if not args.yuv or args.track_dist is None:
            p.error("--track is for --yuv and needs --track_dist")
        if zoom != 1 or args.regions_json is not None:
            p.error("--track is for --zoom 1, without --regions_json")
        if args.trail < 0 or (args.mark_scale is not None and not 1 <= args.mark_scale <= 8):
            p.error("--trail is >= 0 and --mark_scale is 1..8")
        args.points = True
    elif args.flow:
        if not args.yuv or args.lines_json is None or args.track_dist is not None:
            p.error("--flow is for --yuv, needs --lines_json and excludes --track")
        if zoom != 1 or args.regions_json is not None or args.out_yuv is not None or args.device_viz or args.points:
            p.error("--flow is for --zoom 1, without --points, --regions_json, --out_yuv and --device_viz")
    elif args.track_dist is not None or args.lines_json is not None:
        p.error("--track_dist and --lines_json are for --track or --flow")
    if args.flow and args.track:
        p.error("--flow excludes --track")
    if zoom != 1 and args.regions_json is not None:
        p.error("--regions_json is for --zoom 1")
    clip = None
    if args.yuv:                      # read before the model is built: a truncated clip fails at once
        yw, yh, ykw = parse_yuv(args.yuv)
        clip = read_clip(args.input_path, yw, yh, ykw, args.max_frames)
    args.output_path.mkdir(exist_ok=True, parents=True)
    device = torch.device("cuda")
    region_names, polygons = load_regions(args.regions_json)

    if not args.model_path:
        torch.manual_seed(0)          # dry runs without a checkpoint: the same random model every time
    model = models_mae_cross.__dict__["mae_vit_base_patch16"](norm_pix_loss="store_true", precision=args.precision)
    if args.model_path:
        checkpoint = torch.load(args.model_path, map_location="cpu", weights_only=False)   # raises if the file is missing, as upstream
        model.load_state_dict(checkpoint["model"], strict=False)
        print("Resume checkpoint %s" % args.model_path)
    model.to(device).eval()

    if args.track:
        return run_track(args, model, device, clip)
    if args.flow:
        return run_flow(args, model, device, clip)
    if args.yuv:
        return run_yuv(args, model, device, zoom, region_names, polygons, clip)
    if args.input_path.is_dir():
        inputs = sorted(chain(args.input_path.glob("*.jpg"), args.input_path.glob("*.png")))
    else:
        inputs = [args.input_path]
    done = 0
    for g0 in range(0, len(inputs), max(args.group_images, 1)):
        paths = inputs[g0:g0 + max(args.group_images, 1)]
        if args.device_viz:           # the picture composed on the device from the decoded frame's own pixels
            raw = [np.asarray(Image.open(pth).convert("RGB"), dtype=np.uint8) for pth in paths]
            t0 = time.perf_counter()
            got = annotate_group(model, raw, args, zoom, polygons, "rgb")
            dt = (time.perf_counter() - t0) / len(paths)
            for pth, (pred_cnt, dm, pic, pts, score, total, reg) in zip(paths, got):
                done += 1
                if pts is not None:
                    write_points(args.output_path / ("points_%s.json" % pth.stem), pred_cnt, total, pts, score)
                if not args.no_viz:
                    Image.fromarray(pic.cpu().numpy()).save(args.output_path / ("viz_%s.jpg" % pth.stem))
                if len(inputs) > 1:
                    print("[%3d/%d] %s:\tcount = %5.2f  -  time = %5.2f" % (done, len(inputs), pth.name, pred_cnt, dt))
                else:
                    print("Count:", pred_cnt, "- Time:", dt)
                if reg is not None:
                    report_regions(args.output_path / ("regions_%s.json" % pth.stem), pred_cnt, region_names, reg[0], reg[1])
            continue
        if zoom != 1:                 # from the image's own pixels: the decoded frames go to the device as they are
            raw = [np.asarray(Image.open(pth).convert("RGB"), dtype=np.uint8) for pth in paths]
            t0 = time.perf_counter()
            got = count_zoomed(model, raw, None, zoom, args, False)
            dt = (time.perf_counter() - t0) / len(paths)
            for pth, r, (pred_cnt, dm, pts, score, total, sample, k) in zip(paths, raw, got):
                done += 1
                old_w, old_h = r.shape[1], r.shape[0]
                if pts is not None:
                    write_points(args.output_path / ("points_%s.json" % pth.stem), pred_cnt, total, pts, score)
                if not args.no_viz:
                    w, h = (sample.shape[2], sample.shape[1]) if k > 1 else (old_w, old_h)      # a zoomed picture stays at its size
                    save_visualisation(sample, dm.float(), pred_cnt, args.output_path / ("viz_%s.jpg" % pth.stem), w, h,
                                       points=points_on(pts, old_w, old_h, w, h) if pts is not None else None)
                if len(inputs) > 1:
                    print("[%3d/%d] %s:\tcount = %5.2f  -  time = %5.2f" % (done, len(inputs), pth.name, pred_cnt, dt))
                else:
                    print("Count:", pred_cnt, "- Time:", dt)
            continue
        if args.device_prep:
            raw = [np.asarray(Image.open(pth).convert("RGB"), dtype=np.uint8) for pth in paths]      # decoding stays on the host
            t0 = time.perf_counter()
            items = frames.prepare_items(device, raw)
            loaded = [(im[0], None, r.shape[1], r.shape[0]) for (im, _b, _p), r in zip(items, raw)]
        else:
            loaded = [load_image(pth) for pth in paths]
            t0 = time.perf_counter()
            items = [(s.unsqueeze(0).to(device, non_blocking=True), b.unsqueeze(0).to(device), None) for s, b, _w, _h in loaded]
        results = inference.count_images(model, items, normalization=False)
        located = [None] * len(paths)
        if args.points:
            located = frames.locate_maps(results, [(w, h) for _s, _b, w, h in loaded], radius=args.points_radius,
                                         rel_threshold=args.points_rel_threshold, keep=args.points_keep)
        summed = [None] * len(paths)
        if polygons is not None:
            sizes = [(w, h) for _s, _b, w, h in loaded]
            summed = frames.region_maps(results, sizes, None, polygons)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / len(paths)
        for pth, (sample, _b, old_w, old_h), (pred_cnt, dm), loc, reg in zip(paths, loaded, results, located, summed):
            done += 1
            if loc is not None:
                write_points(args.output_path / ("points_%s.json" % pth.stem), pred_cnt, loc[2], loc[0], loc[1])
            if not args.no_viz:
                save_visualisation(sample.to(device), dm.float(), pred_cnt, args.output_path / ("viz_%s.jpg" % pth.stem), old_w, old_h,
                                   points=loc[0] if loc is not None else None, regions=polygons)
            if len(inputs) > 1:
                print("[%3d/%d] %s:\tcount = %5.2f  -  time = %5.2f" % (done, len(inputs), pth.name, pred_cnt, dt))
            else:
                print("Count:", pred_cnt, "- Time:", dt)
            if reg is not None:
                report_regions(args.output_path / ("regions_%s.json" % pth.stem), pred_cnt, region_names, reg[0], reg[1])


if __name__ == "__main__":
    main()
