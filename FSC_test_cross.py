#!/usr/bin/env python3
"""Few-/zero-shot evaluation CLI with the reference's flags (FSC_test_cross(few-shot).py:26-78), running the MI355X engine.

`--box_bound 0` = zero-shot.  With the FSC147 files present (--data_path/--anno_file/--data_split_file/--im_dir) images are
loaded as TestData does (countr_amd/data/fsc147.py::test_item, pinned against the reference class in tests/golden/data_test.npz;
`--external`: the split's own exemplar crops, cut to --box_bound, serve every image -- :96-129).
Without a dataset (none is available offline) `--synthetic N` evaluates N synthetic wide images through the same
sliding-window / stitching / normalisation code (countr_amd/inference.py).
`--localize` scores WHERE the objects are: the peaks of the density maps (frames.locate_maps) are matched one to one to the annotated dots
(countr_amd/match.py states the rule; csrc/match.hip computes it) and precision / recall / F1 are printed per image and over the run, at
the distances of --localize_dist in pixels of the 384-high evaluated image.  Off by default; without it the output is unchanged.
`--game L` (0..3) adds the grid average mean absolute error, a localisation-aware figure that needs no peak finder and so none of its
settings: GAME(l) = the mean over images of the sum over the 2^l x 2^l cells of |predicted count in the cell - dots in the cell|; GAME(0)
is the MAE.  The per-cell predictions are sums of the density maps the run already has (the nine crop maps of the 3 x 3 path included) over
the level-L grid, on the device (countr_amd.frames.region_maps, one RegionSummer.sum per group of images), scaled so that they add up to
the printed count; the levels below L are sums of those level-L cell values computed in fp64 on the host.
`--report` writes the reference's evaluation report into --output_dir (:379-453: full_<stem>__<count>.png and boxes_<stem>.png per image,
results.csv, log.txt, test_stat.png), composed on the device (countr_amd/report.py); without it nothing is written."""
import argparse
import json
import os
import time

import numpy as np
import torch

import models_mae_cross
from countr_amd import inference
from countr_amd.util import misc


def get_args_parser():
    p = argparse.ArgumentParser("CounTR testing (MI355X engine)", add_help=True)
    p.add_argument("--model", default="mae_vit_base_patch16", type=str)
    p.add_argument("--mask_ratio", default=0.5, type=float)
    p.add_argument("--norm_pix_loss", action="store_true")
    p.add_argument("--data_path", default="./data/FSC147/", type=str)
    p.add_argument("--anno_file", default="annotation_FSC147_384.json", type=str)
    p.add_argument("--data_split_file", default="Train_Test_Val_FSC_147.json", type=str)
    p.add_argument("--im_dir", default="images_384_VarV2", type=str)
    p.add_argument("--output_dir", default="./Image")
    p.add_argument("--device", default="cuda")
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--resume", default="./output_fim6_dir/checkpoint-0.pth")
    p.add_argument("--external", action="store_true")
    p.add_argument("--box_bound", default=-1, type=int)
    p.add_argument("--split", default="test", type=str)
    p.add_argument("--max_s_cnt", default=1, type=int)
    p.add_argument("--num_workers", default=0, type=int)
    p.add_argument("--pin_mem", action="store_true")
    p.add_argument("--no_pin_mem", action="store_false", dest="pin_mem")
    p.set_defaults(pin_mem=True)
    p.add_argument("--normalization", default=True)
    p.add_argument("--world_size", default=1, type=int)
    p.add_argument("--local_rank", default=-1, type=int)
    p.add_argument("--dist_on_itp", action="store_true")
    p.add_argument("--dist_url", default="env://")
    # additions
    p.add_argument("--precision", default="fp32", choices=["fp32", "bf16", "fp16"], help="the reference tests in fp32")
    p.add_argument("--synthetic", default=0, type=int, help="evaluate N synthetic images instead of FSC147")
    p.add_argument("--group_images", default=8, type=int, help="images whose sliding windows share forward batches (up to 32 windows each)")
    p.add_argument("--report", action="store_true", help="write the reference's evaluation report (pictures, results.csv, log.txt, test_stat.png) into --output_dir")
    p.add_argument("--report_workers", default=4, type=int, help="threads that encode the report's PNGs (at most 8)")
    p.add_argument("--localize", action="store_true", help="match the density maps' peaks to the annotated dots: precision / recall per image and over the run")
    p.add_argument("--localize_dist", default="4,8,16", type=str, help="comma-separated matching distances, in pixels of the 384-high evaluated image")
    p.add_argument("--localize_box_scale", default=0.0, type=float, help="> 0: a further per-image distance, this factor x the mean shorter side of the image's exemplar rectangles")
    p.add_argument("--game", default=-1, type=int, choices=[-1, 0, 1, 2, 3],
                   help="L: print GAME(0..L) per image and over the run; the density maps are summed over the 2^L x 2^L grid on the device, and "
                        "the levels below L are sums of level-L cell values computed in fp64 on the host (-1: off)")
    p.add_argument("--points_radius", default=4, type=int, help="peak window radius (locate_frames' radius)")
    p.add_argument("--points_rel_threshold", default=0.1, type=float, help="peaks below this fraction of the map maximum are dropped")
    p.add_argument("--points_keep", default="all", choices=["all", "count"], help='"count": keep the first floor(count + 0.5) peaks by score')
    return p


def localize_distances(text):
    """--localize_dist -> the distances, each finite and > 0."""
    dists = [float(t) for t in str(text).split(",") if t.strip()]
    if not dists or not all(np.isfinite(d) and d > 0 for d in dists):
        raise ValueError("--localize_dist: comma-separated distances > 0")
    return dists


def box_distance(pos, scale):
    """--localize_box_scale: scale x the mean shorter side of the exemplar rectangles (y1, x1, y2, x2), inclusive; None without any."""
    if scale <= 0 or not pos:
        return None
    return scale * float(np.mean([min(y2 - y1, x2 - x1) + 1 for y1, x1, y2, x2 in pos]))


def main(args):
    misc.init_distributed_mode(args)
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    device = torch.device(args.device)
    model = models_mae_cross.__dict__[args.model](norm_pix_loss=args.norm_pix_loss, precision=args.precision)
    misc.load_model_FSC(args, model)
    model.to(device).eval()
    items = []
    if args.synthetic:
        rs = np.random.RandomState(args.seed)
        for i in range(args.synthetic):
            w = 16 * int(rs.randint(24, 60))
            img = torch.from_numpy(rs.uniform(0, 1, size=(3, 384, w)).astype(np.float32))
            k = 3 if args.box_bound < 0 else min(args.box_bound, 3)
            boxes = torch.from_numpy(rs.uniform(0, 1, size=(k, 3, 64, 64)).astype(np.float32)) if k else torch.zeros(0)
            pos = [(10 * j, 10 * j, 10 * j + 40, 10 * j + 40) for j in range(k)]
            gt_cnt = int(rs.randint(5, 200))
            gt_map = pts = None
            if args.report or args.localize or args.game >= 0:       # a generator of its own: the images and counts above are those of a run without the flags
                ds = np.random.RandomState(args.seed + 1000003 * (i + 1))
                rows, cols = ds.randint(0, 384, gt_cnt), ds.randint(0, w, gt_cnt)      # (rows first: the two flags describe the same objects)
                pts = np.stack([cols, rows], 1).astype(np.float32)
            if args.report:
                from scipy import ndimage
                dots = np.zeros((384, w), dtype=np.float32)
                dots[rows, cols] = 1
                gt_map = torch.from_numpy(ndimage.gaussian_filter(dots, sigma=(1, 1), order=0)) * 60
            items.append(("synthetic_%d" % i, img, boxes, pos, gt_cnt, gt_map, pts))
    else:
        from countr_amd.data import fsc147
        annotations = json.load(open(os.path.join(args.data_path, args.anno_file)))
        split = json.load(open(os.path.join(args.data_path, args.data_split_file)))[args.split]
        im_dir = os.path.join(args.data_path, args.im_dir)
        ext = None
        if args.external:     # FSC_test_cross(few-shot).py:96-129: the split's own exemplar crops, cut to --box_bound, for every image
            ext = fsc147.external_exemplars(annotations, split, im_dir, args.box_bound)
        for im_id in split:
            img, dots, boxes, pos, gt_map = fsc147.test_item(annotations, im_dir, im_id, args.box_bound, ext)
            items.append((im_id, img, boxes, [tuple(r) for r in pos], dots.shape[0], gt_map if args.report else None,
                          fsc147.test_dots(annotations, im_dir, im_id) if args.localize or args.game >= 0 else None))
    from countr_amd.parallel import shard_batch
    lo, hi = shard_batch(len(items), misc.get_rank(), misc.get_world_size())   # replicas only: images sharded, no collective
    mae = rmse = nae = 0.0
    # windows are batched ACROSS images (every 384-px window is an independent forward): groups of --group_images images go
    # through inference.count_images together
    mine = items[lo:hi]
    writer = None
    if args.report:      # every rank writes the pictures of its own images; rank 0 writes the summary files (of its shard, as the reference's does)
        from countr_amd.report import ReportItem, ReportWriter
        writer = ReportWriter(args.output_dir, workers=args.report_workers, external=args.external, summary=misc.is_main_process())
    dists, located = (localize_distances(args.localize_dist), []) if args.localize else (None, None)
    games = []
    t0 = time.time()
    preds = []
    for g0 in range(0, len(mine), args.group_images):
        grp = mine[g0:g0 + args.group_images]
        its = [(img.unsqueeze(0).to(device), boxes.unsqueeze(0).to(device), pos) for _name, img, boxes, pos, _gt, _map, _pts in grp]
        if writer is None and not args.localize and args.game < 0:
            preds += [p for p, _dm in inference.count_images(model, its, normalization=bool(args.normalization), max_s_cnt=args.max_s_cnt)]
            continue
        res = inference.count_images(model, its, normalization=bool(args.normalization), max_s_cnt=args.max_s_cnt, return_crops=True)
        preds += [r[0] for r in res]
        if args.localize:
            located += localize_group(args, dists, grp, res)
        if args.game >= 0:
            games += game_group(args.game, grp, res)
        for c0 in range(0, len(grp), 16) if writer is not None else ():      # (a report launch takes 16 images); the encodes overlap the next group's forward
            writer.add_group([ReportItem(name, s, b, pos, gt_cnt, gt_map) for (name, _i, _b, pos, gt_cnt, gt_map, _pts), (s, b, _p)
                              in zip(grp[c0:c0 + 16], its[c0:c0 + 16])], res[c0:c0 + 16])
    torch.cuda.synchronize()
    t_inf = time.time() - t0
    for (name, _img, _boxes, _pos, gt_cnt, _map, _pts), pred in zip(mine, preds):
        err = abs(pred - gt_cnt)
        mae += err; rmse += err ** 2; nae += err / gt_cnt if gt_cnt > 0 else 0
        print("%s: pred_cnt: %5.3f, gt_cnt: %5.3f, error: %5.3f" % (name, pred, gt_cnt, err))
    n = max(hi - lo, 1)
    print(json.dumps({"MAE": mae / n, "RMSE": (rmse / n) ** 0.5, "NAE": nae / n, "images": hi - lo, "mean_infer_time_s": t_inf / n}))
    columns = None
    if args.localize:
        columns = print_localization(args, dists, [it[0] for it in mine], located)
    if args.game >= 0:
        header, cells = print_game(args.game, [it[0] for it in mine], games)
        columns = (header, cells) if columns is None else (columns[0] + header, {k: v + cells[k] for k, v in columns[1].items()})
    if writer is not None:
        writer.close(timing={"Mean infer time": t_inf / n, "Mean overall time": (time.time() - t0) / n}, columns=columns)


def localize_group(args, dists, grp, res):
    """The points of one group's maps (the nine crop maps of the 3 x 3 path included) against the group's dots: ONE matcher run per image
    at its largest distance; the smaller distances are read off the same matching (the prefix property of the rule).
    -> per image (P, G, rows of localization_metrics, labels)."""
    from countr_amd import frames, match
    # sizes = the evaluated image's own: frame_points is then the identity, and points and dots share one coordinate system
    pts = frames.locate_maps(res, [(int(r[1].shape[1]), frames.NEW_H) for r in res], radius=args.points_radius,
                             rel_threshold=args.points_rel_threshold, keep=args.points_keep)
    use, sets = [], []
    for (_name, _img, _boxes, pos, _gt, _map, dots), (xy, _score, _total) in zip(grp, pts):
        box = box_distance(pos, args.localize_box_scale)
        use.append(dists + ([box] if box is not None else []))
        sets.append((xy, dots, max(use[-1])))
    out = []
    for (xy, dots, _md), d, (_m, d2, _cnt) in zip(sets, use, match.point_matcher(res[0][1].device).match(sets)):
        labels = ["%g" % v for v in dists] + (["box"] if len(d) > len(dists) else [])
        out.append((len(xy), len(dots), match.localization_metrics(d2, len(xy), len(dots), d), labels))
    return out


def game_group(L, grp, res):
    """GAME(0..L) of one group's images: ONE RegionSummer.sum over the group's maps (the nine crop maps of the 3 x 3 path add into their
    image's cells) on the level-L grid of each 384-high image; the dots are binned by the grid's own half-open rule on the host.
    -> per image [GAME(0), ..., GAME(L)]."""
    from countr_amd import frames, regions
    sizes = [(int(r[1].shape[1]), frames.NEW_H) for r in res]      # the evaluated image's own size: the placement is the identity
    grids = [regions.game_grid(h, w, L) for w, h in sizes]
    cells = frames.region_maps([(r[0], r[1]) for r in res], sizes, [r[2] for r in res], [[g] for g in grids])
    n = 1 << L
    return [regions.game_levels(counts.reshape(n, n), regions.grid_dot_counts(it[6], g)) for it, g, (counts, _area) in zip(grp, grids, cells)]


def print_game(L, names, games):
    """One line per image, then the run's (this rank's shard's) {"GAME": ...} line -> the results.csv columns of --report."""
    header = ["game_%d" % l for l in range(L + 1)]
    cells = {}
    for name, g in zip(names, games):
        print("%s: game: %s" % (name, json.dumps({str(l): v for l, v in enumerate(g)})))
        cells[name] = ["%.4f" % v for v in g]
    n = max(len(games), 1)
    print(json.dumps({"GAME": {str(l): sum(g[l] for g in games) / n for l in range(L + 1)}, "images": len(games)}))
    return header, cells


def print_localization(args, dists, names, located):
    """One line per image, then the run's (this rank's shard's) {"localization": ...} line -> the results.csv columns of --report."""
    from countr_amd import match
    totals = match.LocalizationTotals()
    every = ["%g" % v for v in dists] + (["box"] if args.localize_box_scale > 0 else [])
    header = ["points", "dots"] + ["%s_%s" % (k, lab) for lab in every for k in ("tp", "precision", "recall")]
    cells = {}
    for name, (P, G, rows, labels) in zip(names, located):
        by = dict(zip(labels, rows))
        for lab, row in by.items():
            totals.add(lab, row, P, G)
        print("%s: localization: %s" % (name, json.dumps({"points": P, "dots": G, "dist": by})))
        cells[name] = [P, G] + [v for lab in every for v in (
            (by[lab]["tp"], "%.4f" % by[lab]["precision"], "%.4f" % by[lab]["recall"]) if lab in by else ("", "", ""))]
    print(json.dumps({"localization": {"images": len(located), "radius": args.points_radius, "rel_threshold": args.points_rel_threshold,
                                       "keep": args.points_keep, "dist": totals.summary()}}))
    return header, cells


if __name__ == "__main__":
    main(get_args_parser().parse_args())
