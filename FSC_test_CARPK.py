#!/usr/bin/env python3
"""CARPK evaluation CLI with the reference's flags (FSC_test_CARPK.py:27-90), running the MI355X engine.

The reference fetches the dataset with hub.load("hub://activeloop/carpk-test"); here `--data_path` is the CARPK devkit's `data`
directory on disk (Images/, Annotations/, ImageSets/test.txt: countr_amd/data/carpk.py), or `--synthetic N` evaluates N seeded
synthetic samples.  Per image (:153-245): the tensor resize to 384 x 683, two exemplars cut from the full-resolution frame, four
sliding windows, and the script's count rule -- all on the device (countr_amd/carpk.py::count_carpk).  The scatter plot (:269-272) is
written only when --output_dir is given; nothing is shown."""
import argparse
import json
import os
import time
from pathlib import Path

import numpy as np
import torch

import models_mae_cross
from countr_amd.carpk import count_carpk
from countr_amd.data import carpk as D
from countr_amd.util import misc


def get_args_parser():
    p = argparse.ArgumentParser("CounTR CARPK testing (MI355X engine)", add_help=True)
    p.add_argument("--batch_size", default=1, type=int)
    p.add_argument("--epochs", default=1, type=int)
    p.add_argument("--accum_iter", default=1, type=int)
    p.add_argument("--model", default="mae_vit_base_patch16", type=str)
    p.add_argument("--mask_ratio", default=0.5, type=float)
    p.add_argument("--norm_pix_loss", action="store_true")
    p.add_argument("--weight_decay", type=float, default=0.05)
    p.add_argument("--lr", type=float, default=None)
    p.add_argument("--blr", type=float, default=1e-3)
    p.add_argument("--min_lr", type=float, default=0.0)
    p.add_argument("--warmup_epochs", type=int, default=10)
    p.add_argument("--data_path", default="./data/CARPK_devkit/data", type=str, help="the devkit's data directory")
    p.add_argument("--output_dir", default="./test_dir")
    p.add_argument("--log_dir", default="./test_dir")
    p.add_argument("--device", default="cuda")
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--resume", default="./output_CARPK_dir/checkpoint-20.pth")
    p.add_argument("--start_epoch", default=0, type=int)
    p.add_argument("--num_workers", default=10, type=int)
    p.add_argument("--pin_mem", action="store_true")
    p.add_argument("--no_pin_mem", action="store_false", dest="pin_mem")
    p.set_defaults(pin_mem=True)
    p.add_argument("--world_size", default=1, type=int)
    p.add_argument("--local_rank", default=-1, type=int)
    p.add_argument("--dist_on_itp", action="store_true")
    p.add_argument("--dist_url", default="env://")
    # additions
    p.add_argument("--precision", default="fp32", choices=["fp32", "bf16", "fp16"], help="the reference tests in fp32")
    p.add_argument("--synthetic", default=0, type=int, help="evaluate N synthetic samples instead of the devkit's test split")
    p.add_argument("--group_images", default=8, type=int, help="frames whose sliding windows share one forward (4 windows each)")
    return p


def main(args):
    misc.init_distributed_mode(args)
    device = torch.device(args.device)
    seed = args.seed + misc.get_rank()          # :103-105
    torch.manual_seed(seed)
    np.random.seed(seed)
    if args.synthetic:
        data = D.Synthetic(args.synthetic, seed=args.seed)
    elif D.available(args.data_path, "test"):
        data = D.Devkit(args.data_path, "test")
    else:
        raise SystemExit("no CARPK devkit under %s (Images/, Annotations/, ImageSets/test.txt); --synthetic N runs without one" % args.data_path)
    model = models_mae_cross.__dict__[args.model](norm_pix_loss=args.norm_pix_loss, precision=args.precision)
    misc.load_model_FSC(args, model)
    model.to(device).eval()
    print("Start testing.")
    start_time = time.time()
    train_mae = train_rmse = 0.0
    error_array, gt_array = [], []
    n = len(data)
    per_call = max(1, args.group_images)
    for g0 in range(0, n, per_call):
        items = [data[k] for k in range(g0, min(g0 + per_call, n))]
        res = count_carpk(model, [it["images"] for it in items], [it["boxes"] for it in items], max_batch=4 * per_call)
        for k, (it, (pred_cnt, _dm, _stats)) in enumerate(zip(items, res)):
            gt_cnt = len(it["boxes"])           # labels.shape[1] (:245): one label per box
            cnt_err = abs(pred_cnt - gt_cnt)
            train_mae += cnt_err
            train_rmse += cnt_err ** 2
            print(f"{g0 + k}/{n}: pred_cnt: {pred_cnt},  gt_cnt: {gt_cnt},  error: {cnt_err},  AE: {cnt_err},  SE: {cnt_err ** 2} ")
            error_array.append(cnt_err)
            gt_array.append(gt_cnt)
    log_stats = {"MAE": train_mae / n, "RMSE": (train_rmse / n) ** 0.5}
    print("Current MAE: {:5.2f}, RMSE: {:5.2f} ".format(log_stats["MAE"], log_stats["RMSE"]))
    if args.output_dir and misc.is_main_process():
        with open(os.path.join(args.output_dir, "log.txt"), mode="a", encoding="utf-8") as f:
            f.write(json.dumps(log_stats) + "\n")
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
        plt.scatter(gt_array, error_array)
        plt.xlabel("Ground Truth")
        plt.ylabel("Error")
        plt.savefig(os.path.join(args.output_dir, "CAR_stat.png"))
    print("Testing time %.1fs" % (time.time() - start_time))


if __name__ == "__main__":
    args = get_args_parser().parse_args()
    if args.output_dir:
        Path(args.output_dir).mkdir(parents=True, exist_ok=True)
    main(args)
