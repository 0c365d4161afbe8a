#!/usr/bin/env python3
"""CARPK finetuning CLI with the reference's flags (FSC_finetune_CARPK.py:38-103) and its loop body (:198-270), running the MI355X engine.

The reference file does not start (it imports util.FSC147.TransformTrain, which does not exist); what is ported is its loop: batch 1,
1-shot, one random exemplar per step cut from the full-resolution frame, the left 384 columns of the 384 x 683 tensor resize, the
target from the box centres, an UNMASKED squared error (the Bernoulli mask is drawn and never used, :246-252), the per-iteration LR
schedule and util/misc.save_model's default name (checkpoint.pth).  --batch_size only enters the learning rate and the printed
averages, as upstream (:148-151, :319-332): the loader's batch is 1 (:136).  Preparation runs as HIP kernels on the step's stream
(countr_amd/carpk.py::CarpkPrep.train_sample); the step is the fused FinetuneStep with an all-ones mask.
Data: `--data_path` is the CARPK devkit's `data` directory (countr_amd/data/carpk.py), or `--synthetic N` trains on N seeded samples."""
import argparse
import json
import os
import time
from pathlib import Path

import numpy as np
import torch

import models_mae_cross
from countr_amd.carpk import CarpkPrep
from countr_amd.data import carpk as D
from countr_amd.trainer import FinetuneStep
from countr_amd.util import lr_sched, misc


def get_args_parser():
    p = argparse.ArgumentParser("CounTR CARPK finetuning (MI355X engine)", add_help=True)
    p.add_argument("--batch_size", default=8, type=int, help="enters the learning rate and the averages only; samples come one at a time")
    p.add_argument("--epochs", default=200, type=int)
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
    p.add_argument("--output_dir", default="./output_CARPK_dir")
    p.add_argument("--log_dir", default="./output_CARPK_dir")
    p.add_argument("--device", default="cuda")
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--resume", default="./output_CARPK_dir/checkpoint-6.pth")
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
    p.add_argument("--precision", default="bf16", choices=["bf16", "fp16", "fp32"])
    p.add_argument("--synthetic", default=0, type=int, help="train on N synthetic samples instead of the devkit's train split")
    return p


def main(args):
    misc.init_distributed_mode(args)
    device = torch.device("cuda", args.gpu)
    torch.cuda.set_device(device)
    seed = args.seed + misc.get_rank()          # :116-118
    torch.manual_seed(seed)
    np.random.seed(seed)
    if args.synthetic:
        data = D.Synthetic(args.synthetic, seed=args.seed)
    elif D.available(args.data_path, "train"):
        data = D.Devkit(args.data_path, "train")
    else:
        raise SystemExit("no CARPK devkit under %s (Images/, Annotations/, ImageSets/train.txt); --synthetic N runs without one" % args.data_path)
    model = models_mae_cross.__dict__[args.model](norm_pix_loss=args.norm_pix_loss, precision=args.precision)
    misc.load_model_FSC(args, model)
    model.to(device).train()
    eff_batch_size = args.batch_size * args.accum_iter * misc.get_world_size()
    if args.lr is None:
        args.lr = args.blr * eff_batch_size / 256     # :150-151
    print("base lr: %.2e" % (args.lr * 256 / eff_batch_size))
    print("actual lr: %.2e" % args.lr)
    print("accumulate grad iterations: %d" % args.accum_iter)
    print("effective batch size: %d" % eff_batch_size)
    step = FinetuneStep(model, batch=1, lr=args.lr, weight_decay=args.weight_decay, betas=(0.9, 0.95), accum_iter=args.accum_iter)
    prep = CarpkPrep(device)
    ones = torch.ones(384, 384, device=device)       # the loss is unmasked (:251-252)
    shot_num = 1                                     # :242
    n_iter = len(data)
    min_MAE = 99999
    print(f"Start training for {args.epochs} epochs")
    start_time = time.time()
    for epoch in range(args.start_epoch, args.epochs):
        train_mae = train_rmse = 0.0
        losses = []
        with step.on_stream():
            for it in range(n_iter):
                if it % args.accum_iter == 0:
                    lr = lr_sched.adjust_learning_rate(None, it / n_iter + epoch, args)      # :201-202
                item = data[it]
                idx = D.train_draw(len(item["boxes"]))                                       # :210
                imgs, boxes, gt = prep.train_sample(item["images"], item["boxes"], idx)
                D.train_mask_draw()                                                          # :246
                step.load(imgs, boxes, gt, ones, shot_num)
                sums = step.step(shot_num, lr=lr)
                s = sums.float().cpu().numpy()       # the reference reads loss.item() in every iteration too (:255)
                loss_value, pred_cnt = float(s[0]), float(s[1])
                gt_cnt = len(item["boxes"])          # labels.shape[1] (:261)
                cnt_err = abs(pred_cnt - gt_cnt)
                train_mae += cnt_err
                train_rmse += cnt_err ** 2
                losses.append(loss_value)
                print(f"{it}/{n_iter}: loss: {loss_value},  pred_cnt: {pred_cnt},  gt_cnt: {gt_cnt},  error: {cnt_err},  AE: {cnt_err},  "
                      f"SE: {cnt_err ** 2}, {shot_num}-shot, exemplar {idx} ", flush=True)
                if not np.isfinite(loss_value):
                    raise SystemExit("Loss is {}, stopping training".format(loss_value))     # :281-283
        step.flush()
        opt_state = step.optimizer_state()
        sc_state = step.scaler_state()
        denom = n_iter * args.batch_size             # :319-332 divide by len(loader) * args.batch_size
        if args.output_dir and (epoch % 20 == 0 or epoch + 1 == args.epochs):                # :315-318
            misc.save_model(args, epoch, model, opt_state, scaler_state=sc_state)
        if args.output_dir and train_mae / denom < min_MAE:                                  # :319-323
            min_MAE = train_mae / denom
            misc.save_model(args, 666, model, opt_state, scaler_state=sc_state)
        log_stats = {"train_loss": float(np.mean(losses)), "train_lr": lr, "Current MAE": train_mae / denom,
                     "RMSE": (train_rmse / denom) ** 0.5, "epoch": epoch}
        print("Current MAE: {:5.2f}, RMSE: {:5.2f} ".format(log_stats["Current MAE"], log_stats["RMSE"]))
        if args.output_dir and misc.is_main_process():
            with open(os.path.join(args.output_dir, "log.txt"), mode="a", encoding="utf-8") as f:
                f.write(json.dumps(log_stats) + "\n")
    print("Training time %.1fs" % (time.time() - start_time))


if __name__ == "__main__":
    args = get_args_parser().parse_args()
    if args.output_dir:
        Path(args.output_dir).mkdir(parents=True, exist_ok=True)
    main(args)
