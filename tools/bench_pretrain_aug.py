#!/usr/bin/env python3
"""Pretraining transform: host path against --device_aug, in one process on one GPU.

  (a) one worker's time per sample, one thread: transform_pretrain (two Pillow resizes, crop, flip, ToTensor) against recipe_pretrain
      (the draws and the copy of the decoded frame), over the same seeded samples, alternated; and the bytes either hands over
  (b) PretrainAug.batch for 16 samples at realistic frame sizes (height 384, width 384-1024): wall and device-event time, launch count,
      beside the pretraining step's own time in the same run
  (c) sustained images/s of "loader + transform + PretrainStep": host path against the recipe path, alternated, two repeats each

Frames are generated from a seed (no dataset needed); a frame is "decoded" by building it in the worker, on both paths alike.
Usage: python tools/bench_pretrain_aug.py [--batch 16] [--iters 120] [--workers 12] [--samples 24]"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from countr_amd.data import fsc147  # noqa: E402


class SynthPretrain(torch.utils.data.Dataset):
    """FSC147-shaped frames from a seed: height 384, as the dataset's images_384_VarV2 are, width 384..1024."""

    def __init__(self, n, seed, mode):
        rs = np.random.RandomState(seed)
        self.mode = mode                                # "host" | "recipe"
        self.sizes = [(384, int(rs.randint(384, 1025))) for _ in range(n)]

    def open_image(self, idx):
        from PIL import Image
        h, w = self.sizes[idx]
        rs = np.random.RandomState(idx + 77)
        x, y = np.arange(w, dtype=np.int32)[None, :], np.arange(h, dtype=np.int32)[:, None]
        arr = np.empty((h, w, 3), np.uint8)               # ramps plus 5 bits of noise: a stand-in for a decoded photograph
        arr[..., 0] = x * 223 // w
        arr[..., 1] = y * 223 // h
        arr[..., 2] = (x * 3 + y * 5) % 224
        return Image.fromarray(arr + (np.frombuffer(rs.bytes(h * w * 3), np.uint8).reshape(h, w, 3) & 31))

    def __len__(self):
        return len(self.sizes)

    def __getitem__(self, idx):
        image = self.open_image(idx)
        return fsc147.recipe_pretrain(image) if self.mode == "recipe" else fsc147.transform_pretrain(image)


def stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=120)
    ap.add_argument("--workers", type=int, default=12)
    ap.add_argument("--samples", type=int, default=24)
    ap.add_argument("--model", default="mae_vit_base_patch16")
    ap.add_argument("--precision", default="bf16")
    args = ap.parse_args()
    if args.workers > 16:
        raise SystemExit("--workers: 16 at most")
    import models_mae_noct
    from countr_amd.pretrain_aug import PretrainAug
    from countr_amd.trainer import PretrainStep
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(0)
    B = args.batch
    model = models_mae_noct.__dict__[args.model](precision=args.precision).to(dev).train()
    step = PretrainStep(model, batch=B, mask_ratio=0.5, lr=1e-4, weight_decay=0.05, betas=(0.9, 0.95))
    aug = PretrainAug(dev)
    n_items = B * (args.iters + 2 * args.workers + 4)
    ds_host, ds_rec = SynthPretrain(n_items, 0, "host"), SynthPretrain(n_items, 0, "recipe")
    res = {"batch": B, "workers": args.workers, "model": args.model, "precision": args.precision}

    # ---- (a) one worker's time per sample, the two paths alternated over the same seeded samples
    torch.set_num_threads(1)
    ms = {"transform_pretrain": [], "recipe_pretrain": [], "build_frame": []}
    nbytes = {"transform_pretrain": [], "recipe_pretrain": []}
    for i in range(args.samples):
        t0 = time.perf_counter()
        image = ds_host.open_image(i)
        ms["build_frame"].append((time.perf_counter() - t0) * 1e3)
        best = {}
        for name in ("transform_pretrain", "recipe_pretrain", "recipe_pretrain", "transform_pretrain"):
            t0 = time.perf_counter()
            getattr(fsc147, name)(image, random.Random(i))
            dt = (time.perf_counter() - t0) * 1e3
            best[name] = min(best.get(name, dt), dt)
        for name, v in best.items():
            ms[name].append(v)
        nbytes["transform_pretrain"].append(3 * 384 * 384 * 4)
        nbytes["recipe_pretrain"].append(int(np.prod(image.size)) * 3)
    res["a_worker_ms_per_sample"] = {k: stats(v) for k, v in ms.items()}
    res["a_bytes_handed_over"] = {k: stats(v) for k, v in nbytes.items()}

    # ---- (b) PretrainAug.batch for one batch, and the step alone on device-resident batches
    random.seed(0)
    recipes = [ds_rec[i] for i in range(B)]
    res["frame_sizes_hw"] = [list(r["frame"].shape[:2]) for r in recipes]
    res["crops"] = [list(r["crop"]) for r in recipes]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dev_ms = []
    with step.on_stream():
        for _ in range(3):
            out = aug.batch(recipes)
        torch.cuda.synchronize()
        for _ in range(30):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            out = aug.batch(recipes)
            e1.record()
            torch.cuda.synchronize()
            dev_ms.append(((time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)))
        res["b_device_ms_per_batch"] = {"wall_median": float(np.median([d[0] for d in dev_ms])), "gpu_median": float(np.median([d[1] for d in dev_ms])),
                                        "gpu_min": float(min(d[1] for d in dev_ms)), "launches": aug.launches, "n": len(dev_ms),
                                        "workspace_mb": aug.workspace_bytes() / 2 ** 20}
        # the transform without the upload: the frames already on the device
        stage = aug._stages[aug._turn ^ 1]
        offs, o = [], 0
        for r in recipes:
            offs.append(o)
            o += (r["frame"].numel() + 15) & ~15
        entries = [(stage.dev.data_ptr() + o, r["frame"].shape[0], r["frame"].shape[1], r["crop"], r["flip"]) for o, r in zip(offs, recipes)]
        k_ms = []
        for _ in range(30):
            torch.cuda.synchronize()
            e0.record()
            aug.run(entries)
            e1.record()
            torch.cuda.synchronize()
            k_ms.append(e0.elapsed_time(e1))
        res["b_kernels_only_ms_per_batch"] = stats(k_ms)
        pair = [out, aug.batch(recipes)]
        for k in range(6):
            step.load(pair[k % 2])
            step.step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        K = 30
        for k in range(K):
            step.load(pair[k % 2])
            step.step()
        torch.cuda.synchronize()
        res["pretrain_step_ms"] = (time.perf_counter() - t0) * 1e3 / K

        # ---- (c) loader + transform + step, sustained
        def run(mode):
            ds = ds_rec if mode == "device" else ds_host
            kw = dict(collate_fn=fsc147.collate_pretrain_recipes) if mode == "device" else dict(pin_memory=True)
            dl = torch.utils.data.DataLoader(ds, batch_size=B, shuffle=False, num_workers=args.workers, drop_last=True, **kw)
            it = iter(dl)

            def fetch():
                b = next(it)
                return aug.batch(b) if mode == "device" else b
            for k in range(2 * args.workers + 2):     # warm-up: workers up, and everything they had prefetched (2 batches each) consumed
                step.load(fetch())
                step.step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(args.iters):
                step.load(fetch())
                step.step()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            del it
            return B * args.iters / dt
        order = ["host", "device", "host", "device"]
        rates = {mode: [] for mode in order}
        for mode in order:
            rates[mode].append(run(mode))
        res["c_images_per_s"] = rates
    print(json.dumps(res))


if __name__ == "__main__":
    main()
