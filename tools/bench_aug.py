#!/usr/bin/env python3
"""Train-time augmentation: host path against --device_aug, in one process on one GPU.

  (a) host transform_train_aug per sample, one thread (what a DataLoader worker pays per image)
  (b) DeviceAug.batch per batch of 8 at realistic frame sizes (height 384-700, width 384-1024), with its launch count, beside the
      finetune step's own time in the same run
  (c) sustained images/s of "10-worker loader + augmentation + FinetuneStep": host path against the recipe path, alternated, two
      repeats each

With --device_mosaic the two recipe paths are compared instead, mosaic samples finished by the host's mosaic() against "mosaic_dev"
recipes for countr_aug_mosaic, alternated in the same run:
  (m1) one worker's time per MOSAIC recipe on either path over the same seeded samples, and the bytes a recipe hands over
  (m2) DeviceAug.batch for the batch of (b) with its mosaic samples on either path (device events)
  (c)  sustained images/s, --device_aug against --device_aug --device_mosaic, two repeats each

Frames, dots and boxes are generated from a seed (no dataset needed); a frame is "decoded" by building it in the worker.
Usage: python tools/bench_aug.py [--batch 8] [--iters 60] [--workers 10] [--samples 6] [--device_mosaic [--mosaic_samples 24]]"""
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


class SynthTrain(torch.utils.data.Dataset):
    """FSC147-shaped items from a seed, with what fsc147.mosaic needs of a dataset (train_set, annotations, class_dict, open_image)."""

    def __init__(self, n, seed, mode, epoch_len=None, device_mosaic=False):
        rs = np.random.RandomState(seed)
        self.mode = mode                                # "host" | "recipe"
        self.device_mosaic = device_mosaic              # recipe mode: mosaic samples as mosaic_dev recipes
        self.train_set = ["%d.png" % k for k in range(n)]
        self.img = list(self.train_set)
        self.sizes, self.annotations, self.class_dict = {}, {}, {}
        for k, im_id in enumerate(self.train_set):
            h, w = int(rs.randint(384, 701)), int(rs.randint(384, 1025))
            nd = int(rs.choice([12, 30, 60, 90, 200]))
            dots = np.stack([rs.uniform(2, w - 2, nd), rs.uniform(2, h - 2, nd)], 1)
            boxes = []
            for _ in range(3):
                x1, y1 = int(rs.uniform(0, w - 80)), int(rs.uniform(0, h - 80))
                x2, y2 = x1 + int(rs.uniform(20, 70)), y1 + int(rs.uniform(20, 70))
                boxes.append([[x1, y1], [x1, y2], [x2, y2], [x2, y1]])
            self.sizes[im_id] = (h, w)
            self.annotations[im_id] = {"points": dots.tolist(), "box_examples_coordinates": boxes}
            self.class_dict[im_id] = ["c%d" % (k % 3)]
        self.epoch = 0

    def open_image(self, im_id):
        from PIL import Image
        h, w = self.sizes[im_id]
        rs = np.random.RandomState(int(im_id.split(".")[0]) + 77)
        x, y = np.arange(w, dtype=np.int32)[None, :], np.arange(h, dtype=np.int32)[:, None]
        arr = np.empty((h, w, 3), np.uint8)               # ramps plus 5 bits of noise: a stand-in for a decoded photograph
        arr[..., 0] = x * 223 // w
        arr[..., 1] = y * 223 // h
        arr[..., 2] = (x * 3 + y * 5) % 224
        return Image.fromarray(arr + (np.frombuffer(rs.bytes(h * w * 3), np.uint8).reshape(h, w, 3) & 31))

    def __len__(self):
        return len(self.img)

    def item(self, idx):
        im_id = self.img[idx]
        anno = self.annotations[im_id]
        rects = [[b[0][1], b[0][0], b[2][1], b[2][0]] for b in anno["box_examples_coordinates"]]
        return self.open_image(im_id), rects, np.array(anno["points"]), im_id

    def __getitem__(self, idx):
        image, rects, dots, im_id = self.item(idx)
        nprng = np.random.RandomState((torch.initial_seed() + idx) % (2 ** 32))
        if self.mode == "recipe":
            return fsc147.recipe_train(image, rects, dots, im_id, self, do_aug=True, nprng=nprng, noise_counter=self.epoch * len(self) + idx,
                                       device_mosaic=self.device_mosaic)
        s = fsc147.transform_train_aug(image, rects, dots, im_id, self, nprng=nprng)
        return s["image"], s["gt_density"], len(dots), s["boxes"], s["m_flag"]


def recipe_bytes(rec):
    """Bytes of the arrays a recipe carries from the worker to the main process."""
    n = 0
    for key, v in rec.items():
        if key == "frame" and "frames" in rec:          # frames[0] again
            continue
        for t in (v if key == "frames" else [v]):
            if isinstance(t, torch.Tensor):
                n += t.numel() * t.element_size()
            elif isinstance(t, np.ndarray):
                n += t.nbytes
    return n


def stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "n": len(v)}


def time_mosaic_recipes(ds, n):
    """(m1): recipe_train for the first n samples whose seeded mosaic coin comes up, host mosaic() and mosaic_dev plan in turn."""
    ms, nbytes, flags = {"host": [], "device": []}, {"host": [], "device": []}, []
    torch.set_num_threads(1)
    idx = seed = 0
    while len(flags) < n:
        seed += 1
        if random.Random(seed).random() >= 0.25:
            continue
        image, rects, dots, im_id = ds.item(idx % len(ds))
        idx += 1
        for path in ("host", "device", "device", "host"):
            t0 = time.perf_counter()
            rec = fsc147.recipe_train(image, rects, dots, im_id, ds, do_aug=True, rng=random.Random(seed), nprng=None,
                                      device_mosaic=path == "device")
            ms[path].append((time.perf_counter() - t0) * 1e3)
            nbytes[path].append(recipe_bytes(rec))
        flags.append(rec["m_flag"])
    return {"host_mosaic_ms": stats(ms["host"]), "mosaic_dev_ms": stats(ms["device"]), "host_mosaic_bytes": stats(nbytes["host"][::2]),
            "mosaic_dev_bytes": stats(nbytes["device"][::2]), "cross_image_mosaics": int(sum(flags)), "samples": len(flags)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=60, help="timed iterations of (c) per repeat")
    ap.add_argument("--workers", type=int, default=10)
    ap.add_argument("--samples", type=int, default=6, help="host samples timed in (a) per round")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--device_mosaic", action="store_true", help="compare the two recipe paths: host mosaic() against mosaic_dev recipes")
    ap.add_argument("--mosaic_samples", type=int, default=24, help="mosaic recipes timed in (m1)")
    args = ap.parse_args()
    import models_mae_cross
    from countr_amd.device_aug import DeviceAug
    from countr_amd.trainer import FinetuneStep
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B = args.batch
    torch.manual_seed(0)
    model = models_mae_cross.__dict__["mae_vit_base_patch16"](norm_pix_loss=False, precision=args.precision)
    model.to(dev).train()
    step = FinetuneStep(model, batch=B, lr=1e-5, weight_decay=0.05, mask_seed=1, pipeline_encoder=True, defer_optimizer=True)
    da = DeviceAug(dev, batch=B, noise_seed=1)
    n_items = B * (args.iters + 2 * args.workers + 4)
    ds_host, ds_rec = SynthTrain(n_items, 0, "host"), SynthTrain(n_items, 0, "recipe")
    ds_mos = SynthTrain(n_items, 0, "recipe", device_mosaic=True)
    res = {"batch": B, "workers": args.workers}
    if args.device_mosaic:
        res["m1_worker_per_mosaic_recipe"] = time_mosaic_recipes(ds_rec, args.mosaic_samples)

    # ---- (a) and (b), alternated
    random.seed(0)
    recipes = [ds_rec[i] for i in range(B)]
    res["frame_sizes_hw"] = [list(r["frame"].shape[:2]) for r in recipes]
    res["recipe_kinds"] = [r["kind"] for r in recipes]
    random.seed(0)
    recipes_m = [ds_mos[i] for i in range(B)]             # the same draws: the same samples, mosaics as mosaic_dev
    host_ms, dev_ms = [], []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with step.on_stream():
        for _ in range(3):
            out = da.batch(recipes)
        torch.cuda.synchronize()
        for rnd in range(args.rounds):
            torch.set_num_threads(1)
            for i in range(args.samples):
                image, rects, dots, im_id = ds_host.item(rnd * args.samples + i)
                t0 = time.perf_counter()
                fsc147.transform_train_aug(image, rects, dots, im_id, ds_host, nprng=np.random.RandomState(i))
                host_ms.append((time.perf_counter() - t0) * 1e3)
            for _ in range(10):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record()
                out = da.batch(recipes)
                e1.record()
                torch.cuda.synchronize()
                dev_ms.append(((time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)))
        res["a_host_ms_per_sample"] = {"median": float(np.median(host_ms)), "min": float(min(host_ms)), "max": float(max(host_ms)), "n": len(host_ms)}
        res["b_device_ms_per_batch"] = {"wall_median": float(np.median([d[0] for d in dev_ms])), "gpu_median": float(np.median([d[1] for d in dev_ms])),
                                        "gpu_min": float(min(d[1] for d in dev_ms)), "launches": da.launches, "n": len(dev_ms)}
        if args.device_mosaic:
            gpu = {"host_mosaic": [], "mosaic_dev": []}
            launches = {}
            for _ in range(3):
                da.batch(recipes_m)
            for rnd in range(2 * args.rounds):
                for name, recs in (("host_mosaic", recipes), ("mosaic_dev", recipes_m)):
                    for _ in range(5):
                        torch.cuda.synchronize()
                        e0.record()
                        da.batch(recs)
                        e1.record()
                        torch.cuda.synchronize()
                        gpu[name].append(e0.elapsed_time(e1))
                    launches[name] = da.launches
            res["m2_device_ms_per_batch"] = {"host_mosaic": stats(gpu["host_mosaic"]), "mosaic_dev": stats(gpu["mosaic_dev"]), "launches": launches,
                                            "kinds": [r["kind"] for r in recipes_m],
                                            "uploaded_frames": sum(len(r["frames"]) if r["kind"] == "mosaic_dev" else 1 for r in recipes_m)}
        # the finetune step alone, on device-resident batches (as bench.py times it)
        imgs, boxes, gt, _ = out
        nxt = da.batch(recipes)
        pair = [(imgs, boxes, gt), nxt[:3]]
        for k in range(6):
            step.load(*pair[k % 2], None, 3, next_imgs=pair[(k + 1) % 2][0])
            step.step(3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        K = 20
        for k in range(K):
            step.load(*pair[k % 2], None, 3, next_imgs=pair[(k + 1) % 2][0] if k + 1 < K else None)
            step.step(3)
        torch.cuda.synchronize()
        res["finetune_step_ms"] = (time.perf_counter() - t0) * 1e3 / K

        # ---- (c) loader + augmentation + step, sustained
        def run(mode):
            ds = {"device": ds_rec, "device_mosaic": ds_mos, "host": ds_host}[mode]
            kw = dict(collate_fn=fsc147.collate_recipes) if mode != "host" else dict(pin_memory=True)
            dl = torch.utils.data.DataLoader(ds, batch_size=B, shuffle=False, num_workers=args.workers, drop_last=True, **kw)
            it = iter(dl)

            def fetch():
                b = next(it)
                if mode != "host":
                    i_, b_, g_, _m = da.batch(b)
                    return i_, b_, g_
                return b[0], b[3], b[1]
            ahead = fetch()
            for k in range(2 * args.workers + 2):     # warm-up: workers up, and everything they had prefetched (2 batches each) consumed
                cur, ahead = ahead, fetch()
                step.load(*cur, None, 3, next_imgs=ahead[0])
                step.step(3)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(args.iters):
                cur, ahead = ahead, (fetch() if k + 1 < args.iters else None)
                step.load(*cur, None, 3, next_imgs=ahead[0] if ahead is not None else None)
                step.step(3)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            del it
            return B * args.iters / dt
        torch.set_num_threads(1)
        order = ["device", "device_mosaic", "device", "device_mosaic"] if args.device_mosaic else ["host", "device", "host", "device"]
        rates = {mode: [] for mode in order}
        for mode in order:
            rates[mode].append(run(mode))
        res["c_images_per_s"] = rates
        # what bounds the recipe path: one worker's time per recipe (decode + draws + host mosaic for a quarter of the samples)
        random.seed(1)
        t0 = time.perf_counter()
        kinds = [ds_rec[i]["kind"] for i in range(16)]
        res["recipe_ms_per_sample_one_thread"] = (time.perf_counter() - t0) * 1e3 / 16
        res["recipe_mosaics_in_16"] = kinds.count("mosaic")
        if args.device_mosaic:
            random.seed(1)                               # the same draws: the same sixteen samples
            t0 = time.perf_counter()
            kinds = [ds_mos[i]["kind"] for i in range(16)]
            res["mosaic_dev_recipe_ms_per_sample_one_thread"] = (time.perf_counter() - t0) * 1e3 / 16
            res["mosaic_dev_recipes_in_16"] = kinds.count("mosaic_dev")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
