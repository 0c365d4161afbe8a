#!/usr/bin/env python3
"""Golden vectors of the reference's CARPK scripts (runs only in the build container).

FSC_test_CARPK.py and FSC_finetune_CARPK.py cannot be imported (hub, timm 0.3.2, torchvision and a network are missing; the finetune
script also imports a name that does not exist).  Their loop bodies are read from the reference at run time and executed UNCHANGED --
FSC_test_CARPK.py:153-245 (one pass of the loop per case) and FSC_finetune_CARPK.py:204-240 plus the mask draw of :246 -- with
stand-ins for what is absent:
  transforms.Resize(size)   tensor -> F.interpolate(bilinear, align_corners=False), no antialias: what torchvision 0.14.1 does to a
                            tensor (antialias=None -> False); 16-bit tensors are resized in fp32 and cast back (the CPU has no half
                            kernel in every torch; only the training target and the random streams are recorded from that script)
  TF.crop(img, t, l, h, w)  tensor slicing
  data                      countr_amd.data.carpk.synthetic_item(seed) in hub's batch-1 field shapes
  model                     toy_model below: a small deterministic function of the window and the exemplars; tests/test_carpk_cpu.py
                            restates it
  metric_logger.log_every   yields its iterable
What running the lines unchanged showed: :238 slices density_map AFTER its two unsqueeze(0) of :224-225, so the box's (x, y, w, h)
cut the two leading axes of length 1 -- e_cnt is the whole map's count for a box at x = y = 0 and 0 otherwise.  The synthetic source
puts box 0 of every third seed into that corner, so both branches of `e_cnt <= 0.5` are recorded (data/carpk.py::script_rects).
Output: tests/golden/carpk.npz -- seeds, boxes, cells [24, 42] (the script's d_m), pred_cnt, e_cnt, window starts, the training
target's nonzero cells and its sum, and the next draw of `random` / numpy behind one item.  No frames, no source text."""
import os
import random
import sys
import textwrap
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden", "carpk.npz")
SEEDS = [0, 1, 2, 3, 4, 5]
STREAM_SEED = 1234


def toy_model(window, boxes, shot_num):
    """[1, 3, 384, 384], [1, S, 3, 64, 64] -> [1, 384, 384]: channel mean of the window times a gain read from the exemplars."""
    gain = 0.2 + 0.4 * boxes[:, :shot_num].mean()
    return window.mean(1) * gain


class Resize:
    def __init__(self, size):
        self.size = tuple(size)

    def __call__(self, img):
        out = F.interpolate(img.float().unsqueeze(0), size=self.size, mode="bilinear", align_corners=False)[0]
        return out.to(img.dtype)


def body(path, first, last, indent):
    lines = open(os.path.join(REF, path)).read().split("\n")[first - 1:last]
    return textwrap.dedent("\n".join(l[indent:] if l.strip() else "" for l in lines))


def hub_batch(item):
    nb = len(item["boxes"])
    return {"images": torch.from_numpy(item["images"])[None], "boxes": torch.tensor(item["boxes"], dtype=torch.float32)[None],
            "labels": torch.zeros(1, nb, 1, dtype=torch.int64)}


class Logger:
    def log_every(self, it, *_a):
        return it


def main():
    from countr_amd.data import carpk as D
    transforms = types.SimpleNamespace(Resize=Resize)
    TF = types.SimpleNamespace(crop=lambda img, t, l, h, w: img[..., t:t + h, l:l + w])
    test_src = body("FSC_test_CARPK.py", 153, 245, 4)
    train_src = body("FSC_finetune_CARPK.py", 204, 239, 12)          # ... up to the fp32 target; :240 (its 16-bit cast) and :246 follow
    train_tail = body("FSC_finetune_CARPK.py", 240, 240, 12) + "\n" + body("FSC_finetune_CARPK.py", 246, 246, 12)
    from scipy import ndimage
    rec = {k: [] for k in ("cells", "pred_cnt", "e_cnt", "n_over", "starts", "nboxes", "target_sum", "ntarget")}
    boxes_all, target_cells = [], []
    for seed in SEEDS:
        item = D.synthetic_item(seed)
        windows = []

        def model(w, b, s):
            windows.append(w.clone())
            return toy_model(w, b, s)
        ns = dict(torch=torch, nn=nn, np=np, random=random, transforms=transforms, device=torch.device("cpu"), model=model,
                  metric_logger=Logger(), dataloader_test=[hub_batch(item)], print_freq=20, header="")
        random.seed(STREAM_SEED + seed)
        exec(test_src, ns)
        after_test = random.random()
        r_image = ns["r_image"]
        starts = [next(s for s in range(r_image.shape[-1] - 383) if torch.equal(r_image[:, :, :, s:s + 384], w)) for w in windows]
        d_m = ns["d_m"][0, 0].detach().numpy()
        rec["cells"].append(d_m)
        rec["pred_cnt"].append(ns["pred_cnt"])
        rec["e_cnt"].append(ns["e_cnt"])
        rec["n_over"].append(int((d_m > 1.224).sum()))
        rec["starts"].append(starts)
        rec["nboxes"].append(len(item["boxes"]))
        boxes_all += item["boxes"]
        # ---- the training sample of the same item
        ns = dict(torch=torch, np=np, random=random, transforms=transforms, TF=TF, ndimage=ndimage, device=torch.device("cpu"),
                  data=hub_batch(item), output=torch.zeros(1, 384, 384))
        random.seed(STREAM_SEED + seed)
        np.random.seed(STREAM_SEED + seed)
        exec(train_src, ns)
        gt = ns["gt_density"].numpy().copy()          # fp32, before the script casts it to 16 bits
        exec(train_tail, ns)
        after_train = (random.random(), float(np.random.random_sample()))
        assert tuple(ns["samples"].shape) == (1, 3, 384, 384) and tuple(ns["boxes"].shape) == (1, 1, 3, 64, 64)
        # the cells come from the script's own dot map: gaussian_filter of a 0/1 map is > 0 exactly in the 9 x 9 neighbourhoods, so the
        # dots are read back from an fp32 rerun of lines :229-236 -- ns keeps `gt_density` only after the filter; recompute the dots
        dots = np.zeros((384, 384), dtype="float32")
        exec(body("FSC_finetune_CARPK.py", 230, 236, 12).replace("gt_density", "dots"), dict(data=ns["data"], dots=dots))
        ys, xs = np.nonzero(dots)
        target_cells += [[int(y), int(x)] for y, x in zip(ys, xs)]
        rec["ntarget"].append(len(ys))
        rec["target_sum"].append(float(gt.astype(np.float64).sum()))
        rec.setdefault("after_test", []).append(after_test)
        rec.setdefault("after_train", []).append(after_train)
        rec.setdefault("train_idx", []).append(int(ns["idx"]))
    cells = np.stack(rec["cells"]).astype(np.float32)
    e_cnt = np.array(rec["e_cnt"], dtype=np.float64)
    n_over = np.array(rec["n_over"])
    assert len(SEEDS) >= 4 and cells.shape[1:] == (24, 42)
    assert (n_over >= 1).any(), n_over
    assert (e_cnt <= 0.5).any() and (e_cnt > 0.5).any(), e_cnt
    assert np.abs(cells - 1.224).min() > 1e-3, np.abs(cells - 1.224).min()
    assert np.abs(e_cnt - 0.5).min() > 1e-3, e_cnt
    np.savez_compressed(OUT, seeds=np.array(SEEDS), stream_seed=np.array(STREAM_SEED), nboxes=np.array(rec["nboxes"]),
                        boxes=np.array(boxes_all, dtype=np.int32), cells=cells, pred_cnt=np.array(rec["pred_cnt"], dtype=np.float64),
                        e_cnt=e_cnt, n_over=n_over, starts=np.array(rec["starts"], dtype=np.int32),
                        ntarget=np.array(rec["ntarget"]), target_cells=np.array(target_cells, dtype=np.int32),
                        target_sum=np.array(rec["target_sum"], dtype=np.float64), after_test=np.array(rec["after_test"]),
                        after_train=np.array(rec["after_train"]), train_idx=np.array(rec["train_idx"]))
    print("wrote %s (%d bytes): n_over %s, e_cnt %s, pred %s" % (OUT, os.path.getsize(OUT), n_over.tolist(), np.round(e_cnt, 3).tolist(),
                                                                  np.round(rec["pred_cnt"], 3).tolist()))


if __name__ == "__main__":
    main()
