"""CARPK for the two CARPK CLIs: a loader over local files in the devkit layout, a seeded synthetic source, and the host restatements
of what FSC_test_CARPK.py / FSC_finetune_CARPK.py do around the model (the tests compare the HIP path against them; the golden file
tests/golden/carpk.npz pins them against the reference's own lines).

The reference loads its data with hub.load("hub://activeloop/carpk-{train,test}") and reads three fields per sample: `images` uint8
[H, W, 3], `boxes` [[x, y, w, h], ...] and `labels` (one per box: only their number is used).  Here the same fields come from the CARPK
devkit on disk:

    <data_path>/Images/<name>.png
    <data_path>/Annotations/<name>.txt      one "x1 y1 x2 y2 class" line per car
    <data_path>/ImageSets/{train,test}.txt  one <name> per line

with w = x2 - x1 and h = y2 - y1 (whether hub's own conversion is exactly that cannot be checked offline)."""
import os
import random

import numpy as np
import torch
import torch.nn.functional as F

OUT_H, OUT_W = 384, 683        # FSC_test_CARPK.py:188-189 (683 is not a multiple of 16: the last window is snapped to 299)
TRAIN_COLS = 384               # FSC_finetune_CARPK.py:226: the left 384 columns of the resized frame
BOX = 64
THRESHOLD = 1.224              # FSC_test_CARPK.py:230


class Devkit:
    """One split of the devkit: item k -> {"name", "images": uint8 [H, W, 3], "boxes": [[x, y, w, h], ...]}."""

    def __init__(self, data_path, split):
        self.root = data_path
        with open(os.path.join(data_path, "ImageSets", split + ".txt")) as f:
            self.names = [l.strip() for l in f if l.strip()]

    def __len__(self):
        return len(self.names)

    def __getitem__(self, k):
        from PIL import Image
        name = self.names[k]
        with Image.open(os.path.join(self.root, "Images", name + ".png")) as im:
            frame = np.asarray(im.convert("RGB"), dtype=np.uint8).copy()
        boxes = []
        with open(os.path.join(self.root, "Annotations", name + ".txt")) as f:
            for line in f:
                v = line.split()
                if len(v) >= 4:
                    x1, y1, x2, y2 = (int(t) for t in v[:4])
                    boxes.append([x1, y1, x2 - x1, y2 - y1])
        return {"name": name, "images": frame, "boxes": boxes}


def available(data_path, split):
    return os.path.exists(os.path.join(data_path, "ImageSets", split + ".txt"))


def synthetic_item(seed, H=720, W=1280):
    """A seeded CARPK-shaped sample: dim noise with one bright block per box ("cars"), 6..30 boxes of 40..120 x 30..80 pixels.  Box 0
    of every third seed sits in the frame's corner (x = y = 0): the only position at which the script's exemplar test sees any mass
    (script_rects), so both of its branches occur."""
    rs = np.random.RandomState(50000 + seed)
    frame = rs.randint(0, 48, size=(H, W, 3)).astype(np.uint8)
    n = int(rs.randint(6, 31))
    boxes = []
    for k in range(n):
        w, h = int(rs.randint(40, 121)), int(rs.randint(30, 81))
        x, y = int(rs.randint(0, W - w)), int(rs.randint(0, H - h))
        if k == 0 and seed % 3 == 0:
            x = y = 0
        boxes.append([x, y, w, h])
        frame[y:y + h + 1, x:x + w + 1] = rs.randint(150, 256, size=frame[y:y + h + 1, x:x + w + 1].shape).astype(np.uint8)
    return {"name": "synthetic_%d" % seed, "images": frame, "boxes": boxes}


class Synthetic:
    def __init__(self, n, seed=0):
        self.n, self.seed = n, seed

    def __len__(self):
        return self.n

    def __getitem__(self, k):
        if not 0 <= k < self.n:
            raise IndexError(k)
        return synthetic_item(self.seed * 1000 + k)


def box_rect(box):
    """[x, y, w, h] -> the inclusive rectangle (y1, x1, y2, x2) the scripts cut (FSC_test_CARPK.py:168-170)."""
    x, y, w, h = (int(v) for v in box)
    return [y, x, y + h, x + w]


def test_draws(nboxes):
    """The two random.randint draws of FSC_test_CARPK.py:160-164.  The script ignores their result (it takes boxes 0 and 1) but they
    move `random`'s stream, so they are made."""
    random.randint(0, int(nboxes / 2))
    random.randint(int(nboxes / 2) - 1, nboxes - 1)
    return 0, 1


def train_draw(nboxes):
    """The exemplar index of FSC_finetune_CARPK.py:210."""
    return random.randint(0, nboxes - 1)


def train_mask_draw():
    """FSC_finetune_CARPK.py:246: drawn and never used (the loss is unmasked, :252); made so that numpy's stream stays in step."""
    return np.random.binomial(n=1, p=0.8, size=[384, 384])


def prepare_host(frame, rects, out_cols=OUT_W):
    """torch-op restatement of the scripts' preparation: frame uint8 [H, W, 3], rects [(y1, x1, y2, x2), ...] inclusive, in original
    pixels -> (image [1, 3, 384, out_cols], exemplars [1, S, 3, 64, 64]).  transforms.Resize on a tensor is, at the reference's
    torchvision 0.14.1, F.interpolate(bilinear, align_corners=False) without antialiasing."""
    samples = (torch.as_tensor(np.asarray(frame)) / 255).permute(2, 0, 1)
    ex = [F.interpolate(samples[None, :, y1:y2 + 1, x1:x2 + 1], size=(BOX, BOX), mode="bilinear", align_corners=False)[0]
          for y1, x1, y2, x2 in rects]
    image = F.interpolate(samples[None], size=(OUT_H, OUT_W), mode="bilinear", align_corners=False)[..., :out_cols]
    return image.contiguous(), (torch.stack(ex)[None] if ex else torch.zeros(1, 0))


def stitch_host(model, image, exemplars, shot_num=2):
    """The window loop of FSC_test_CARPK.py:194-218 with inference's restatement of it: -> (map [384, w], window starts)."""
    from .. import inference
    w = image.shape[-1]
    starts = inference.window_starts(w)
    outs = torch.cat([model(image[:, :, :, s:s + 384], exemplars, shot_num) for s in starts], 0)
    return inference.blend_windows(outs, starts, w, image.shape[-2]), starts


def cells_host(dm):
    """d_m of FSC_test_CARPK.py:220-226: sums of the 16 x 16 blocks of map / 60 (stride-16 convolution with ones; trailing rows and
    columns dropped)."""
    dm = np.asarray(dm, dtype=np.float32)
    ch, cw = dm.shape[0] // 16, dm.shape[1] // 16
    return (dm[:ch * 16, :cw * 16] / np.float32(60)).reshape(ch, 16, cw, 16).sum((1, 3), dtype=np.float32)


def script_rects(boxes_xywh, H=OUT_H, W=OUT_W):
    """The two (a, b, c, d) rectangles of the count rule for the exemplar boxes 0 and 1, as the script's line :238 really slices.
    It writes density_map[x : x + w + 1, y : y + h + 1] with the box's (x, y, w, h) of the ORIGINAL frame -- but by then the map has been
    unsqueezed twice (:224-225) and is [1, 1, 384, 683], so the two slices cut the two leading axes of length 1, not rows and columns:
    the slice is the WHOLE map when x == 0 and y == 0 and empty otherwise.  Expressed for count_rule_host / countr_carpk_count (whose
    rectangles are rows and columns of the map, clipped to it): the whole map, or a rectangle that starts outside it."""
    out = []
    for box in boxes_xywh[:2]:
        x, y, w, h = (int(v) for v in box)
        whole = x == 0 and y == 0 and w >= 0 and h >= 0
        out.append([0, 0, H - 1, W - 1] if whole else [H, W, 0, 0])
    return out


def count_rule_host(dm, rects):
    """FSC_test_CARPK.py:220-243 on a stitched map [H, W] and two rectangles (a, b, c, d) = map[a : a + c + 1, b : b + d + 1], clipped
    to the map, empty = 0 (for the script's own behaviour pass script_rects(boxes)) ->
    (pred_cnt, {"total", "n_over", "e_cnt", "cells"})."""
    dm = np.asarray(dm, dtype=np.float32)
    cells = cells_host(dm)
    total = float(cells.sum(dtype=np.float32))
    n_over = int((cells > np.float32(THRESHOLD)).sum())
    e_cnt = 0.0
    for a, b, c, d in rects:
        a, b, c, d = int(a), int(b), int(c), int(d)
        e_cnt += float((dm[a:a + c + 1, b:b + d + 1] / np.float32(60)).sum(dtype=np.float32))
    e_cnt /= 2
    pred = total - n_over + (2 if e_cnt <= 0.5 else 0)
    return pred, {"total": total, "n_over": n_over, "e_cnt": e_cnt, "cells": cells}


def train_cells(boxes):
    """Box centres -> the set cells (row, col) of the 384 x 384 target, in first-occurrence order (FSC_finetune_CARPK.py:229-236: a
    centre with x < 720 lands at int(x * 384 / 720), int(y * 384 / 720); the cell is SET, so duplicates collapse)."""
    seen, out = set(), []
    for box in boxes:
        b = [int(k) for k in box]
        x, y = int(b[0] + b[2] / 2), int(b[1] + b[3] / 2)
        if x < 720:
            x, y = int(x * 384 / 720), int(y * 384 / 720)
            if not (0 <= y < 384):
                raise IndexError("box centre row %d outside the 384 x 384 target (the reference raises here too)" % y)
            if (y, x) not in seen:
                seen.add((y, x))
                out.append((y, x))
    return out


def train_target_host(boxes):
    """gt_density of FSC_finetune_CARPK.py:229-238: 60 * scipy gaussian_filter(sigma 1) of the cell map."""
    from scipy import ndimage
    gt = np.zeros((384, 384), dtype="float32")
    for y, x in train_cells(boxes):
        gt[y][x] = 1
    return ndimage.gaussian_filter(gt, sigma=(1, 1), order=0) * 60
