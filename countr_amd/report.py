"""The evaluation report of the reference's few-shot test script (FSC_test_cross(few-shot).py:379-453): per image `full_<stem>__<count>.png`
(error / exemplar / true-positive panels, or exemplar / density panels when the image holds no object) and `boxes_<stem>.png` (the
exemplar crops), and per run `results.csv`, `log.txt` and `test_stat.png`.

    compose_host / exemplar_strip_host   the script's lines restated operation by operation in torch / numpy: the yardstick of the GPU
                                         tests, and what runs when the tensors live on the CPU
    ReportWriter                         the same bytes from csrc/report.hip on the stream the forward runs on: per group of <= 16 images
                                         one upload (rectangles, label rasters, host gt maps), one launch for the panels, one for the
                                         exemplar pictures, one asynchronous download; a small thread pool encodes the PNGs with PIL while
                                         the next group's forward runs

The labels are rasterised on the host with PIL as the script does (Pillow's default font: the glyphs depend on the installed Pillow); only
each raster's non-zero bounding rectangle goes to the device."""
import csv
import ctypes as C
import json
import os
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image, ImageDraw

from . import _lib

MAX_GROUP = _lib.REPORT_MAX_IMAGES
MAX_WORKERS = 8
GRID_ROW, GRID_PAD = 8, 2   # torchvision.utils.make_grid's defaults, which save_image passes on

# name: the image's file name (its stem names the pictures); sample fp32 [3, h, w] or [1, 3, h, w]; boxes fp32 [S, 3, eh, ew] (or
# [1, S, ...], or empty: no exemplar picture); pos [(y1, x1, y2, x2), ...] inclusive; gt_cnt; gt_map fp32 [h, w] (host or device)
ReportItem = namedtuple("ReportItem", "name sample boxes pos gt_cnt gt_map")


# ---- the host statement
def text_raster(w, h, pred_cnt):
    """FSC_test_cross(few-shot).py:386-389 -> PIL RGB image (w, h)."""
    im = Image.new(mode="RGB", size=(w, h), color=(0, 0, 0))
    draw = ImageDraw.Draw(im)
    draw.text((w - 50, h - 50), f"{pred_cnt:.3f}", (255, 255, 255))
    return im


def label_raster(w, h, gt_cnt, pred_cnt):
    """FSC_test_cross(few-shot).py:403-409 -> PIL RGB image (w, h)."""
    im = Image.new(mode="RGB", size=(w, h), color=(0, 0, 0))
    draw = ImageDraw.Draw(im)
    draw.text((w - 150, h - 130), f"GT: {gt_cnt:.3f}", (255, 255, 255))
    draw.text((w - 150, h - 110), f"Pred: {pred_cnt:.3f}", (255, 255, 255))
    draw.text((w - 150, h - 90), "True Positives", (0, 255, 0))
    draw.text((w - 150, h - 70), "False Positives", (255, 255, 0))
    draw.text((w - 150, h - 50), "False Negatives", (255, 0, 0))
    return im


def raster_patch(im):
    """The non-zero bounding rectangle of a raster: (px, py, uint8 [ph, pw, 3]) or None when nothing was drawn inside the canvas."""
    if not isinstance(im, Image.Image):
        im = Image.fromarray(np.ascontiguousarray(im))
    bbox = im.getbbox()
    if bbox is None:
        return None
    return bbox[0], bbox[1], np.ascontiguousarray(np.asarray(im.crop(bbox), dtype=np.uint8))


def box_map(h, w, pos, external=False):
    """misc.get_box_map -> uint8 [h, w, 3]: cv2.rectangle(..., (255, 255, 255), 1) per rectangle (y1, x1, y2, x2), i.e. the pixels with
    y in {y1, y2}, x1 <= x <= x2 or x in {x1, x2}, y1 <= y <= y2, clipped to the image; nothing with external exemplars."""
    m = np.zeros((h, w, 3), np.uint8)
    if not external:
        for rect in pos:
            ya, xa, yb, xb = (int(v) for v in rect)
            y1, y2, x1, x2 = min(ya, yb), max(ya, yb), min(xa, xb), max(xa, xb)
            xs, ys = slice(max(x1, 0), max(min(x2, w - 1) + 1, 0)), slice(max(y1, 0), max(min(y2, h - 1) + 1, 0))
            for y in (y1, y2):
                if 0 <= y < h:
                    m[y, xs] = 255
            for x in (x1, x2):
                if 0 <= x < w:
                    m[ys, x] = 255
    return m


def make_grid_host(maps, h, w):
    """misc.make_grid: nine [h, w] maps tiled 3 x 3 in list order, resized back to [h, w] as transforms.Resize does to a tensor
    (bilinear, align_corners=False, no antialias -- the convention inference.count_image uses)."""
    assert len(maps) == 9
    rows = [torch.cat((maps[i], maps[i + 1], maps[i + 2]), -1) for i in range(0, 9, 3)]
    grid = torch.cat(rows, 0)
    return F.interpolate(grid[None, None], size=(h, w), mode="bilinear", align_corners=False)[0, 0]


def grid_sample_points(maps, h, w):
    """What csrc/report.hip reads instead: the resize's source coordinate is 3 d + 1 with weight 1 on one tap, so the resized grid is
    grid[3 y + 1, 3 x + 1] exactly."""
    rows = [torch.cat((maps[i], maps[i + 1], maps[i + 2]), -1) for i in range(0, 9, 3)]
    return torch.cat(rows, 0)[1::3, 1::3][:h, :w]


def quantize_host(t):
    """torchvision.utils.save_image's bytes of a [3, H, W] tensor: mul(255).add_(0.5).clamp_(0, 255), HWC, uint8 -> np [H, W, 3]."""
    return t.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8).numpy()


def compose_host(sample, pred, gt_map, pos, gt_cnt, pred_cnt, external=False, labels=None, text=None):
    """`full` of FSC_test_cross(few-shot).py:380-421 as the bytes save_image writes: uint8 np [h, P w, 3], P = 3 (gt_cnt != 0) or 2.
    sample fp32 [3, h, w]; pred: the stitched map [h, w] or the list of the nine maps of the 3 x 3 path; gt_map [h, w]; pos
    [(y1, x1, y2, x2), ...].  labels / text: the uint8 [h, w, 3] raster to use instead of label_raster / text_raster (tests)."""
    sam = sample.reshape(3, sample.shape[-2], sample.shape[-1]).float()
    device = sam.device
    _, h, w = sam.shape
    gt_map = gt_map.reshape(1, h, w).to(device=device, dtype=torch.float32)
    gt_img = torch.cat((gt_map, torch.zeros_like(gt_map), torch.zeros_like(gt_map)))
    box = torch.tensor(box_map(h, w, pos, external).transpose(2, 0, 1), device=device)
    pred_img = (make_grid_host(list(pred), h, w) if isinstance(pred, (list, tuple)) else pred.reshape(h, w)).to(device).float().unsqueeze(0)
    pred_img = torch.cat((pred_img, pred_img, torch.zeros_like(pred_img)))
    if gt_cnt != 0:
        fp_img = torch.zeros_like(pred_img)
        mask = (gt_img - pred_img) < -0.01
        fp_img[mask] = pred_img[mask]
        tp_img = sam * 0.6 + (pred_img - fp_img)[[1, 0, 2], ...]
        mix1 = (pred_img.clamp(0, 1) - gt_img.clamp(0, 1)).abs()
        mix2 = sam * 0.6 + mix1
        lab = np.array(label_raster(w, h, gt_cnt, pred_cnt)) if labels is None else np.asarray(labels)
        lab = torch.tensor(lab.transpose((2, 0, 1)), device=device)
        sam_box = torch.clamp(sam + box + lab, 0, 1)
        full = torch.cat((mix2, sam_box, tp_img), -1)
    else:
        den_pr = np.array(text_raster(w, h, pred_cnt)) if text is None else np.asarray(text)
        den_pr = torch.tensor(den_pr.transpose((2, 0, 1)), device=device)
        den_pr = sam * 0.6 + den_pr + pred_img
        den_pr = torch.clamp(den_pr, 0, 1)
        sam_box = torch.clamp(sam + box, 0, 1)
        full = torch.cat((sam_box, den_pr), -1)
    return quantize_host(full)


def strip_shape(S, eh=64, ew=64):
    """(GH, GW) of make_grid over S exemplars: a single one comes back as it is, otherwise 8 per row with padding 2."""
    if S == 1:
        return eh, ew
    cols = min(GRID_ROW, S)
    rows = -(-S // cols)
    return (eh + GRID_PAD) * rows + GRID_PAD, (ew + GRID_PAD) * cols + GRID_PAD


def exemplar_strip_host(boxes):
    """`boxes_img` of FSC_test_cross(few-shot).py:423-425 as save_image writes it: the script cats a ONE-element list (boxes is
    [1, S, 3, 64, 64] there), so the picture is make_grid of the S exemplars (nrow 8, padding 2, pad value 0) -> uint8 np [GH, GW, 3]."""
    t = boxes.reshape(-1, 3, boxes.shape[-2], boxes.shape[-1]).float()
    S, _, eh, ew = t.shape
    if S == 1:
        return quantize_host(t[0].clone())
    gh, gw = strip_shape(S, eh, ew)
    cols = min(GRID_ROW, S)
    grid = t.new_full((3, gh, gw), 0.0)
    for k in range(S):
        y, x = divmod(k, cols)
        grid[:, y * (eh + GRID_PAD) + GRID_PAD:][:, :eh, x * (ew + GRID_PAD) + GRID_PAD:][:, :, :ew].copy_(t[k])
    return quantize_host(grid)


# ---- the writer
def _align(v, a=16):
    return (v + a - 1) // a * a


class _Stage:
    """One group's buffers: the pinned blob and its device copy, the device pictures and their pinned copy, the event behind the
    download, the encodes that still read the pinned pictures and the tensors the launch reads."""

    def __init__(self):
        self.blob_host = self.blob_dev = self.out_dev = self.out_host = None
        self.event = None
        self.pending = []
        self.keep = None

    def reserve(self, blob_bytes, out_bytes, device):
        if self.blob_host is None or self.blob_host.numel() < blob_bytes:
            size = _align(max(blob_bytes, 1 << 16) * 5 // 4, 4096)
            self.blob_host = torch.empty(size, dtype=torch.uint8).pin_memory()
            self.blob_dev = torch.empty(size, dtype=torch.uint8, device=device)
        if self.out_host is None or self.out_host.numel() < out_bytes:
            size = _align(max(out_bytes, 1 << 16) * 5 // 4, 4096)
            self.out_host = torch.empty(size, dtype=torch.uint8).pin_memory()
            self.out_dev = torch.empty(size, dtype=torch.uint8, device=device)
        if self.event is None:
            self.event = torch.cuda.Event()

    def drain(self):
        for f in self.pending:
            f.result()
        self.pending = []
        self.keep = None


def _encode(path, array, event=None):
    if event is not None:
        event.synchronize()          # the group's download has landed in the pinned buffer `array` views
    Image.fromarray(array).save(path)


class ReportWriter:
    """Writes the report of one evaluation run into output_dir.  add_group(items, results) per group of <= 16 images right after
    inference.count_images(..., return_crops=True); close() drains the encodes and writes results.csv / log.txt / test_stat.png
    (summary=False: pictures only, for the ranks > 0 of a sharded run).  Device tensors go through csrc/report.hip on the caller's
    current stream; CPU tensors through compose_host.  A steady stream of groups allocates nothing but what PIL needs: the staging
    buffers grow to the largest group and alternate between two groups, so group k's encodes overlap group k + 1's forward."""

    def __init__(self, output_dir, workers=4, external=False, summary=True):
        self.output_dir = str(output_dir)
        os.makedirs(self.output_dir, exist_ok=True)
        self.external = bool(external)
        self.summary = bool(summary)
        self.pool = ThreadPoolExecutor(max_workers=max(1, min(int(workers), MAX_WORKERS)))
        self.rows = []              # (name, pred_cnt, gt_cnt)
        self._stages = [_Stage(), _Stage()]
        self._turn = 0
        self._descs = None          # the ctypes descriptor arrays, made on the first device group
        self._strips = None
        self._host_pending = []
        self.last_stage = None
        self.closed = False

    # -- paths
    def full_path(self, name, pred_cnt):
        return os.path.join(self.output_dir, "full_%s__%d.png" % (Path(name).stem, round(pred_cnt)))

    def boxes_path(self, name):
        return os.path.join(self.output_dir, "boxes_%s.png" % Path(name).stem)

    # -- groups
    def add_group(self, items, results):
        """items: ReportItem per image; results: per image (pred_cnt, density_map[, crops]) as inference.count_images returns them --
        crops (the nine maps of the 3 x 3 path, or None) draw the prediction when present.  Returns the paths of the `full` pictures."""
        if self.closed:
            raise RuntimeError("ReportWriter.add_group after close()")
        if len(items) != len(results) or not 1 <= len(items) <= MAX_GROUP:
            raise ValueError("ReportWriter.add_group: 1..16 images and one result per image")
        items = [it if isinstance(it, ReportItem) else ReportItem(*it) for it in items]
        preds = [(r[2] if len(r) > 2 and r[2] is not None else r[1]) for r in results]
        for it, r in zip(items, results):
            self.rows.append((it.name, float(r[0]), it.gt_cnt))
        if items[0].sample.is_cuda:
            self._device_group(items, [float(r[0]) for r in results], preds)
        else:
            self._host_group(items, [float(r[0]) for r in results], preds)
        return [self.full_path(it.name, r[0]) for it, r in zip(items, results)]

    def _host_group(self, items, cnts, preds):
        done = [f for f in self._host_pending if f.done()]
        self._host_pending = [f for f in self._host_pending if not f.done()]
        for f in done:
            f.result()               # (an encode's exception surfaces at the next group)
        for it, cnt, pred in zip(items, cnts, preds):
            full = compose_host(it.sample, pred, it.gt_map, it.pos, it.gt_cnt, cnt, self.external)
            self._host_pending.append(self.pool.submit(_encode, self.full_path(it.name, cnt), full))
            if it.boxes is not None and it.boxes.nelement() > 0:
                self._host_pending.append(self.pool.submit(_encode, self.boxes_path(it.name), exemplar_strip_host(it.boxes)))

    def _device_group(self, items, cnts, preds):
        device = items[0].sample.device
        L = _lib.lib()
        if self._descs is None:
            self._descs = (_lib.ReportImage * MAX_GROUP)()
            self._strips = (_lib.ReportStrip * MAX_GROUP)()
        stage = self._stages[self._turn]
        self._turn ^= 1
        stage.drain()                                # its previous group's encodes have left the pinned pictures
        h = items[0].sample.shape[-2]
        # the blob: rectangles, label rasters, host gt maps -- laid out first, filled once the pinned buffer is large enough
        nrects = 0 if self.external else sum(len(it.pos or ()) for it in items)
        off = _align(16 * nrects)
        plan, keep = [], []
        out_off = 0
        for it, cnt, pred in zip(items, cnts, preds):
            w = it.sample.shape[-1]
            if it.sample.shape[-2] != h:
                raise ValueError("ReportWriter.add_group: the images of a group share one height")
            raster = label_raster(w, h, it.gt_cnt, cnt) if it.gt_cnt != 0 else text_raster(w, h, cnt)
            patch = raster_patch(raster)
            p_off = off
            if patch is not None:
                off = _align(off + patch[2].size)
            gt_off = None
            if not it.gt_map.is_cuda:
                gt_off = off
                off = _align(off + 4 * h * w)
            layout = 3 if it.gt_cnt != 0 else 2
            plan.append((w, layout, patch, p_off, gt_off, out_off))
            out_off = _align(out_off + h * layout * w * 3)
        strips = []
        for k, it in enumerate(items):
            if it.boxes is not None and it.boxes.nelement() > 0:
                ex = self._f32(it.boxes, keep)
                S = ex.numel() // (3 * ex.shape[-2] * ex.shape[-1])
                gh, gw = strip_shape(S, ex.shape[-2], ex.shape[-1])
                strips.append((k, ex, S, gh, gw, out_off))
                out_off = _align(out_off + gh * gw * 3)
        if strips and any(s[1].shape[-2:] != strips[0][1].shape[-2:] for s in strips):
            raise ValueError("ReportWriter.add_group: the exemplars of a group share one size")
        blob_bytes, out_bytes = max(off, 16), out_off
        with torch.cuda.device(device):
            stage.reserve(blob_bytes, out_bytes, device)
            blob = stage.blob_host.numpy()
            base = stage.blob_dev.data_ptr()
            rects = blob[:16 * nrects].view(np.int32).reshape(nrects, 4)
            r0 = 0
            for i, (it, pred, (w, layout, patch, p_off, gt_off, o_off)) in enumerate(zip(items, preds, plan)):
                d = self._descs[i]
                d.sam = self._f32(it.sample, keep).data_ptr()
                grid = isinstance(pred, (list, tuple))
                maps = [self._f32(m, keep) for m in pred] if grid else [self._f32(pred, keep)]
                if (len(maps) != 9 and grid) or any(m.numel() != h * w for m in maps):
                    raise ValueError("ReportWriter.add_group: a map does not have the sample's size")
                for k in range(9):
                    d.maps[k] = maps[k].data_ptr() if k < len(maps) else None
                if gt_off is None:
                    d.gt = self._f32(it.gt_map, keep).data_ptr()
                else:
                    blob[gt_off:gt_off + 4 * h * w].view(np.float32)[:] = it.gt_map.reshape(-1).float().numpy()
                    d.gt = base + gt_off
                if it.gt_map.numel() != h * w:
                    raise ValueError("ReportWriter.add_group: gt_map does not have the sample's size")
                d.out_off, d.w, d.layout, d.grid = o_off, w, layout, int(grid)
                cnt_r = 0 if self.external else len(it.pos or ())
                d.rect_off, d.rect_cnt = r0, cnt_r
                for k in range(cnt_r):
                    rects[r0 + k] = [int(v) for v in it.pos[k]]
                r0 += cnt_r
                pt = _lib.ReportPatch()
                if patch is not None:
                    px, py, arr = patch
                    blob[p_off:p_off + arr.size] = arr.reshape(-1)
                    pt.off, pt.px, pt.py, pt.pw, pt.ph = p_off, px, py, arr.shape[1], arr.shape[0]
                d.labels = pt if layout == 3 else _lib.ReportPatch()
                d.text = pt if layout == 2 else _lib.ReportPatch()
            cur = torch.cuda.current_stream(device)
            st = C.c_void_p(cur.cuda_stream)
            stage.blob_dev[:blob_bytes].copy_(stage.blob_host[:blob_bytes], non_blocking=True)       # the one upload
            _lib.check(L.countr_report_panels(self._descs, len(items), h, base, blob_bytes, 0, nrects, stage.out_dev.data_ptr(),
                                              out_bytes, st), "countr_report_panels")
            if strips:
                for j, (k, ex, S, gh, gw, o_off) in enumerate(strips):
                    self._strips[j].ex, self._strips[j].out_off, self._strips[j].S = ex.data_ptr(), o_off, S
                eh, ew = strips[0][1].shape[-2:]
                _lib.check(L.countr_report_quantize(self._strips, len(strips), eh, ew, stage.out_dev.data_ptr(), out_bytes, st),
                           "countr_report_quantize")
            stage.out_host[:out_bytes].copy_(stage.out_dev[:out_bytes], non_blocking=True)           # the one download
            stage.event.record(cur)
        stage.keep = keep
        host = stage.out_host.numpy()
        for it, cnt, (w, layout, _p, _po, _g, o_off) in zip(items, cnts, plan):
            view = host[o_off:o_off + h * layout * w * 3].reshape(h, layout * w, 3)
            stage.pending.append(self.pool.submit(_encode, self.full_path(it.name, cnt), view, stage.event))
        for k, _ex, _S, gh, gw, o_off in strips:
            view = host[o_off:o_off + gh * gw * 3].reshape(gh, gw, 3)
            stage.pending.append(self.pool.submit(_encode, self.boxes_path(items[k].name), view, stage.event))
        self.last_stage = stage

    @staticmethod
    def _f32(t, keep):
        """The tensor as the kernel reads it (fp32, contiguous); whatever had to be made for that lives until the stage is reused."""
        u = t if (t.dtype == torch.float32 and t.is_contiguous()) else t.float().contiguous()
        keep.append(u)
        return u

    def wait_download(self):
        """Blocks until the last device group's pictures are in host memory (tools/bench_report.py times up to here)."""
        st = self.last_stage
        if st is not None and st.event is not None:
            st.event.synchronize()

    def flush(self):
        """Blocks until every picture submitted so far is on disk; an encode's exception is raised here."""
        for st in self._stages:
            st.drain()
        for f in self._host_pending:
            f.result()
        self._host_pending = []

    # -- the summary
    def stats(self):
        n = max(len(self.rows), 1)
        errs = [abs(p - g) for _n, p, g in self.rows]
        return {"MAE": sum(errs) / n, "RMSE": (sum(e ** 2 for e in errs) / n) ** 0.5,
                "NAE": sum(e / g if g > 0 else 0 for e, (_n, _p, g) in zip(errs, self.rows)) / n}

    def close(self, timing=None, columns=None):
        """Drains the pool; with summary=True writes results.csv (time, name, prediction = round(pred)), appends one JSON line of
        MAE / RMSE / NAE and the `timing` keys to log.txt (FSC_test_cross(few-shot).py:429-445) and draws test_stat.png (:447-450).
        columns = (header names, {image name: values}) appends further columns to results.csv (--localize; an image without values
        gets empty cells); without it the file is the reference's.  Returns the logged dictionary."""
        if self.closed:
            return None
        self.closed = True
        try:
            self.flush()
        finally:
            self.pool.shutdown(wait=True)
        log_stats = dict(self.stats(), **(timing or {}))
        if not self.summary:
            return log_stats
        with open(os.path.join(self.output_dir, "results.csv"), "w", newline="") as f:
            wr = csv.writer(f, lineterminator="\n")
            more, cells = columns if columns is not None else ([], {})
            wr.writerow(["time", "name", "prediction"] + list(more))
            for k, (name, pred, _gt) in enumerate(self.rows):
                wr.writerow([k + 1, name, round(pred)] + list(cells.get(name, [""] * len(more))))
        with open(os.path.join(self.output_dir, "log.txt"), mode="a", encoding="utf-8") as f:
            f.write(json.dumps(log_stats) + "\n")
        try:
            import matplotlib
            matplotlib.use("Agg")
            import matplotlib.pyplot as plt
        except ImportError:
            print("ReportWriter: matplotlib is not installed, test_stat.png is not written")
            return log_stats
        fig = plt.figure()
        plt.scatter([g for _n, _p, g in self.rows], [abs(p - g) for _n, p, g in self.rows])
        plt.xlabel("Ground Truth")
        plt.ylabel("Error")
        fig.savefig(os.path.join(self.output_dir, "test_stat.png"))
        plt.close(fig)
        return log_stats
