"""CARPK on the device: what FSC_test_CARPK.py and FSC_finetune_CARPK.py do around the model, as HIP kernels on the stream the forward
runs on (csrc/carpk.hip).

    frames uint8 [H, W, 3] + boxes --countr_carpk_prep_u8--> image [n, 3, 384, 683] (torchvision's TENSOR resize: plain bilinear, no
    antialias) and exemplars [2 n, 3, 64, 64] cut from the original-resolution frame, one launch per group of frames
    --inference.density_maps_stream (4 windows per frame, the next group's encoder forward beside this group's decoder)-->
    maps [n, 384, 683] --countr_carpk_count--> {pred, total, n_over, e_cnt} per frame, one device-to-host copy per group

The host restatements the tests compare against live in countr_amd/data/carpk.py.  There is no host fallback."""
import ctypes as C

import torch

from . import _lib, _owned, inference
from .data import carpk as D
from .frames import FramePrep, _Slot, _is_u8, _stream

MAX_FRAMES = _lib.CARPK_MAX_FRAMES         # (and two rectangles per frame)
GROUP = 8                   # frames per forward: 8 x 4 windows = one batch of 32


class CarpkPrep(FramePrep):
    """countr_carpk_prep_u8 / countr_carpk_count with everything that must not be allocated per call: FramePrep's pinned staging and
    device uint8 buffers per frame shape, the count kernel's workspace, the training target's cell upload and the pinned buffers the
    results come back through.  Only the returned tensors are new."""

    def __init__(self, device="cuda"):
        super().__init__(device)
        self._count_ws = None
        self._results = []      # pinned [MAX_FRAMES, 4] per group position of a call
        self._cells = None      # (pinned int32, device int32) of the training target's cell list

    def _upload(self, frames):
        """The frames' bytes on the device (a slot per frame of one shape, as FramePrep.prepare deals them)."""
        used, srcs = {}, []
        for f in frames:
            if not _is_u8(f) or len(f.shape) != 3 or f.shape[2] != 3:
                raise ValueError("CarpkPrep: frames are uint8 [H, W, 3], got %s %s" % (f.dtype, tuple(f.shape)))
            key = (int(f.shape[0]), int(f.shape[1]))
            k = used.get(key, 0)
            used[key] = k + 1
            slots = self._slots.setdefault(key, [])
            if len(slots) <= k and not (isinstance(f, torch.Tensor) and f.is_cuda):
                slots.append(_Slot(key[0], key[1], self.device))
            srcs.append(self._frame_on_device(f, slots[k] if k < len(slots) else None))
        return srcs

    def prepare(self, frames, rects, out_cols=D.OUT_W):
        """frames: up to 16 uint8 [H, W, 3] (np.ndarray, CPU or device tensor; shapes free per frame); rects: [(frame, y1, x1, y2, x2),
        ...] inclusive, in pixels of the original frame -> (image [n, 3, 384, out_cols], exemplars [len(rects), 3, 64, 64]), fp32, in
        ONE launch.  out_cols = 683 for testing, 384 for training (the left 384 columns of the resized frame)."""
        n = len(frames)
        if not 1 <= n <= MAX_FRAMES or len(rects) > 2 * MAX_FRAMES:
            raise ValueError("CarpkPrep.prepare: 1..16 frames and at most 32 rectangles per call")
        with torch.cuda.device(self.device):
            cur = torch.cuda.current_stream(self.device)
            if self._last is not None and self._last[0] != cur:
                cur.wait_event(self._last[1])
            srcs = self._upload(frames)
            img = torch.empty(n, 3, D.OUT_H, out_cols, device=self.device, dtype=torch.float32)
            ex = torch.empty(len(rects), 3, D.BOX, D.BOX, device=self.device, dtype=torch.float32)
            fp = (C.c_void_p * n)(*[s.data_ptr() for s in srcs])
            shapes = (C.c_int * (2 * n))(*[int(v) for s in srcs for v in s.shape[:2]])
            flat = [int(v) for r in rects for v in r]
            ra = (C.c_int * max(len(flat), 1))(*flat)
            _lib.check(self.L.countr_carpk_prep_u8(fp, shapes, n, ra, len(rects), D.OUT_H, D.OUT_W, out_cols, img.data_ptr(),
                                                   ex.data_ptr() if len(rects) else None, _stream(self.device)), "countr_carpk_prep_u8")
            if self._last is None or self._last[0] != cur:
                self._last = (cur, torch.cuda.Event())
            self._last[1].record(cur)
        return img, ex

    def count(self, maps, rects):
        """maps [n, H, W] fp32 contiguous on the device, rects: per map two (a, b, c, d) = map[a : a + c + 1, b : b + d + 1] ->
        device fp32 [n, 4] = {pred, total, n_over, e_cnt} (countr_carpk_count)."""
        n, H, W = maps.shape
        if not (maps.is_cuda and maps.dtype == torch.float32 and maps.is_contiguous()) or not 1 <= n <= MAX_FRAMES or len(rects) != n:
            raise ValueError("CarpkPrep.count: contiguous fp32 device maps [n <= 16, H, W] and one pair of rectangles per map")
        with torch.cuda.device(self.device):
            if self._count_ws is None:
                self._count_ws = torch.empty(MAX_FRAMES * 32 * 4, device=self.device, dtype=torch.float32)
            if n * self.L.countr_carpk_count_blocks(H, W) * 4 > self._count_ws.numel():
                raise _lib.CountrError("countr_carpk_count_blocks exceeds the workspace")
            flat = [int(v) for pair in rects for r in pair for v in r]
            if len(flat) != 8 * n:
                raise ValueError("CarpkPrep.count: two (a, b, c, d) rectangles per map")
            out = torch.empty(n, 4, device=self.device, dtype=torch.float32)
            _lib.check(self.L.countr_carpk_count(maps.data_ptr(), n, H, W, (C.c_int * len(flat))(*flat), out.data_ptr(),
                                                 self._count_ws.data_ptr(), _stream(self.device)), "countr_carpk_count")
        return out

    def result_buffer(self, k):
        while len(self._results) <= k:
            self._results.append(torch.empty(MAX_FRAMES, 4, dtype=torch.float32).pin_memory())
        return self._results[k]

    def train_target(self, boxes):
        """gt_density of FSC_finetune_CARPK.py:229-238 -> [1, 384, 384] on the device: the host turns box centres into cells
        (data.carpk.train_cells), countr_aug_density filters them (60 * gaussian_filter(sigma 1))."""
        cells = D.train_cells(boxes)
        cap = max(len(cells), 1)
        with torch.cuda.device(self.device):
            if self._cells is None or self._cells[0].numel() < cap:
                size = max(1024, cap)
                self._cells = (torch.empty(size, dtype=torch.int32).pin_memory(), torch.empty(size, dtype=torch.int32, device=self.device),
                               torch.cuda.Event())
            host, dev, copied = self._cells
            copied.synchronize()            # the pinned list's previous upload has left it
            host[:cap] = 0
            if cells:
                host[:len(cells)] = torch.tensor([(y << 16) | x for y, x in cells], dtype=torch.int32)
            dev[:cap].copy_(host[:cap], non_blocking=True)
            copied.record(torch.cuda.current_stream(self.device))
            gt = torch.empty(1, 384, 384, device=self.device, dtype=torch.float32)
            d = _lib.AugImage()
            d.cell_off, d.cell_cnt = 0, len(cells)
            _lib.check(self.L.countr_aug_density(C.byref(d), 1, dev.data_ptr(), cap, gt.data_ptr(), _stream(self.device)), "countr_aug_density")
        return gt

    def train_sample(self, frame, boxes, idx):
        """One training sample of FSC_finetune_CARPK.py:204-240 (batch 1, 1-shot): exemplar `idx` cut from the full-resolution frame,
        the left 384 columns of the 384 x 683 resize, the target from the box centres ->
        (imgs [1, 3, 384, 384], boxes [1, 1, 3, 64, 64], gt [1, 384, 384])."""
        img, ex = self.prepare([frame], [[0] + D.box_rect(boxes[idx])], out_cols=D.TRAIN_COLS)
        return img, ex.unsqueeze(0), self.train_target(boxes)


def carpk_prep(device):
    """The CarpkPrep of a device, made on first use (count_carpk keeps its buffers here between calls)."""
    return _owned.instance(CarpkPrep, device)


def _stacked(dms):
    """The maps of one group as [n, H, W]: density_maps blends frames of one width into one tensor, so this is normally a view."""
    d0 = dms[0]
    step = d0.numel() * d0.element_size()
    if d0.is_contiguous() and all(d.shape == d0.shape and d.is_contiguous() and d.data_ptr() == d0.data_ptr() + k * step for k, d in enumerate(dms)):
        base = d0._base if d0._base is not None else d0
        if base.dim() == 3 and base.shape[0] >= len(dms) and base.data_ptr() == d0.data_ptr():
            return base[:len(dms)]
    return torch.stack(dms)


@torch.no_grad()
def count_carpk(model, frames, boxes_xywh, max_batch=32, prep=None):
    """FSC_test_CARPK.py:153-245 over many frames: frames uint8 [H, W, 3] each (host or device), boxes_xywh per frame the list of
    [x, y, w, h] boxes (at least two: boxes 0 and 1 are the exemplars, shot_num = 2) ->
    [(pred_cnt, density map [384, 683], {"total", "n_over", "e_cnt"}), ...].  Groups of up to 8 frames share one forward of up to
    max_batch windows; nothing is read back per image or per rectangle."""
    device = next(model.parameters()).device
    prep = prep or carpk_prep(device)
    per = max(1, min(GROUP, max_batch // len(inference.window_starts(D.OUT_W))))
    groups = [list(range(g0, min(g0 + per, len(frames)))) for g0 in range(0, len(frames), per)]
    for bx in boxes_xywh:
        if len(bx) < 2:
            raise ValueError("count_carpk: every frame needs at least two boxes (the script's two exemplars)")
        D.test_draws(len(bx))       # FSC_test_CARPK.py:160-164: drawn, then ignored

    def prepared():
        for sel in groups:
            rects = [[k] + D.box_rect(boxes_xywh[i][j]) for k, i in enumerate(sel) for j in (0, 1)]
            img, ex = prep.prepare([frames[i] for i in sel], rects)
            ex = ex.view(len(sel), 1, 2, 3, D.BOX, D.BOX)
            yield [img[k:k + 1] for k in range(len(sel))], [ex[k] for k in range(len(sel))]

    res, pending = [None] * len(frames), []
    with torch.cuda.device(device):
        for g, (sel, dms) in enumerate(zip(groups, inference.density_maps_stream(model, prepared(), 2, max_batch))):
            pairs = [D.script_rects(boxes_xywh[i]) for i in sel]             # what the script's slices of the exemplar boxes really cut
            out = prep.count(_stacked(dms), pairs)
            host = prep.result_buffer(g)
            host[:len(sel)].copy_(out, non_blocking=True)
            pending.append((sel, dms, host))
        torch.cuda.current_stream(device).synchronize()
    for sel, dms, host in pending:
        vals = host[:len(sel)].numpy()
        for k, i in enumerate(sel):
            res[i] = (float(vals[k, 0]), dms[k], {"total": float(vals[k, 1]), "n_over": int(vals[k, 2]), "e_cnt": float(vals[k, 3])})
    return res
