"""Pretraining batches from recipes: fsc147.transform_pretrain on the device.

A loader built with PretrainData(..., device_aug=True) hands over recipes (fsc147.recipe_pretrain): the decoded uint8 frame, the crop
rectangle of RandomResizedCrop and the flip coin.  PretrainAug.batch turns a list of them into the tensor PretrainStep.load() takes --
imgs [B, 3, 384, 384] fp32 -- with HIP kernels on the current stream (csrc/pretrain_aug.hip):

    frame --Pillow BILINEAR, horizontal then vertical--> 16-multiple frame --Pillow BICUBIC over the crop, horizontal--> [ch, 384]
    --vertical + flip + ToTensor--> imgs[b]

equal to transform_pretrain bit for bit.  Every sample has its own frame and crop size, so the tap tables are per sample: a fifth
kernel computes the four tables of each sample on the device (fp64, Pillow's operation order), equal to countr_pil_tables bit for
bit.  One host-to-device copy (the frames) and five launches per group of <= 16 samples whatever their sizes; the descriptors travel
as kernel arguments.  There is no host fallback."""
import ctypes as C

import numpy as np
import torch

from . import _lib, _owned
from .data import fsc147
from .device_aug import _Stage, _pad16

OUT = fsc147.MAX_HW
GROUP = _lib.PRETRAIN_MAX_IMAGES


def descriptors(entries, first_row=0):
    """countr_pretrain_image array of entries [(device address, H, W, (i, j, ch, cw), flip), ...] for batch rows first_row ..."""
    table = (_lib.PretrainImage * len(entries))()
    for k, (ptr, H, W, (i, j, ch, cw), flip) in enumerate(entries):
        d = table[k]
        d.frame, d.H, d.W, d.i, d.j, d.ch, d.cw, d.flip, d.row = (int(ptr) if ptr else None), int(H), int(W), int(i), int(j), int(ch), int(cw), int(bool(flip)), first_row + k
    return table


def layout(table):
    """countr_pretrain_aug_layout -> (tap stride, table ints, workspace bytes, [[first int of the table of axis a] per sample])."""
    n = len(table)
    sizes = (C.c_int64 * (3 + 4 * n))()
    _lib.check(_lib.lib().countr_pretrain_aug_layout(table, n, sizes), "countr_pretrain_aug_layout")
    return int(sizes[0]), int(sizes[1]), int(sizes[2]), [[int(sizes[3 + 4 * s + a]) for a in range(4)] for s in range(n)]


class PretrainAug:
    """Owns what must not be allocated per batch: two upload arenas used in turn (so that filling one does not wait for the previous
    batch's copy) and the device workspaces -- the tap tables and the uint8 intermediates of a group.  All grow on demand and never
    shrink.  Only the returned tensor is new in every call: PretrainStep.load() keeps a reference to it until the following step()."""

    def __init__(self, device="cuda"):
        self.device = _owned.resolve(device, "PretrainAug")
        self.L = _lib.lib()
        self._stages = [_Stage(self.device), _Stage(self.device)]
        self._turn = 0
        self._tables = self._ws = None
        self._last = None                              # (stream, event) of the previous batch, for a call from another stream
        self.launches = 0                              # kernel launches of the last call

    def workspace_bytes(self):
        ts = [self._tables, self._ws] + [t for s in self._stages for t in (s.host, s.dev)]
        return sum(t.numel() * t.element_size() for t in ts if t is not None)

    def tables(self, table):
        """The table workspace of one group (<= 16 descriptors), filled by countr_pretrain_aug_tables on the current stream ->
        (int32 device tensor, tap stride, [[first int per axis] per sample]).  The tensor is this object's workspace: the next call
        overwrites it."""
        stride, ints, _bytes, offs = layout(table)
        tabs = _owned.grow(self, "_tables", ints, torch.int32)
        with torch.cuda.device(self.device):
            st = _owned.stream_handle(self.device)
            _lib.check(self.L.countr_pretrain_aug_tables(table, len(table), tabs.data_ptr(), st), "countr_pretrain_aug_tables")
        return tabs, stride, offs

    def run(self, entries):
        """entries: [(device address of a uint8 [H, W, 3] frame, H, W, (i, j, ch, cw), flip), ...], the frames valid on the current
        stream -> imgs [len(entries), 3, 384, 384].  Groups of 16 follow each other on the current stream and share the workspaces."""
        B = len(entries)
        dev = self.device
        with torch.cuda.device(dev):
            cur = torch.cuda.current_stream(dev)
            st = C.c_void_p(cur.cuda_stream)
            if self._last is not None and self._last[0] != cur:
                cur.wait_event(self._last[1])
            self.launches = 0
            groups = [descriptors(entries[g0:g0 + GROUP], g0) for g0 in range(0, B, GROUP)]
            sizes = [layout(t) for t in groups]        # (every argument is checked here, before the first launch)
            tabs = _owned.grow(self, "_tables", max(s[1] for s in sizes), torch.int32)
            ws = _owned.grow(self, "_ws", max(s[2] for s in sizes), torch.uint8)
            imgs = torch.empty(B, 3, OUT, OUT, device=dev, dtype=torch.float32)
            for t in groups:
                _lib.check(self.L.countr_pretrain_aug_tables(t, len(t), tabs.data_ptr(), st), "countr_pretrain_aug_tables")
                _lib.check(self.L.countr_pretrain_aug(t, len(t), tabs.data_ptr(), ws.data_ptr(), imgs.data_ptr(), B, st), "countr_pretrain_aug")
                self.launches += 5
            if self._last is None or self._last[0] != cur:
                self._last = (cur, torch.cuda.Event())
            self._last[1].record(cur)
        return imgs

    def batch(self, recipes):
        """recipes: a list of fsc147.recipe_pretrain results -> imgs [B, 3, 384, 384] fp32 on the device, row b equal to
        transform_pretrain of recipe b's image with the same draws."""
        if len(recipes) < 1:
            raise ValueError("PretrainAug.batch: empty batch")
        frames, off, f_off = [], 0, []
        for r in recipes:
            fr = r["frame"]
            fr = fr.numpy() if isinstance(fr, torch.Tensor) else np.asarray(fr)
            if fr.dtype != np.uint8 or fr.ndim != 3 or fr.shape[2] != 3:
                raise ValueError("PretrainAug.batch: frames are uint8 [H, W, 3]")
            if fr.shape[0] < 16 or fr.shape[1] < 16:
                raise ValueError("PretrainAug.batch: a %d x %d frame resizes to a zero size (height and width must be >= 16)" % (fr.shape[1], fr.shape[0]))
            frames.append(fr)
            f_off.append(off)
            off += _pad16(fr.size)
        with torch.cuda.device(self.device):
            stage = self._stages[self._turn]
            self._turn ^= 1
            stage.reserve(off)
            hb = stage.host.numpy()
            for o, fr in zip(f_off, frames):
                hb[o:o + fr.size] = fr.reshape(-1)
            stage.upload(off)                          # the one upload of the batch: every frame, 16-byte aligned each
            base = stage.dev.data_ptr()
            return self.run([(base + o, fr.shape[0], fr.shape[1], r["crop"], r["flip"]) for o, fr, r in zip(f_off, frames, recipes)])
