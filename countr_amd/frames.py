"""Counting from raw frames: uint8 [H, W, 3] images and pixel-coordinate exemplar boxes in, counts and density maps out.

The preparation the reference leaves to PIL / torchvision on the host -- resize to height 384 with the width a multiple of 16
(demo_zero.py:23-38, demo.py:42-49), ToTensor, the 64 x 64 exemplar crops (demo.py:60-68) and the 3 x 3 crop-and-upscale for tiny
exemplars (:84-99) -- runs as HIP kernels on the stream the forward runs on (csrc/frames.hip: countr_frame_resize_u8,
countr_crop_resize_f32).  The prepared image equals PIL's BILINEAR resize + ToTensor bit for bit, and everything behind it is
inference.count_images / density_maps unchanged, so the results equal the host-prepared path's.  There is no host fallback.
count_frames(zoom=k) resizes to height 384 k instead and counts on a 2-D grid of tiles (countr_amd/tiles.py, csrc_tiles/tiles.hip)."""
import collections
import ctypes as C

import numpy as np
import torch

from . import _lib, _owned, classes as classes_, inference, overlay as overlay_, peaks, regions as regions_, tiles as tiles_, yuv as yuv_

NEW_H = 384
BOX = 64                    # exemplar crops are 64 x 64 (demo.py:67)
MAX_BATCHED = _lib.FRAMES_MAX              # frames / rectangles of one call


def new_width(W, H, new_h=NEW_H):
    """Width of the frame resized to height new_h (demo_zero.py:28-31, demo.py:42-44 with 384 = new_h)."""
    return 16 * int((W / H * new_h) / 16)


def scale_boxes(boxes_xyxy, W, H, new_h=NEW_H):
    """Boxes [(x1, y1, x2, y2), ...] in pixels of the ORIGINAL W x H frame -> rects [[y1, x1, y2, x2], ...] of the frame resized to height
    new_h, with the reference's scale factors and int() truncation (demo.py:45-46, 60-65).  The corners are inclusive (:66)."""
    sw, sh = float(new_width(W, H, new_h)) / W, float(new_h) / H
    return [[int(y1 * sh), int(x1 * sw), int(y2 * sh), int(x2 * sw)] for x1, y1, x2, y2 in boxes_xyxy]


BILINEAR, BICUBIC = 0, 1   # countr_pil_tables' filters


def _tables(export, *args):
    """(ksize, bounds int32 [out, 2], weights int32 [out, ksize]) of a host table export (..., in_size, out_size, bounds, weights)."""
    fn = getattr(_lib.lib(), export)
    ksize = fn(*args, None, None)
    _lib.check(min(ksize, 0), export)
    bounds = np.empty((args[-1], 2), np.int32)
    weights = np.empty((args[-1], ksize), np.int32)
    _lib.check(min(fn(*args, bounds.ctypes.data, weights.ctypes.data), 0), export)
    return ksize, bounds, weights


def pil_tables(in_size, out_size):
    """The tables of countr_pil_bilinear_tables, as numpy arrays: equal to pil_filter_tables(BILINEAR, ...), through the older export."""
    return _tables("countr_pil_bilinear_tables", in_size, out_size)


def pil_filter_tables(filter, in_size, out_size):
    """The tables of countr_pil_tables for BILINEAR or BICUBIC, as numpy arrays.  The bicubic weights have negative lobes: a pixel's sum
    is shifted arithmetically and then clamped to 0..255."""
    return _tables("countr_pil_tables", filter, in_size, out_size)


def _stream(device):
    return _owned.stream_handle(device)


def crop_resize(image, rects, oh, ow):
    """countr_crop_resize_f32: image [1, 3, h, w] (or [3, h, w]) fp32 on the device, rects [[y1, x1, y2, x2], ...] inclusive ->
    [n, 3, oh, ow] = F.interpolate(image[:, y1:y2 + 1, x1:x2 + 1], (oh, ow), bilinear) per rectangle."""
    if not (image.is_cuda and image.dtype == torch.float32 and image.is_contiguous() and image.shape[-3] == 3 and image.numel() == 3 * image.shape[-2] * image.shape[-1]):
        raise ValueError("crop_resize: a contiguous fp32 device image [1, 3, h, w] is required")
    h, w = image.shape[-2:]
    n = len(rects)
    out = torch.empty(n, 3, oh, ow, device=image.device, dtype=torch.float32)
    L = _lib.lib()
    with torch.cuda.device(image.device):
        for r0 in range(0, n, MAX_BATCHED):
            part = [int(v) for r in rects[r0:r0 + MAX_BATCHED] for v in r]
            arr = (C.c_int * len(part))(*part)
            _lib.check(L.countr_crop_resize_f32(image.data_ptr(), h, w, arr, len(part) // 4, oh, ow, out[r0:].data_ptr(), _stream(image.device)),
                       "countr_crop_resize_f32")
    return out


def exemplars(image, boxes_xyxy, W, H, new_h=NEW_H):
    """Exemplar tensors of one prepared frame: image [1, 3, new_h, new_W] (FramePrep.prepare), boxes in pixels of the original W x H frame
    -> (boxes [1, S, 3, 64, 64] on the device, rects [[y1, x1, y2, x2], ...]) as demo.py:60-71 builds them."""
    rects = scale_boxes(boxes_xyxy, W, H, new_h)
    return crop_resize(image, rects, BOX, BOX).unsqueeze(0), rects


def split_rects(h, w):
    """The nine h // 3 x w // 3 rectangles of the 3 x 3 split, in the order inference.count_image cuts them
    (FSC_test_cross(few-shot).py:273-320)."""
    return [[top, left, top + h // 3 - 1, left + w // 3 - 1]
            for top, left in ((0, 0), (h // 3, 0), (0, w // 3), (h // 3, w // 3), (h * 2 // 3, 0), (h * 2 // 3, w // 3),
                              (0, w * 2 // 3), (h // 3, w * 2 // 3), (h * 2 // 3, w * 2 // 3))]


def split_crops(image):
    """The nine crops of the 3 x 3 split, each upscaled back to the image's size: [[1, 3, h, w], ...] (views of one buffer)."""
    h, w = image.shape[-2:]
    up = crop_resize(image, split_rects(h, w), h, w)
    return [up[k:k + 1] for k in range(9)]


def _is_u8(f):
    return f.dtype == (torch.uint8 if isinstance(f, torch.Tensor) else np.uint8)


class _Slot:
    """The buffers of one frame position of one frame shape: pinned staging, the device copy, and the event of their last use."""

    def __init__(self, H, W, device):
        self.host = torch.empty(H, W, 3, dtype=torch.uint8).pin_memory()
        self.dev = torch.empty(H, W, 3, dtype=torch.uint8, device=device)
        self.copied = None


class FramePrep:
    """Resize + ToTensor of raw frames on the device.  Owns everything that must not be allocated per call: the tap tables per
    (in, out) size pair (device copies), and per frame shape in use the uint8 intermediate of the horizontal pass, pinned host staging
    buffers and device uint8 buffers (one per frame of that shape in a call).  Only the returned fp32 tensors are new."""

    def __init__(self, device="cuda"):
        self.device = _owned.resolve(device, "FramePrep")
        self.L = _lib.lib()
        self._tables = {}      # (in, out) -> (bounds, weights) on the device
        self._slots = {}       # (H, W) -> [_Slot, ...]
        self._tmp = {}         # (H, W, out height) -> uint8 [n, H, out_w, 3]
        self._last = None      # (stream, event) of the previous prepare: a call on another stream waits for it before it reuses the buffers
        self.yuv = None       # the YuvConverter of the YuvFrame items, made on first use

    def tables(self, in_size, out_size):
        t = self._tables.get((in_size, out_size))
        if t is None:
            _k, bounds, weights = pil_filter_tables(BILINEAR, in_size, out_size)
            t = self._tables[(in_size, out_size)] = (torch.from_numpy(bounds).to(self.device), torch.from_numpy(weights).to(self.device))
        return t

    def _frame_on_device(self, frame, slot):
        """The frame's bytes on the device: a contiguous uint8 device tensor is used where it is; a host frame goes through the slot's
        pinned buffer with an asynchronous copy."""
        if isinstance(frame, torch.Tensor) and frame.is_cuda:
            if frame.device != self.device:
                raise ValueError("FramePrep: frame on %s, this FramePrep is for %s" % (frame.device, self.device))
            return frame if frame.is_contiguous() else frame.contiguous()
        if slot.copied is not None:
            slot.copied.synchronize()          # the pinned buffer's previous copy must have left it (long done unless calls are back to back)
        if isinstance(frame, torch.Tensor):
            slot.host.copy_(frame)
        else:
            np.copyto(slot.host.numpy(), frame)
        slot.dev.copy_(slot.host, non_blocking=True)
        if slot.copied is None:
            slot.copied = torch.cuda.Event()
        slot.copied.record(torch.cuda.current_stream(self.device))
        return slot.dev

    def _convert_yuv(self, frames):
        """frames with every YuvFrame replaced by its RGB device buffer.  The buffers are reused from call to call like the slots, so the
        cross-stream guard of prepare() comes first."""
        with torch.cuda.device(self.device):
            cur = torch.cuda.current_stream(self.device)
            if self._last is not None and self._last[0] != cur:
                cur.wait_event(self._last[1])
            if self.yuv is None:
                self.yuv = yuv_.YuvConverter(self.device)
            idxs = [i for i, f in enumerate(frames) if isinstance(f, yuv_.YuvFrame)]
            for i, rgb in zip(idxs, self.yuv.convert([frames[i] for i in idxs])):
                frames[i] = rgb
        return frames

    def device_frames(self, frames):
        """The uint8 RGB device tensor [H, W, 3] of every item: the front part of prepare().  A host array goes through the pinned
        staging of its slot, a YuvFrame through the converter this FramePrep owns, a device tensor is used where it lies.  Handing the
        result to prepare() (or to an entry point) uploads and converts nothing again, so a frame goes to the device once for counting
        and for drawing.  The tensors of host and YuvFrame items are this FramePrep's buffers: the next call overwrites them."""
        frames = list(frames)
        if any(isinstance(f, yuv_.YuvFrame) for f in frames):
            frames = self._convert_yuv(frames)
        out, seen = [None] * len(frames), {}
        with torch.cuda.device(self.device):
            cur = torch.cuda.current_stream(self.device)
            if self._last is not None and self._last[0] != cur:
                cur.wait_event(self._last[1])
            for i, f in enumerate(frames):
                if not _is_u8(f) or len(f.shape) != 3 or f.shape[2] != 3:
                    raise ValueError("FramePrep.device_frames: frames are uint8 [H, W, 3], got %s %s" % (f.dtype, tuple(f.shape)))
                key = (int(f.shape[0]), int(f.shape[1]))
                k = seen[key] = seen.get(key, -1) + 1
                slot = None
                if not (isinstance(f, torch.Tensor) and f.is_cuda):
                    slots = self._slots.setdefault(key, [])
                    while len(slots) <= k:
                        slots.append(_Slot(key[0], key[1], self.device))
                    slot = slots[k]
                out[i] = self._frame_on_device(f, slot)
            if self._last is None or self._last[0] != cur:
                self._last = (cur, torch.cuda.Event())
            self._last[1].record(cur)
        return out

    def prepare(self, frames, new_h=NEW_H):
        """frames: uint8 [H, W, 3] each (np.ndarray, CPU tensor or device tensor) -> [[1, 3, new_h, new_W] fp32 device tensors], each equal
        to ToTensor(PIL resize((new_W, new_h), BILINEAR)) bit for bit.  Frames of one shape share launches (up to 16 per launch pair).
        A YuvFrame item (countr_amd/yuv.py) is first converted to RGB on the device, into a buffer of the YuvConverter this FramePrep
        owns, and is from there on a device frame like any other."""
        new_h = int(new_h)
        if any(isinstance(f, yuv_.YuvFrame) for f in frames):
            frames = self._convert_yuv(list(frames))
        out = [None] * len(frames)
        by_shape = {}
        for i, f in enumerate(frames):
            if not _is_u8(f) or len(f.shape) != 3 or f.shape[2] != 3:
                raise ValueError("FramePrep.prepare: frames are uint8 [H, W, 3], got %s %s" % (f.dtype, tuple(f.shape)))
            by_shape.setdefault((int(f.shape[0]), int(f.shape[1])), []).append(i)
        with torch.cuda.device(self.device):
            st = _stream(self.device)
            cur = torch.cuda.current_stream(self.device)
            if self._last is not None and self._last[0] != cur:
                cur.wait_event(self._last[1])
            for (H, W), idxs in by_shape.items():
                ow = new_width(W, H, new_h)
                if ow < 16:
                    raise ValueError("FramePrep.prepare: a %d x %d frame resizes to width %d" % (W, H, ow))
                hb, hw = self.tables(W, ow)
                vb, vw = self.tables(H, new_h)
                slots = self._slots.setdefault((H, W), [])
                while len(slots) < len(idxs):
                    slots.append(_Slot(H, W, self.device))
                nb = min(len(idxs), MAX_BATCHED)
                tmp = self._tmp.get((H, W, new_h))
                if tmp is None or tmp.shape[0] < nb:
                    tmp = self._tmp[(H, W, new_h)] = torch.empty(nb, H, ow, 3, dtype=torch.uint8, device=self.device)
                for g0 in range(0, len(idxs), MAX_BATCHED):
                    sel = idxs[g0:g0 + MAX_BATCHED]
                    srcs = [self._frame_on_device(frames[i], slots[g0 + k]) for k, i in enumerate(sel)]
                    for i in sel:
                        out[i] = torch.empty(1, 3, new_h, ow, device=self.device, dtype=torch.float32)
                    fp = (C.c_void_p * len(sel))(*[s.data_ptr() for s in srcs])
                    op = (C.c_void_p * len(sel))(*[out[i].data_ptr() for i in sel])
                    _lib.check(self.L.countr_frame_resize_u8(fp, op, len(sel), H, W, new_h, ow, hb.data_ptr(), hw.data_ptr(), vb.data_ptr(),
                                                             vw.data_ptr(), tmp.data_ptr(), st), "countr_frame_resize_u8")
            if self._last is None or self._last[0] != cur:
                self._last = (cur, torch.cuda.Event())
            self._last[1].record(cur)
        return out


def frame_prep(device):
    """The FramePrep of a device, made on first use (count_frames keeps its tables and workspaces here between calls)."""
    return _owned.instance(FramePrep, device)


def _sizes(frames):
    """(W, H) of every frame."""
    return [(int(f.shape[1]), int(f.shape[0])) for f in frames]


def _frame_exemplars(im, frame, boxes, i, new_h=NEW_H):
    """Frame i's boxes (boxes: None or one list per frame) cut from its prepared image im -> exemplars()' (crops, rects), or (an empty
    [1, 0] tensor, None) for a frame without boxes.  frame: the original frame, for its size."""
    if boxes is None or boxes[i] is None or len(boxes[i]) == 0:
        return torch.zeros(1, 0, device=im.device), None
    return exemplars(im, boxes[i], int(frame.shape[1]), int(frame.shape[0]), new_h)


def prepare_items(device, frames, boxes=None, prep=None, new_h=NEW_H):
    """Raw frames (+ per-frame lists of (x1, y1, x2, y2) boxes in original pixels, or None) -> the items inference.count_images takes:
    [(image [1, 3, new_h, new_W], exemplars [1, S, 3, 64, 64] or an empty [1, 0] tensor, rects or None), ...], all made on the device."""
    prep = prep or frame_prep(device)
    images = prep.prepare(frames, new_h)
    return [(im,) + _frame_exemplars(im, frames[i], boxes, i, new_h) for i, im in enumerate(images)]


@torch.no_grad()
def count_items_crops(model, items, normalization=True, max_s_cnt=1, max_batch=32):
    """count_items, which also hands back the nine maps of a frame that took the 3 x 3 path: [(count, density map, crops or None), ...]."""
    res = [None] * len(items)
    rest = []
    for idx, (im, ex, rects) in enumerate(items):
        if rects is not None and inference._small_exemplars(rects) >= max_s_cnt:
            dms = inference.density_maps(model, split_crops(im), [ex] * 9, ex.shape[1], max_batch)
            res[idx] = inference.split_count(dms, rects, normalization) + (dms,)
        else:
            rest.append(idx)
    if rest:
        for idx, r in zip(rest, inference.count_images(model, [items[i] for i in rest], normalization, max_s_cnt, max_batch, return_crops=True)):
            res[idx] = r
    return res


def count_items(model, items, normalization=True, max_s_cnt=1, max_batch=32):
    """inference.count_images over device-prepared items, with the 3 x 3 split of frames with tiny exemplars (demo.py:79-99) cut and
    upscaled by countr_crop_resize_f32.  The reference's quirks stay: the count of a split frame is the sum over its nine maps and its
    normalisation reads the LAST crop's map."""
    return [r[:2] for r in count_items_crops(model, items, normalization, max_s_cnt, max_batch)]


def frame_zooms(frames, boxes, zoom, zoom_max=3, max_s_cnt=1):
    """The zoom of every frame: `zoom` itself, or under zoom="auto" tiles.auto_zoom of the frame's boxes."""
    if zoom != "auto":
        return [int(zoom)] * len(frames)
    return [tiles_.auto_zoom(boxes[i] if boxes is not None else None, W, H, max_s_cnt, zoom_max) for i, (W, H) in enumerate(_sizes(frames))]


@torch.no_grad()
def count_frames_zoomed(model, frames, boxes, ks, normalization=True, max_s_cnt=1, max_batch=32, band_stride=128, crops=False):
    """count_frames with a zoom per frame (ks): [(count, density map), ...], or with crops=True [(count, density map, the nine maps of the
    3 x 3 path or None), ...].  The frames at zoom 1 run as ONE call of the existing path over just those frames.  A frame at k > 1 is
    resized from its own pixels to height 384 k (FramePrep), its exemplars are cut from that image, and its tiles run as forwards of
    their own (tiles.count_zoomed); it never takes the 3 x 3 split."""
    device = next(model.parameters()).device
    res = [None] * len(frames)
    ones = [i for i, k in enumerate(ks) if k == 1]
    if ones:
        items = prepare_items(device, [frames[i] for i in ones], [boxes[i] for i in ones] if boxes is not None else None)
        for i, r in zip(ones, count_items_crops(model, items, normalization, max_s_cnt, max_batch)):
            res[i] = r
    for k in sorted(set(ks) - {1}):
        sel = [i for i, kk in enumerate(ks) if kk == k]
        items = prepare_items(device, [frames[i] for i in sel], [boxes[i] for i in sel] if boxes is not None else None, new_h=NEW_H * k)
        for i, (im, ex, rects) in zip(sel, items):
            res[i] = tiles_.count_zoomed(model, im, ex, rects, normalization, max_batch, band_stride) + (None,)
    return res if crops else [r[:2] for r in res]


def _count_at_zoom(model, frames, boxes, zoom, zoom_max, band_stride, normalization, max_s_cnt, max_batch):
    """The counting of count_frames, locate_frames and annotate_frames behind their check_zoom: ([(count, density map, crops or None),
    ...], the height every frame was resized to).  zoom=1 is count_frames_zoomed with every k = 1: one count_items_crops call over all
    the frames."""
    ks = frame_zooms(frames, boxes, zoom, zoom_max, max_s_cnt)
    res = count_frames_zoomed(model, frames, boxes, ks, normalization, max_s_cnt, max_batch, band_stride, crops=True)
    return res, [NEW_H * k for k in ks]


def count_frames(model, frames, boxes=None, normalization=True, max_s_cnt=1, max_batch=32, *, zoom=1, zoom_max=3, band_stride=128):
    """Raw frames in, [(count, density map [384, new_W]), ...] out.  frames: uint8 [H, W, 3] each, on the host or on the model's device;
    boxes: None (zero-shot) or one list of (x1, y1, x2, y2) exemplar boxes per frame, in pixels of the original frame (an empty list =
    zero-shot for that frame).  Preparation runs on the device (FramePrep, exemplars); frames are then grouped by shot count and
    counted as inference.count_images counts them -- one forward per <= max_batch windows, the encoder pipelined across groups.
    zoom=k (2..4) counts from the frame's own pixels: the frame is resized to height 384 k instead of 384 and covered by a 2-D grid of
    384 x 384 tiles -- columns at the reference's stride 128, rows at band_stride (128, 192, 256 or 384) -- each tile one forward row,
    the tile maps stitched in both directions by the reference's sequential rule (countr_amd/tiles.py states it; csrc_tiles/tiles.hip
    computes it).  Such a frame returns (count, density map [384 k, Wk]) and never takes the 3 x 3 split.  zoom="auto" gives every
    frame the smallest k in 1..zoom_max at which fewer than max_s_cnt of its exemplars are under 10 px (zoom_max if none, 1 without
    boxes); its frames at 1 are counted as count_frames counts just them.  zoom=1 is the path above, untouched."""
    tiles_.check_zoom(zoom, zoom_max, band_stride)
    return [r[:2] for r in _count_at_zoom(model, frames, boxes, zoom, zoom_max, band_stride, normalization, max_s_cnt, max_batch)[0]]


ClassCounts = collections.namedtuple("ClassCounts", "names counts maps labels won total area")


@torch.no_grad()
def count_classes(model, frames, classes, *, normalization=True, max_s_cnt=1, max_batch=32, fold=True, floor=0.0):
    """Several object classes per frame from one encoder pass.  frames: as for count_frames; classes: a dict name -> boxes, boxes being
    what count_frames takes (None = zero-shot, or one list of (x1, y1, x2, y2) per frame); insertion order is the class index.  Returns
    per frame a ClassCounts(names, counts, maps, labels, won, total, area): counts[c] and maps[c] are what count_frames(model, frames,
    classes[names[c]]) returns for that frame, bit for bit -- the 3 x 3 split for tiny exemplars, the test-time normalisation and the
    grouping by shot count included.
    Sharing.  The frames are prepared once.  Every class forms its forward batches as count_frames forms them
    (inference.class_batches); batches of different classes over the same windows and of the same batch size run ONE encoder forward
    (inference.density_maps_shared): the encoder and the first decoder block's self-attention half never see the exemplars.  A class
    whose frames take another path (one frame on the 3 x 3 split, say) has other batches and runs its own encoder for them.
    The fold (fold=True, at most 16 classes; countr_amd/classes.py states the rule, csrc_classes/classes.hip computes it): labels is a
    uint8 device tensor [384, new_W] naming per pixel the class with the largest scale[c] * maps[c] (255: none above floor), with
    scale[c] = counts[c] / sum(maps[c]) (1 / 60 where the sum is 0), so that total[c] ~ counts[c]; won[c] is the part of total[c] on
    the pixels class c owns and area[c] their number (numpy arrays).  A frame on which ANY class took the 3 x 3 split has, for that
    class, nine maps of another geometry: it gets labels = won = total = area = None.  With fold=False the four fields are None and any
    number of classes is allowed."""
    names = list(classes)
    if fold and len(names) > classes_.MAX_CLASSES:
        raise ValueError("count_classes: the fold takes at most %d classes, got %d (fold=False takes any number)"
                         % (classes_.MAX_CLASSES, len(names)))
    device = next(model.parameters()).device
    images = frame_prep(device).prepare(frames)
    F_ = len(images)
    widths = [int(im.shape[-1]) for im in images]
    ex, rects, split, groups = [], [], [], collections.OrderedDict()
    for c, name in enumerate(names):
        ex.append([]); rects.append([]); split.append([])
        for f, im in enumerate(images):
            e, r = _frame_exemplars(im, frames[f], classes[name], f)
            ex[c].append(e); rects[c].append(r)
            split[c].append(r is not None and inference._small_exemplars(r) >= max_s_cnt)
        shots = [int(e.shape[1]) if e.nelement() > 0 else 0 for e in ex[c]]
        for S, variants, _windows, bucket in inference.class_batches(widths, shots, split[c], max_batch):
            groups.setdefault((bucket, tuple(variants)), []).append((c, S))
    crops, dm = {}, {}                      # frame -> its nine upscaled crops; (class, variant) -> map
    for (_bucket, variants), members in groups.items():
        for f, k in variants:
            if k >= 0 and f not in crops:
                crops[f] = split_crops(images[f])
        ims = [images[f] if k < 0 else crops[f][k] for f, k in variants]
        jobs = [([ex[c][f] for f, _k in variants], S) for c, S in members]
        for (c, _S), maps in zip(members, inference.density_maps_shared(model, ims, jobs, max_batch)):
            for v, m in zip(variants, maps):
                dm[(c, v)] = m
    counts = [[None] * len(names) for _ in range(F_)]
    maps = [[None] * len(names) for _ in range(F_)]
    sums = {}
    for f in range(F_):
        for c in range(len(names)):
            if split[c][f]:
                counts[f][c], maps[f][c] = inference.split_count([dm[(c, (f, k))] for k in range(9)], rects[c][f], normalization)
            else:
                maps[f][c] = m = dm[(c, (f, -1))]
                sums[(f, c)] = tot = m.sum()
                counts[f][c] = inference._normalise((tot / 60).item(), m, rects[c][f], normalization)
    folded = {}
    if fold and names:
        plain = [f for f in range(F_) if not any(split[c][f] for c in range(len(names)))]
        if plain:
            tot = torch.stack([sums[(f, c)] for f in plain for c in range(len(names))]).tolist()       # one transfer for every sum
            sets = []
            for i, f in enumerate(plain):
                t = tot[i * len(names):(i + 1) * len(names)]
                sets.append((maps[f], [counts[f][c] / t[c] if t[c] != 0 else 1.0 / 60 for c in range(len(names))]))
            for f, r in zip(plain, classes_.class_folder(device).fold(sets, floor)):
                folded[f] = r
    return [ClassCounts(tuple(names), tuple(counts[f]), tuple(maps[f]), *folded.get(f, (None, None, None, None))) for f in range(F_)]


def frame_points(cy, cx, W, H, new_w, new_h=NEW_H):
    """Centroids (cy, cx) of the resized [new_h, new_w] map -> (x, y) in pixel-centre coordinates of the ORIGINAL W x H frame, in float64:
    x = (cx + 0.5) W / new_w - 0.5, y = (cy + 0.5) H / new_h - 0.5."""
    cy, cx = np.asarray(cy, np.float64), np.asarray(cx, np.float64)
    return (cx + 0.5) * W / new_w - 0.5, (cy + 0.5) * H / new_h - 0.5


def crop_points(cy, cx, k, h, w):
    """Centroids of crop k of the 3 x 3 split (the crop was upscaled from h // 3 x w // 3 back to h x w) -> (cy, cx) of the [h, w] image
    the crops were cut from: cy_img = top + (cy + 0.5) (h // 3) / h - 0.5 with split_rects(h, w)[k] = (top, left, ., .), cx likewise."""
    top, left = split_rects(h, w)[k][:2]
    cy, cx = np.asarray(cy, np.float64), np.asarray(cx, np.float64)
    return top + (cy + 0.5) * (h // 3) / h - 0.5, left + (cx + 0.5) * (w // 3) / w - 0.5


def _keep_count(P, count, keep):
    if keep == "all":
        return P
    if keep != "count":
        raise ValueError('keep is "all" or "count"')
    return min(P, max(0, int(np.floor(count + 0.5))))


def _crops_of(results, crops):
    """The crops per frame that locate_maps and region_maps read: the explicit list, or without one every (count, map, crops) entry's own
    third field and None for a (count, map) entry."""
    return crops or [r[2] if len(r) == 3 else None for r in results]


def _fp32_maps(maps):
    """The maps as the side libraries take them: fp32 and contiguous (a map that is both is used where it lies)."""
    return [m if (m.dtype == torch.float32 and m.is_contiguous()) else m.float().contiguous() for m in maps]


def locate_maps(results, sizes, crops=None, *, radius=4, threshold=0.0, rel_threshold=0.1, max_points=4096, keep="all", new_h=NEW_H):
    """The points of counted frames: results [(count, density map [384, new_W] on the device), ...], sizes [(W, H), ...] of the original
    frames, crops per frame None or the nine maps of the 3 x 3 path -> [(points float32 [P, 2] as (x, y), score [P], total), ...].
    Every map of the call (the nine crop maps of a split frame included) goes through ONE PeakFinder.find.  new_h: the height the
    frames were resized to, one number or one per frame (384 k for a frame counted at zoom k).  A results entry may also be (count,
    density map, crops) as count_items_crops returns it: without crops= its third field is the frame's crops."""
    crops = _crops_of(results, crops)
    heights = [int(new_h)] * len(results) if np.ndim(new_h) == 0 else [int(v) for v in new_h]
    if len(heights) != len(results):
        raise ValueError("locate_maps: new_h is one height, or one per frame")
    maps, first = [], []
    for r, cr in zip(results, crops):
        first.append(len(maps))
        maps.extend(cr if cr is not None else [r[1]])
    if not maps:
        return []
    found = peaks.peak_finder(maps[0].device).find(_fp32_maps(maps), radius, threshold, rel_threshold, max_points)
    out = []
    for (count, dm, *_cr), (W, H), cr, f0, nh in zip(results, sizes, crops, first, heights):
        h, w = dm.shape
        if cr is None:
            pk = found[f0]
            cy, cx, score, total = pk.centroid[:, 0], pk.centroid[:, 1], pk.score, pk.total
        else:
            nine = found[f0:f0 + 9]
            parts = [crop_points(pk.centroid[:, 0], pk.centroid[:, 1], k, h, w) for k, pk in enumerate(nine)]
            cy, cx = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
            score = np.concatenate([pk.score for pk in nine])
            crop = np.concatenate([np.full(len(pk.score), k) for k, pk in enumerate(nine)])
            idx = np.concatenate([pk.yx[:, 0].astype(np.int64) * w + pk.yx[:, 1] for pk in nine])
            order = np.lexsort((idx, crop, -score))                    # (score descending, crop, idx)
            cy, cx, score = cy[order], cx[order], score[order]
            total = sum(pk.total for pk in nine)
        x, y = frame_points(cy, cx, W, H, w, nh)
        P = _keep_count(len(score), count, keep)
        out.append((np.stack([x, y], 1).astype(np.float32)[:P], np.asarray(score, np.float32)[:P], total))
    return out


@torch.no_grad()
def locate_items(model, items, sizes, *, radius=4, threshold=0.0, rel_threshold=0.1, max_points=4096, keep="all", normalization=True,
                 max_s_cnt=1, max_batch=32, crops=False):
    """count_items + locate_maps over device-prepared items: [(count, density map, points, score, total peaks), ...]; with crops=True
    each tuple ends with the nine maps of the 3 x 3 path, or None."""
    res = count_items_crops(model, items, normalization, max_s_cnt, max_batch)
    pts = locate_maps(res, sizes, radius=radius, threshold=threshold, rel_threshold=rel_threshold, max_points=max_points, keep=keep)
    return [(c, dm, p, s, t) + ((cr,) if crops else ()) for (c, dm, cr), (p, s, t) in zip(res, pts)]


@torch.no_grad()
def locate_frames(model, frames, boxes=None, *, radius=4, threshold=0.0, rel_threshold=0.1, max_points=4096, keep="all", normalization=True,
                  max_s_cnt=1, max_batch=32, regions=None, zoom=1, zoom_max=3, band_stride=128):
    """count_frames that also says WHERE: [(count, density map, points float32 [P, 2] as (x, y), score [P]), ...].  count and density map
    are count_frames' bit for bit.  points are the sub-pixel centroids of the map's peaks (countr_amd/peaks.py states the rule) in
    pixel-centre coordinates of the original frame (frame_points), ordered by score; keep="count" keeps the first
    min(P, floor(count + 0.5)) of them.  A frame that takes the 3 x 3 split gets the peaks of its nine crop maps, mapped back through
    crop_points and re-ordered by (score descending, crop, raster index); its returned map stays the last crop's.  The defaults
    radius=4 and rel_threshold=0.1 are unmeasured: no localisation accuracy figure exists for them.
    With regions (count_regions' argument) each tuple gains region_counts float32 [R] and point_region int32 [P]: the first region that
    contains each point by the regions' own rule (countr_amd/regions.py), -1 = none.
    zoom, zoom_max, band_stride: count_frames' arguments.  The peaks of a zoomed frame's [384 k, Wk] map go through the same PeakFinder
    and map to the original frame through frame_points(..., new_h=384 k).  radius stays in pixels of the map that is searched: an
    object is k times larger there, so a radius chosen at zoom 1 is k times tighter at zoom k.  regions together with a zoom other than
    1 raises ValueError."""
    tiles_.check_zoom(zoom, zoom_max, band_stride)
    sizes = _sizes(frames)
    if zoom != 1 and regions is not None:
        raise ValueError("locate_frames: regions are counted at zoom=1 only")
    res, heights = _count_at_zoom(model, frames, boxes, zoom, zoom_max, band_stride, normalization, max_s_cnt, max_batch)
    pts = locate_maps(res, sizes, radius=radius, threshold=threshold, rel_threshold=rel_threshold, max_points=max_points, keep=keep,
                      new_h=heights)
    out = [(c, dm, p, s) for (c, dm, _cr), (p, s, _t) in zip(res, pts)]
    if regions is None:
        return out
    per = frame_regions(regions, sizes)
    sums = _region_sums(res, sizes, None, per)
    return [r + (counts, regions_.point_regions(r[2], rs)) for r, rs, (counts, _area) in zip(out, per, sums)]


def cut_exemplars(device, frame, boxes, prep=None):
    """The exemplar crops [1, S, 3, 64, 64] of one frame's boxes (pixels of that frame), cut on the device as prepare_items cuts them."""
    if boxes is None or len(boxes) == 0:
        raise ValueError("shared exemplars: at least one box")
    return prepare_items(device, [frame], [boxes], prep)[0][1]


def shared_exemplar_items(device, frames, crops, prep=None):
    """The items of frames that all count with ONE set of exemplar crops (cut_exemplars): every item is (image, crops, None) -- no
    rectangles, so no frame takes the 3 x 3 split or the rectangle normalisation.  What a user who outlines objects on the first frame of
    a clip means."""
    return [(im, crops, None) for im, _ex, _r in prepare_items(device, frames, None, prep)]


def _is_shared(boxes):
    return isinstance(boxes, tuple) and len(boxes) == 2 and isinstance(boxes[0], (int, np.integer))


def _clip_groups(who, device, frames, boxes, group, on_device=False):
    """count_clip's and count_flow's walk over a clip: (items, sizes, frames) of every consecutive group of `group` frames.  boxes: None,
    one list per frame, or (k, boxes): the exemplar crops are then cut once, from frame k of the call, before the first group.  who: the
    calling function's name, for the error texts.  on_device: the group's frames go through FramePrep.device_frames first and are
    yielded as those device tensors, so that what draws on them uploads nothing again."""
    if int(group) != group or group < 1:
        raise ValueError("%s: group is >= 1" % who)
    frames = list(frames)
    cut = None
    if _is_shared(boxes):
        k, bx = boxes
        if not 0 <= int(k) < len(frames):
            raise ValueError("%s: (k, boxes) names a frame of the call" % who)
        cut = cut_exemplars(device, frames[int(k)], bx)
    for g0 in range(0, len(frames), int(group)):
        part = frames[g0:g0 + int(group)]
        if on_device:
            part = frame_prep(device).device_frames(part)
        if cut is not None:
            items = shared_exemplar_items(device, part, cut)
        else:
            items = prepare_items(device, part, boxes[g0:g0 + int(group)] if boxes is not None else None)
        yield items, _sizes(part), part


@torch.no_grad()
def count_clip(model, frames, boxes=None, *, max_dist, lines=None, group=8, max_missed=2, min_hits=3, beta=0.5, tracker=None, radius=4,
               threshold=0.0, rel_threshold=0.1, max_points=4096, keep="all", normalization=True, max_s_cnt=1, max_batch=32, summaries=False,
               camera=None, search=4, interval=1, min_gain=256, min_texture=128, cam_tol=8, min_voters=16, counter=None):
    """locate_frames over a clip, its points joined over time: ([(count, density map, points, score, ids int32 [P], events uint32 [P]),
    ...] per frame, ClipCounts(started, confirmed, dropped, line_counts int [L, 2] as (forward, backward), live)).  frames: whatever
    count_frames takes, YuvFrames included, in time order.  Consecutive groups of `group` frames go through locate_frames' path -- count,
    map, points and score are locate_frames' over the same group bit for bit -- and each group's points then go through Tracker.run on
    the same stream: one more synchronisation per group, not per frame.  ids[i] is the track of point i (-1: dropped at the 4096-track
    limit); bit k of events[i] says the point's track crossed line k forward on this frame, bit 16 + k backward (countr_amd/tracks.py
    and include/countr_hip_tracks.h state the rule).  Points are pixel centres of the original frame, so max_dist is in pixels of the
    frame per frame interval, and lines -- up to 16 segments (ax, ay, bx, by) -- are in the same pixels.
    boxes: None, one list per frame, or (k, boxes): the exemplar crops are cut once from frame k of the call and reused for every frame
    (cut_exemplars, shared_exemplar_items), equal to count_items on those items bit for bit.
    tracker=: a Tracker(streams=1) to continue -- the live-stream case; max_dist, lines, max_missed, min_hits and beta are then the
    tracker's own and lines must be left None.  summaries=True: each frame's tuple ends with its step's summary int32 [40] (live,
    started, confirmed, matched, born, died, dropped, frame, counts[16][2]).  zoom is not taken: the clip is tracked at zoom 1.  The defaults of max_missed, min_hits
    and beta, like radius and rel_threshold, are unmeasured: no accuracy figure exists.
    camera="translation": the clip is tracked in scene coordinates under a panning camera (countr_amd/cam.py states the rule).  The
    luma, motion (search, interval, min_gain) and camera estimate (min_texture, cam_tol, min_voters: unmeasured on real video) of each
    group's prepared images run through a line-less FlowCounter, and the detections go to the Tracker as fl32(p + C_t), one fp64 add per
    coordinate, rounded once: max_dist and the lines are then in pixels of the FIRST frame.  The returned points stay locate_frames'
    bytes, and each frame's tuple ends with C_t float64 (x, y).  counter=: a FlowCounter(lines=(), camera=...) to continue with
    tracker=; camera and its settings are then the counter's own."""
    rows, clip = [], None
    for part, clip in _track_groups("count_clip", model, frames, boxes, max_dist=max_dist, lines=lines, group=group, max_missed=max_missed,
                                    min_hits=min_hits, beta=beta, tracker=tracker, radius=radius, threshold=threshold,
                                    rel_threshold=rel_threshold, max_points=max_points, keep=keep, normalization=normalization,
                                    max_s_cnt=max_s_cnt, max_batch=max_batch, camera=camera, search=search, interval=interval,
                                    min_gain=min_gain, min_texture=min_texture, cam_tol=cam_tol, min_voters=min_voters, counter=counter):
        if part is not None:
            rows += [r[:6] + ((summary,) if summaries else ()) + where for r, summary, where, _crops, _frame in part]
    return rows, clip


def _track_groups(who, model, frames, boxes, *, max_dist, lines, group, max_missed, min_hits, beta, tracker, radius, threshold, rel_threshold,
                  max_points, keep, normalization, max_s_cnt, max_batch, camera, search, interval, min_gain, min_texture, cam_tol, min_voters,
                  counter, on_device=False):
    """count_clip's walk, a group at a time, for count_clip and annotate_clip: yields ([((count, map, points, score, ids, events), summary,
    (C_t,) or (), the nine crop maps or None, the frame), ...], ClipCounts so far) per group, and at the end (None, the clip's ClipCounts)
    -- the tracker's own state when the clip had no frame.  on_device: _clip_groups' argument; `the frame` is then its device tensor."""
    from . import flow as flow_, tracks as tracks_
    device = next(model.parameters()).device
    if tracker is None:
        tracker = tracks_.Tracker(device, max_dist=max_dist, max_missed=max_missed, min_hits=min_hits, beta=beta, lines=lines if lines is not None else ())
    elif tracker.streams != 1 or lines is not None:
        raise ValueError("%s: tracker= is a Tracker of one stream, and the lines are its own" % who)
    if counter is not None and (camera is not None or counter.camera is None or counter.lines.shape[0]):
        raise ValueError("%s: counter= is a line-less FlowCounter with a camera, and the camera is its own" % who)
    if counter is None and camera is not None:
        counter = flow_.FlowCounter(device, lines=(), search=search, interval=interval, min_gain=min_gain, camera=camera,
                                    min_texture=min_texture, cam_tol=cam_tol, min_voters=min_voters)
    L, last = tracker.lines.shape[0], None
    for items, sizes, part in _clip_groups(who, device, frames, boxes, group, on_device):
        res = locate_items(model, items, sizes, radius=radius, threshold=threshold, rel_threshold=rel_threshold, max_points=max_points,
                           keep=keep, normalization=normalization, max_s_cnt=max_s_cnt, max_batch=max_batch, crops=True)
        points, where = [r[2] for r in res], [()] * len(res)
        if counter is not None:
            t0 = counter.frames
            counter.run([it[0] for it in items], [None] * len(items), sizes)
            path = counter.camera_path()
            where = [(path.position(t0 + k, counter.placement),) for k in range(len(res))]
            points = [(p.astype(np.float64) + c).astype(np.float32) for p, (c,) in zip(points, where)]
        out = []
        for r, c, f, (ids, events, summary) in zip(res, where, part, tracker.run(points)):
            out.append((r[:4] + (ids, events), summary, c, r[5], f))
            last = summary
        yield out, tracks_.clip_counts(last, L)
    if last is None:
        st = tracker.state()
        yield None, tracks_.ClipCounts(st["started"], st["confirmed"], st["dropped"], st["counts"][:L].astype(np.int64), st["id"].shape[0])
    else:
        yield None, tracks_.clip_counts(last, L)


@torch.no_grad()
def count_flow(model, frames, boxes=None, *, lines, search=4, interval=1, min_gain=256, band=None, group=8, counter=None, motion=False,
               normalization=True, max_s_cnt=1, max_batch=32, camera=None, min_texture=128, cam_tol=8, min_voters=16):
    """count_frames over a clip, with the number of objects that crossed each line read from the flux of the density map -- the
    peak-free counterpart of count_clip's line counts: ([(count, density map, flux float32 [L, 2] as (forward, backward) or None), ...]
    per frame, FlowCounts(line_counts float64 [L, 2], frames, counted)); with motion=True each tuple ends with the frame's motion field
    int16 [48, new_W / 8, 2] as (x, y) in 1/16 map px (zeros for the first `interval` frames).  frames: whatever count_frames takes,
    YuvFrames included, in time order and of ONE shape.  Consecutive groups of `group` frames go through count_frames' path -- count and
    map are count_frames' over the same group bit for bit -- and then through FlowCounter.run on the same stream: the luma of the
    prepared image the forward read, its motion against the frame `interval` back (the history crosses the groups), the flux of the map
    through the lines (countr_amd/flow.py and include/countr_hip_flow.h state the rule); one more synchronisation per group.
    flux is scale * the frame's flux with scale = count / (total / 60), the test-time normalisation carried as count_regions carries it;
    line_counts is its sum over the clip in float64.  The first `interval` frames count nothing (flux None), and so does a frame that
    took the 3 x 3 split: it has no frame map; its luma still enters the history.  lines: up to 16 segments (ax, ay, bx, by) in pixels of
    the original frame, the tracker's lines: forward ends on its side 1.  band: the width of the counting band in frame pixels (default
    8 H / 384).  boxes: None, one list per frame, or (k, boxes) as in count_clip.  counter=: a FlowCounter to continue -- the live-stream
    case; lines, search, interval, min_gain and band are then the counter's own and lines must be None.  zoom is not taken.  The defaults
    of search, min_gain and band are unmeasured and no accuracy figure exists; motion under about half a map pixel per interval is
    underestimated, which is what interval is for.
    camera="translation": the lines are counted in scene coordinates under a panning camera (countr_amd/cam.py states the rule;
    FlowCounter the order of a chunk): the lines are in pixels of the FIRST frame, each frame's tuple ends with the camera's position
    C_t float64 (x, y) in frame pixels, and a group costs two synchronisations instead of one.  count and map are untouched.  min_texture,
    cam_tol and min_voters are unmeasured on real video.  With counter= the camera is the counter's own.  motion=True still returns the
    raw field."""
    from . import flow as flow_
    device = next(model.parameters()).device
    if counter is None:
        counter = flow_.FlowCounter(device, lines=lines if lines is not None else (), search=search, interval=interval, min_gain=min_gain, band=band,
                                    camera=camera, min_texture=min_texture, cam_tol=cam_tol, min_voters=min_voters)
    elif lines is not None or camera is not None:
        raise ValueError("count_flow: counter= is a FlowCounter, and the lines are its own" + (", and so is the camera" if lines is None else ""))
    out = []
    for items, sizes, _part in _clip_groups("count_flow", device, frames, boxes, group):
        res = count_items_crops(model, items, normalization, max_s_cnt, max_batch)
        t0 = counter.frames
        got = counter.run([it[0] for it in items], [None if cr is not None else dm for _c, dm, cr in res], sizes,
                          counts=[c for c, _dm, _cr in res], motion=motion)
        path = counter.camera_path() if counter.camera is not None else None
        for k, ((c, dm, _cr), (flux, mv, total)) in enumerate(zip(res, got)):
            if flux is not None:
                flux = (flow_.frame_scale(c, total) * flux.astype(np.float64)).astype(np.float32)
            if motion and mv is None:
                mv = np.zeros((dm.shape[0] // flow_.CELL, dm.shape[1] // flow_.CELL, 2), np.int16)
            out.append((c, dm, flux) + ((mv,) if motion else ()) + ((path.position(t0 + k, counter.placement),) if path is not None else ()))
    return out, counter.counts()


def _frame_polygons(regions, n):
    """annotate_frames' `regions` -> one list of polygons per frame (one list for every frame, or one list per frame)."""
    if regions is None:
        return [None] * n
    per = _per_frame(regions, n)
    if any(_is_grid(r) for rs in per for r in rs):
        raise ValueError("annotate_frames draws polygons: a grid has no outline")
    return per


@torch.no_grad()
def annotate_frames(model, frames, boxes=None, *, out="rgb", gain=127.5, colormap="red", points=False, point_radius=2, regions=None,
                    label=True, matrix=None, range=None, radius=4, threshold=0.0, rel_threshold=0.1, max_points=4096, keep="all",
                    normalization=True, max_s_cnt=1, max_batch=32, zoom=1, zoom_max=3, band_stride=128):
    """count_frames that also shows what it found: [(count, density map, annotated, points or None, score or None), ...].  count and
    density map are count_frames' bit for bit and, with points=True, points and score are locate_frames' (radius, threshold,
    rel_threshold, max_points, keep: its peak settings).  annotated is the frame's own pixels at the frame's own size with the density map
    as a colour overlay (gain, colormap), the count as a label (label=True), the outlines of `regions` (polygons as count_regions takes
    them; they are drawn, not counted) and a dot of point_radius per point, composed on the device (countr_amd/overlay.py states the
    rule): a uint8 device tensor [H, W, 3], or for out = "nv12" / "nv21" / "i420" the packed 4:2:0 buffer YuvFrame.from_buffer reads,
    in `matrix` / `range` (default: a YuvFrame's own, bt709 / limited for other frames).  The tensors are buffers of the device's
    Overlay: the next call overwrites them.  Every frame goes to the device once (FramePrep.device_frames) for counting and drawing.
    A frame that took the 3 x 3 split has no single map of the frame: it is drawn WITHOUT heat, with label and marks only.  Under zoom
    the heat comes from the [384 k, Wk] map."""
    tiles_.check_zoom(zoom, zoom_max, band_stride)
    device = next(model.parameters()).device
    n = len(frames)
    sizes = _sizes(frames)
    spaces = [(matrix or (f.matrix if isinstance(f, yuv_.YuvFrame) else "bt709"), range or (f.range if isinstance(f, yuv_.YuvFrame) else "limited"))
              for f in frames]
    polygons = _frame_polygons(regions, n)
    dev = frame_prep(device).device_frames(frames)
    res, heights = _count_at_zoom(model, dev, boxes, zoom, zoom_max, band_stride, normalization, max_s_cnt, max_batch)
    located = [(None, None, None)] * n
    if points:
        located = locate_maps(res, sizes, radius=radius, threshold=threshold, rel_threshold=rel_threshold, max_points=max_points, keep=keep,
                              new_h=heights)
    pictures = overlay_.overlay_for(device).render(
        dev, [None if cr is not None else dm for _c, dm, cr in res], gain=gain, colormap=colormap, points=[p for p, _s, _t in located],
        point_radius=point_radius, regions=polygons, labels=[overlay_.count_label(r[0], *wh) if label else None for r, wh in zip(res, sizes)],
        out=out, matrix=[s[0] for s in spaces], range=[s[1] for s in spaces])
    return [(c, dm, pic, p, s) for (c, dm, _cr), pic, (p, s, _t) in zip(res, pictures, located)]


@torch.no_grad()
def annotate_clip(model, frames, boxes=None, *, max_dist, lines=None, line_names=None, out="rgb", heat=True, gain=127.5, colormap="red",
                  trail=16, tags=True, tally=True, hud=True, scale=None, matrix=None, range=None, trails=None, group=8, max_missed=2,
                  min_hits=3, beta=0.5, tracker=None, radius=4, threshold=0.0, rel_threshold=0.1, max_points=4096, keep="all",
                  normalization=True, max_s_cnt=1, max_batch=32, summaries=False, camera=None, search=4, interval=1, min_gain=256,
                  min_texture=128, cam_tol=8, min_voters=16, counter=None):
    """count_clip that also shows what it found.  A GENERATOR over the clip's groups of `group` frames: each iteration yields
    ([(count, density map, points, score, ids, events, annotated), ...] of the group's frames, ClipCounts so far); with summaries=True
    each tuple gains the step's summary behind annotated, and with a camera it ends with C_t, as count_clip's.  count through events are
    count_clip's bit for bit, and every other argument is count_clip's.
    annotated is the frame's own pixels at the frame's own size: the density map as a colour overlay (heat, gain, colormap: the
    Overlay's; a frame that took the 3 x 3 split is drawn without heat, as annotate_frames draws it), then what clip_marks draws --
    every track's trail of the last `trail` positions (0: none) in the track's colour, the counting lines with their names
    (line_names, default "0", "1", ...) and running tallies, a disc and the id per point, and count, live tracks and confirmed total at
    the top left; scale: the marks' size, default by the frame's height (countr_amd/draw.py states the rule).  It is a uint8 device
    tensor [H, W, 3], or for out = "nv12" / "nv21" / "i420" the packed 4:2:0 buffer YuvFrame.from_buffer reads, in `matrix` / `range`
    (default: a YuvFrame's own, bt709 / limited for other frames).  THE TENSORS ARE BUFFERS of the device's Overlay and Painter: they are
    valid until the next iteration, which overwrites them -- that is why this is a generator; copy what must outlive the step.
    Every frame goes to the device once (FramePrep.device_frames).  Per group: count_clip's locate path and Tracker.run, then
    Overlay.render and Painter.paint on the same stream, with no synchronisation beyond count_clip's one per group -- the marks are built
    from what that download brought.  trails=: a draw.Trails to continue with tracker= (the live-stream case; `trail` is then its own).
    zoom is not taken."""
    from . import draw as draw_
    device = next(model.parameters()).device
    frames = list(frames)
    spaces = [(matrix or (f.matrix if isinstance(f, yuv_.YuvFrame) else "bt709"), range or (f.range if isinstance(f, yuv_.YuvFrame) else "limited"))
              for f in frames]
    if trails is None and trail:
        trails = draw_.Trails(trail)
    done = 0
    for part, clip in _track_groups("annotate_clip", model, frames, boxes, max_dist=max_dist, lines=lines, group=group, max_missed=max_missed,
                                    min_hits=min_hits, beta=beta, tracker=tracker, radius=radius, threshold=threshold,
                                    rel_threshold=rel_threshold, max_points=max_points, keep=keep, normalization=normalization,
                                    max_s_cnt=max_s_cnt, max_batch=max_batch, camera=camera, search=search, interval=interval,
                                    min_gain=min_gain, min_texture=min_texture, cam_tol=cam_tol, min_voters=min_voters, counter=counter,
                                    on_device=True):
        if part is None:
            return
        if tracker is None:          # the lines as the tracker holds them: what was counted is what is drawn
            drawn = np.asarray(lines if lines is not None else (), np.float32).reshape(-1, 4)
        else:
            drawn = tracker.lines
        names = list(line_names) if line_names is not None else ["%d" % k for k in np.arange(len(drawn))]
        if len(names) != len(drawn):
            raise ValueError("annotate_clip: one name per line")
        pictures = overlay_.overlay_for(device).render(
            [f for _r, _s, _c, _cr, f in part], [r[1] if (heat and cr is None) else None for r, _s, _c, cr, _f in part], gain=gain,
            colormap=colormap, out="rgb")
        marks = []
        for r, summary, where, _cr, f in part:
            pos = r[2].astype(np.float64) + (where[0] if where else 0.0)                   # scene pixels under a camera
            marks.append(draw_.clip_marks(r[2], r[4], r[5], summary, names, drawn, r[0], where[0] if where else None,
                                          size=(int(f.shape[1]), int(f.shape[0])), trails=trails.update(pos, r[4]) if trails is not None else None,
                                          scale=scale, tags=tags, tally=tally, hud=hud))
        sp = spaces[done:done + len(part)]
        done += len(part)
        painted = draw_.painter_for(device).paint(pictures, marks, out=out, matrix=[a for a, _b in sp], range=[b for _a, b in sp])
        yield [r + (pic,) + ((summary,) if summaries else ()) + where for (r, summary, where, _cr, _f), pic in zip(part, painted)], clip


def map_placement(W, H, new_w, new_h=NEW_H):
    """The placement (ax, bx, ay, by) of a frame's [new_h, new_w] map in pixel-centre coordinates of the original W x H frame, in float64:
    frame_points as one multiply and one add per axis -- x = (W / new_w) cx + frame_points(0, 0)'s x."""
    x0, y0 = frame_points(0.0, 0.0, W, H, new_w, new_h)
    return (np.float64(W) / new_w, np.float64(x0), np.float64(H) / new_h, np.float64(y0))


def crop_placement(k, h, w, placement):
    """The placement of crop k's [h, w] map (3 x 3 split of an [h, w] image whose own placement is given): crop_points composed with it.
    Crop pixel cx lies at image column (w // 3) / w * cx + crop_points(0, 0)'s column, and an image column c at ax * c + bx."""
    ax, bx, ay, by = placement
    cy0, cx0 = crop_points(0.0, 0.0, k, h, w)
    return (ax * (np.float64(w // 3) / w), ax * np.float64(cx0) + bx, ay * (np.float64(h // 3) / h), ay * np.float64(cy0) + by)


def _is_grid(r):
    return isinstance(r, (tuple, list)) and len(r) == 3 and isinstance(r[0], str)


def _is_region(r):
    if _is_grid(r):
        return True
    try:
        v = np.asarray(r, np.float64)
    except (TypeError, ValueError):
        return False
    return v.ndim == 2 and v.shape[1] == 2


def _per_frame(regions, n):
    """`regions` -- one list of regions for every frame, or one list per frame -- as one list per frame of n frames."""
    regions = list(regions)
    per = [regions] * n if all(_is_region(r) for r in regions) else regions
    if len(per) != n:
        raise ValueError("regions: one list for every frame, or one list per frame")
    return per


def frame_regions(regions, sizes):
    """count_regions' `regions` -> one list of regions.region() per frame.  regions: one list for every frame, or one list per frame; a
    region is a polygon [(x, y), ...] in pixels of the original frame, or ("grid", gy, gx) = the uniform grid over the frame (explicit
    boundaries ("grid", ys, xs) pass through)."""
    return [[regions_.frame_grid(W, H, int(r[1]), int(r[2])) if _is_grid(r) and np.ndim(r[1]) == 0 else regions_.region(r) for r in rs]
            for rs, (W, H) in zip(_per_frame(regions, len(sizes)), sizes)]


def region_maps(results, sizes, crops, regions):
    """The regional counts of counted frames: results [(count, density map [384, new_W] on the device), ...], sizes [(W, H), ...] of the
    original frames, crops per frame None or the nine maps of the 3 x 3 path, regions as count_regions takes them (frame_regions) ->
    [(region_counts float32 [R], region_area int32 [R]), ...].  Every map of the call goes through ONE RegionSummer.sum; a split
    frame's nine crop maps add into the frame's regions.  region_counts[r] = scale * mass[r] / 60 with scale = count / (total / 60)
    when total > 0, else 1: the scale carries the test-time normalisation and nothing else, so regions that partition the frame sum
    to count up to the reduction's rounding.  A results entry may also be (count, density map, crops) as count_items_crops returns it:
    with crops None its third field is the frame's crops."""
    return _region_sums(results, sizes, crops, frame_regions(regions, sizes))


def _region_sums(results, sizes, crops, regions):
    """region_maps behind its frame_regions: regions is that function's result, which count_regions and locate_frames already hold."""
    crops = _crops_of(results, crops)
    maps, places, set_of_map = [], [], []
    for f, ((_c, dm, *_cr), (W, H), cr) in enumerate(zip(results, sizes, crops)):
        h, w = dm.shape
        pl = map_placement(W, H, w)
        for k, m in enumerate(cr if cr is not None else [dm]):
            maps.append(m)
            places.append(pl if cr is None else crop_placement(k, h, w, pl))
            set_of_map.append(f)
    if not maps:
        return []
    sums = regions_.region_summer(maps[0].device).sum(_fp32_maps(maps), places, set_of_map, regions)
    out = []
    for r, (mass, area, total) in zip(results, sums):
        pred = np.float64(total) / 60
        scale = np.float64(r[0]) / pred if total > 0 else np.float64(1.0)
        out.append(((scale * mass.astype(np.float64) / 60).astype(np.float32), area))
    return out


@torch.no_grad()
def count_regions(model, frames, regions, boxes=None, *, normalization=True, max_s_cnt=1, max_batch=32):
    """count_frames that also answers "how many in this part of the frame": [(count, density map, region_counts float32 [R], region_area
    int32 [R]), ...].  regions: one list for every frame or one list per frame; a region is a polygon [(x, y), ...] in pixel-centre
    coordinates of the original frame (pixel i has centre i) or ("grid", gy, gx), the uniform grid over the frame, which owns gy * gx
    results, row-major.  count and the map are count_frames' bit for bit.  The counts are sums of the density map over the regions
    (countr_amd/regions.py states the rule; csrc_ext/regions.hip computes it), scaled as region_maps says; region_area is the number of
    map pixels whose centre lies in the region.  A frame that takes the 3 x 3 split is summed over its nine crop maps."""
    device = next(model.parameters()).device
    items = prepare_items(device, frames, boxes)
    sizes = _sizes(frames)
    per = frame_regions(regions, sizes)
    res = count_items_crops(model, items, normalization, max_s_cnt, max_batch)
    sums = _region_sums(res, sizes, None, per)
    return [(c, dm, counts, area) for (c, dm, _cr), (counts, area) in zip(res, sums)]
