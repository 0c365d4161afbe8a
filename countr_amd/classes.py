"""Several object classes in one frame: the fold of a frame's class density maps into a dominant-class label map.

    classes_host   the rule of countr_class_fold (include/countr_hip_classes.h) restated in numpy: the product in float32 as a ufunc of
                   its own, the sums in float64 -- the yardstick of the GPU tests, as regions_host and peaks_host are
    ClassFolder    the same fold from csrc_classes/classes.hip on the stream the forward runs on: one packed upload, two launches per
                   <= 16 frames, one asynchronous download and one synchronisation per call

The rule.  A set is one frame: nc class maps [h, w] and one scale per class.  v_c(p) = scale[c] * map_c[p], one fp32 multiply.
label(p) is the smallest c that attains max_c v_c(p), and 255 when that maximum is <= floor.  won[c] is the sum of v_c over the pixels
with label c, total[c] the sum of v_c over all pixels, area[c] the number of pixels with label c.  CounTR puts mass on every salient
object, so the maps of two classes overlap; won[c] is the part of class c's count that lies where c is the strongest class."""
import ctypes as C

import numpy as np

from . import _lib, _owned

MAX_SETS, MAX_CLASSES = _lib.CLASSES_CONSTS["COUNTR_CLASSES_MAX_SETS"], _lib.CLASSES_CONSTS["COUNTR_CLASSES_MAX"]
NONE = 255                  # the label of a pixel whose largest v_c is <= floor
MAX_PIXELS = 1 << 28


def classes_host(maps, scale, floor=0.0, members=False):
    """maps: nc arrays [h, w], scale: nc numbers -> (labels uint8 [h, w], won float64 [nc], total float64 [nc], area int64 [nc]); with
    members=True also (won_abs, total_abs) = the sums of |v_c| over the same pixels (the tests' error bound)."""
    v = np.stack([np.multiply(np.float32(s), np.asarray(m, dtype=np.float32)) for m, s in zip(maps, scale)])      # float32 products
    best = v.max(axis=0)
    labels = v.argmax(axis=0).astype(np.uint8)                 # (argmax: the first index that attains the maximum)
    labels[best <= np.float32(floor)] = NONE
    d = v.astype(np.float64)
    nc = len(v)
    mine = [labels == c for c in range(nc)]
    won = np.array([d[c][mine[c]].sum() for c in range(nc)])
    total = d.reshape(nc, -1).sum(axis=1)
    area = np.array([int(m.sum()) for m in mine], np.int64)
    if not members:
        return labels, won, total, area
    return labels, won, total, area, np.array([np.abs(d[c][mine[c]]).sum() for c in range(nc)]), np.abs(d).reshape(nc, -1).sum(axis=1)


class ClassFolder:
    """countr_class_fold on device maps.  Owns the workspace, the packed upload (pinned + device) and the result buffers (device +
    pinned); they grow monotonically, so a steady stream of calls allocates nothing but its results (the label maps and host arrays)."""

    def __init__(self, device="cuda"):
        self.device = _owned.resolve(device, "ClassFolder")
        self.L = _lib.classes_lib()
        self._ws = None             # uint8, one chunk's scratch (the chunks of a call follow each other on one stream)
        self._sets = self._sets_host = None         # uint8: the countr_class_set structs of every chunk of a call
        self._out = self._out_host = None           # int32: per set won [16] (float bits) | total [16] (float bits) | area [16]
        self._guard = _owned.Guard(self.device)     # a call on another stream than the previous one waits before it reuses the buffers

    def _reserve(self, ws_bytes, nsets):
        import torch
        _owned.grow(self, "_ws", ws_bytes, torch.uint8)
        _owned.grow(self, "_sets", nsets * C.sizeof(_lib.ClassSet), torch.uint8, pinned=True)
        _owned.grow(self, "_out", nsets * 3 * MAX_CLASSES, torch.int32, pinned=True)

    def fold(self, sets, floor=0.0):
        """sets: [(maps, scale), ...], a set = one frame: maps = nc contiguous fp32 [h, w] device tensors of one shape, scale = nc numbers
        -> per set (labels uint8 [h, w] on the device, won float32 [nc], total float32 [nc], area int32 [nc]), on the current stream.
        Any number of sets: 16 go into one pair of launches."""
        import torch
        sets = [(list(maps), np.asarray(scale, np.float32).reshape(-1)) for maps, scale in sets]
        if not sets:
            return []
        who = "countr_class_fold"
        for s, (maps, scale) in enumerate(sets):
            if not 1 <= len(maps) <= MAX_CLASSES:
                raise _lib.CountrError("%s: set %d: a set has 1..16 classes, got %d" % (who, s, len(maps)))
            if len(scale) != len(maps):
                raise _lib.CountrError("%s: set %d: a scale per class" % (who, s))
            for c, m in enumerate(maps):
                if m is None:
                    raise _lib.CountrError("%s: set %d: map %d: null or misaligned" % (who, s, c))
                if not (isinstance(m, torch.Tensor) and m.is_cuda and m.device == self.device and m.dtype == torch.float32 and m.dim() == 2
                        and m.is_contiguous()):
                    raise _lib.CountrError("%s: set %d: map %d: maps are contiguous fp32 [h, w] tensors on %s" % (who, s, c, self.device))
                if m.shape != maps[0].shape:
                    raise _lib.CountrError("%s: set %d: the maps of a set have one shape, got %s and %s"
                                           % (who, s, tuple(maps[0].shape), tuple(m.shape)))
        n, size = len(sets), C.sizeof(_lib.ClassSet)
        with torch.cuda.device(self.device):
            self._reserve(16, n)
            desc = (_lib.ClassSet * n).from_buffer(self._sets_host.numpy())
            labels = []
            for d, (maps, scale) in zip(desc, sets):
                h, w = int(maps[0].shape[0]), int(maps[0].shape[1])
                # (the library refuses what breaks its limits; a refused call must not have allocated a 2^28-pixel label map first)
                lab = torch.empty((h, w) if 0 < h * w <= MAX_PIXELS else (1, 1), dtype=torch.uint8, device=self.device)
                labels.append(lab)
                C.memset(C.addressof(d), 0, size)
                d.nc, d.h, d.w, d.labels = len(maps), h, w, lab.data_ptr()
                for c, m in enumerate(maps):
                    d.map[c], d.scale[c] = m.data_ptr(), float(scale[c])
            chunks = [(k, min(MAX_SETS, n - k)) for k in range(0, n, MAX_SETS)]
            ws_bytes = 16
            for k, cnt in chunks:
                b = self.L.countr_classes_workspace(C.byref(desc[k]), cnt)
                _lib.classes_check(min(b, 0), "countr_classes_workspace")
                ws_bytes = max(ws_bytes, b)
            self._reserve(ws_bytes, n)
            cur = self._guard.enter()
            self._sets[:n * size].copy_(self._sets_host[:n * size], non_blocking=True)        # the one upload
            st = C.c_void_p(cur.cuda_stream)
            out, per = self._out.data_ptr(), 4 * MAX_CLASSES
            for k, cnt in chunks:
                _lib.classes_check(self.L.countr_class_fold(
                    C.byref(desc[k]), cnt, self._sets.data_ptr() + k * size, float(floor), out + k * per, out + (n + k) * per,
                    out + (2 * n + k) * per, self._ws.data_ptr(), st), who)
            ints = 3 * n * MAX_CLASSES
            self._out_host[:ints].copy_(self._out[:ints], non_blocking=True)                  # the one download
            self._guard.leave(cur)
        self._guard.event.synchronize()              # the one wait of the call
        got = self._out_host[:ints].numpy().reshape(3, n, MAX_CLASSES)
        res = []
        for s, (maps, _scale) in enumerate(sets):
            nc = len(maps)
            res.append((labels[s], got[0, s, :nc].view(np.float32).copy(), got[1, s, :nc].view(np.float32).copy(), got[2, s, :nc].copy()))
        return res


def class_folder(device):
    """The ClassFolder of a device, made on first use (count_classes keeps its buffers here between calls)."""
    return _owned.instance(ClassFolder, device)
