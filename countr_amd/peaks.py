"""Object locations from density maps: where the counted objects are.

    peaks_host    the rule of countr_density_peaks (include/countr_hip.h) restated in numpy: decisions in float32, sums in float64 -- the
                  yardstick of the GPU tests, as compose_host is for the report
    PeakFinder    the same peaks from csrc/peaks.hip on the stream the forward runs on: one call of the export per <= 16 maps, one
                  asynchronous download per call, one synchronisation at its end

The rule: with m the map's maximum (a NaN never wins), pixel p = (y, x) with value v is a peak iff v > threshold, v >= rel_threshold * m
(one fp32 multiply) and, for every other q of the (2 r + 1)^2 window around p clipped to the map, v > d(q) or v == d(q) and p comes first
in raster order.  Per peak, with w(q) = max(d(q), 0) over the window: score = v, mass = sum(w) / 60, centroid = p + sum(w (q - p)) / sum(w).
At most `cap` peaks are kept, the first in raster order, and the kept ones are ordered by (score descending, raster index ascending)."""
import ctypes as C
from collections import namedtuple

import numpy as np

from . import _lib, _owned

MAX_MAPS, MAX_RADIUS, MAX_CAP = _lib.PEAKS_MAX_MAPS, _lib.PEAKS_MAX_RADIUS, _lib.PEAKS_MAX_POINTS
REC = 6                     # {y, x, score, cy, cx, mass}

# total: the true number of peaks (beyond max_points too); the arrays hold the P = min(total, max_points) kept ones in score order
Peaks = namedtuple("Peaks", "total yx score centroid mass")


def _check(radius, threshold, rel_threshold, cap):
    if not (1 <= int(radius) <= MAX_RADIUS and 1 <= int(cap) <= MAX_CAP and threshold >= 0 and 0 <= rel_threshold <= 1):
        raise ValueError("peaks: radius is 1..8, max_points 1..8192, threshold >= 0 and 0 <= rel_threshold <= 1")


def peaks_host(map, radius=4, threshold=0.0, rel_threshold=0.1, cap=4096):
    """map [h, w] (anything np.asarray takes, or a CPU tensor) -> (total, recs float64 [P, 6] = {y, x, score, cy, cx, mass}) in the
    kernel's order and layout."""
    _check(radius, threshold, rel_threshold, cap)
    d = np.ascontiguousarray(np.asarray(map, dtype=np.float32))
    if d.ndim != 2 or d.size == 0:
        raise ValueError("peaks_host: a map is [h, w] with h, w >= 1")
    h, w = d.shape
    r = int(radius)
    finite = d[~np.isnan(d)]
    m = np.float32(finite.max()) if finite.size else np.float32(-np.inf)
    with np.errstate(invalid="ignore"):
        rel = np.float32(rel_threshold) * m                      # one fp32 multiply
        ok = (d > np.float32(threshold)) & (d >= rel)
        pad = np.full((h + 2 * r, w + 2 * r), -np.inf, np.float32)        # outside the map: below every candidate
        pad[r:r + h, r:r + w] = d
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                if dy == 0 and dx == 0:
                    continue
                q = pad[r + dy:r + dy + h, r + dx:r + dx + w]
                behind = dy > 0 or (dy == 0 and dx > 0)           # idx(p) < idx(q)
                ok &= ((d > q) | (d == q)) if behind else (d > q)
    idx = np.flatnonzero(ok)
    total = int(idx.size)
    idx = idx[:int(cap)]
    recs = np.empty((idx.size, REC), np.float64)
    for k, i in enumerate(idx):
        y, x = divmod(int(i), w)
        ya, yb, xa, xb = max(y - r, 0), min(y + r, h - 1), max(x - r, 0), min(x + r, w - 1)
        win = d[ya:yb + 1, xa:xb + 1].astype(np.float64)
        wt = np.where(win > 0, win, 0.0)
        s = wt.sum()
        oy = np.arange(ya, yb + 1, dtype=np.float64)[:, None] - y
        ox = np.arange(xa, xb + 1, dtype=np.float64)[None, :] - x
        recs[k] = (y, x, d[y, x], y + (wt * oy).sum() / s, x + (wt * ox).sum() / s, s / 60.0)
    order = np.lexsort((idx, -recs[:, 2]))
    return total, recs[order]


def _split(total, recs):
    recs = np.asarray(recs)
    return Peaks(int(total), np.ascontiguousarray(recs[:, 0:2]).astype(np.int32), recs[:, 2].astype(np.float32),
                 np.ascontiguousarray(recs[:, 3:5]).astype(np.float32), recs[:, 5].astype(np.float32))


class PeakFinder:
    """countr_density_peaks on device maps.  Owns the workspace, the `totals` / `recs` device buffers and their pinned mirrors; they grow
    monotonically, so a steady stream of calls allocates nothing but its (host) results."""

    def __init__(self, device="cuda"):
        self.device = _owned.resolve(device, "PeakFinder")
        self.L = _lib.lib()
        self._descs = (_lib.PeakMap * MAX_MAPS)()
        self._ws = None             # uint8, one chunk's scratch (the chunks of a call follow each other on one stream)
        self._totals = self._recs = self._totals_host = self._recs_host = None
        self._guard = _owned.Guard(self.device)     # a call on another stream than the previous one waits before it reuses the buffers

    def _reserve(self, ws_bytes, nmaps, cap):
        import torch
        _owned.grow(self, "_ws", ws_bytes, torch.uint8)
        _owned.grow(self, "_totals", nmaps, torch.int32, pinned=True)
        _owned.grow(self, "_recs", nmaps * cap * REC, torch.float32, pinned=True)

    def find(self, maps, radius=4, threshold=0.0, rel_threshold=0.1, max_points=4096):
        """maps: fp32 [h, w] device tensors (contiguous; sizes free per map) -> [Peaks(total, yx int32 [P, 2], score [P], centroid
        float32 [P, 2] as (cy, cx), mass [P]), ...] as numpy arrays, on the current stream."""
        import torch
        _check(radius, threshold, rel_threshold, max_points)
        cap, n = int(max_points), len(maps)
        if n == 0:
            return []
        for m in maps:
            if not (isinstance(m, torch.Tensor) and m.is_cuda and m.device == self.device and m.dtype == torch.float32 and m.dim() == 2
                    and m.numel() > 0 and m.is_contiguous()):
                raise ValueError("PeakFinder.find: maps are contiguous fp32 [h, w] tensors on %s" % self.device)
        ws_bytes = 0
        for c0 in range(0, n, MAX_MAPS):
            part = maps[c0:c0 + MAX_MAPS]
            b = self.L.countr_peaks_workspace(len(part), max(m.shape[0] for m in part), max(m.shape[1] for m in part), cap)
            _lib.check(min(b, 0), "countr_peaks_workspace")
            ws_bytes = max(ws_bytes, b)
        with torch.cuda.device(self.device):
            self._reserve(ws_bytes, n, cap)
            cur = self._guard.enter()
            st = C.c_void_p(cur.cuda_stream)
            for c0 in range(0, n, MAX_MAPS):
                part = maps[c0:c0 + MAX_MAPS]
                for j, m in enumerate(part):
                    self._descs[j].map, self._descs[j].h, self._descs[j].w = m.data_ptr(), m.shape[0], m.shape[1]
                _lib.check(self.L.countr_density_peaks(self._descs, len(part), int(radius), float(threshold), float(rel_threshold), cap,
                                                       self._totals[c0:].data_ptr(), self._recs[c0 * cap * REC:].data_ptr(),
                                                       self._ws.data_ptr(), st), "countr_density_peaks")
            self._totals_host[:n].copy_(self._totals[:n], non_blocking=True)
            self._recs_host[:n * cap * REC].copy_(self._recs[:n * cap * REC], non_blocking=True)
            self._guard.leave(cur)
        self._guard.event.synchronize()                   # the one wait of the call
        totals = self._totals_host[:n].numpy()
        recs = self._recs_host[:n * cap * REC].numpy().reshape(n, cap, REC)
        return [_split(totals[i], recs[i, :min(int(totals[i]), cap)]) for i in range(n)]


def peak_finder(device):
    """The PeakFinder of a device, made on first use (locate_frames keeps its buffers here between calls)."""
    return _owned.instance(PeakFinder, device)
