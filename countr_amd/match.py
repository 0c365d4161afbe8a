"""Predicted points against annotated dots: a one-to-one matching under one written rule, and the precision / recall built on it.

    match_host            the rule of countr_match_points (include/countr_hip.h) as the sequential greedy pass in numpy, fp32 arithmetic
                          as the kernel's -- the yardstick of the GPU tests, as peaks_host is for the peaks
    match_rounds_host     the same matching as rounds of locally dominant pairs, the form csrc/match.hip computes (and the round count)
    PointMatcher          the same matching from csrc/match.hip on the stream the forward runs on: one packed upload, one call of the
                          export per <= 16 sets, one asynchronous download, one synchronisation
    localization_metrics  TP / precision / recall / F1 / mean matched distance at several distances from ONE matching at the largest
    LocalizationTotals    micro precision / recall / F1 (sums of TP, P, G over images) and the macro mean F1

The rule: d2(i, j) = fl(fl(dx*dx) + fl(dy*dy)) with dx = fl(px_i - gx_j), dy likewise (fp32, nothing contracted).  Pair (i, j) is
eligible iff d2 <= fl(max_dist * max_dist); a point with a non-finite coordinate has no eligible pair.  The eligible pairs are ordered by
the key (d2, i, j), and the matching is the greedy one over that order.  The matching under a smaller max_dist is the subset of this one
whose d2 is within the smaller bound (the prefix property), which is what localization_metrics relies on."""
import ctypes as C

import numpy as np

from . import _lib, _owned

MAX_SETS, MAX_POINTS = _lib.MATCH_MAX_SETS, _lib.MATCH_MAX_POINTS


def _points(a, what):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float32))
    if a.size == 0:
        a = a.reshape(0, 2)
    if a.ndim != 2 or a.shape[1] != 2 or a.shape[0] > MAX_POINTS:
        raise ValueError("%s: points are [N, 2] as (x, y), N <= %d" % (what, MAX_POINTS))
    return a


def _bound(max_dist):
    md = np.float32(max_dist)
    if not (np.isfinite(md) and md > 0):
        raise ValueError("max_dist is finite and > 0")
    return md * md                                                       # one fp32 multiply


def _d2(pred, gt):
    """fp32 [P, G]: numpy's elementwise float32 operations round once each and fuse nothing."""
    with np.errstate(invalid="ignore", over="ignore"):
        dx = pred[:, None, 0] - gt[None, :, 0]
        dy = pred[:, None, 1] - gt[None, :, 1]
        return dx * dx + dy * dy


def match_host(pred, gt, max_dist):
    """pred [P, 2], gt [G, 2] as (x, y), max_dist > 0 -> (match int32 [P]: the gt index or -1, d2 float32 [P]: the pair's d2 or +inf)."""
    pred, gt = _points(pred, "match_host"), _points(gt, "match_host")
    md2 = _bound(max_dist)
    P, G = pred.shape[0], gt.shape[0]
    match, out = np.full(P, -1, np.int32), np.full(P, np.inf, np.float32)
    if P == 0 or G == 0:
        return match, out
    d2 = _d2(pred, gt)
    with np.errstate(invalid="ignore"):
        ii, jj = np.nonzero(d2 <= md2)                                   # in (i, j) order; a NaN fails the comparison
    order = np.argsort(d2[ii, jj], kind="stable")                        # stable: ties keep (i, j) order
    taken, left = np.zeros(G, bool), min(P, G)
    for i, j in zip(ii[order].tolist(), jj[order].tolist()):
        if match[i] < 0 and not taken[j]:
            match[i], out[i], taken[j] = j, d2[i, j], True
            left -= 1
            if left == 0:
                break
    return match, out


def match_rounds_host(pred, gt, max_dist):
    """The matching as the kernel computes it -> (match, d2, rounds): in every round each pair that is the smallest remaining key of
    both its pred and its gt is matched; `rounds` counts the rounds that matched something."""
    pred, gt = _points(pred, "match_rounds_host"), _points(gt, "match_rounds_host")
    md2 = _bound(max_dist)
    P, G = pred.shape[0], gt.shape[0]
    match, out = np.full(P, -1, np.int32), np.full(P, np.inf, np.float32)
    if P == 0 or G == 0:
        return match, out, 0
    d2 = _d2(pred, gt)
    with np.errstate(invalid="ignore"):
        live = d2 <= md2
    rounds = 0
    while live.any():
        key = np.where(live, d2, np.float32(np.inf))
        # argmin takes the first of equal values: the smallest j of a pred's row, the smallest i of a gt's column
        bj, bi = key.argmin(1), key.argmin(0)
        hits = [(i, int(bj[i])) for i in range(P) if live[i, bj[i]] and bi[bj[i]] == i]
        assert hits                                                      # the smallest remaining key is always locally dominant
        for i, j in hits:
            match[i], out[i] = j, d2[i, j]
            live[i, :] = False
            live[:, j] = False
        rounds += 1
    return match, out, rounds


def localization_metrics(match_d2, P, G, dists):
    """match_d2: the matcher's d2 per pred (+inf = unmatched) at a max_dist >= max(dists) -> per distance a dict {dist, tp, precision,
    recall, f1, mean_dist}: tp = |{d2 <= fl(dist * dist)}| (fp32), precision = tp / P, recall = tp / G, f1 their harmonic mean, mean_dist
    the mean of sqrt(d2) over the counted matches; every ratio is 0 when its denominator is 0."""
    d2 = np.asarray(match_d2, dtype=np.float32).reshape(-1)
    rows = []
    for dist in dists:
        hit = d2 <= _bound(dist)
        tp = int(hit.sum())
        prec, rec = (tp / P if P > 0 else 0.0), (tp / G if G > 0 else 0.0)
        rows.append({"dist": float(dist), "tp": tp, "precision": prec, "recall": rec,
                     "f1": 2 * prec * rec / (prec + rec) if prec + rec > 0 else 0.0,
                     "mean_dist": float(np.sqrt(d2[hit].astype(np.float64)).mean()) if tp else 0.0})
    return rows


class LocalizationTotals:
    """Sums over images, one column per label (a distance, or "box" for the per-image box-scaled distance): add(label, row, P, G) with a
    row of localization_metrics; summary() -> {label: {images, tp, pred, gt, precision, recall, f1 (micro: from the sums), macro_f1 (the
    mean of the images' f1)}}."""

    def __init__(self):
        self.cols = {}

    def add(self, label, row, P, G):
        c = self.cols.setdefault(str(label), {"images": 0, "tp": 0, "pred": 0, "gt": 0, "f1_sum": 0.0})
        c["images"] += 1; c["tp"] += int(row["tp"]); c["pred"] += int(P); c["gt"] += int(G); c["f1_sum"] += float(row["f1"])

    def summary(self):
        out = {}
        for label, c in self.cols.items():
            prec, rec = (c["tp"] / c["pred"] if c["pred"] else 0.0), (c["tp"] / c["gt"] if c["gt"] else 0.0)
            out[label] = {"images": c["images"], "tp": c["tp"], "pred": c["pred"], "gt": c["gt"], "precision": prec, "recall": rec,
                          "f1": 2 * prec * rec / (prec + rec) if prec + rec > 0 else 0.0,
                          "macro_f1": c["f1_sum"] / c["images"] if c["images"] else 0.0}
        return out


class PointMatcher:
    """countr_match_points on host point sets.  Owns the workspace, the packed point buffer, the packed result buffer and their pinned
    mirrors; they grow monotonically, so a steady stream of calls allocates nothing but its (host) results."""

    def __init__(self, device="cuda"):
        self.device = _owned.resolve(device, "PointMatcher")
        self.L = _lib.lib()
        self._descs = (_lib.MatchSet * MAX_SETS)()
        self._ws = None             # uint8, one chunk's scratch (the chunks of a call follow each other on one stream)
        self._pts = self._pts_host = None           # float32: every set's pred then gt, as (x, y) pairs
        self._out = self._out_host = None           # int32: match [sum P] | match_d2 [sum P] (float bits) | counts [n]
        self._guard = _owned.Guard(self.device)     # a call on another stream than the previous one waits before it reuses the buffers

    def _reserve(self, ws_bytes, floats, ints):
        import torch
        _owned.grow(self, "_ws", ws_bytes, torch.uint8)
        _owned.grow(self, "_pts", floats, torch.float32, pinned=True)
        _owned.grow(self, "_out", ints, torch.int32, pinned=True)

    def match(self, sets):
        """sets: [(pred [P, 2], gt [G, 2], max_dist), ...] on the host -> [(match int32 [P], d2 float32 [P], matched), ...] as numpy
        arrays, on the current stream."""
        import torch
        n = len(sets)
        if n == 0:
            return []
        sets = [(_points(p, "PointMatcher.match"), _points(g, "PointMatcher.match"), float(md)) for p, g, md in sets]
        for _p, _g, md in sets:
            _bound(md)
        ws_bytes = 0
        for c0 in range(0, n, MAX_SETS):
            part = sets[c0:c0 + MAX_SETS]
            b = self.L.countr_match_workspace(len(part), max(p.shape[0] for p, _g, _m in part), max(g.shape[0] for _p, g, _m in part))
            _lib.check(min(b, 0), "countr_match_workspace")
            ws_bytes = max(ws_bytes, b)
        total_p = sum(p.shape[0] for p, _g, _m in sets)
        floats = max(2 * sum(p.shape[0] + g.shape[0] for p, g, _m in sets), 2)
        ints = 2 * total_p + n
        with torch.cuda.device(self.device):
            self._reserve(ws_bytes, floats, ints)
            cur = self._guard.enter()
            stage = self._pts_host.numpy()
            at, where = 0, []
            for p, g, _m in sets:
                where.append((at, at + p.size))
                stage[at:at + p.size] = p.reshape(-1); at += p.size
                stage[at:at + g.size] = g.reshape(-1); at += g.size
            self._pts[:floats].copy_(self._pts_host[:floats], non_blocking=True)          # the one upload
            base, st = self._pts.data_ptr(), C.c_void_p(cur.cuda_stream)
            out = self._out.data_ptr()
            for c0 in range(0, n, MAX_SETS):
                part = sets[c0:c0 + MAX_SETS]
                off = sum(p.shape[0] for p, _g, _m in sets[:c0])
                for k, (p, g, md) in enumerate(part):
                    d = self._descs[k]
                    d.pred, d.gt = base + 4 * where[c0 + k][0], base + 4 * where[c0 + k][1]
                    d.P, d.G, d.max_dist, d.offset = p.shape[0], g.shape[0], md, off
                    off += p.shape[0]
                _lib.check(self.L.countr_match_points(self._descs, len(part), out, out + 4 * total_p, out + 4 * (2 * total_p + c0),
                                                      self._ws.data_ptr(), st), "countr_match_points")
            self._out_host[:ints].copy_(self._out[:ints], non_blocking=True)              # the one download
            self._guard.leave(cur)
        self._guard.event.synchronize()              # the one wait of the call
        got = self._out_host[:ints].numpy()
        res, off = [], 0
        for s, (p, _g, _m) in enumerate(sets):
            P = p.shape[0]
            res.append((got[off:off + P].copy(), got[total_p + off:total_p + off + P].view(np.float32).copy(), int(got[2 * total_p + s])))
            off += P
        return res


def point_matcher(device):
    """The PointMatcher of a device, made on first use (the evaluation CLI keeps its buffers here between groups)."""
    return _owned.instance(PointMatcher, device)
