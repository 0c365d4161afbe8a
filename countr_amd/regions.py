"""Regional counts: sums of density maps over polygons and grids -- "how many in this part of the frame", and the cells of GAME.

    regions_host   the rule of countr_region_sums (include/countr_hip_ext.h) restated in numpy: membership in float64 with separate
                   multiply and add ufuncs, sums in float64 -- the yardstick of the GPU tests, as peaks_host and match_host are
    RegionSummer   the same sums from csrc_ext/regions.hip on the stream the forward runs on: one packed upload, two launches per
                   <= 16 maps, one asynchronous download and one synchronisation per call
    game_grid      the 2^L x 2^L grid of GAME(L) over an h x w image;  game_levels: GAME(0..L) read off the level-L cells

The rule.  Coordinates are pixel-centre coordinates of the original frame (frames.frame_points).  Map pixel (cy, cx) has its centre at
x = ax * cx + bx, y = ay * cy + by (one multiply, one add, fp64).  A centre is inside a polygon iff the number of edges (x0, y0) ->
(x1, y1), the closing edge included, with (y0 <= y) != (y1 <= y) and x < x0 + (y - y0) * (x1 - x0) / (y1 - y0) is odd; it belongs to
cell (i, j) of a grid iff ys[i] <= y < ys[i + 1] and xs[j] <= x < xs[j + 1].  A region is an [nv, 2] array of (x, y) vertices or
("grid", ys, xs); a grid owns gy * gx result slots, row-major.  Per slot: mass = the sum of the member pixels' values over the set's
maps, area = their number; per set: total = the sum of all pixels of its maps."""
import ctypes as C

import numpy as np

from . import _lib, _owned

MAX_MAPS, MAX_POLYGONS = _lib.EXT_CONSTS["COUNTR_REGIONS_MAX_MAPS"], _lib.EXT_CONSTS["COUNTR_REGIONS_MAX_REGIONS"]
MAX_VERTICES, MAX_CELLS = _lib.EXT_CONSTS["COUNTR_REGIONS_MAX_VERTICES"], _lib.EXT_CONSTS["COUNTR_REGIONS_MAX_CELLS"]
MAX_GRIDS = MAX_MAPS                     # grids of one call


def region(r):
    """A region as the kernel takes it: ("grid", ys float64 [gy + 1], xs float64 [gx + 1]) or a float64 [nv, 2] array of (x, y).  Only the
    form is checked here; the export refuses what breaks its limits (nv < 3, boundaries that do not increase, ...)."""
    if isinstance(r, (tuple, list)) and len(r) == 3 and isinstance(r[0], str):
        if r[0] != "grid":
            raise ValueError('regions: a region is [(x, y), ...] or ("grid", ys, xs)')
        ys, xs = np.ascontiguousarray(r[1], np.float64).reshape(-1), np.ascontiguousarray(r[2], np.float64).reshape(-1)
        if ys.size < 2 or xs.size < 2:
            raise ValueError("regions: a grid has at least two boundaries each way")
        return ("grid", ys, xs)
    v = np.ascontiguousarray(r, np.float64)
    if v.ndim != 2 or v.shape[1] != 2:
        raise ValueError('regions: a region is [(x, y), ...] or ("grid", ys, xs)')
    return v


def slots(r):
    """Result slots of a region(): 1 for a polygon, gy * gx for a grid."""
    return (r[1].size - 1) * (r[2].size - 1) if isinstance(r, tuple) else 1


def game_grid(h, w, L):
    """GAME(L)'s grid over an h x w image: ("grid", ys, xs) with ys[i] = i * h / 2^L - 0.5 and xs[j] = j * w / 2^L - 0.5.  Where 2^L
    divides h and w the boundaries are half-integers and never tie with a centre; a boundary that does fall on a centre puts it into the
    upper cell (the half-open rule)."""
    n = 1 << int(L)
    k = np.arange(n + 1, dtype=np.float64)
    return ("grid", k * h / n - 0.5, k * w / n - 0.5)


def frame_grid(W, H, gy, gx):
    """The uniform gy x gx grid over a W x H frame, which covers [-0.5, W - 0.5) x [-0.5, H - 0.5)."""
    return ("grid", np.arange(gy + 1, dtype=np.float64) * H / gy - 0.5, np.arange(gx + 1, dtype=np.float64) * W / gx - 0.5)


def inside_polygon(x, y, verts):
    """x [n], y [m] float64 centres, verts float64 [nv, 2] -> bool [m, n] by the crossing rule, every operation a ufunc of its own."""
    odd = np.zeros((y.size, x.size), bool)
    nv = verts.shape[0]
    for k in range(nv):
        x0, y0 = verts[k - 1]
        x1, y1 = verts[k]
        rows = np.flatnonzero((y0 <= y) != (y1 <= y))
        if rows.size == 0:
            continue
        t = np.add(x0, np.divide(np.multiply(np.subtract(y[rows], y0), np.subtract(x1, x0)), np.subtract(y1, y0)))
        odd[rows] ^= x[None, :] < t[:, None]
    return odd


def grid_cells(x, y, ys, xs):
    """x [n], y [m] centres -> (i [m], j [n]): the grid row / column each belongs to, -1 outside (ys[i] <= y < ys[i + 1])."""
    i = np.searchsorted(ys, y, side="right") - 1
    j = np.searchsorted(xs, x, side="right") - 1
    return np.where((i >= 0) & (i < ys.size - 1), i, -1), np.where((j >= 0) & (j < xs.size - 1), j, -1)


def centres(shape, placement):
    """(x [w], y [h]) float64 of a map's pixel centres: one multiply and one add each."""
    ax, bx, ay, by = (np.float64(v) for v in placement)
    h, w = shape
    return (np.add(np.multiply(ax, np.arange(w, dtype=np.float64)), bx), np.add(np.multiply(ay, np.arange(h, dtype=np.float64)), by))


def _set_of_map(n, nsets, set_of_map):
    if set_of_map is None:
        if nsets not in (1, n):
            raise ValueError("regions: without set_of_map there is one set, or one per map")
        set_of_map = [0] * n if nsets == 1 else list(range(n))
    set_of_map = [int(s) for s in set_of_map]
    if len(set_of_map) != n or any(not 0 <= s < nsets for s in set_of_map):
        raise ValueError("regions: set_of_map names a set per map")
    return set_of_map


def regions_host(maps, placements, sets, set_of_map=None, members=False):
    """maps [h, w] each, placements (ax, bx, ay, by) each, sets [[region, ...], ...] -> per set (mass float64 [slots], area int64 [slots],
    total float64); with members=True also abs = the sum of |v| over each slot's members and over the set (the tests' error bound).
    set_of_map: the set of each map (default: one set for all maps, or set i = map i when there is a set per map)."""
    sets = [[region(r) for r in rs] for rs in sets]
    som = _set_of_map(len(maps), len(sets), set_of_map)
    out = []
    for s, rs in enumerate(sets):
        n = sum(slots(r) for r in rs)
        mass, area, absm = np.zeros(n), np.zeros(n, np.int64), np.zeros(n)
        total = tabs = 0.0
        for mp, pl, sm in zip(maps, placements, som):
            if sm != s:
                continue
            d = np.asarray(mp, dtype=np.float32).astype(np.float64)
            x, y = centres(d.shape, pl)
            total += d.sum(); tabs += np.abs(d).sum()
            at = 0
            for r in rs:
                if isinstance(r, tuple):
                    i, j = grid_cells(x, y, r[1], r[2])
                    gx = r[2].size - 1
                    ok = (i >= 0)[:, None] & (j >= 0)[None, :]
                    cell = (i[:, None] * gx + j[None, :])[ok]
                    k = slots(r)
                    mass[at:at + k] += np.bincount(cell, weights=d[ok], minlength=k)
                    absm[at:at + k] += np.bincount(cell, weights=np.abs(d[ok]), minlength=k)
                    area[at:at + k] += np.bincount(cell, minlength=k)
                    at += k
                else:
                    ok = inside_polygon(x, y, r)
                    mass[at] += d[ok].sum(); absm[at] += np.abs(d[ok]).sum(); area[at] += int(ok.sum())
                    at += 1
        out.append((mass, area, total, absm, tabs) if members else (mass, area, total))
    return out


def point_regions(points, regions):
    """points [P, 2] as (x, y) -> int32 [P]: the first result slot of `regions` that contains each point by the rule above, -1 = none."""
    pts = np.asarray(points, np.float64).reshape(-1, 2)
    out = np.full(len(pts), -1, np.int32)
    at = 0
    for r in (region(r) for r in regions):
        for p in np.flatnonzero(out < 0):
            x, y = pts[p, 0:1], pts[p, 1:2]
            if isinstance(r, tuple):
                i, j = grid_cells(x, y, r[1], r[2])
                if i[0] >= 0 and j[0] >= 0:
                    out[p] = at + i[0] * (r[2].size - 1) + j[0]
            elif inside_polygon(x, y, r)[0, 0]:
                out[p] = at
        at += slots(r)
    return out


def grid_dot_counts(points, grid):
    """Dots [G, 2] as (x, y) per cell of a ("grid", ys, xs), by the grid's own half-open rule: int64 [gy, gx]."""
    _g, ys, xs = region(grid)
    pts = np.asarray(points, np.float64).reshape(-1, 2)
    out = np.zeros((ys.size - 1, xs.size - 1), np.int64)
    i, _ = grid_cells(np.zeros(0), pts[:, 1], ys, xs)
    _, j = grid_cells(pts[:, 0], np.zeros(0), ys, xs)
    ok = (i >= 0) & (j >= 0)
    np.add.at(out, (i[ok], j[ok]), 1)
    return out


def game_levels(pred_cells, dot_cells):
    """GAME(0..L) of one image from its level-L cells: pred_cells, dot_cells [2^L, 2^L] -> [GAME(0), ..., GAME(L)].  A cell of level
    l < L is the sum of its level-L cells, added up in float64 on the host (exact in the dot counts)."""
    diff = np.asarray(pred_cells, np.float64) - np.asarray(dot_cells, np.float64)
    n = diff.shape[0]
    L = n.bit_length() - 1
    if diff.shape != (n, n) or n != 1 << L:
        raise ValueError("game_levels: the cells are [2^L, 2^L]")
    return [float(np.abs(diff.reshape(1 << l, n >> l, 1 << l, n >> l).sum(axis=(1, 3))).sum()) for l in range(L + 1)]


class RegionSummer:
    """countr_region_sums on device maps.  Owns the workspace, the packed upload (pinned + device) and the result buffers (device +
    pinned); they grow monotonically, so a steady stream of calls allocates nothing but its (host) results."""

    def __init__(self, device="cuda"):
        self.device = _owned.resolve(device, "RegionSummer")
        self.L = _lib.ext_lib()
        self._maps = (_lib.RegionMap * MAX_MAPS)()
        self._regs = (_lib.Region * (MAX_POLYGONS + MAX_GRIDS))()
        self._ws = None             # uint8, one chunk's scratch (the chunks of a call follow each other on one stream)
        self._data = self._data_host = None         # float64: per chunk its maps' placements, then its regions' coordinates
        self._out = self._out_host = None           # int32: mass [slots] (float bits) | area [slots] | total [jobs] (float bits)
        self._guard = _owned.Guard(self.device)     # a call on another stream than the previous one waits before it reuses the buffers

    def _reserve(self, ws_bytes, doubles, ints):
        import torch
        _owned.grow(self, "_ws", ws_bytes, torch.uint8)
        _owned.grow(self, "_data", doubles, torch.float64, pinned=True)
        _owned.grow(self, "_out", ints, torch.int32, pinned=True)

    def _describe(self, maps, cm, cr, base):
        """The host descriptors of one chunk (indices into data are relative to the chunk's part of the upload)."""
        for j, (i, k, at) in enumerate(cm):
            d = self._maps[j]
            d.map, d.h, d.w, d.set, d.place = maps[i].data_ptr(), maps[i].shape[0], maps[i].shape[1], k, at - base
        for j, (k, r, at) in enumerate(cr):
            d = self._regs[j]
            d.set, d.data = k, at - base
            d.nv, d.gy, d.gx = (0, r[1].size - 1, r[2].size - 1) if isinstance(r, tuple) else (r.shape[0], 0, 0)

    @staticmethod
    def _chunks(sets, maps_of):
        """jobs (set, first region, end region): a set's regions in pieces of <= 64 polygons and <= 16 grids; chunks: lists of jobs
        with <= 16 maps, <= 16 jobs, <= 64 polygons and <= 16 grids together.  A set's maps stay in one chunk."""
        jobs = []
        for s, rs in enumerate(sets):
            if len(maps_of[s]) > MAX_MAPS:
                raise ValueError("RegionSummer.sum: set %d spans %d maps, a call takes %d" % (s, len(maps_of[s]), MAX_MAPS))
            r0 = polys = grids = 0
            for k, r in enumerate(rs):
                g = isinstance(r, tuple)
                if (polys + (not g) > MAX_POLYGONS) or (grids + g > MAX_GRIDS):
                    jobs.append((s, r0, k))
                    r0, polys, grids = k, 0, 0
                polys += not g; grids += g
            jobs.append((s, r0, len(rs)))
        chunks, cur, nm, polys, grids = [], [], 0, 0, 0
        for job in jobs:
            s, r0, r1 = job
            p = sum(1 for r in sets[s][r0:r1] if not isinstance(r, tuple))
            g = (r1 - r0) - p
            if cur and (nm + len(maps_of[s]) > MAX_MAPS or len(cur) == MAX_MAPS or polys + p > MAX_POLYGONS or grids + g > MAX_GRIDS):
                chunks.append(cur)
                cur, nm, polys, grids = [], 0, 0, 0
            cur.append(job)
            nm += len(maps_of[s]); polys += p; grids += g
        if cur:
            chunks.append(cur)
        return chunks

    def sum(self, maps, placements, set_of_map, sets):
        """maps: contiguous fp32 [h, w] device tensors, placements: (ax, bx, ay, by) per map, set_of_map: the set each map adds to, sets:
        [[region, ...], ...] -> per set (mass float32 [slots], area int32 [slots], total float32) as numpy, on the current stream."""
        import torch
        sets = [[region(r) for r in rs] for rs in sets]
        if not sets:
            return []
        som = _set_of_map(len(maps), len(sets), set_of_map)
        if len(placements) != len(maps):
            raise ValueError("RegionSummer.sum: a placement per map")
        for m in maps:
            if not (isinstance(m, torch.Tensor) and m.is_cuda and m.device == self.device and m.dtype == torch.float32 and m.dim() == 2
                    and m.numel() > 0 and m.is_contiguous()):
                raise ValueError("RegionSummer.sum: maps are contiguous fp32 [h, w] tensors on %s" % self.device)
        maps_of = [[i for i, s in enumerate(som) if s == k] for k in range(len(sets))]
        chunks = self._chunks(sets, maps_of)
        # the layout of the packed upload and of the results
        plan, doubles, nslots = [], 0, 0
        for chunk in chunks:
            cm, cr, base = [], [], doubles                   # (map, set of the call, place), (set of the call, region, data)
            for k, (s, r0, r1) in enumerate(chunk):
                for i in maps_of[s]:
                    cm.append((i, k, doubles)); doubles += 4
                for r in sets[s][r0:r1]:
                    cr.append((k, r, doubles))
                    doubles += (r[1].size + r[2].size) if isinstance(r, tuple) else r.size
            plan.append((chunk, cm, cr, base, doubles, nslots))
            nslots += sum(slots(r) for _k, r, _d in cr)
        njobs = sum(len(c) for c in chunks)
        doubles = max(doubles, 4)
        ints = 2 * nslots + njobs
        with torch.cuda.device(self.device):
            self._reserve(1, doubles, ints)
            stage = self._data_host.numpy()
            for chunk, cm, cr, base, end, _s0 in plan:
                for i, _k, at in cm:
                    stage[at:at + 4] = np.asarray(placements[i], np.float64).reshape(4)
                for _k, r, at in cr:
                    flat = np.concatenate([r[1], r[2]]) if isinstance(r, tuple) else r.reshape(-1)
                    stage[at:at + flat.size] = flat
            ws_bytes = 16
            for chunk, cm, cr, base, _end, _s0 in plan:
                if cm:                                       # (a chunk of sets without maps launches nothing: zeros)
                    self._describe(maps, cm, cr, base)
                    b = self.L.countr_regions_workspace(self._maps, len(cm), self._regs, len(cr), len(chunk))
                    _lib.ext_check(min(b, 0), "countr_regions_workspace")
                    ws_bytes = max(ws_bytes, b)
            self._reserve(ws_bytes, doubles, ints)
            cur = self._guard.enter()
            self._data[:doubles].copy_(self._data_host[:doubles], non_blocking=True)      # the one upload
            st = C.c_void_p(cur.cuda_stream)
            out, job0 = self._out.data_ptr(), 0
            for chunk, cm, cr, base, end, s0 in plan:
                if cm:
                    self._describe(maps, cm, cr, base)
                    _lib.ext_check(self.L.countr_region_sums(
                        self._maps, len(cm), self._regs, len(cr), len(chunk), self._data_host.data_ptr() + 8 * base,
                        self._data.data_ptr() + 8 * base, max(end - base, 4), out + 4 * s0, out + 4 * (nslots + s0),
                        out + 4 * (2 * nslots + job0), self._ws.data_ptr(), st), "countr_region_sums")
                else:
                    k = sum(slots(r) for _k, r, _d in cr)
                    self._out[s0:s0 + k].zero_(); self._out[nslots + s0:nslots + s0 + k].zero_()
                    self._out[2 * nslots + job0:2 * nslots + job0 + len(chunk)].zero_()
                job0 += len(chunk)
            self._out_host[:ints].copy_(self._out[:ints], non_blocking=True)              # the one download
            self._guard.leave(cur)
        self._guard.event.synchronize()              # the one wait of the call
        got = self._out_host[:ints].numpy()
        res = [[[], [], None] for _ in sets]
        at, job = 0, 0
        for chunk, _cm, cr, _b, _e, _s0 in plan:
            for k, (s, r0, r1) in enumerate(chunk):
                n = sum(slots(r) for kk, r, _d in cr if kk == k)
                res[s][0].append(got[at:at + n].view(np.float32).copy())
                res[s][1].append(got[nslots + at:nslots + at + n].copy())
                res[s][2] = np.float32(got[2 * nslots + job:2 * nslots + job + 1].view(np.float32)[0])
                at += n; job += 1
        return [(np.concatenate(m), np.concatenate(a), t) for m, a, t in res]


def region_summer(device):
    """The RegionSummer of a device, made on first use (count_regions and the evaluation CLI keep its buffers here between calls)."""
    return _owned.instance(RegionSummer, device)
