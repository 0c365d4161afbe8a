"""Line counts from density flux: how many objects crossed a line, from the density map and a motion field -- no peaks, no tracks.

    luma_host / motion_host / flux_host   the three parts of the rule of include/countr_hip_flow.h in numpy
    flow_host     the rule over a clip -- the yardstick of the GPU tests: luma and motion bytes are the device's, the flux sums are fp64
    FlowCounter   the same from csrc_flow/flow.hip on the stream the forward runs on: per group of frames the launches (luma, motion, flux,
                  fold), one download and one synchronisation; it owns the luma history and every workspace
    FlowCounts    what a clip adds up to: line_counts float64 [L, 2] (forward, backward), frames, counted
    blob_scene    a synthetic clip with a known answer (Gaussian density blobs on textured patches that cross the lines both ways)

The rule in short (the header states it in full).  The luma of a frame is read back from the prepared image the forward already reads
(the resized bytes, 77 / 150 / 29 weights).  Every 8 x 8 cell gets a backward offset against the luma `interval` frames earlier: the
first minimum, in (distance, oy, ox) order, of the 16 x 16 window's SAD over the search square, set to zero unless it beats staying
still by min_gain, refined to 1/16 px by the equiangular fit -- integers only.  A map pixel inside a line's band (half-open, `band`
frame pixels wide, as long as the line) adds M vn / band / 60 to forward or backward, vn being its cell's move per frame along the line's
normal towards the tracker's side 1 -- fp64 decisions, fp32 sums in a fixed order.  Over time the band integrates every object that
passes to its count.

The defaults min_gain = 256 (one grey level per window pixel), band = 8 H / 384 frame pixels and search = 4 are unmeasured: there is
neither a checkpoint nor an annotated clip to tune them on, and no accuracy figure on real video exists.  What exists is the instrument,
pinned on synthetic scenes with known answers.  Motion below about half a map pixel per interval is underestimated: use interval > 1.

All of this assumes a camera that stands still.  camera="translation" (flow_host, FlowCounter) puts the rule of countr_amd/cam.py
between motion and flux: the camera's own move is estimated from the field, the field is compensated for it and every map is placed at
the camera's position, so that lines and flux are in pixels of the first frame.  camera=None is the rule above and nothing else."""
import collections
import ctypes as C

import numpy as np

from . import _lib, _owned
from . import cam as cam_

_K = {k[len("COUNTR_FLOW_"):]: v for k, v in _lib.FLOW_CONSTS.items()}
MAX_FRAMES, MAX_LINES, MAX_SEARCH, MAX_INTERVAL = _K["MAX_FRAMES"], _K["MAX_LINES"], _K["MAX_SEARCH"], _K["MAX_INTERVAL"]
CELL, MAX_SIDE, OUT_FLOATS = _K["CELL"], _K["MAX_SIDE"], _K["OUT_FLOATS"]

FlowCounts = collections.namedtuple("FlowCounts", "line_counts frames counted")


def _lines(lines):
    """Up to 16 finite segments (ax, ay, bx, by): the tracker's lines -- fp32 values, carried in fp64."""
    a = np.ascontiguousarray(np.asarray(lines if lines is not None else (), dtype=np.float32))
    if a.size == 0:
        a = a.reshape(0, 4)
    if a.ndim != 2 or a.shape[1] != 4 or a.shape[0] > MAX_LINES or not np.isfinite(a).all():
        raise ValueError("flow: lines are up to %d finite segments (ax, ay, bx, by)" % MAX_LINES)
    return np.ascontiguousarray(a.astype(np.float64))


def _settings(search, interval, min_gain, band):
    if int(search) != search or not 1 <= search <= MAX_SEARCH:
        raise ValueError("search is 1..%d" % MAX_SEARCH)
    if int(interval) != interval or not 1 <= interval <= MAX_INTERVAL:
        raise ValueError("interval is 1..%d" % MAX_INTERVAL)
    if int(min_gain) != min_gain or not 0 <= min_gain < 2 ** 31:
        raise ValueError("min_gain is an integer >= 0")
    if band is not None and not (np.isfinite(band) and band > 0):
        raise ValueError("band is finite and > 0")
    return int(search), int(interval), int(min_gain), None if band is None else float(band)


def _check_side(h, w):
    if h % CELL or w % CELL or not (CELL <= h <= MAX_SIDE and CELL <= w <= MAX_SIDE):
        raise ValueError("flow: h and w are multiples of %d in %d..%d, got %d x %d" % (CELL, CELL, MAX_SIDE, h, w))


def default_band(H):
    """The default band in frame pixels: 8 map pixels of a 384-row map.  Unmeasured."""
    return 8.0 * H / 384.0


def luma_host(image):
    """A prepared image fp32 [3, h, w] (or [1, 3, h, w]) -> its luma uint8 [h, w], by the header's rule."""
    v = np.asarray(image, np.float32)
    v = v.reshape(v.shape[-3:])
    with np.errstate(invalid="ignore"):
        q = np.clip((v * np.float32(255) + np.float32(0.5)).astype(np.int32), 0, 255)      # fp32 multiply, fp32 add, truncation
    return ((77 * q[0] + 150 * q[1] + 29 * q[2] + 128) >> 8).astype(np.uint8)


def candidates(search):
    """The offsets (oy, ox) of the search square in the rule's order (oy^2 + ox^2, oy, ox)."""
    r = int(search)
    return sorted(((oy, ox) for oy in range(-r, r + 1) for ox in range(-r, r + 1)), key=lambda o: (o[0] * o[0] + o[1] * o[1], o[0], o[1]))


def sad_host(cur, old, search):
    """S(o) of every cell and every offset: uint32 [2 r + 1, 2 r + 1, h / 8, w / 8], indexed [oy + r, ox + r]."""
    cur, old = np.asarray(cur), np.asarray(old)
    if cur.dtype != np.uint8 or old.dtype != np.uint8 or cur.ndim != 2 or cur.shape != old.shape:
        raise ValueError("flow: lumas are uint8 [h, w] of one shape")
    h, w = cur.shape
    _check_side(h, w)
    r, half = int(search), CELL // 2
    Hc, Wc = h // CELL, w // CELL
    # window pixels p run over -4 .. h + 3, p + o over -4 - r .. h + 3 + r: edge padding is the rule's clamp
    a = np.pad(cur.astype(np.int32), half, mode="edge")
    b = np.pad(old.astype(np.int32), half + r, mode="edge")
    S = np.empty((2 * r + 1, 2 * r + 1, Hc, Wc), np.uint32)
    for oy in range(-r, r + 1):
        for ox in range(-r, r + 1):
            d = np.abs(a - b[r + oy:r + oy + h + 2 * half, r + ox:r + ox + w + 2 * half])
            blk = d.reshape(Hc + 1, CELL, Wc + 1, CELL).sum((1, 3))                    # 8 x 8 blocks: a window is four of them
            S[oy + r, ox + r] = blk[:-1, :-1] + blk[1:, :-1] + blk[:-1, 1:] + blk[1:, 1:]
    return S


def _subpel(sm, s0, sp):
    sm, s0, sp = (np.asarray(v, np.int64) for v in (sm, s0, sp))
    den = np.maximum(sm, sp) - s0
    safe = np.where(den > 0, den, 1)
    return np.where(den > 0, np.floor_divide(16 * (sm - sp) + safe, 2 * safe), 0)


def motion_host(cur, old, search=4, min_gain=256):
    """The motion field int16 [h / 8, w / 8, 2] as (x, y) in 1/16 px of the current luma against an earlier one, by the header's rule."""
    r = int(search)
    S = sad_host(cur, old, r).astype(np.int64)
    order = candidates(r)
    stack = np.stack([S[oy + r, ox + r] for oy, ox in order])                          # argmin takes the first minimum
    pick = stack.argmin(0)
    oys, oxs = np.array([o[0] for o in order])[pick], np.array([o[1] for o in order])[pick]
    jj, ii = np.indices(pick.shape)
    s0, sz = S[oys + r, oxs + r, jj, ii], S[r, r]
    rest = ((oys != 0) | (oxs != 0)) & (sz - s0 < int(min_gain))
    inx, iny = np.abs(oxs) < r, np.abs(oys) < r
    xm, xp = np.clip(oxs - 1, -r, r), np.clip(oxs + 1, -r, r)
    ym, yp = np.clip(oys - 1, -r, r), np.clip(oys + 1, -r, r)
    fx = np.where(inx, _subpel(S[oys + r, xm + r, jj, ii], s0, S[oys + r, xp + r, jj, ii]), 0)
    fy = np.where(iny, _subpel(S[ym + r, oxs + r, jj, ii], s0, S[yp + r, oxs + r, jj, ii]), 0)
    mx, my = np.where(rest, 0, 16 * oxs + fx), np.where(rest, 0, 16 * oys + fy)
    return np.stack([mx, my], -1).astype(np.int16)


def flux_host(M, V, placement, lines, band, interval=1, members=False):
    """The flux of map M fp32 [h, w] with motion V int16 [h / 8, w / 8, 2] through the lines -> (flux float64 [L, 2], total float64): the
    header's decisions and fp32 terms, summed in float64.  members=True adds the number of terms int [L, 2], the sum of their absolute
    values float64 [L, 2] and the map's sum of absolute values -- what the a-priori bound of the device's fp32 sums needs."""
    M = np.asarray(M, np.float32)
    h, w = M.shape
    _check_side(h, w)
    V = np.asarray(V, np.int16).reshape(h // CELL, w // CELL, 2)
    lines = _lines(lines)
    sx, tx, sy, ty = (np.float64(v) for v in placement)
    band, step = np.float64(band), np.float64(16 * int(interval))
    Px, Py = sx * np.arange(w, dtype=np.float64) + tx, sy * np.arange(h, dtype=np.float64) + ty
    ox, oy = V[..., 0].astype(np.float64), V[..., 1].astype(np.float64)
    dx, dy = -((sx * ox) / step), -((sy * oy) / step)
    M64 = M.astype(np.float64)
    flux, n, ab = np.zeros((len(lines), 2)), np.zeros((len(lines), 2), np.int64), np.zeros((len(lines), 2))
    for k, (ax, ay, bx, by) in enumerate(lines):
        ex, ey = bx - ax, by - ay
        len2 = ex * ex + ey * ey
        if len2 == 0:
            continue
        ln = np.sqrt(len2)
        hw = (band / 2) * ln
        ux, uy = (Px - ax)[None, :], (Py - ay)[:, None]
        cr, t = ex * uy - ey * ux, ex * ux + ey * uy
        inside = (-hw <= cr) & (cr < hw) & (0 <= t) & (t < len2)
        vn = ((dy * ex) - (dx * ey)) / ln
        g = np.repeat(np.repeat((vn / band) / 60, CELL, 0), CELL, 1)
        with np.errstate(over="ignore", invalid="ignore"):
            fw = (M64 * g).astype(np.float32)[inside & (g > 0)].astype(np.float64)
            bw = (M64 * -g).astype(np.float32)[inside & (g < 0)].astype(np.float64)
        flux[k] = fw.sum(), bw.sum()
        n[k] = fw.size, bw.size
        ab[k] = np.abs(fw).sum(), np.abs(bw).sum()
    if members:
        return flux, M64.sum(), n, ab, np.abs(M64).sum()
    return flux, M64.sum()


def frame_scale(count, total):
    """scale = count / (total / 60): the test-time normalisation, carried exactly as count_regions carries it (1 when total <= 0)."""
    return np.float64(count) / (np.float64(total) / 60) if total > 0 else np.float64(1.0)


def flow_host(lumas, maps, *, lines, placement=(1.0, 0.0, 1.0, 0.0), search=4, interval=1, min_gain=256, band=8.0, counts=None,
              camera=None, min_texture=128, cam_tol=8, min_voters=16, fields=None):
    """The rule over a clip.  lumas: uint8 [h, w] per frame, in time order; maps: fp32 [h, w] per frame, or None for a frame without a
    frame map (the 3 x 3 split); placement: the maps' (sx, tx, sy, ty); counts: the frames' counts, or None for scale 1 -> ([(flux float64
    [L, 2] or None, motion int16 [h / 8, w / 8, 2] or None, total or None), ...], FlowCounts).  The first `interval` frames count nothing
    (flux and motion None); a frame without a map has flux None, and its luma still is the earlier luma of a later frame.
    camera="translation": the rule of countr_amd/cam.py runs between motion and flux -- every frame's field is compensated for the
    camera's estimated move and its map is placed at (sx, tx + sx * Gx / 16, sy, ty + sy * Gy / 16), so lines and flux are in pixels of
    the FIRST frame; the motion returned stays the raw field, and a third result is the CameraPath.  camera=None is the rule above and
    nothing else.  fields: the frames' motion fields if they are at hand (None entries for the first `interval` frames)."""
    search, interval, min_gain, band = _settings(search, interval, min_gain, band)
    min_texture, cam_tol, min_voters = cam_.settings(camera, min_texture, cam_tol, min_voters)
    lines = _lines(lines)
    out, acc, counted = [], np.zeros((len(lines), 2)), 0
    records, path = np.zeros((len(lumas), cam_.RECORD_INTS), np.int32), np.zeros((len(lumas), 2), np.int64)
    for t, (L, M) in enumerate(zip(lumas, maps)):
        if t < interval:
            out.append((None, None, None))
            continue
        V = fields[t] if fields is not None else motion_host(L, lumas[t - interval], search, min_gain)
        moved, placed = V, placement
        if camera is not None:
            records[t], flags = cam_.estimate_host(V, L, min_texture, cam_tol, min_voters)
            path[t] = path[t - interval] + records[t, :2]
            moved, placed = cam_.compensate_host(V, records[t], flags), cam_.shifted_placement(path[t], placement)
        if M is None:
            out.append((None, V, None))
            continue
        flux, total = flux_host(M, moved, placed, lines, band, interval)
        acc += frame_scale(counts[t], total) * flux if counts is not None else flux
        counted += 1
        out.append((flux, V, total))
    if camera is not None:
        return out, FlowCounts(acc, len(out), counted), cam_.CameraPath(path, cam_.lost_frames(records), records)
    return out, FlowCounts(acc, len(out), counted)


def blob_scene(h=96, w=192, objects=5, frames=60, speed=(1.0, 3.0), seed=0, noise=0.0, sigma=2.0, patch=(14, 22), line_x=None):
    """A synthetic clip with a known answer: `objects` objects, one per lane, each a Gaussian density blob (sigma map pixels, mass 60 = one
    object) in the middle of a smooth-textured patch (patch = (height, width), wider than the blob) on a flat background, moving along x
    at a constant speed in `speed` px/frame, to the left or to the right (at least two each way when objects >= 4), so that it is
    centred on the line's neighbourhood half-way through the clip and crosses every line completely.  The texture is a sum of sinusoids
    evaluated at the moving coordinates, so sub-pixel moves are exact.  noise: sigma of Gaussian noise on the luma, in grey levels.
    -> (lumas uint8 [h, w] per frame, maps fp32 [h, w] per frame, lines fp32 [3, 4], truth int [3, 2] as (forward, backward)): a vertical
    line at a fractional x, one at an integer x and a tilted one; the truth is read from every object's first and last centre with the
    tracker's side test."""
    rs = np.random.RandomState(seed)
    lx = w / 2 if line_x is None else line_x
    sign = np.array([1.0, -1.0] * objects)[:objects]
    rs.shuffle(sign)
    v = rs.uniform(speed[0], speed[1], objects) * sign
    yc = (np.arange(objects) + 0.5) * h / objects
    xc = lx + rs.uniform(-3.0, 3.0, objects)
    ph, pw = patch
    waves = [(rs.uniform(2 * np.pi / 16, 2 * np.pi / 6, (4, 2)) * rs.choice([-1.0, 1.0], (4, 2)), rs.uniform(0, 2 * np.pi, 4)) for _ in range(objects)]
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    lumas, maps = [], []
    centre = lambda k, t: (xc[k] + v[k] * (t - (frames - 1) / 2.0), yc[k])
    for t in range(frames):
        img, dm = np.full((h, w), 128.0), np.zeros((h, w))
        for k in range(objects):
            cx, cy = centre(k, t)
            dx, dy = xx - cx, yy - cy
            tex = 128.0 + 22.0 * sum(np.sin(f[0] * dx + f[1] * dy + p) for f, p in zip(*waves[k]))
            mask = np.clip(pw / 2.0 - np.abs(dx) + 0.5, 0, 1) * np.clip(ph / 2.0 - np.abs(dy) + 0.5, 0, 1)
            img = img * (1 - mask) + tex * mask
            dm += 60.0 * np.exp(-(dx * dx + dy * dy) / (2 * sigma * sigma)) / (2 * np.pi * sigma * sigma)
        if noise:
            img = img + rs.normal(0.0, noise, (h, w))
        lumas.append(np.clip(np.floor(img + 0.5), 0, 255).astype(np.uint8))
        maps.append(dm.astype(np.float32))
    lines = np.array([(lx + 0.3, -10.0, lx + 0.3, h + 10.0), (np.floor(lx) - 1, -10.0, np.floor(lx) - 1, h + 10.0),
                      (lx - 12.0, -10.0, lx + 12.0, h + 10.0)], np.float32)
    side = lambda ln, p: ((np.float64(ln[2]) - ln[0]) * (p[1] - np.float64(ln[1])) - (np.float64(ln[3]) - ln[1]) * (p[0] - np.float64(ln[0]))) >= 0
    truth = np.zeros((len(lines), 2), np.int64)
    for j, ln in enumerate(lines):
        for k in range(objects):
            s0, s1 = side(ln, centre(k, 0)), side(ln, centre(k, frames - 1))
            truth[j, 0] += (not s0) and s1
            truth[j, 1] += s0 and (not s1)
    return lumas, maps, lines, truth


def image_of_luma(luma):
    """A prepared image fp32 [1, 3, h, w] whose luma is `luma` exactly: the three planes are luma / 255 (77 + 150 + 29 = 256)."""
    v = np.asarray(luma, np.uint8).astype(np.float32) / np.float32(255)
    return np.ascontiguousarray(np.broadcast_to(v, (1, 3) + v.shape))


class FlowCounter:
    """countr_flow_luma / _motion / _flux on the prepared images and density maps of one camera: it serves ONE frame shape -- the first
    run fixes the original size (W, H) and the map size, a second shape raises.  Owns the luma planes (the history of `interval` frames
    and the 16 of a launch, as one ring), the motion fields, the flux workspace, the packed result buffer and its pinned mirror: all made
    by the first run, so a steady stream allocates nothing but its (host) results.  Lines and placements travel as kernel arguments: a
    run uploads nothing.  Calls follow each other on the current stream; a call on another stream waits for the previous call's event
    first.  The defaults of search, min_gain and band (8 H / 384 frame pixels) are unmeasured.
    camera="translation": a chunk runs luma, motion, the camera estimate (countr_amd/cam.py), a download of its records and a wait,
    the compensation into a second field buffer, and the flux of the compensated fields with every map placed at the camera's position:
    lines and flux are then in pixels of the first frame.  The placement is a host-side kernel argument, so that is TWO waits per chunk
    instead of one.  min_texture, cam_tol and min_voters are the estimate's settings, unmeasured on real video.  camera=None is the
    path above, launch for launch."""

    def __init__(self, device="cuda", *, lines, search=4, interval=1, min_gain=256, band=None, camera=None, min_texture=128, cam_tol=8,
                 min_voters=16):
        self.device = _owned.resolve(device, "FlowCounter")
        self.search, self.interval, self.min_gain, self.band = _settings(search, interval, min_gain, band)
        self.lines = _lines(lines)
        self.camera = camera
        cam_set = cam_.settings(camera, min_texture, cam_tol, min_voters)
        self.L = _lib.flow_lib()
        self._cam = None
        if camera is not None:
            self._cam = cam_.CameraEstimator(self.device, min_texture=cam_set[0], tol=cam_set[1], min_voters=cam_set[2])
        self._path, self._records = [], []          # per frame since the counter was made: G int64 (x, y), record int32 [8]
        self.shape = None           # (W, H, h, w): the original frame and its map
        self.placement = None
        self.frames = self.counted = 0
        self.line_counts = np.zeros((self.lines.shape[0], 2), np.float64)
        self._ring = MAX_FRAMES + self.interval
        self._maps = (_lib.FlowMap * MAX_FRAMES)()
        self._a, self._b, self._c = ((C.c_void_p * MAX_FRAMES)() for _ in range(3))
        self._lines_c = (C.c_double * max(4 * self.lines.shape[0], 1))(*self.lines.reshape(-1))
        import torch
        with torch.cuda.device(self.device):
            self._guard = _owned.Guard(self.device, recorded=True)      # the first call on another stream waits for the constructing one
        self._planes = self._out = self._out_host = self._ws = None

    def counts(self):
        """What the frames so far add up to."""
        return FlowCounts(self.line_counts.copy(), self.frames, self.counted)

    def camera_path(self):
        """The CameraPath of the frames so far (camera="translation" only)."""
        if self._cam is None:
            raise ValueError("FlowCounter.camera_path: the counter was made with camera=None")
        return cam_.CameraPath(np.array(self._path, np.int64).reshape(-1, 2), cam_.lost_frames(self._records),
                               np.array(self._records, np.int32).reshape(-1, cam_.RECORD_INTS))

    def luma(self, back=0):
        """The luma plane uint8 [h, w] (a view of the device ring) of the frame `back` frames before the latest, 0 <= back <= interval."""
        if self._planes is None or not 0 <= back <= min(self.interval, self.frames - 1):
            raise ValueError("FlowCounter.luma: the ring holds the latest frame and the %d before it" % self.interval)
        return self._planes[(self.frames - 1 - back) % self._ring]

    def _fix_shape(self, size, image):
        import torch
        from .frames import map_placement
        W, H = int(size[0]), int(size[1])
        h, w = int(image.shape[-2]), int(image.shape[-1])
        if self.shape is None:
            _check_side(h, w)
            self.shape, self.placement = (W, H, h, w), tuple(float(v) for v in map_placement(W, H, w, h))
            if self.band is None:
                self.band = default_band(H)
            cells = (h // CELL) * (w // CELL)
            self._mv_at = MAX_FRAMES * OUT_FLOATS * 4                              # the motion fields follow the results
            ws = self.L.countr_flow_workspace(MAX_FRAMES, h)
            _lib.flow_check(min(ws, 0), "countr_flow_workspace")
            self._planes = torch.zeros(self._ring, h, w, dtype=torch.uint8, device=self.device)
            self._out = torch.zeros(self._mv_at + MAX_FRAMES * cells * 4, dtype=torch.uint8, device=self.device)
            self._out_host = torch.zeros(self._out.numel(), dtype=torch.uint8).pin_memory()
            self._ws = torch.empty(ws, dtype=torch.uint8, device=self.device)
            if self._cam is not None:
                self._comp = torch.zeros(MAX_FRAMES * cells * 4, dtype=torch.uint8, device=self.device)      # the compensated fields
                self._rec_host = torch.zeros(MAX_FRAMES, cam_.RECORD_INTS, dtype=torch.int32).pin_memory()
        elif self.shape != (W, H, h, w):
            raise ValueError("FlowCounter serves one frame shape: it holds %r, got %r" % (self.shape, (W, H, h, w)))

    def run(self, images, maps, sizes, counts=None, motion=False):
        """images: the prepared images fp32 [1, 3, h, w] on the device (FramePrep.prepare), in time order; maps: each frame's density map
        (fp32 or a 16-bit type, [h, w], on the device) or None for a frame without a frame map; sizes: (W, H) of the original frames;
        counts: the frames' counts (scale = count / (total / 60)), or None for scale 1 -> [(flux float32 [L, 2] or None, motion int16
        [h / 8, w / 8, 2] or None, total or None), ...]: the unscaled device sums; scale * flux adds into line_counts in float64.  The
        motion fields are downloaded only with motion=True.  Per 16 frames: four launches at most, one download, one synchronisation
        (with a camera: the estimate and the compensation on top, two downloads, two synchronisations)."""
        import torch
        n = len(images)
        if len(maps) != n or len(sizes) != n or (counts is not None and len(counts) != n):
            raise ValueError("FlowCounter.run: one map (or None), one size and one count per image")
        res = []
        for c0 in range(0, n, MAX_FRAMES):
            c1 = min(c0 + MAX_FRAMES, n)
            res += self._chunk(images[c0:c1], maps[c0:c1], sizes[c0:c1], counts[c0:c1] if counts is not None else None, motion)
        return res

    def _chunk(self, images, maps, sizes, counts, motion):
        import torch
        n, s, nl = len(images), self.interval, self.lines.shape[0]
        for im, size in zip(images, sizes):
            if not (isinstance(im, torch.Tensor) and im.is_cuda and im.dtype == torch.float32 and im.is_contiguous() and im.dim() in (3, 4)
                    and im.shape[-3] == 3 and im.numel() == 3 * im.shape[-2] * im.shape[-1]):
                raise ValueError("FlowCounter.run: images are contiguous fp32 [1, 3, h, w] device tensors")
            self._fix_shape(size, im)
        _W, _H, h, w = self.shape
        for m in maps:
            if m is not None and not (isinstance(m, torch.Tensor) and m.is_cuda and tuple(m.shape) == (h, w)):
                raise ValueError("FlowCounter.run: a map is a [%d, %d] device tensor or None" % (h, w))
        cells = (h // CELL) * (w // CELL)
        keep = []                                    # (converted maps stay alive until the call is waited for)
        with torch.cuda.device(self.device):
            cur = self._guard.enter()
            st = C.c_void_p(cur.cuda_stream)
            g0 = self.frames                         # the index of the chunk's first frame since the counter was made
            plane = lambda g: self._planes[g % self._ring].data_ptr()
            for k, im in enumerate(images):
                self._a[k], self._b[k] = im.data_ptr(), plane(g0 + k)
            _lib.flow_check(self.L.countr_flow_luma(self._a, self._b, n, h, w, st), "countr_flow_luma")
            # a ring of 16 + interval planes: the n <= 16 planes written here and the planes they are matched against are n + interval
            # consecutive frames, so none of them shares a slot
            moved = [k for k in range(n) if g0 + k >= s]
            out = self._out.data_ptr()
            for q, k in enumerate(moved):
                self._a[q], self._b[q], self._c[q] = plane(g0 + k), plane(g0 + k - s), out + self._mv_at + 4 * cells * k
            if moved:
                _lib.flow_check(self.L.countr_flow_motion(self._a, self._b, self._c, len(moved), h, w, self.search, self.min_gain, st),
                                "countr_flow_motion")
            fields, place = out + self._mv_at, {}
            if self._cam is not None:
                recs = np.zeros((0, cam_.RECORD_INTS), np.int32)
                if moved:
                    raw = [out + self._mv_at + 4 * cells * k for k in moved]
                    self._cam.launch(raw, [plane(g0 + k) for k in moved], h, w, st)
                    self._rec_host[:len(moved)].copy_(self._cam.records[:len(moved)], non_blocking=True)
                    self._guard.event.record(cur)
                    self._guard.event.synchronize()  # the wait the camera adds: the placements below are host-side kernel arguments
                    recs = self._rec_host[:len(moved)].numpy().copy()
                    fields = self._comp.data_ptr()
                    self._cam.compensate(raw, [fields + 4 * cells * k for k in moved], h, w, st)
                first = n - len(moved)               # (the frames that moved are the chunk's tail)
                for k in range(n):
                    rec = recs[k - first] if k >= first else np.zeros(cam_.RECORD_INTS, np.int32)
                    self._path.append(self._path[g0 + k - s] + rec[:2] if k >= first else np.zeros(2, np.int64))
                    self._records.append(rec)
                    place[k] = cam_.shifted_placement(self._path[g0 + k], self.placement)
            flowed = [k for k in moved if maps[k] is not None]
            for q, k in enumerate(flowed):
                m = maps[k]
                if m.dtype != torch.float32 or not m.is_contiguous():
                    m = m.float().contiguous()
                    keep.append(m)
                d = self._maps[q]
                d.map, d.motion, d.out = m.data_ptr(), fields + 4 * cells * k, out + 4 * OUT_FLOATS * k
                d.sx, d.tx, d.sy, d.ty = place.get(k, self.placement)
            if flowed:
                _lib.flow_check(self.L.countr_flow_flux(self._maps, len(flowed), h, w, self._lines_c if nl else None, nl, self.band, s,
                                                        self._ws.data_ptr(), st), "countr_flow_flux")
            nbytes = self._mv_at + (4 * cells * n if motion else 0)
            if flowed or (motion and moved):
                self._out_host[:nbytes].copy_(self._out[:nbytes], non_blocking=True)      # the one download
            self._guard.leave(cur)
        self._guard.event.synchronize()              # the one wait of the call
        got = self._out_host.numpy()
        res = []
        for k in range(n):
            mv = None
            if motion and k in moved:
                mv = got[self._mv_at + 4 * cells * k:self._mv_at + 4 * cells * (k + 1)].view(np.int16).reshape(h // CELL, w // CELL, 2).copy()
            if k in flowed:
                o = got[4 * OUT_FLOATS * k:4 * OUT_FLOATS * (k + 1)].view(np.float32)
                flux, total = o[:2 * nl].reshape(nl, 2).copy(), float(o[OUT_FLOATS - 1])
                scale = frame_scale(counts[k], total) if counts is not None else np.float64(1.0)
                self.line_counts += scale * flux.astype(np.float64)
                self.counted += 1
                res.append((flux, mv, total))
            else:
                res.append((None, mv, None))
        self.frames += n
        return res
