"""Annotated frames on the device: the density map as a colour overlay on the frame's own pixels at the frame's own size, a label, region
outlines and points, as packed RGB [H, W, 3] or as the NV12 / NV21 / I420 buffer a video encoder takes (csrc_overlay/overlay.hip:
countr_overlay_render), on the stream the forward runs on.

include/countr_hip_overlay.h states the rule; overlay_host restates it in numpy.  Everything behind the heat's one fp32 multiply and one
fp32 add is integer arithmetic, so the device bytes equal overlay_host's.  The 4:2:0 buffer has the layout YuvFrame.from_buffer reads.
There is no host fallback."""
import ctypes as C

import numpy as np

from . import _lib, _owned

K = {k[len("COUNTR_OVERLAY_"):]: v for k, v in _lib.OVERLAY_CONSTS.items()}
OUTPUTS = {"rgb": K["RGB"], "nv12": K["NV12"], "nv21": K["NV21"], "i420": K["I420"]}
MATRICES = {"bt601": K["BT601"], "bt709": K["BT709"]}
RANGES = {"limited": K["LIMITED"], "full": K["FULL"]}
MAX_FRAMES, MAX_SIDE, MAX_POINTS, MAX_POLYGONS, MAX_VERTICES, MAX_RADIUS = (K[n] for n in (
    "MAX_FRAMES", "MAX_SIDE", "MAX_POINTS", "MAX_POLYGONS", "MAX_VERTICES", "MAX_RADIUS"))
PATCH_H, PATCH_W = K["PATCH_H"], K["PATCH_W"]
COORD = 1 << 20                # a mark's rounded coordinates lie in -COORD .. COORD
# (matrix, range) -> yr, yg, yb, yoff, ur, ug, ub, vr, vg, vb: a red or blue coefficient is floor(256 x the exact one + 0.5), green takes
# what is left of the row's total (256 full-range luma, 220 limited-range luma, 0 chroma)
COEFFICIENTS = {("bt601", "full"): (77, 150, 29, 0, -43, -85, 128, 128, -107, -21),
                ("bt601", "limited"): (66, 129, 25, 16, -38, -74, 112, 112, -94, -18),
                ("bt709", "full"): (54, 184, 18, 0, -29, -99, 128, 128, -116, -12),
                ("bt709", "limited"): (47, 157, 16, 16, -26, -86, 112, 112, -102, -10)}
POINT_COLOR, REGION_COLOR = (0, 255, 0), (255, 255, 0)


def colormap_table(colormap):
    """"red", "heat" or a caller's own [256, 4] array of (r, g, b, a) -> uint8 [256, 4]."""
    if isinstance(colormap, str):
        q = np.arange(256)
        if colormap == "red":
            cols = (np.full(256, 255), np.zeros(256), np.zeros(256), q)
        elif colormap == "heat":
            cols = (np.minimum(255, 3 * q), np.clip(3 * q - 255, 0, 255), np.clip(3 * q - 510, 0, 255), np.minimum(255, 2 * q))
        else:
            raise ValueError('colormap is "red", "heat" or a uint8 [256, 4] array, got %r' % colormap)
        return np.stack(cols, 1).astype(np.uint8)
    lut = np.asarray(colormap)
    if lut.shape != (256, 4) or lut.dtype != np.uint8:
        raise ValueError("colormap: a uint8 [256, 4] array of (r, g, b, a), got %s %s" % (lut.dtype, lut.shape))
    return np.ascontiguousarray(lut)


def div255(v):
    """(v * 0x8081) >> 23: v // 255 for 0 <= v < 65536, the form the kernel uses."""
    return (np.asarray(v, np.int64) * 0x8081) >> 23


def gain_host(m, gain):
    """The fp32 gain of a map: `gain` itself, or under "max" 255.0f / the largest value above 0 (0 where there is none)."""
    if isinstance(gain, str):
        if gain != "max":
            raise ValueError('gain is a number or "max", got %r' % gain)
        m = np.asarray(m, np.float32)
        pos = m[m > 0]
        return np.float32(255.0) / pos.max() if pos.size else np.float32(0.0)
    return np.float32(gain)


def heat_host(m, gain):
    """Step 1: fp32 map, fp32 gain -> int32 levels 0 .. 255."""
    with np.errstate(all="ignore"):
        t = np.asarray(m, np.float32) * np.float32(gain) + np.float32(0.5)           # float32 arrays: two roundings, no fma
        return np.where(t >= 0, np.where(t >= 255, 255, np.floor(np.where(t >= 0, np.minimum(t, 255), 0))), 0).astype(np.int32)


def axis_host(size, msize):
    """Step 2's (i0, i1, fraction) of every output coordinate of a side `size` over a map side `msize`."""
    n = (2 * np.arange(size, dtype=np.int64) + 1) * msize - size
    i = np.where(n < 0, 0, n // (2 * size))
    fr = np.where(n < 0, 0, ((n % (2 * size)) * 256) // (2 * size))
    return np.minimum(i, msize - 1), np.minimum(i + 1, msize - 1), fr


def upsample_host(q, H, W):
    """Step 2: levels [mh, mw] -> int64 [H, W]."""
    q = np.asarray(q, np.int64)
    iy0, iy1, fy = axis_host(H, q.shape[0])
    ix0, ix1, fx = axis_host(W, q.shape[1])
    fy, fx = fy[:, None], fx[None, :]
    top = q[iy0][:, ix0] * (256 - fx) + q[iy0][:, ix1] * fx
    bot = q[iy1][:, ix0] * (256 - fx) + q[iy1][:, ix1] * fx
    return (top * (256 - fy) + bot * fy + 32768) >> 16


def blend_host(frame, h, lut):
    """Step 3: uint8 [H, W, 3], levels [H, W], lut [256, 4] -> uint8 [H, W, 3]."""
    c = lut[h].astype(np.int64)
    a = c[..., 3:4]
    return div255(frame.astype(np.int64) * (255 - a) + c[..., :3] * a + 127).astype(np.uint8)


def round_coords(v, what="coordinates"):
    """Float (x, y) rows -> int64 [N, 2] as floor(v + 0.5); the rounded values lie in -2^20 .. 2^20."""
    v = np.asarray(v, np.float64).reshape(-1, 2)
    if not np.isfinite(v).all():
        raise ValueError("overlay: %s must be finite" % what)
    r = np.floor(v + 0.5)
    if r.size and np.abs(r).max() > COORD:
        raise ValueError("overlay: %s lie in -%d .. %d after rounding" % (what, COORD, COORD))
    return r.astype(np.int64)


def polygon_edges(regions):
    """Polygons ([V, 2] of (x, y) each) -> (vertex counts, int64 [E, 4] of (x0, y0, x1, y1)): a polygon of V vertices has the V edges
    (v[k], v[(k + 1) % V])."""
    counts, edges = [], []
    for poly in regions:
        v = round_coords(poly, "region vertices")
        if not 1 <= len(v) <= MAX_VERTICES:
            raise ValueError("overlay: a polygon has 1..%d vertices, got %d" % (MAX_VERTICES, len(v)))
        counts.append(len(v))
        edges.append(np.concatenate([v, np.roll(v, -1, 0)], 1))
    if len(counts) > MAX_POLYGONS:
        raise ValueError("overlay: at most %d polygons a frame, got %d" % (MAX_POLYGONS, len(counts)))
    return counts, (np.concatenate(edges) if edges else np.zeros((0, 4), np.int64))


def draw_label_host(rgb, patch, lx, ly):
    H, W, _ = rgb.shape
    lh, lw = patch.shape
    y0, y1, x0, x1 = max(ly, 0), min(ly + lh, H), max(lx, 0), min(lx + lw, W)
    if y0 < y1 and x0 < x1:
        m = patch[y0 - ly:y1 - ly, x0 - lx:x1 - lx].astype(np.int64)[..., None]
        rgb[y0:y1, x0:x1] = div255(rgb[y0:y1, x0:x1].astype(np.int64) * (255 - m) + 255 * m + 127).astype(np.uint8)


def draw_edges_host(rgb, edges, color):
    H, W, _ = rgb.shape
    for x0, y0, x1, y1 in np.asarray(edges, np.int64):
        dx, dy = x1 - x0, y1 - y0
        n = max(abs(dx), abs(dy))
        i = np.arange(n + 1, dtype=np.int64)
        x = x0 + ((2 * i * dx + n) // (2 * n) if n else 0 * i)
        y = y0 + ((2 * i * dy + n) // (2 * n) if n else 0 * i)
        ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        rgb[y[ok], x[ok]] = color


def draw_points_host(rgb, centres, radius, color):
    H, W, _ = rgb.shape
    d = np.arange(-radius, radius + 1)
    dy, dx = np.meshgrid(d, d, indexing="ij")
    disc = dx * dx + dy * dy <= radius * radius
    dx, dy = dx[disc], dy[disc]
    c = np.asarray(centres, np.int64).reshape(-1, 2)
    x, y = (c[:, 0:1] + dx[None, :]).ravel(), (c[:, 1:2] + dy[None, :]).ravel()
    ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)
    rgb[y[ok], x[ok]] = color


def frame_bytes(out, width, height):
    """Bytes of one returned frame: H W 3 for rgb, the Y plane and the chroma plane(s) otherwise."""
    if out == "rgb":
        return width * height * 3
    return width * height + 2 * ((width + 1) // 2) * ((height + 1) // 2)


def rgb_to_yuv_host(rgb, out="nv12", matrix="bt709", range="limited"):
    """Step 5: uint8 [H, W, 3] -> the packed 4:2:0 buffer, uint8 [H W + 2 Hc Wc]."""
    yr, yg, yb, yoff, ur, ug, ub, vr, vg, vb = COEFFICIENTS[(matrix, range)]
    H, W, _ = rgb.shape
    p = rgb.astype(np.int32)
    Y = ((yr * p[..., 0] + yg * p[..., 1] + yb * p[..., 2] + 128) >> 8) + yoff
    hc, wc = (H + 1) // 2, (W + 1) // 2
    rows = p[0::2] + p[np.minimum(2 * np.arange(hc) + 1, H - 1)]                        # coordinates clamped to the frame
    s = (rows[:, 0::2] + rows[:, np.minimum(2 * np.arange(wc) + 1, W - 1)] + 2) >> 2     # [Hc, Wc, 3]
    U = np.clip(((ur * s[..., 0] + ug * s[..., 1] + ub * s[..., 2] + 128) >> 8) + 128, 0, 255)
    V = np.clip(((vr * s[..., 0] + vg * s[..., 1] + vb * s[..., 2] + 128) >> 8) + 128, 0, 255)
    if out == "i420":
        c = [U.ravel(), V.ravel()]
    elif out in ("nv12", "nv21"):
        c = [np.stack((U, V) if out == "nv12" else (V, U), -1).ravel()]
    else:
        raise ValueError("overlay: a 4:2:0 output is nv12, nv21 or i420, got %r" % out)
    return np.concatenate([Y.ravel()] + c).astype(np.uint8)


def _check_names(out, matrix, range):
    for value, table, what in ((out, OUTPUTS, "out"), (matrix, MATRICES, "matrix"), (range, RANGES, "range")):
        if value not in table:
            raise ValueError("overlay: %s is one of %s, got %r" % (what, ", ".join(table), value))


def _check_label(label):
    patch, lx, ly = label
    patch = np.ascontiguousarray(patch)
    if patch.dtype != np.uint8 or patch.ndim != 2 or not (1 <= patch.shape[0] <= PATCH_H and 1 <= patch.shape[1] <= PATCH_W):
        raise ValueError("overlay: a label patch is uint8 [lh, lw] of at most %d x %d, got %s %s" % (PATCH_H, PATCH_W, patch.dtype, patch.shape))
    lx, ly = int(lx), int(ly)
    if max(abs(lx), abs(ly)) > COORD:
        raise ValueError("overlay: the label's position lies in -%d .. %d" % (COORD, COORD))
    return patch, lx, ly


def _check_points(points, radius):
    if not 0 <= int(radius) <= MAX_RADIUS:
        raise ValueError("overlay: point_radius is 0..%d, got %r" % (MAX_RADIUS, radius))
    c = round_coords(points, "points")
    if len(c) > MAX_POINTS:
        raise ValueError("overlay: at most %d points a frame, got %d" % (MAX_POINTS, len(c)))
    return c


def overlay_host(frame, density, *, gain=127.5, colormap="red", points=None, point_radius=2, regions=None, label=None, out="rgb",
                 matrix="bt709", range="limited", point_color=POINT_COLOR, region_color=REGION_COLOR):
    """The rule in numpy.  frame uint8 [H, W, 3]; density fp32 [mh, mw], or None for a frame drawn without heat; gain a number or "max";
    points [P, 2] of (x, y); regions a list of polygons, [V, 2] of (x, y) each; label (coverage patch uint8 [lh, lw], lx, ly).
    -> uint8 [H, W, 3], or for out = nv12 / nv21 / i420 the packed buffer."""
    _check_names(out, matrix, range)
    frame = np.asarray(frame)
    if frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3:
        raise ValueError("overlay_host: the frame is uint8 [H, W, 3], got %s %s" % (frame.dtype, frame.shape))
    H, W, _ = frame.shape
    if density is None:
        rgb = frame.copy()
    else:
        m = np.asarray(density, np.float32)
        rgb = blend_host(frame, upsample_host(heat_host(m, gain_host(m, gain)), H, W), colormap_table(colormap))
    if label is not None:
        draw_label_host(rgb, *_check_label(label))
    if regions is not None and len(regions):
        draw_edges_host(rgb, polygon_edges(regions)[1], region_color)
    if points is not None and len(points):
        draw_points_host(rgb, _check_points(points, point_radius), int(point_radius), point_color)
    return rgb if out == "rgb" else rgb_to_yuv_host(rgb, out, matrix, range)


_FONT = None


def label_patch(text):
    """`text` rasterised with PIL's default font as a coverage patch uint8 [lh, lw] (the demos' ImageDraw.text), cropped to
    64 x 256 at the most."""
    from PIL import Image, ImageDraw, ImageFont
    global _FONT
    if _FONT is None:
        _FONT = ImageFont.load_default()          # what ImageDraw.text loads on every call when no font is given
    im = Image.new("L", (PATCH_W, PATCH_H), 0)
    ImageDraw.Draw(im).text((0, 0), text, 255, font=_FONT)
    a = np.asarray(im, dtype=np.uint8)
    ys, xs = np.nonzero(a)
    if len(ys) == 0:
        return np.zeros((1, 1), np.uint8)
    return np.ascontiguousarray(a[:ys.max() + 1, :xs.max() + 1])


def count_label(count, W, H):
    """The demos' label of a frame: "%.3f" % count at (W - 70, H - 50)."""
    return label_patch("%.3f" % count), W - 70, H - 50


def _rgb24(color):
    r, g, b = (int(v) for v in color)
    if not all(0 <= v <= 255 for v in (r, g, b)):
        raise ValueError("overlay: a colour is (r, g, b) in 0..255, got %r" % (color,))
    return (r << 16) | (g << 8) | b


# the largest packed upload of a call: the fixed part, and per frame the points, the edges and the patch
PACK_BYTES = K["PACK_HEAD"] + MAX_FRAMES * (8 * MAX_POINTS + 16 * MAX_POLYGONS * MAX_VERTICES + PATCH_H * PATCH_W)


class _Pack:
    """The packed upload of one call position: a pinned host buffer, its device copy, the maxima's workspace and the event of the last
    copy."""

    def __init__(self, device):
        import torch
        self.host = torch.empty(PACK_BYTES, dtype=torch.uint8).pin_memory()
        self.dev = torch.empty(PACK_BYTES, dtype=torch.uint8, device=device)
        self.maxbits = torch.empty(MAX_FRAMES, dtype=torch.int32, device=device)
        self.copied = None


class Overlay:
    """Annotated frames on the device.  Owns what must not be allocated per call: the packed uploads (pinned staging and device copy, one
    per call of a render), a 1 x 1 map for frames drawn without heat, and per frame shape in use the output buffers -- the composed RGB
    and, for a 4:2:0 output, the packed buffer -- one per frame of that shape in a render.  The returned tensors are these buffers: the
    next render() overwrites them (on the same stream in order; a render on another stream first waits for the previous one)."""

    def __init__(self, device="cuda"):
        import torch
        self.device = _owned.resolve(device, "Overlay")
        self.L = _lib.overlay_lib()
        self._packs = []       # [_Pack, ...], one per call of a render
        self._rgb = {}         # (H, W) -> [uint8 [H, W, 3], ...]
        self._yuv = {}         # (H, W) -> [uint8 [frame_bytes], ...]
        self._zero = torch.zeros(1, 1, dtype=torch.float32, device=self.device)
        self._last = None      # (stream, event) of the previous render

    def buffers(self):
        """The addresses of every buffer the overlay owns (a steady stream leaves this list as it is)."""
        return sorted([p.host.data_ptr() for p in self._packs] + [p.dev.data_ptr() for p in self._packs]
                      + [p.maxbits.data_ptr() for p in self._packs] + [self._zero.data_ptr()]
                      + [t.data_ptr() for v in self._rgb.values() for t in v] + [t.data_ptr() for v in self._yuv.values() for t in v])

    def _buffer(self, table, key, taken, shape):
        import torch
        bufs = table.setdefault(key, [])
        k = taken[(id(table), key)] = taken.get((id(table), key), -1) + 1          # (the frames of this shape so far, per table)
        if k == len(bufs):
            bufs.append(torch.empty(*shape, dtype=torch.uint8, device=self.device))
        return bufs[k]

    def render(self, frames_rgb, maps, *, gain=127.5, colormap="red", points=None, point_radius=2, regions=None, labels=None, out="rgb",
               matrix="bt709", range="limited", point_color=POINT_COLOR, region_color=REGION_COLOR):
        """frames_rgb: uint8 [H, W, 3] device tensors; maps: one device map [mh, mw] per frame (a 16-bit map is widened with .float(),
        which is exact), or None for a frame drawn without heat.  gain: a number, "max", or one of either per frame.  points: None or per
        frame None / [P, 2] of (x, y) in pixel-centre coordinates of the frame; regions: None or per frame None / a list of polygons;
        labels: None or per frame None / (coverage patch uint8 [lh, lw], lx, ly) (count_label makes the demos').  Returns per frame a
        uint8 device tensor [H, W, 3], or for out = nv12 / nv21 / i420 the packed 1-D buffer YuvFrame.from_buffer reads.  Frames of
        one frame shape and one map shape share calls of up to 16; every call is one packed upload and its launches on the current
        stream.  matrix and range of a 4:2:0 output: one name each, or one per frame."""
        import torch
        n = len(frames_rgb)
        spaces = list(zip(list(matrix) if isinstance(matrix, (list, tuple)) else [matrix] * n,
                          list(range) if isinstance(range, (list, tuple)) else [range] * n))
        if len(spaces) != n:
            raise ValueError("Overlay.render: matrix and range are one name each, or one per frame")
        for mx, rg in spaces or [("bt709", "limited")]:
            _check_names(out, mx, rg)
        if len(maps) != n:
            raise ValueError("Overlay.render: one map (or None) per frame")
        per = lambda v, what: [None] * n if v is None else list(v)
        points, regions, labels = per(points, "points"), per(regions, "regions"), per(labels, "labels")
        gains = list(gain) if isinstance(gain, (list, tuple)) else [gain] * n
        if not (len(points) == len(regions) == len(labels) == len(gains) == n):
            raise ValueError("Overlay.render: points, regions, labels and a list of gains have one entry per frame")
        lut, zero_lut = colormap_table(colormap), np.zeros((256, 4), np.uint8)
        prgb, ergb = _rgb24(point_color), _rgb24(region_color)
        groups, jobs = {}, [None] * n
        for i, (f, m) in enumerate(zip(frames_rgb, maps)):
            if not (isinstance(f, torch.Tensor) and f.dtype == torch.uint8 and f.dim() == 3 and f.shape[2] == 3):
                raise ValueError("Overlay.render: frames are uint8 [H, W, 3] device tensors")
            if f.device != self.device or (m is not None and m.device != self.device):
                raise ValueError("Overlay.render: frame or map on another device, this Overlay is for %s" % self.device)
            H, W = int(f.shape[0]), int(f.shape[1])
            if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
                raise ValueError("Overlay.render: H and W are 1..%d, got %d x %d" % (MAX_SIDE, H, W))
            if m is None:
                m, g = self._zero, 0.0
            else:
                if m.dim() != 2 or not (1 <= m.shape[0] <= MAX_SIDE and 1 <= m.shape[1] <= MAX_SIDE):
                    raise ValueError("Overlay.render: a map is [mh, mw] with sides 1..%d, got %s" % (MAX_SIDE, tuple(m.shape)))
                m = m if (m.dtype == torch.float32 and m.is_contiguous()) else m.float().contiguous()
                g = gains[i]
                if isinstance(g, str) and g != "max":
                    raise ValueError('Overlay.render: gain is a number or "max", got %r' % g)
            pts = _check_points(points[i], point_radius) if points[i] is not None and len(points[i]) else None
            counts, edges = polygon_edges(regions[i]) if regions[i] is not None and len(regions[i]) else ([], None)
            lab = _check_label(labels[i]) if labels[i] is not None else None
            jobs[i] = (f if f.is_contiguous() else f.contiguous(), m, g, pts, counts, edges, lab)
            groups.setdefault((H, W, int(m.shape[0]), int(m.shape[1]), maps[i] is None) + spaces[i], []).append(i)
        if not 0 <= int(point_radius) <= MAX_RADIUS:
            raise ValueError("overlay: point_radius is 0..%d, got %r" % (MAX_RADIUS, point_radius))
        result, taken, call = [None] * n, {}, 0
        with torch.cuda.device(self.device):
            cur = torch.cuda.current_stream(self.device)
            if self._last is not None and self._last[0] != cur:
                cur.wait_event(self._last[1])
            st = C.c_void_p(cur.cuda_stream)
            for (H, W, mh, mw, noheat, mx, rg), idxs in groups.items():
                for g0 in np.arange(0, len(idxs), MAX_FRAMES):
                    sel = idxs[g0:g0 + MAX_FRAMES]
                    if call == len(self._packs):
                        self._packs.append(_Pack(self.device))
                    pack, call = self._packs[call], call + 1
                    if pack.copied is not None:
                        pack.copied.synchronize()          # the pinned buffer's previous copy must have left it
                    host = pack.host.numpy()
                    host[K["PACK_LUT"]:K["PACK_LUT"] + 1024] = (zero_lut if noheat else lut).ravel()
                    fgain = host[K["PACK_GAINS"]:K["PACK_GAINS"] + 64].view(np.float32)
                    recs = (_lib.OverlayFrame * len(sel))()
                    keep, off, any_max = [], K["PACK_HEAD"], False
                    for k, i in enumerate(sel):
                        f, m, g, pts, counts, edges, lab = jobs[i]
                        r = recs[k]
                        rgb = self._buffer(self._rgb, (H, W), taken, (H, W, 3))
                        if f.data_ptr() == rgb.data_ptr():               # a frame that is this position's own output of the last render
                            f = f.clone()
                        keep.append(f)
                        r.rgb, r.map, r.out = f.data_ptr(), m.data_ptr(), rgb.data_ptr()
                        result[i] = rgb
                        if out != "rgb":
                            result[i] = self._buffer(self._yuv, (H, W), taken, (frame_bytes(out, W, H),))
                            r.yuv = result[i].data_ptr()
                        r.gain_max = int(isinstance(g, str))
                        any_max |= bool(r.gain_max)
                        fgain[k] = 0.0 if r.gain_max else np.float32(g)
                        if pts is not None:
                            r.n_points, r.points_off = len(pts), off
                            host[off:off + 8 * len(pts)].view(np.int32)[:] = pts.ravel()
                            off += 8 * len(pts)
                        if edges is not None:
                            verts = (C.c_int * len(counts))(*counts)
                            keep.append(verts)
                            r.poly_verts, r.n_polys, r.n_edges, r.edges_off = C.addressof(verts), len(counts), len(edges), off
                            host[off:off + 16 * len(edges)].view(np.int32)[:] = edges.ravel()
                            off += 16 * len(edges)
                        if lab is not None:
                            patch, lx, ly = lab
                            r.lh, r.lw, r.lx, r.ly, r.patch_off = patch.shape[0], patch.shape[1], lx, ly, off
                            host[off:off + patch.size] = patch.ravel()
                            off += (patch.size + 3) // 4 * 4
                    pack.dev[:off].copy_(pack.host[:off], non_blocking=True)
                    if pack.copied is None:
                        pack.copied = torch.cuda.Event()
                    pack.copied.record(cur)
                    _lib.overlay_check(self.L.countr_overlay_render(
                        recs, len(sel), H, W, mh, mw, pack.dev.data_ptr(), off, int(point_radius), prgb, ergb, OUTPUTS[out],
                        MATRICES[mx], RANGES[rg], pack.maxbits.data_ptr() if any_max else None, st), "countr_overlay_render")
            if self._last is None or self._last[0] != cur:
                self._last = (cur, torch.cuda.Event())
            self._last[1].record(cur)
        return result


def overlay_for(device):
    """The Overlay of a device, made on first use (annotate_frames keeps its buffers here between calls)."""
    return _owned.instance(Overlay, device)
