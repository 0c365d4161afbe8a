"""Marks drawn onto frames on the device: thick segments, discs and text, each mark in a colour of its own, in place on packed RGB, and
behind the marks the NV12 / NV21 / I420 buffer a video encoder takes (csrc_draw/draw.hip: countr_draw_paint).  What a tracked clip shows:
every object's id and trail, every counting line's tally.

    draw_host    the rule of include/countr_hip_draw.h in numpy -- the yardstick of the GPU tests.  The rule is integers only, so the
                 device bytes equal draw_host's
    Marks        the marks of one frame, built on the host: segment, polyline, disc, text
    Painter      the same marks from the device on the stream the forward runs on: one packed upload and one call per 16 frames
    Trails       the last positions of every track, kept on the host
    clip_marks   what count_clip found on a frame -> its Marks; annotate_clip and its host reference both use it
    font         the 5 x 7 font of csrc_draw/draw.hip, read from the library

There is no host fallback.  No accuracy figure is involved: this draws what count_clip found."""
import ctypes as C

import numpy as np

from . import _lib, _owned
from .overlay import MATRICES, OUTPUTS, RANGES, _check_names, _rgb24, frame_bytes, rgb_to_yuv_host, round_coords

K = {k[len("COUNTR_DRAW_"):]: v for k, v in _lib.DRAW_CONSTS.items()}
assert all(K[n] == OUTPUTS[n.lower()] for n in ("RGB", "NV12", "NV21", "I420")) and K["BT709"] == MATRICES["bt709"] and K["FULL"] == RANGES["full"]
MAX_FRAMES, MAX_SIDE, MAX_SEGMENTS, MAX_DISCS, MAX_TEXTS = (K[n] for n in ("MAX_FRAMES", "MAX_SIDE", "MAX_SEGMENTS", "MAX_DISCS", "MAX_TEXTS"))
MAX_HALF_WIDTH, MAX_RADIUS, MAX_SCALE, TEXT_BYTES = K["MAX_HALF_WIDTH"], K["MAX_RADIUS"], K["MAX_SCALE"], K["TEXT_BYTES"]
SEGMENT_WORDS, DISC_WORDS, TEXT_WORDS = K["SEGMENT_WORDS"], K["DISC_WORDS"], K["TEXT_WORDS"]
# 16 clearly distinct colours for track ids, grey for a point without a track
PALETTE = ((230, 25, 75), (60, 180, 75), (255, 225, 25), (0, 130, 200), (245, 130, 48), (145, 30, 180), (70, 240, 240), (240, 50, 230),
           (210, 245, 60), (250, 190, 212), (0, 128, 128), (220, 190, 255), (170, 110, 40), (255, 250, 200), (128, 0, 0), (170, 255, 195))
NO_TRACK_COLOR = (128, 128, 128)
LINE_COLOR, HIT_COLOR = (0, 255, 255), (255, 255, 255)         # a counting line, and on a frame in which a track crossed it
TEXT_COLOR, TEXT_BACKGROUND = (255, 255, 255), (32, 32, 32)
_font = None


def track_color(track_id):
    """PALETTE[id % 16]; grey for id -1."""
    return PALETTE[int(track_id) % 16] if track_id >= 0 else NO_TRACK_COLOR


def font():
    """The font uint8 [95, 7]: row r of the glyph of character 32 + g is font()[g, r], column c its bit 4 - c."""
    global _font
    if _font is None:
        f = np.zeros((K["FONT_GLYPHS"], K["FONT_ROWS"]), np.uint8)
        _lib.draw_check(_lib.draw_lib().countr_draw_font(f.ctypes.data), "countr_draw_font")
        _font = f
    return _font


class Marks:
    """The marks of one frame.  Coordinates are (x, y) in pixel-centre coordinates of the frame; floats are rounded once, as
    floor(v + 0.5) (overlay.round_coords).  Within a kind the marks keep the order they were added in; whatever the order of the calls,
    segments lie below discs and discs below texts."""

    def __init__(self):
        self._segments, self._discs, self._texts = [], [], []

    def segments(self, p0, p1, half_width=0, color=LINE_COLOR):
        """Segments p0[i] -> p1[i], [N, 2] each; color: one (r, g, b) or [N, 3]."""
        a, b = round_coords(p0, "segment ends"), round_coords(p1, "segment ends")
        if len(a) != len(b) or not 0 <= int(half_width) <= MAX_HALF_WIDTH:
            raise ValueError("draw: segments are pairs of points with a half_width of 0..%d" % MAX_HALF_WIDTH)
        rec = np.empty((len(a), SEGMENT_WORDS), np.int32)
        rec[:, 0:2], rec[:, 2:4], rec[:, 4], rec[:, 5] = a, b, int(half_width), _colors(color, len(a))
        self._segments.append(rec)
        return self

    def segment(self, p0, p1, half_width=0, color=LINE_COLOR):
        return self.segments([p0], [p1], half_width, color)

    def polyline(self, points, half_width=0, color=LINE_COLOR):
        """The segments between consecutive points [N, 2]; one point is a segment of length zero."""
        p = np.asarray(points, np.float64).reshape(-1, 2)
        return self.segments(p[:-1], p[1:], half_width, color) if len(p) > 1 else self.segments(p, p, half_width, color)

    def discs(self, centres, r=2, color=LINE_COLOR):
        """Discs at centres [N, 2]; color: one (r, g, b) or [N, 3]."""
        c = round_coords(centres, "disc centres")
        if not 0 <= int(r) <= MAX_RADIUS:
            raise ValueError("draw: a disc's r is 0..%d, got %r" % (MAX_RADIUS, r))
        rec = np.empty((len(c), DISC_WORDS), np.int32)
        rec[:, 0:2], rec[:, 2], rec[:, 3] = c, int(r), _colors(color, len(c))
        self._discs.append(rec)
        return self

    def disc(self, centre, r=2, color=LINE_COLOR):
        return self.discs([centre], r, color)

    def text(self, x, y, text, scale=1, color=TEXT_COLOR, background=None):
        """`text` (str as latin-1, or bytes; up to 32) with its top-left corner at (x, y)."""
        return self.texts([(x, y)], [text], scale, color, background)

    def texts(self, positions, texts, scale=1, color=TEXT_COLOR, background=None):
        """One text per position [N, 2]: text() for many at once; color: one (r, g, b) or [N, 3]."""
        p = round_coords(positions, "a text's position")
        raws = [t if isinstance(t, bytes) else str(t).encode("latin-1", "replace") for t in texts]
        if len(raws) != len(p) or any(len(r) > TEXT_BYTES for r in raws) or not 1 <= int(scale) <= MAX_SCALE:
            raise ValueError("draw: one text of up to %d bytes per position, and a scale of 1..%d" % (TEXT_BYTES, MAX_SCALE))
        rec = np.zeros((len(p), TEXT_WORDS), np.int32)
        rec[:, 0:2], rec[:, 2], rec[:, 3] = p, int(scale), _colors(color, len(p))
        rec[:, 4], rec[:, 5] = -1 if background is None else _rgb24(background), [len(r) for r in raws]
        rec[:, 6:].view(np.uint8)[:] = np.frombuffer(b"".join(r.ljust(TEXT_BYTES, b"\0") for r in raws), np.uint8).reshape(len(p), TEXT_BYTES)
        self._texts.append(rec)
        return self

    def arrays(self):
        """-> (segments int32 [S, 6], discs int32 [D, 4], texts int32 [T, 14]): the records of the header, in key order."""
        out = []
        for parts, words, limit, what in ((self._segments, SEGMENT_WORDS, MAX_SEGMENTS, "segments"), (self._discs, DISC_WORDS, MAX_DISCS, "discs"),
                                          (self._texts, TEXT_WORDS, MAX_TEXTS, "texts")):
            a = np.concatenate(parts) if parts else np.zeros((0, words), np.int32)
            if len(a) > limit:
                raise ValueError("draw: at most %d %s a frame, got %d" % (limit, what, len(a)))
            out.append(a)
        return tuple(out)


def _colors(color, n):
    """One (r, g, b) or [n, 3] -> int64 [n] of 0xRRGGBB."""
    c = np.asarray(color, np.int64)
    if c.ndim == 1:
        return np.full(n, _rgb24(color), np.int64)
    if c.shape != (n, 3) or (c < 0).any() or (c > 255).any():
        raise ValueError("draw: colours are (r, g, b) in 0..255, one or one per mark")
    return (c[:, 0] << 16) | (c[:, 1] << 8) | c[:, 2]


def _rgb(v):
    return ((v >> 16) & 255, (v >> 8) & 255, v & 255)


def _put(rgb, x, y, color):
    H, W, _ = rgb.shape
    ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)
    rgb[y[ok], x[ok]] = color


def _brush(r):
    d = np.arange(-r, r + 1)
    v, u = np.meshgrid(d, d, indexing="ij")
    keep = u * u + v * v <= r * r
    return u[keep], v[keep]


def centres_host(x0, y0, x1, y1, lo=None, hi=None):
    """The centres of a segment, int64 (x [n + 1], y [n + 1]), by the edge rule."""
    dx, dy = x1 - x0, y1 - y0
    n = max(abs(dx), abs(dy))
    i = np.arange(n + 1, dtype=np.int64)
    if n == 0:
        return x0 + 0 * i, y0 + 0 * i
    return x0 + (2 * i * dx + n) // (2 * n), y0 + (2 * i * dy + n) // (2 * n)


def text_mask_host(raw, scale):
    """The foreground of a text's box: bool [8 s, 6 s len]."""
    f = font()
    g = np.array([b if 32 <= b <= 126 else ord("?") for b in raw], np.int64) - 32
    cell = np.zeros((len(raw), 8, 6), bool)
    cell[:, :7, :5] = (f[g][:, :, None] >> (4 - np.arange(5))) & 1
    box = cell.transpose(1, 0, 2).reshape(8, 6 * len(raw))
    return np.repeat(np.repeat(box, scale, 0), scale, 1)


def draw_host(rgb, marks, out="rgb", matrix="bt709", range="limited"):
    """The rule in numpy: the marks painted one after another in key order onto a copy of rgb uint8 [H, W, 3].  -> uint8 [H, W, 3], or
    for out = nv12 / nv21 / i420 the packed buffer."""
    _check_names(out, matrix, range)
    rgb = np.array(rgb, dtype=np.uint8)
    if rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError("draw_host: the frame is uint8 [H, W, 3], got %s" % (rgb.shape,))
    H, W, _ = rgb.shape
    segments, discs, texts = marks.arrays() if marks is not None else Marks().arrays()
    for x0, y0, x1, y1, w, c in segments.astype(np.int64):
        # (only the centres whose brush can reach the frame: the others cover nothing of it)
        x, y = centres_host(x0, y0, x1, y1)
        near = (x >= -w) & (x < W + w) & (y >= -w) & (y < H + w)
        u, v = _brush(w)
        _put(rgb, (x[near, None] + u[None, :]).ravel(), (y[near, None] + v[None, :]).ravel(), _rgb(c))
    for cx, cy, r, c in discs.astype(np.int64):
        u, v = _brush(r)
        _put(rgb, cx + u, cy + v, _rgb(c))
    for rec in texts:
        x, y, s, fg, bg, n = (int(v) for v in rec[:6])
        fore = text_mask_host(rec[6:].view(np.uint8)[:n], s)
        yy, xx = np.mgrid[y:y + 8 * s, x:x + 6 * s * n]
        if bg >= 0:
            _put(rgb, xx[~fore], yy[~fore], _rgb(bg))
        _put(rgb, xx[fore], yy[fore], _rgb(fg))
    return rgb if out == "rgb" else rgb_to_yuv_host(rgb, out, matrix, range)


class _Pack:
    """The packed upload of one call position: a pinned host buffer and its device copy, grown together, and the event of the last copy."""

    def __init__(self, device):
        self.device, self.buf, self.buf_host, self.copied = device, None, None, None


class Painter:
    """Marks on the device.  Owns what must not be allocated per call: the packed uploads (pinned staging and device copy, one per call of
    a paint, grown to the largest upload seen), and per frame shape in use the owner planes and, for a 4:2:0 output, the packed buffers
    -- one per frame of that shape in a paint.  The frames are painted in place; the 4:2:0 tensors are these buffers: the next paint()
    overwrites them (on the same stream in order; a paint on another stream first waits for the previous one)."""

    def __init__(self, device="cuda"):
        self.device = _owned.resolve(device, "Painter")
        self.L = _lib.draw_lib()
        self._packs = []       # [_Pack, ...], one per call of a paint
        self._owner = {}       # (H, W) -> [int32 [H, W], all zero between calls, ...]
        self._yuv = {}         # (H, W) -> [uint8 [frame_bytes], ...]
        self._last = None      # (stream, event) of the previous paint

    def buffers(self):
        """The addresses of every buffer the painter owns (a steady stream leaves this list as it is)."""
        return sorted([t.data_ptr() for p in self._packs for t in (p.buf, p.buf_host) if t is not None]
                      + [t.data_ptr() for v in self._owner.values() for t in v] + [t.data_ptr() for v in self._yuv.values() for t in v])

    def owners(self):
        """The owner planes (all zero between calls)."""
        return [t for v in self._owner.values() for t in v]

    def _buffer(self, table, key, taken, make):
        bufs = table.setdefault(key, [])
        k = taken[(id(table), key)] = taken.get((id(table), key), -1) + 1          # (the frames of this shape so far, per table)
        if k == len(bufs):
            bufs.append(make())
        return bufs[k]

    def paint(self, frames_rgb, marks, *, out="rgb", matrix="bt709", range="limited"):
        """frames_rgb: contiguous uint8 [H, W, 3] device tensors, painted IN PLACE; marks: per frame a Marks or None.  Returns the frames,
        or for out = nv12 / nv21 / i420 per frame the packed 1-D buffer YuvFrame.from_buffer reads, made from the painted frame.  Frames
        of one shape share calls of up to 16; every call is one packed upload and its launches on the current stream.  matrix and range
        of a 4:2:0 output: one name each, or one per frame."""
        import torch
        n = len(frames_rgb)
        spaces = list(zip(list(matrix) if isinstance(matrix, (list, tuple)) else [matrix] * n,
                          list(range) if isinstance(range, (list, tuple)) else [range] * n))
        if len(spaces) != n or len(marks) != n:
            raise ValueError("Painter.paint: one Marks (or None) per frame; matrix and range are one name each, or one per frame")
        for mx, rg in spaces or [("bt709", "limited")]:
            _check_names(out, mx, rg)
        groups, recs = {}, [None] * n
        for i, f in enumerate(frames_rgb):
            if not (isinstance(f, torch.Tensor) and f.dtype == torch.uint8 and f.dim() == 3 and f.shape[2] == 3 and f.is_contiguous()):
                raise ValueError("Painter.paint: frames are contiguous uint8 [H, W, 3] device tensors")
            if f.device != self.device:
                raise ValueError("Painter.paint: frame on another device, this Painter is for %s" % self.device)
            H, W = int(f.shape[0]), int(f.shape[1])
            if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
                raise ValueError("Painter.paint: H and W are 1..%d, got %d x %d" % (MAX_SIDE, H, W))
            recs[i] = (marks[i] if marks[i] is not None else Marks()).arrays()
            groups.setdefault((H, W) + spaces[i], []).append(i)
        result, taken, call = list(frames_rgb), {}, 0
        with torch.cuda.device(self.device):
            cur = torch.cuda.current_stream(self.device)
            if self._last is not None and self._last[0] != cur:
                cur.wait_event(self._last[1])
            st = C.c_void_p(cur.cuda_stream)
            for (H, W, mx, rg), idxs in groups.items():
                for g0 in np.arange(0, len(idxs), MAX_FRAMES):
                    sel = idxs[g0:g0 + MAX_FRAMES]
                    if call == len(self._packs):
                        self._packs.append(_Pack(self.device))
                    pack, call = self._packs[call], call + 1
                    nbytes = sum(a.nbytes for i in sel for a in recs[i])
                    if pack.copied is not None:
                        pack.copied.synchronize()          # the pinned buffer's previous copy must have left it
                    if pack.buf is None or pack.buf.numel() < nbytes:     # (with room to spare: a steady stream stops growing)
                        _owned.grow(pack, "buf", max(2 * nbytes, 1 << 16), torch.uint8, pinned=True)
                    host = pack.buf_host.numpy()
                    frs = (_lib.DrawFrame * len(sel))()
                    off = 0
                    for k, i in enumerate(sel):
                        r = frs[k]
                        r.rgb = frames_rgb[i].data_ptr()
                        r.owner = self._buffer(self._owner, (H, W), taken,
                                               lambda: torch.zeros(H, W, dtype=torch.int32, device=self.device)).data_ptr()
                        if out != "rgb":
                            result[i] = self._buffer(self._yuv, (H, W), taken, lambda: torch.empty(
                                frame_bytes(out, W, H), dtype=torch.uint8, device=self.device))
                            r.yuv = result[i].data_ptr()
                        for a, count, where in zip(recs[i], ("n_segments", "n_discs", "n_texts"), ("segments_off", "discs_off", "texts_off")):
                            setattr(r, count, len(a))
                            setattr(r, where, off)
                            host[off:off + a.nbytes] = a.reshape(-1).view(np.uint8)
                            off += a.nbytes
                    if off:
                        pack.buf[:off].copy_(pack.buf_host[:off], non_blocking=True)
                        if pack.copied is None:
                            pack.copied = torch.cuda.Event()
                        pack.copied.record(cur)
                    _lib.draw_check(self.L.countr_draw_paint(frs, len(sel), H, W, pack.buf_host.data_ptr(), pack.buf.data_ptr(), off, OUTPUTS[out],
                                                             MATRICES[mx], RANGES[rg], st), "countr_draw_paint")
            if self._last is None or self._last[0] != cur:
                self._last = (cur, torch.cuda.Event())
            self._last[1].record(cur)
        return result


def painter_for(device):
    """The Painter of a device, made on first use (annotate_clip keeps its buffers here between calls)."""
    return _owned.instance(Painter, device)


class Trails:
    """The last `length` positions of every track, kept on the host in arrays (a row per track; no loop over points).  update() is called
    once per frame, in time order.  A track that update() has not seen for more than `length` frames is dropped; id -1 (a point without a
    track) has no trail."""

    def __init__(self, length=16):
        if int(length) != length or length < 1:
            raise ValueError("Trails: length is >= 1")
        self.length = int(length)
        self.frame = 0
        self.ids = np.zeros(0, np.int64)                           # ascending
        self.xy = np.zeros((0, self.length, 2), np.float64)        # a row's positions, oldest first, right-aligned
        self.n = np.zeros(0, np.int64)                             # how many of a row's positions are valid: min(observations, length)
        self.seen = np.zeros(0, np.int64)                          # the frame of a row's last position

    def update(self, points, ids):
        """points [P, 2] as (x, y) and their track ids [P] of the next frame -> (ids int64 [T] ascending, xy float64 [T, length, 2], n
        int64 [T]) of the live trails: trail t is xy[t, length - n[t]:], oldest first, its last position the newest.  The arrays are
        the store's own: the next update() changes them."""
        p = np.asarray(points, np.float64).reshape(-1, 2)
        ids = np.asarray(ids, np.int64).reshape(-1)
        if len(p) != len(ids):
            raise ValueError("Trails.update: one id per point")
        self.frame += 1
        p, ids = p[ids >= 0], ids[ids >= 0]
        ids, first = np.unique(ids, return_index=True)             # (an id names one point of a frame)
        p = p[first]
        new = ids[~np.isin(ids, self.ids)]
        if len(new):
            order = np.argsort(np.concatenate([self.ids, new]), kind="stable")
            grow = lambda a: np.concatenate([a, np.zeros((len(new),) + a.shape[1:], a.dtype)])[order]
            self.ids, self.xy, self.n, self.seen = np.concatenate([self.ids, new])[order], grow(self.xy), grow(self.n), grow(self.seen)
        rows = np.searchsorted(self.ids, ids)
        self.xy[rows, :-1] = self.xy[rows, 1:]
        self.xy[rows, -1] = p
        self.n[rows] = np.minimum(self.n[rows] + 1, self.length)
        self.seen[rows] = self.frame
        live = self.frame - self.seen <= self.length
        if not live.all():
            self.ids, self.xy, self.n, self.seen = self.ids[live], self.xy[live], self.n[live], self.seen[live]
        return self.ids, self.xy, self.n

    def polylines(self):
        """{id: float64 [n, 2]} of the live trails, oldest position first."""
        return {int(i): self.xy[t, self.length - self.n[t]:].copy() for t, i in enumerate(self.ids)}


def mark_scale(H, scale=None):
    """The size of a clip's marks: `scale`, or 1 up to 809 rows, 2 up to 1349 (1080p), 3 up to 1889, ..."""
    return int(scale) if scale else max(1, (int(H) + 270) // 540)


def tally_text(name, forward, backward):
    return "%s %d/%d" % (name, forward, backward)


def clip_marks(points, ids, events, summary, line_names, lines, count, C_t=None, *, size, trails=None, scale=None, tags=True, tally=True,
               hud=True):
    """What count_clip found on one frame -> its Marks.  points float [P, 2], ids [P] and events [P] of the frame, the step's summary
    int32 [40], the lines [(ax, ay, bx, by), ...] and their names, the frame's count; size = (W, H) of the frame; trails: None or what
    Trails.update returned for this frame.  In this order: the trails (half-width s - 1, the track's colour), the counting lines
    (half-width s; HIT_COLOR on a frame in which an event bit of that line is set, LINE_COLOR otherwise), a disc of radius 2 s per point
    in its track's colour (grey without a track), beside each point that has a track the tag "%d" % id, at each line's midpoint
    "<name> <forward>/<backward>" with the cumulative counts of the summary, and at the top left three lines on a dark background:
    "count %.1f", "tracks <live>", "total <confirmed>".  s = scale or max(1, (H + 270) // 540).  Floats are rounded once, by Marks.
    C_t: the camera's position float64 (x, y) under camera="translation"; trails and lines are then in scene pixels (pixels of the first
    frame) and are drawn at p - C_t, one fp64 subtraction before the rounding, so a line stays on the scene it was drawn on.  The points
    are the frame's own pixels either way."""
    W, H = size
    s = mark_scale(H, scale)
    points = np.asarray(points, np.float64).reshape(-1, 2)
    ids, events = np.asarray(ids, np.int64).reshape(-1), np.asarray(events, np.uint32).reshape(-1)
    summary = np.asarray(summary).reshape(-1)
    lines = np.asarray(lines, np.float64).reshape(-1, 4)
    shift = np.zeros(2) if C_t is None else np.asarray(C_t, np.float64).reshape(2)
    palette = np.concatenate([np.asarray(PALETTE, np.int64), np.asarray([NO_TRACK_COLOR], np.int64)])
    m = Marks()
    if trails is not None and len(trails[0]):
        tid, xy, n = trails
        L = xy.shape[1]
        t, j = np.nonzero(np.arange(1, L)[None, :] >= (L - n)[:, None] + 1)      # segment (j, j + 1) of trail t has both ends valid
        if len(t):
            m.segments(xy[t, j] - shift, xy[t, j + 1] - shift, s - 1, palette[tid[t] % 16])
    hit = [bool(((events >> k) & 1).any() or ((events >> (16 + k)) & 1).any()) for k in np.arange(len(lines))]
    for (ax, ay, bx, by), h in zip(lines, hit):
        m.segment((ax - shift[0], ay - shift[1]), (bx - shift[0], by - shift[1]), s, HIT_COLOR if h else LINE_COLOR)
    if len(points):
        m.discs(points, 2 * s, palette[np.where(ids >= 0, ids % 16, 16)])
    if tags and (ids >= 0).any():
        known = ids >= 0
        m.texts(points[known] + (2 * s + 2, -4 * s), ["%d" % i for i in ids[known]], s, palette[ids[known] % 16])
    if tally and len(lines):
        m.texts((lines[:, 0:2] + lines[:, 2:4]) / 2 - shift + 2 * s,
                [tally_text(name, summary[8 + 2 * k], summary[9 + 2 * k])[:TEXT_BYTES] for k, name in enumerate(line_names)], s, TEXT_COLOR,
                TEXT_BACKGROUND)
    if hud:
        m.texts([(0, 0), (0, 8 * s), (0, 16 * s)], ["count %.1f" % count, "tracks %d" % summary[0], "total %d" % summary[2]], s, TEXT_COLOR,
                TEXT_BACKGROUND)
    return m
