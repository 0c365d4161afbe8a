"""The camera's own motion, from the motion field the flow library already computes: what lets count_flow and count_clip count in scene
coordinates under a panning camera.

    texture_host / estimate_host / compensate_host   the three parts of the rule of include/countr_hip_cam.h in numpy
    camera_host       the rule over a clip: records, the camera's path and the compensated fields -- the yardstick of the GPU tests, byte
                      for byte (all of it is integer arithmetic)
    CameraEstimator   the same from csrc_cam/cam.hip on the current stream: it owns workspace, flags and records
    CameraPath        what a clip adds up to: path int64 [T, 2] in 1/16 map pixel, lost, position(t, placement) in frame pixels
    pan_scene         a synthetic clip under a panning camera with a known answer

The rule in short (the header states it in full).  The model is camera="translation": a pan in the image plane; rotation and zoom are
not modelled.  A cell's texture T is the sum of its 64 pixels' absolute differences to the right and to the lower neighbour.  A cell
votes iff T >= min_texture and its offset lies in [-264, 264]^2; g is, per axis, the lower median of the voters' offsets; the estimate is
valid iff there are at least min_voters voters and at least half of them lie within tol of g on both axes, else g = (0, 0).  A flat
resting cell stays (0, 0), every other cell's offset becomes V - g, saturated.  The path adds g along each of the `interval` chains:
G_t = G_{t - interval} + g_t, in 1/16 map pixel, and an invalid estimate adds nothing and counts as lost.  With the flow library's sign
g = 16 (cam_t - cam_{t - interval}) when image pixel p shows scene point p + cam_t: the scene is the first frame's pixel grid.

The defaults min_texture = 128, tol = 8 and min_voters = 16 are unmeasured on real video; what exists is the instrument, pinned on
synthetic scenes with known answers."""
import ctypes as C

import numpy as np

from . import _lib, _owned

_K = {k[len("COUNTR_CAM_"):]: v for k, v in _lib.CAM_CONSTS.items()}
MAX_FRAMES, CELL, MAX_SIDE, RANGE, BINS, RECORD_INTS = (_K[k] for k in ("MAX_FRAMES", "CELL", "MAX_SIDE", "RANGE", "BINS", "RECORD_INTS"))
MODELS = ("translation",)
DEFAULTS = dict(min_texture=128, tol=8, min_voters=16)      # unmeasured on real video


def settings(camera, min_texture=128, tol=8, min_voters=16):
    """camera: None or a model's name (a string, so that a later model has a place) -> (min_texture, tol, min_voters) as ints."""
    if camera is not None and camera not in MODELS:
        raise ValueError("camera is None or one of %r, got %r" % (MODELS, camera))
    for name, v, low in (("min_texture", min_texture, 0), ("tol", tol, 0), ("min_voters", min_voters, 1)):
        if int(v) != v or not low <= v < 2 ** 31:
            raise ValueError("%s is an integer >= %d" % (name, low))
    return int(min_texture), int(tol), int(min_voters)


def _check_side(h, w):
    if h % CELL or w % CELL or not (CELL <= h <= MAX_SIDE and CELL <= w <= MAX_SIDE):
        raise ValueError("cam: h and w are multiples of %d in %d..%d, got %d x %d" % (CELL, CELL, MAX_SIDE, h, w))


def texture_host(luma):
    """The texture T uint32 [h / 8, w / 8] of a luma uint8 [h, w], by the header's rule."""
    L = np.asarray(luma)
    if L.dtype != np.uint8 or L.ndim != 2:
        raise ValueError("cam: a luma is uint8 [h, w]")
    h, w = L.shape
    _check_side(h, w)
    v = L.astype(np.int64)
    right, below = np.concatenate([v[:, 1:], v[:, -1:]], 1), np.concatenate([v[1:], v[-1:]], 0)
    d = np.abs(right - v) + np.abs(below - v)
    return d.reshape(h // CELL, CELL, w // CELL, CELL).sum((1, 3)).astype(np.uint32)


def estimate_host(field, luma, min_texture=128, tol=8, min_voters=16):
    """(motion field int16 [h / 8, w / 8, 2], current luma uint8 [h, w]) -> (record int32 [8] = gx, gy, voters, inliers, valid, cells,
    0, 0; flags uint8 [h / 8, w / 8], 1 where T >= min_texture).  The field may hold any int16."""
    T = texture_host(luma)
    V = np.asarray(field, np.int16).reshape(T.shape + (2,)).astype(np.int64)
    flags = T >= min_texture
    votes = flags & (np.abs(V) <= RANGE).all(-1)
    ox, oy = V[..., 0][votes], V[..., 1][votes]
    n = int(ox.size)
    gx = gy = inliers = 0
    if n:
        rank = (n + 1) // 2                                                        # ceil(n / 2): the lower median
        gx, gy = int(np.sort(ox)[rank - 1]), int(np.sort(oy)[rank - 1])
        inliers = int(((np.abs(ox - gx) <= tol) & (np.abs(oy - gy) <= tol)).sum())
    valid = n >= min_voters and 2 * inliers >= n
    rec = np.array([gx if valid else 0, gy if valid else 0, n, inliers, int(valid), T.size, 0, 0], np.int32)
    return rec, flags.astype(np.uint8)


def compensate_host(field, record, flags):
    """V' int16: (0, 0) where V == (0, 0) and the flag is 0, else V - g per component, saturated."""
    flags = np.asarray(flags, np.uint8)
    V = np.asarray(field, np.int16).reshape(flags.shape + (2,)).astype(np.int64)
    g = np.asarray(record, np.int64)[:2]
    out = np.clip(V - g, -32768, 32767)
    out[(V == 0).all(-1) & (flags == 0)] = 0
    return out.astype(np.int16)


class CameraPath:
    """The camera's path over a clip.  path: int64 [T, 2] as (Gx, Gy) in 1/16 map pixel, G_t = G_{t - interval} + g_t and 0 for
    t < interval; lost: the number of frames whose estimate was invalid (they add nothing); records: int32 [T, 8], zero rows for the
    first `interval` frames."""

    def __init__(self, path, lost, records):
        self.path = np.asarray(path, np.int64).reshape(-1, 2)
        self.lost = int(lost)
        self.records = np.asarray(records, np.int32).reshape(-1, RECORD_INTS)

    def position(self, t, placement):
        """C_t float64 (x, y): the camera's position at frame t in pixels of the original frame, (sx * Gx / 16, sy * Gy / 16) with the
        map's placement (sx, tx, sy, ty) -- image pixel p of frame t shows scene point p + C_t, the scene being the first frame's grid."""
        return position(self.path[t], placement)


def position(G, placement):
    sx, _tx, sy, _ty = (np.float64(v) for v in placement)
    return np.array([(sx * np.float64(G[0])) / 16, (sy * np.float64(G[1])) / 16], np.float64)


def shifted_placement(G, placement):
    """The placement of a map whose camera stands at G: (sx, tx + sx * Gx / 16, sy, ty + sy * Gy / 16), in fp64 as written."""
    sx, tx, sy, ty = (np.float64(v) for v in placement)
    return (float(sx), float(tx + (sx * np.float64(G[0])) / 16), float(sy), float(ty + (sy * np.float64(G[1])) / 16))


def camera_host(lumas, fields, interval=1, min_texture=128, tol=8, min_voters=16):
    """The rule over a clip.  lumas: uint8 [h, w] per frame; fields: each frame's motion field against the luma `interval` frames back,
    None for the first `interval` frames (flow_host's) -> (records int32 [T, 8], path int64 [T, 2], [compensated field or None, ...]);
    lost_frames(records) counts the invalid estimates."""
    s, T = int(interval), len(lumas)
    records, path, comp = np.zeros((T, RECORD_INTS), np.int32), np.zeros((T, 2), np.int64), []
    for t in range(T):
        if t < s or fields[t] is None:
            comp.append(None)
            continue
        records[t], flags = estimate_host(fields[t], lumas[t], min_texture, tol, min_voters)
        path[t] = path[t - s] + records[t, :2]
        comp.append(compensate_host(fields[t], records[t], flags))
    return records, path, comp


def lost_frames(records):
    """The number of estimated frames (cells > 0 in the record) whose estimate was invalid."""
    r = np.asarray(records, np.int32).reshape(-1, RECORD_INTS)
    return int(((r[:, 5] > 0) & (r[:, 4] == 0)).sum())


def _texture(rs, components=16, wavelengths=(5.0, 40.0)):
    lam = rs.uniform(wavelengths[0], wavelengths[1], components)
    th = rs.uniform(0, 2 * np.pi, components)
    f = (2 * np.pi / lam)[:, None] * np.stack([np.cos(th), np.sin(th)], 1)
    return f, rs.uniform(0, 2 * np.pi, components)


def pan_scene(h=96, w=192, objects=3, frames=60, speed=(1.0, 3.0), seed=0, pan=(1.3, 0.4), jitter=0.3, noise=0.0, sigma=2.0,
              patch=(26, 34), image_speed=(0.5, 5.0), interval=1):
    """blob_scene under a moving camera: `objects` objects, one per lane, each a Gaussian density blob (mass 60) in the middle of a
    textured patch that moves along x at a constant speed in `speed` px/frame IN THE SCENE, on a textured background that is evaluated at
    scene coordinates.  The camera moves by pan + uniform(-jitter, jitter) px per frame and axis, cam_0 = 0; image pixel p of frame t
    shows scene point p + cam_t.  Everything is laid out around the camera's position half-way through the clip, so the objects cross
    the lines in view.  -> (lumas uint8 [h, w] per frame, maps fp32 [h, w] per frame (in image pixels, as a forward would give them),
    lines fp32 [3, 4] and truth int [3, 2] as (forward, backward) in pixels of the FIRST frame, cam float64 [frames, 2]).
    Three things found when this scene was first built:
      1. The four-sinusoid textures of blob_scene alias inside a search square of radius 6: one cell matched at (-4.75, +6) px and wrecked
         a count.  16 components with wavelengths 5 .. 40 px did not alias, so every texture here has 16.
      2. An object's speed IN THE IMAGE is |v - pan|.  It must stay at least 1 px under `search`, and its patch must fill the 16 x 16
         window: 26 x 34 worked, with three objects on a 96 x 192 map.
      3. An object that nearly rests in the image (|v - pan| under half a pixel per interval) meets the flow rule's known weakness
         below half a pixel: at v = 1.06 under a pan of 1.3 +- 0.3 its speed was read 20 % too high, with the TRUE camera motion in
         place of the estimate just as with it, and one count came out 15.6 % off.  So a speed is drawn again until
         image_speed[0] / interval + jitter <= |v - pan_x| <= image_speed[1] / interval - jitter (1 px under a search of 6)."""
    rs = np.random.RandomState(seed)
    step = np.asarray(pan, np.float64)[None, :] + rs.uniform(-jitter, jitter, (frames, 2)) if jitter else np.tile(np.asarray(pan, np.float64), (frames, 1))
    cam = np.concatenate([np.zeros((1, 2)), np.cumsum(step[1:], 0)])
    mid = cam[(frames - 1) // 2]
    lx = w / 2 + mid[0]
    sign = np.array([1.0, -1.0] * objects)[:objects]
    rs.shuffle(sign)
    lo, hi = image_speed[0] / interval + jitter, image_speed[1] / interval - jitter
    v = np.zeros(objects)
    for k in range(objects):
        for _try in range(1000):
            v[k] = rs.uniform(speed[0], speed[1]) * sign[k]
            if lo <= abs(v[k] - pan[0]) <= hi:
                break
        else:
            raise ValueError("pan_scene: no speed in %r leaves |v - pan| in %r" % (speed, (lo, hi)))
    yc = (np.arange(objects) + 0.5) * h / objects + mid[1]
    xc = lx + rs.uniform(-3.0, 3.0, objects)
    ph, pw = patch
    ground = _texture(rs)
    waves = [_texture(rs) for _ in range(objects)]
    tex = lambda fp, X, Y: 128.0 + 8.0 * np.sin(fp[0][:, 0, None, None] * X + fp[0][:, 1, None, None] * Y + fp[1][:, None, None]).sum(0)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    centre = lambda k, t: (xc[k] + v[k] * (t - (frames - 1) / 2.0), yc[k])
    lumas, maps = [], []
    for t in range(frames):
        X, Y = xx + cam[t, 0], yy + cam[t, 1]                                      # the scene point every pixel shows
        img, dm = tex(ground, X, Y), np.zeros((h, w))
        for k in range(objects):
            cx, cy = centre(k, t)
            dx, dy = X - cx, Y - cy
            mask = np.clip(pw / 2.0 - np.abs(dx) + 0.5, 0, 1) * np.clip(ph / 2.0 - np.abs(dy) + 0.5, 0, 1)
            img = img * (1 - mask) + tex(waves[k], dx, dy) * mask
            dm += 60.0 * np.exp(-(dx * dx + dy * dy) / (2 * sigma * sigma)) / (2 * np.pi * sigma * sigma)
        if noise:
            img = img + rs.normal(0.0, noise, (h, w))
        lumas.append(np.clip(np.floor(img + 0.5), 0, 255).astype(np.uint8))
        maps.append(dm.astype(np.float32))
    y0, y1 = mid[1] - 10.0, mid[1] + h + 10.0
    lines = np.array([(lx + 0.3, y0, lx + 0.3, y1), (np.floor(lx) - 1, y0, np.floor(lx) - 1, y1), (lx - 12.0, y0, lx + 12.0, y1)], np.float32)
    side = lambda ln, p: ((np.float64(ln[2]) - ln[0]) * (p[1] - np.float64(ln[1])) - (np.float64(ln[3]) - ln[1]) * (p[0] - np.float64(ln[0]))) >= 0
    truth = np.zeros((len(lines), 2), np.int64)
    for j, ln in enumerate(lines):
        for k in range(objects):
            s0, s1 = side(ln, centre(k, 0)), side(ln, centre(k, frames - 1))
            truth[j, 0] += (not s0) and s1
            truth[j, 1] += s0 and (not s1)
    return lumas, maps, lines, truth, cam


class CameraEstimator:
    """countr_cam_estimate / _compensate of one frame shape on the current stream: owns the histogram workspace, the flags uint8
    [16, cells] and the records int32 [16, 8], made by the first call.  launch() and compensate() take device addresses and wait for
    nothing; run() is the whole rule on tensors, in chunks of 16, with one wait per chunk.  The defaults are unmeasured on real video."""

    def __init__(self, device="cuda", *, min_texture=128, tol=8, min_voters=16):
        self.device = _owned.resolve(device, "CameraEstimator")
        self.min_texture, self.tol, self.min_voters = settings(None, min_texture, tol, min_voters)
        self.L = _lib.cam_lib()
        self.shape = None
        self._a, self._b = ((C.c_void_p * MAX_FRAMES)() for _ in range(2))
        self.records = self.flags = self._ws = None

    def _fix_shape(self, h, w):
        import torch
        if self.shape is None:
            _check_side(h, w)
            ws = self.L.countr_cam_workspace(MAX_FRAMES, h, w)
            _lib.cam_check(min(ws, 0), "countr_cam_workspace")
            self.shape, self.cells = (h, w), (h // CELL) * (w // CELL)
            self.records = torch.zeros(MAX_FRAMES, RECORD_INTS, dtype=torch.int32, device=self.device)
            self.flags = torch.zeros(MAX_FRAMES, self.cells, dtype=torch.uint8, device=self.device)
            self._ws = torch.empty(ws, dtype=torch.uint8, device=self.device)
        elif self.shape != (h, w):
            raise ValueError("CameraEstimator serves one shape: it holds %r, got %r" % (self.shape, (h, w)))

    def launch(self, fields, lumas, h, w, stream):
        """fields, lumas: device addresses of n <= 16 (field, luma) pairs -> the records and flags of rows 0 .. n - 1, on `stream`."""
        self._fix_shape(h, w)
        n = len(fields)
        for k in range(n):
            self._a[k], self._b[k] = fields[k], lumas[k]
        _lib.cam_check(self.L.countr_cam_estimate(self._a, self._b, self.records.data_ptr(), self.flags.data_ptr(), n, h, w,
                                                  self.min_texture, self.tol, self.min_voters, self._ws.data_ptr(), stream), "countr_cam_estimate")

    def compensate(self, fields, outs, h, w, stream):
        """fields minus the g of the records launch() wrote for the same n, into outs (device addresses; an out may be its field)."""
        n = len(fields)
        for k in range(n):
            self._a[k], self._b[k] = fields[k], outs[k]
        _lib.cam_check(self.L.countr_cam_compensate(self._a, self.records.data_ptr(), self.flags.data_ptr(), self._b, n, h, w, stream),
                       "countr_cam_compensate")

    def run(self, fields, lumas):
        """fields: int16 [h / 8, w / 8, 2] device tensors, lumas: uint8 [h, w] device tensors, one pair per frame -> (records int32
        [T, 8], flags uint8 [T, h / 8, w / 8], compensated fields int16 [T, h / 8, w / 8, 2]) as numpy arrays."""
        import torch
        if len(fields) != len(lumas):
            raise ValueError("CameraEstimator.run: one luma per field")
        recs, flags, comps = [], [], []
        with torch.cuda.device(self.device):
            st = _owned.stream_handle(self.device)
            for c0 in range(0, len(fields), MAX_FRAMES):
                fs, ls = fields[c0:c0 + MAX_FRAMES], lumas[c0:c0 + MAX_FRAMES]
                for f, l in zip(fs, ls):
                    if not (f.is_cuda and f.dtype == torch.int16 and f.is_contiguous() and l.is_cuda and l.dtype == torch.uint8
                            and l.is_contiguous() and l.dim() == 2 and f.numel() == 2 * (l.shape[0] // CELL) * (l.shape[1] // CELL)):
                        raise ValueError("CameraEstimator.run: fields are int16 [h / 8, w / 8, 2], lumas uint8 [h, w], contiguous, on the device")
                h, w = (int(v) for v in ls[0].shape)
                out = [torch.empty_like(f) for f in fs]
                self.launch([f.data_ptr() for f in fs], [l.data_ptr() for l in ls], h, w, st)
                self.compensate([f.data_ptr() for f in fs], [o.data_ptr() for o in out], h, w, st)
                n = len(fs)
                recs.append(self.records[:n].cpu().numpy())
                flags.append(self.flags[:n].cpu().numpy().reshape(n, h // CELL, w // CELL))
                comps.append(torch.stack(out).cpu().numpy().reshape(n, h // CELL, w // CELL, 2))
        return np.concatenate(recs), np.concatenate(flags), np.concatenate(comps)
