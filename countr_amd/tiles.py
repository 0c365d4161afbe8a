"""Counting a frame at k times the model's height: a 2-D grid of 384 x 384 tiles over the frame's own pixels (count_frames(zoom=k)).

    tile_starts    inference.window_starts with 128 replaced by a stride: the starts of one axis
    zoomed_size    (Hk, Wk) of a W x H frame at zoom k
    auto_zoom      the smallest k at which a frame's exemplars stop being "small" (zoom="auto")
    tiles_host     the stitching rule of countr_tile_blend (include/countr_hip_tiles.h) restated with inference.blend_windows, applied
                   along the columns and then, transposed, along the rows -- the yardstick of the GPU tests
    TileStitcher   countr_tile_gather / countr_tile_blend from csrc_tiles/tiles.hip on the stream the forward runs on: owns the
                   tile-output buffer, the workspace and the pinned result; two launches, one download and one synchronisation a frame
    count_zoomed   a zoomed image through the engine: tiles in band-major order, consecutive chunks of max_batch tiles one forward each

The rule.  The zoomed image [3, Hk, Wk] is cut into tiles at rows tile_starts(Hk, band_stride) x columns tile_starts(Wk, 128).  Every tile
is one forward row.  Band b's map is the reference's sequential horizontal blend of its tiles (a column an earlier tile covered becomes
old / 2 + new / 2); the frame's map is the same rule over the band maps along the rows.  The forwards are exactly the batches
inference.density_maps forms for the band images image[:, :, r:r + 384, :], so the map equals that composition bit for bit."""
import ctypes as C

import numpy as np
import torch

from . import _lib, _owned, inference

TILE = _lib.TILES_CONSTS["COUNTR_TILES_SIZE"]
MAX_STARTS, MAX_RECTS = _lib.TILES_CONSTS["COUNTR_TILES_MAX_STARTS"], _lib.TILES_CONSTS["COUNTR_TILES_MAX_RECTS"]
MAX_ZOOM = _lib.TILES_CONSTS["COUNTR_TILES_MAX_ZOOM"]
COL_STRIDE = 128                       # the reference's window stride: not configurable
BAND_STRIDES = (128, 192, 256, 384)


def tile_starts(size, stride=COL_STRIDE):
    """inference.window_starts with 128 replaced by `stride`: 0, stride, ... while the tile fits; the first that would pass the end is
    snapped to size - 384 and closes the list, unless the tile before it already ends at size."""
    starts, start = [], 0
    while start + TILE - 1 < size:
        starts.append(start)
        start += stride
        if start + TILE - 1 >= size:
            if start == size - TILE + stride:
                break
            start = size - TILE
    return starts


def zoomed_size(W, H, k):
    """(Hk, Wk) of a W x H frame at zoom k: frames.new_width with the height 384 k."""
    hk = TILE * int(k)
    return hk, 16 * int((W / H * hk) / 16)


def check_zoom(zoom, zoom_max=3, band_stride=128):
    if not (zoom == "auto" or (isinstance(zoom, (int, np.integer)) and not isinstance(zoom, bool) and 1 <= zoom <= MAX_ZOOM)):
        raise ValueError('zoom is 1..%d or "auto", got %r' % (MAX_ZOOM, zoom))
    if not (isinstance(zoom_max, (int, np.integer)) and 1 <= zoom_max <= MAX_ZOOM):
        raise ValueError("zoom_max is 1..%d, got %r" % (MAX_ZOOM, zoom_max))
    if band_stride not in BAND_STRIDES:
        raise ValueError("band_stride is one of %s, got %r" % (BAND_STRIDES, band_stride))


def auto_zoom(boxes_xyxy, W, H, max_s_cnt=1, zoom_max=3):
    """zoom="auto" for one frame: the smallest k in 1..zoom_max at which fewer than max_s_cnt of the first three scaled exemplar
    rectangles are under 10 px on both sides (inference._small_exemplars); zoom_max if none is; 1 for a frame without boxes."""
    from . import frames
    if boxes_xyxy is None or len(boxes_xyxy) == 0:
        return 1
    for k in range(1, int(zoom_max) + 1):
        if inference._small_exemplars(frames.scale_boxes(boxes_xyxy, W, H, TILE * k)) < max_s_cnt:
            return k
    return int(zoom_max)


def tiles_host(outs, row_starts, col_starts, hk, wk):
    """outs [nrows * ncols, 384, 384], band-major (numpy or torch) -> the stitched map [hk, wk] of the same kind: blend_windows over the
    tiles of every band, then blend_windows over the transposed band maps."""
    t = torch.as_tensor(outs)
    nr, nc = len(row_starts), len(col_starts)
    t = t.reshape(nr, nc, TILE, TILE)
    bands = torch.stack([inference.blend_windows(t[b], col_starts, wk) for b in range(nr)])          # [nr, 384, wk]
    dm = inference.blend_windows(bands.transpose(1, 2), row_starts, hk, wk).t().contiguous()        # rows take the columns' part
    return dm.numpy() if isinstance(outs, np.ndarray) else dm


def _ints(values):
    return (C.c_int * len(values))(*[int(v) for v in values])


class TileStitcher:
    """countr_tile_gather and countr_tile_blend on device buffers.  Owns the tile-output buffer [T, 384, 384], the workspace, the sums
    (device + pinned); they grow monotonically, so a steady stream of equal frames allocates nothing but its maps.  A frame is
    begin(ntiles) -> put(first, rows) per forward -> stitch(...), all on the current stream; stitch waits once."""

    def __init__(self, device="cuda"):
        self.device = _owned.resolve(device, "TileStitcher")
        self.L = _lib.tiles_lib()
        self._outs = None           # fp32 [T, 384, 384]: the tile maps of one frame, band-major
        self._ws = None             # uint8: the blend's partials
        self._sums = torch.empty(1 + MAX_RECTS, dtype=torch.float32, device=self.device)
        self._sums_host = torch.empty(1 + MAX_RECTS, dtype=torch.float32).pin_memory()
        self._guard = _owned.Guard(self.device)     # a frame on another stream than the previous one waits before it reuses the buffers

    def _stream(self):
        return _owned.stream_handle(self.device)

    def gather(self, image, tiles, dst):
        """tiles [(row, col), ...] of image [1, 3, hk, wk] (or [3, hk, wk]; fp32, contiguous) -> dst[:len(tiles)], dst being a contiguous
        fp32 [>= len(tiles), 3, 384, 384] batch.  64 tiles a launch."""
        if not (image.is_cuda and image.dtype == torch.float32 and image.is_contiguous() and image.shape[-3] == 3
                and image.numel() == 3 * image.shape[-2] * image.shape[-1]):
            raise ValueError("TileStitcher.gather: a contiguous fp32 device image [1, 3, hk, wk] is required")
        if not (dst.is_cuda and dst.dtype == torch.float32 and dst.is_contiguous() and tuple(dst.shape[1:]) == (3, TILE, TILE)
                and dst.shape[0] >= len(tiles)):
            raise ValueError("TileStitcher.gather: dst is a contiguous fp32 [>= %d, 3, 384, 384] device batch" % len(tiles))
        hk, wk = int(image.shape[-2]), int(image.shape[-1])
        with torch.cuda.device(self.device):
            for t0 in range(0, len(tiles), MAX_STARTS):
                part = tiles[t0:t0 + MAX_STARTS]
                _lib.tiles_check(self.L.countr_tile_gather(image.data_ptr(), hk, wk, _ints([r for r, _c in part]), _ints([c for _r, c in part]),
                                                           len(part), dst[t0:].data_ptr(), self._stream()), "countr_tile_gather")

    def begin(self, ntiles):
        """The tile-output buffer of a frame of ntiles tiles, [ntiles, 384, 384]; valid until the next begin."""
        with torch.cuda.device(self.device):
            self._guard.enter()
            if self._outs is None or self._outs.shape[0] < ntiles:
                self._outs = torch.empty(ntiles, TILE, TILE, dtype=torch.float32, device=self.device)
        return self._outs[:ntiles]

    def put(self, first, rows):
        """A forward's output rows [n, 384, 384] become tiles first .. first + n - 1 (a forward's output lives until the next forward)."""
        self._outs[first:first + rows.shape[0]].copy_(rows, non_blocking=True)

    def blend(self, outs, row_starts, col_starts, hk, wk, rects=()):
        """countr_tile_blend on outs [nrows * ncols, 384, 384] -> (dm [hk, wk], sums float32 [1 + R] on the device): the launches alone,
        no download and no wait."""
        rects = [[int(v) for v in r] for r in rects]
        if len(rects) > MAX_RECTS:
            raise _lib.CountrError("countr_tile_blend: 0..%d rectangles, got %d" % (MAX_RECTS, len(rects)))
        if not (outs.is_cuda and outs.dtype == torch.float32 and outs.is_contiguous() and tuple(outs.shape[1:]) == (TILE, TILE)
                and outs.shape[0] == len(row_starts) * len(col_starts)):
            raise ValueError("TileStitcher.blend: outs is a contiguous fp32 [nrows * ncols, 384, 384] device tensor")
        with torch.cuda.device(self.device):
            need = self.L.countr_tiles_workspace(int(hk), int(wk))
            _lib.tiles_check(min(need, 0), "countr_tiles_workspace")
            _owned.grow(self, "_ws", need, torch.uint8)
            dm = torch.empty(int(hk), int(wk), dtype=torch.float32, device=self.device)
            flat = [v for r in rects for v in r]
            _lib.tiles_check(self.L.countr_tile_blend(outs.data_ptr(), len(row_starts), len(col_starts), _ints(row_starts), _ints(col_starts),
                                                      int(hk), int(wk), _ints(flat) if flat else None, len(rects), dm.data_ptr(),
                                                      self._sums.data_ptr(), self._ws.data_ptr(), self._stream()), "countr_tile_blend")
        return dm, self._sums[:1 + len(rects)]

    def stitch(self, row_starts, col_starts, hk, wk, rects=(), outs=None):
        """The frame's map and sums from the tile-output buffer (or `outs`): (dm [hk, wk] on the device, sums float32 [1 + R] on the
        host: the map's sum, then the inclusive sums of the rectangles (y1, x1, y2, x2) clipped to the map).  Two launches, one
        download, one wait."""
        if outs is None:
            outs = self._outs[:len(row_starts) * len(col_starts)]
        dm, sums = self.blend(outs, row_starts, col_starts, hk, wk, rects)
        n = sums.shape[0]
        with torch.cuda.device(self.device):
            cur = torch.cuda.current_stream(self.device)
            self._sums_host[:n].copy_(sums, non_blocking=True)
            self._guard.leave(cur)
        self._guard.event.synchronize()
        return dm, self._sums_host[:n].numpy().copy()


def tile_stitcher(device):
    """The TileStitcher of a device, made on first use (count_frames keeps its buffers here between calls)."""
    return _owned.instance(TileStitcher, device)


def normalised_count(sums, rects, normalization=True):
    """inference._normalise's formulas on the sums of the stitch: count = S / 60 in fp32, divided by e_cnt = (the rectangles' fp32
    sums / 60, added) / 3 where that is > 1.8."""
    pred = (np.float32(sums[0]) / np.float32(60)).item()
    if normalization and rects:
        e_cnt = sum((np.float32(s) / np.float32(60)).item() for s in sums[1:1 + len(rects)]) / 3
        if e_cnt > 1.8:
            pred /= e_cnt
    return pred


@torch.no_grad()
def zoomed_map(model, image, ex, rects=None, max_batch=32, band_stride=128, stitcher=None):
    """image [1, 3, Hk, Wk] (fp32, on the model's device), ex [1, S, 3, 64, 64] or an empty tensor, rects [[y1, x1, y2, x2], ...] or None
    -> (dm [Hk, Wk], sums float32 [1 + len(rects)] on the host).  The tiles, band-major, run in consecutive chunks of max_batch, each
    padded to inference._bucket; the exemplars are repeated on every row; consecutive chunks of one bucket use the encoder look-ahead
    (engine.forward_loaded_pipelined).  Every chunk's rows are copied into the stitcher's buffer on the forward's stream."""
    if not hasattr(model, "_engine") or getattr(model, "img_size", TILE) != TILE:
        raise _lib.CountrError("zoom needs the HIP engine of a 384 x 384 model: the tile path has no torch fallback")
    if not (image.is_cuda and image.dtype == torch.float32 and image.dim() == 4 and image.shape[0] == 1 and image.shape[1] == 3
            and image.is_contiguous()):
        raise ValueError("zoomed_map: a contiguous fp32 device image [1, 3, Hk, Wk] is required")
    rects = list(rects or [])
    if len(rects) > MAX_RECTS:
        raise ValueError("zoom: at most %d exemplar rectangles a frame, got %d" % (MAX_RECTS, len(rects)))
    hk, wk = int(image.shape[-2]), int(image.shape[-1])
    dev = image.device
    rows, cols = tile_starts(hk, band_stride), tile_starts(wk, COL_STRIDE)
    if len(rows) > MAX_STARTS or len(cols) > MAX_STARTS:
        raise ValueError("zoom: at most %d tile starts per axis, a %d x %d image has %d x %d" % (MAX_STARTS, wk, hk, len(cols), len(rows)))
    if not rows or not cols:                # narrower than a tile: the reference's loop never runs
        return torch.zeros(hk, wk, device=dev), np.zeros(1 + len(rects), np.float32)
    S = int(ex.shape[1]) if ex.nelement() > 0 else 0
    tiles = [(r, c) for r in rows for c in cols]
    chunks = [tiles[t0:t0 + max_batch] for t0 in range(0, len(tiles), max_batch)]
    buckets = [inference._bucket(len(ch), max_batch) for ch in chunks]
    st = stitcher or tile_stitcher(dev)
    eng = model._engine()
    eng.check_ln_fold(image[:, :, :TILE, :TILE])     # (first use of a weight set only: may rebuild the plans)
    with torch.cuda.device(dev):
        st.begin(len(tiles))
        def fill(chunk):
            def into(dst):
                st.gather(image, chunk, dst)
                if dst.shape[0] > len(chunk):
                    dst[len(chunk):].zero_()           # padding rows only need defined values
            return into

        have, first = None, 0
        for i, (chunk, nb) in enumerate(zip(chunks, buckets)):
            n = len(chunk)

            def load_boxes(bx):
                bx[:n].copy_(ex[:, :S].expand(n, S, 3, 64, 64))
                if nb > n:
                    bx[n:].zero_()

            ahead = i + 1 < len(chunks) and buckets[i + 1] == nb     # the next chunk's encoder runs beside this chunk's decoder
            out, have = inference.forward_ahead(eng, eng.plan(nb, S, False), nb, S, fill(chunk), fill(chunks[i + 1]) if ahead else None,
                                                load_boxes, have)
            st.put(first, out[:n])
            first += n
        return st.stitch(rows, cols, hk, wk, rects)


@torch.no_grad()
def count_zoomed(model, image, ex, rects=None, normalization=True, max_batch=32, band_stride=128, stitcher=None):
    """zoomed_map + normalised_count -> (count, dm [Hk, Wk]).  A zoomed frame never takes the 3 x 3 split."""
    dm, sums = zoomed_map(model, image, ex, rects, max_batch, band_stride, stitcher)
    return normalised_count(sums, rects, normalization), dm
