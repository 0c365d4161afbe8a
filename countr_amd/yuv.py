"""Counting from video-decoder frames: 4:2:0 surfaces (NV12, NV21, I420, P010) in, the packed 8-bit RGB [H, W, 3] of the raw-frame entry
points out, converted on the device (csrc_yuv/yuv.hip: countr_yuv_to_rgb) on the stream the forward runs on.

include/countr_hip_yuv.h states the rule; yuv_host restates it in numpy.  The conversion is integer arithmetic, so the device bytes equal
yuv_host's, and everything behind them is the existing path: count_frames(model, [YuvFrame(...)]) equals
count_frames(model, [yuv_host(frame)]) bit for bit.  P010 is reduced to 8-bit RGB by the rule and nothing else: no tone mapping, no
transfer function.  There is no host fallback."""
import ctypes as C

import numpy as np

from . import _lib, _owned

FORMATS = {"nv12": _lib.YUV_CONSTS["COUNTR_YUV_NV12"], "nv21": _lib.YUV_CONSTS["COUNTR_YUV_NV21"],
           "i420": _lib.YUV_CONSTS["COUNTR_YUV_I420"], "p010": _lib.YUV_CONSTS["COUNTR_YUV_P010"]}
MATRICES = {"bt601": _lib.YUV_CONSTS["COUNTR_YUV_BT601"], "bt709": _lib.YUV_CONSTS["COUNTR_YUV_BT709"]}
RANGES = {"limited": _lib.YUV_CONSTS["COUNTR_YUV_LIMITED"], "full": _lib.YUV_CONSTS["COUNTR_YUV_FULL"]}
CHROMAS = {"nearest": _lib.YUV_CONSTS["COUNTR_YUV_NEAREST"], "linear": _lib.YUV_CONSTS["COUNTR_YUV_LINEAR"]}
MAX_FRAMES = _lib.YUV_CONSTS["COUNTR_YUV_MAX_FRAMES"]
MAX_SIDE = _lib.YUV_CONSTS["COUNTR_YUV_MAX_SIDE"]
# (matrix, range) -> cy, yoff, rv, gu, gv, bu: round(256 x the exact coefficient)
COEFFICIENTS = {("bt601", "full"): (256, 0, 359, -88, -183, 454), ("bt709", "full"): (256, 0, 403, -48, -120, 475),
                ("bt601", "limited"): (298, 16, 409, -100, -208, 516), ("bt709", "limited"): (298, 16, 459, -55, -136, 541)}


def _is_tensor(a):
    return type(a).__module__.split(".")[0] == "torch"          # (yuv_host and YuvFrame on numpy planes stay free of torch)


def _dtype_name(a):
    return str(a.dtype).replace("torch.", "")


def _strides_bytes(a):
    if _is_tensor(a):
        return tuple(int(s) * a.element_size() for s in a.stride())
    return tuple(int(s) for s in a.strides)


def frame_bytes(format, width, height):
    """Bytes of one packed frame: the Y plane followed by the chroma plane(s), without padding."""
    wc, hc = (width + 1) // 2, (height + 1) // 2
    return (width * height + 2 * wc * hc) * (2 if format == "p010" else 1)


class YuvFrame:
    """One 4:2:0 frame as views of its planes.  y [H, W]; c0 [Hc, 2 Wc] interleaved (U, V) pairs for nv12 / p010, (V, U) for nv21, or
    U [Hc, Wc] for i420 with c1 = V [Hc, Wc] (YV12: swap the two); Hc = (H + 1) // 2, Wc = (W + 1) // 2.  The planes are 2-D numpy arrays,
    CPU tensors or device tensors, uint8 (uint16 for p010: a sample is word >> 6); their last stride is 1 and a larger row stride
    expresses the pitch.  .shape is (H, W, 3), the shape of the RGB frame it stands for: the raw-frame entry points read nothing else of
    a frame before FramePrep.prepare converts it."""

    def __init__(self, y, c0, c1=None, *, format="nv12", matrix="bt709", range="limited", chroma="nearest"):
        for value, table, what in ((format, FORMATS, "format"), (matrix, MATRICES, "matrix"), (range, RANGES, "range"),
                                   (chroma, CHROMAS, "chroma")):
            if value not in table:
                raise ValueError("YuvFrame: %s is one of %s, got %r" % (what, ", ".join(table), value))
        if (c1 is not None) != (format == "i420"):
            raise ValueError("YuvFrame: c1 (the V plane) is given for i420 and for no other format, got format %r" % format)
        want = "uint16" if format == "p010" else "uint8"
        planes = [("y", y), ("c0", c0)] + ([("c1", c1)] if c1 is not None else [])
        for name, p in planes:
            if len(p.shape) != 2:
                raise ValueError("YuvFrame: %s is a 2-D plane, got shape %s" % (name, tuple(p.shape)))
            if _dtype_name(p) != want:
                raise ValueError("YuvFrame: %s planes are %s, %s is %s" % (format, want, name, _dtype_name(p)))
        H, W = int(y.shape[0]), int(y.shape[1])
        if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
            raise ValueError("YuvFrame: H and W are 1..%d, got %d x %d" % (MAX_SIDE, H, W))
        hc, wc = (H + 1) // 2, (W + 1) // 2
        cshape = (hc, wc) if format == "i420" else (hc, 2 * wc)
        for name, p in planes[1:]:
            if tuple(int(v) for v in p.shape) != cshape:
                raise ValueError("YuvFrame: a %d x %d %s frame has %s of shape %s, got %s" % (H, W, format, name, cshape, tuple(p.shape)))
        for name, p in planes:
            if int(p.shape[1]) > 1 and _strides_bytes(p)[1] != (2 if format == "p010" else 1):
                raise ValueError("YuvFrame: the last stride of %s must be 1 (a row stride expresses the pitch)" % name)
        on_device = [_is_tensor(p) and p.is_cuda for _n, p in planes]
        if any(on_device) != all(on_device):
            raise ValueError("YuvFrame: the planes of a frame are all on the host or all on one device")
        self.y, self.c0, self.c1 = y, c0, c1
        self.format, self.matrix, self.range, self.chroma = format, matrix, range, chroma
        self.shape = (H, W, 3)
        self.is_cuda = all(on_device)

    @property
    def planes(self):
        return [self.y, self.c0] + ([self.c1] if self.c1 is not None else [])

    @classmethod
    def from_buffer(cls, buf, width, height, **kw):
        """One packed frame -- the Y plane followed by the chroma plane(s), without padding, as raw .yuv files and most capture APIs
        deliver it -- as views of `buf` (bytes-like, a 1-D uint8 numpy array or a 1-D uint8 tensor, on the host or the device).  For
        p010 the buffer holds little-endian 16-bit words."""
        format = kw.get("format", "nv12")
        if format not in FORMATS:
            raise ValueError("YuvFrame: format is one of %s, got %r" % (", ".join(FORMATS), format))
        W, H = int(width), int(height)
        if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
            raise ValueError("YuvFrame: H and W are 1..%d, got %d x %d" % (MAX_SIDE, H, W))
        if not _is_tensor(buf):
            buf = np.frombuffer(buf, np.uint8) if not isinstance(buf, np.ndarray) else buf
        if len(buf.shape) != 1 or _dtype_name(buf) != "uint8":
            raise ValueError("YuvFrame.from_buffer: a 1-D uint8 buffer is required")
        need = frame_bytes(format, W, H)
        if int(buf.shape[0]) != need:
            raise ValueError("YuvFrame.from_buffer: a %d x %d %s frame has %d bytes, the buffer %d" % (W, H, format, need, int(buf.shape[0])))
        wc, hc = (W + 1) // 2, (H + 1) // 2
        if format == "p010":
            if _is_tensor(buf):
                import torch
                words = buf.view(torch.uint16)
            else:
                words = buf.view("<u2")
                words = words if words.dtype == np.uint16 else words.astype(np.uint16)
            return cls(words[:W * H].reshape(H, W), words[W * H:].reshape(hc, 2 * wc), **kw)
        if format == "i420":
            n = W * H
            return cls(buf[:n].reshape(H, W), buf[n:n + wc * hc].reshape(hc, wc), buf[n + wc * hc:].reshape(hc, wc), **kw)
        return cls(buf[:W * H].reshape(H, W), buf[W * H:].reshape(hc, 2 * wc), **kw)


def _host(p):
    return p.cpu().numpy() if _is_tensor(p) else np.asarray(p)


def host_samples(frame):
    """(Y [H, W], U [Hc, Wc], V [Hc, Wc]) of a frame as int32 sample values (p010: word >> 6)."""
    y, c0 = _host(frame.y).astype(np.int32), _host(frame.c0).astype(np.int32)
    if frame.format == "i420":
        u, v = c0, _host(frame.c1).astype(np.int32)
    elif frame.format == "nv21":
        u, v = c0[:, 1::2], c0[:, 0::2]
    else:
        u, v = c0[:, 0::2], c0[:, 1::2]
    if frame.format == "p010":
        y, u, v = y >> 6, u >> 6, v >> 6
    return y, u, v


def upsample_host(c, H, W, chroma):
    """A chroma plane [Hc, Wc] (int32) at every luma position [H, W] by the rule of include/countr_hip_yuv.h."""
    hc, wc = c.shape
    y, x = np.arange(H), np.arange(W)
    j, i = y >> 1, x >> 1
    if chroma == "nearest":
        return c[j][:, i]
    jn = np.where(y & 1, np.minimum(j + 1, hc - 1), np.maximum(j - 1, 0))
    s = 3 * c[j] + c[jn]                                         # [H, Wc]
    even = (s[:, i] + 2) >> 2
    odd = (s[:, i] + s[:, np.minimum(i + 1, wc - 1)] + 4) >> 3
    return np.where((x & 1)[None, :] == 1, odd, even)


def convert_host(y, u, v, matrix, range, bits=8):
    """Samples (int32 arrays of one shape, `bits` = 8 or 10) -> uint8 [..., 3] by the rule: int32, arithmetic shift, clamp."""
    cy, yoff, rv, gu, gv, bu = COEFFICIENTS[(matrix, range)]
    s = bits - 8
    y, u, v = (np.asarray(a, np.int32) for a in (y, u, v))
    c = cy * (y - (yoff << s)) + (128 << s)
    d, e = u - (128 << s), v - (128 << s)
    rgb = np.stack([(c + rv * e) >> (8 + s), (c + gu * d + gv * e) >> (8 + s), (c + bu * d) >> (8 + s)], -1)
    return np.clip(rgb, 0, 255).astype(np.uint8, order="C")       # (C order whatever the inputs' layout: a frame the entry points copy fast)


def yuv_host(frame):
    """The rule in numpy: a YuvFrame -> uint8 [H, W, 3]."""
    H, W, _ = frame.shape
    y, u, v = host_samples(frame)
    return convert_host(y, upsample_host(u, H, W, frame.chroma), upsample_host(v, H, W, frame.chroma), frame.matrix, frame.range,
                        10 if frame.format == "p010" else 8)


def _align16(n):
    return (n + 15) // 16 * 16


class _Staging:
    """The upload buffers of one frame position of one (format, H, W): one pinned host buffer and its device copy, holding the Y plane and
    the chroma plane(s) at pitches rounded up to 16 bytes, and the event of their last copy."""

    def __init__(self, format, H, W, device):
        import torch
        hc, wc = (H + 1) // 2, (W + 1) // 2
        bps = 2 if format == "p010" else 1
        self.row_y = W * bps
        self.row_c = wc if format == "i420" else 2 * wc * bps
        self.pitch_y, self.pitch_c = _align16(self.row_y), _align16(self.row_c)
        self.offsets = [0, self.pitch_y * H] + ([self.pitch_y * H + self.pitch_c * hc] if format == "i420" else [])
        self.rows = [H, hc, hc]
        total = self.pitch_y * H + self.pitch_c * hc * (2 if format == "i420" else 1)
        self.host = torch.empty(total, dtype=torch.uint8).pin_memory()
        self.dev = torch.empty(total, dtype=torch.uint8, device=device)
        self.copied = None

    def upload(self, frame, stream):
        import torch
        if self.copied is not None:
            self.copied.synchronize()          # the pinned buffer's previous copy must have left it
        host = self.host.numpy()
        for k, p in enumerate(frame.planes):
            pitch, row = (self.pitch_y, self.row_y) if k == 0 else (self.pitch_c, self.row_c)
            dst = host[self.offsets[k]:self.offsets[k] + pitch * self.rows[k]].reshape(self.rows[k], pitch)[:, :row]
            src = _host(p)
            np.copyto(dst.view(src.dtype), src)
        self.dev.copy_(self.host, non_blocking=True)
        if self.copied is None:
            self.copied = torch.cuda.Event()
        self.copied.record(stream)
        base = self.dev.data_ptr()
        return [base + o for o in self.offsets], self.pitch_y, self.pitch_c


class YuvConverter:
    """YuvFrames -> uint8 [H, W, 3] device tensors.  Owns, per frame shape in use, what must not be allocated per call: pinned staging and
    device plane buffers for host frames (the upload is 1.5 bytes a pixel, 3 for p010) and the device RGB buffers, one per frame of that
    shape in a call.  Device planes are used where they are, with their pitch.  The returned tensors are the converter's own buffers:
    the next convert() overwrites them (on the same stream in order; FramePrep's guard covers another stream)."""

    def __init__(self, device="cuda"):
        self.device = _owned.resolve(device, "YuvConverter")
        self.L = _lib.yuv_lib()
        self._staging = {}     # (format, H, W) -> [_Staging, ...]
        self._rgb = {}         # (H, W) -> [uint8 [H, W, 3], ...]

    def buffers(self):
        """The device addresses of every buffer the converter owns (a steady stream leaves this list as it is)."""
        return sorted([s.dev.data_ptr() for v in self._staging.values() for s in v] + [s.host.data_ptr() for v in self._staging.values() for s in v]
                      + [t.data_ptr() for v in self._rgb.values() for t in v])

    def _planes(self, frame, used):
        """(plane addresses, pitch_y, pitch_c) of a frame on the device."""
        import torch
        H, W, _ = frame.shape
        if not frame.is_cuda:
            key = (frame.format, H, W)
            slots = self._staging.setdefault(key, [])
            k = used[key] = used.get(key, -1) + 1
            if k == len(slots):
                slots.append(_Staging(frame.format, H, W, self.device))
            return slots[k].upload(frame, torch.cuda.current_stream(self.device))
        for p in frame.planes:
            if p.device != self.device:
                raise ValueError("YuvConverter: plane on %s, this converter is for %s" % (p.device, self.device))
        pitches = [_strides_bytes(p)[0] if int(p.shape[0]) > 1 else _align16(int(p.shape[1]) * p.element_size()) for p in frame.planes]
        if frame.c1 is not None and pitches[1] != pitches[2]:
            if int(frame.c0.shape[0]) > 1:
                raise ValueError("YuvConverter: the U and V planes of an i420 frame share one pitch, got %d and %d" % (pitches[1], pitches[2]))
        return [p.data_ptr() for p in frame.planes], pitches[0], pitches[1]

    def convert(self, frames):
        """[YuvFrame, ...] -> [uint8 [H, W, 3] device tensor, ...] on the current stream.  Frames of one (format, H, W, pitches, matrix,
        range, chroma) share launches, at most 16 each."""
        import torch
        out = [None] * len(frames)
        groups, used, taken = {}, {}, {}
        with torch.cuda.device(self.device):
            st = _owned.stream_handle(self.device)
            for i, f in enumerate(frames):
                if not isinstance(f, YuvFrame):
                    raise ValueError("YuvConverter.convert: a YuvFrame is required, got %s" % type(f).__name__)
                H, W, _ = f.shape
                ptrs, py, pc = self._planes(f, used)
                bufs = self._rgb.setdefault((H, W), [])
                k = taken[(H, W)] = taken.get((H, W), -1) + 1
                if k == len(bufs):
                    bufs.append(torch.empty(H, W, 3, dtype=torch.uint8, device=self.device))
                out[i] = bufs[k]
                groups.setdefault((f.format, H, W, py, pc, f.matrix, f.range, f.chroma), []).append((ptrs, out[i].data_ptr()))
            for (format, H, W, py, pc, matrix, range_, chroma), members in groups.items():
                for g0 in range(0, len(members), MAX_FRAMES):
                    part = members[g0:g0 + MAX_FRAMES]
                    arr = lambda vals: (C.c_void_p * len(vals))(*vals)
                    _lib.yuv_check(self.L.countr_yuv_to_rgb(
                        arr([m[0][0] for m in part]), arr([m[0][1] for m in part]), arr([m[0][2] for m in part]) if format == "i420" else None,
                        arr([m[1] for m in part]), len(part), H, W, py, pc, FORMATS[format], MATRICES[matrix], RANGES[range_],
                        CHROMAS[chroma], st), "countr_yuv_to_rgb")
        return out
