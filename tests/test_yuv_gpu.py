"""GPU: countr_yuv_to_rgb (csrc_yuv/yuv.hip) through ctypes against countr_amd.yuv_host, byte for byte -- the conversion is integer
arithmetic, so there is no tolerance -- and the raw-frame entry points on YuvFrame items against the same call on yuv_host(frame), on the
tiny model: everything behind the conversion is the existing path, so counts, maps, points, regions and classes are equal."""
import ctypes as C
import os
import re
import subprocess
import sys
from functools import partial

import numpy as np
import pytest
import torch

from oracle import weights as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# small sizes (edge clamps, the odd last chroma sample, the tail behind the last full run of 16 columns), and two whose width is
# a multiple of 16: with an aligned pitch those take the 16-byte loads AND stores in every format; 132 = 8 x 16 + 4 takes the 4-byte
# stores with a tail of four pixels (as does 8)
SIZES = [(1, 1), (2, 2), (3, 5), (5, 7), (6, 8), (33, 130), (64, 258), (6, 16), (35, 176), (7, 132)]
PAIRS = {"nv12": [("bt709", "limited"), ("bt601", "full")], "nv21": [("bt601", "limited"), ("bt709", "full")],
         "i420": [("bt709", "full"), ("bt601", "limited")], "p010": [("bt709", "limited"), ("bt601", "full")]}
GUARD = 64


def rows_of(fmt, H, W):
    """[(rows, bytes of a row), ...] of the planes of a frame."""
    hc, wc = (H + 1) // 2, (W + 1) // 2
    bps = 2 if fmt == "p010" else 1
    return [(H, W * bps)] + ([(hc, wc), (hc, wc)] if fmt == "i420" else [(hc, 2 * wc * bps)])


def pitch_of(row, mode, bps):
    """"row": the row itself; "row+3": three elements more (misaligned: the element-wise path); "256": the row rounded up to 256."""
    return {"row": row, "row+3": row + 3 * bps, "256": (row + 255) // 256 * 256}[mode]


class Case:
    """n random frames of one format and shape.  Every plane sits inside a larger host buffer (256 bytes + `shift` elements in front, 256
    behind) filled with a sentinel, the padding between its rows included."""

    def __init__(self, fmt, H, W, mode, n=1, seed=0, shift=0, **kw):
        from countr_amd import YuvFrame
        self.fmt, self.H, self.W, self.n, self.kw = fmt, H, W, n, kw
        bps = 2 if fmt == "p010" else 1
        rs = np.random.RandomState(seed * 7919 + H * 131 + W)
        spec = rows_of(fmt, H, W)
        py, pc = pitch_of(spec[0][1], mode, bps), pitch_of(spec[1][1], mode, bps)
        self.pitches = (py, pc)
        self.lead = 256 + shift * bps
        self.shift = shift
        self.bufs, self.frames, self.masks = [], [], []
        for _ in range(n):
            planes, bufs, masks = [], [], []
            for k, (rows, row) in enumerate(spec):
                pitch = py if k == 0 else pc
                buf = np.zeros(self.lead + rows * pitch + 256, np.uint8)
                mask = np.ones(buf.size, bool)                                       # True: padding, not a sample
                body = buf[self.lead:self.lead + rows * pitch].reshape(rows, pitch)
                if bps == 2:                                                         # all 16 bits random: the low six are not the sample
                    body[:, :row] = rs.randint(0, 65536, (rows, row // 2)).astype("<u2").view(np.uint8)
                else:
                    body[:, :row] = rs.randint(0, 256, (rows, row))
                mask[self.lead:self.lead + rows * pitch].reshape(rows, pitch)[:, :row] = False
                view = body[:, :row]
                planes.append(view.view(np.uint16) if bps == 2 else view)
                bufs.append(buf)
                masks.append(mask)
            self.bufs.append(bufs)
            self.masks.append(masks)
            self.frames.append(YuvFrame(*planes, format=fmt, **kw))

    def want(self):
        from countr_amd import yuv_host
        return [yuv_host(f) for f in self.frames]

    def run(self, sentinel):
        """The kernel on device copies of the buffers with the padding set to `sentinel` -> [uint8 [H, W, 3], ...]; the guard bytes behind
        (and the byte in front of a shifted) rgb buffer are checked here."""
        from countr_amd import _lib, yuv as Y
        L = _lib.yuv_lib()
        dev = []
        for bufs, masks in zip(self.bufs, self.masks):
            for b, m in zip(bufs, masks):
                b[m] = sentinel
            dev.append([torch.from_numpy(b).cuda() for b in bufs])
        size = self.H * self.W * 3
        outs = [torch.full((16 + size + GUARD,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(self.n)]
        front = 16 if self.shift == 0 else 15                                      # a shifted frame writes to an odd address
        arr = lambda vals: (C.c_void_p * len(vals))(*vals)
        planes = [arr([d[k].data_ptr() + self.lead for d in dev]) for k in range(len(dev[0]))]
        rc = L.countr_yuv_to_rgb(planes[0], planes[1], planes[2] if self.fmt == "i420" else None, arr([o.data_ptr() + front for o in outs]),
                                 self.n, self.H, self.W, self.pitches[0], self.pitches[1], Y.FORMATS[self.fmt],
                                 Y.MATRICES[self.kw.get("matrix", "bt709")], Y.RANGES[self.kw.get("range", "limited")],
                                 Y.CHROMAS[self.kw.get("chroma", "nearest")], C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, L.countr_yuv_last_error().decode()
        torch.cuda.synchronize()
        got = []
        for o in outs:
            o = o.cpu().numpy()
            assert (o[:front] == 0xA5).all() and (o[front + size:] == 0xA5).all(), "bytes outside the rgb buffer were written"
            got.append(o[front:front + size].reshape(self.H, self.W, 3))
        return got

    def check(self):
        want = self.want()
        got = self.run(0x5A)
        for j, (g, w) in enumerate(zip(got, want)):
            bad = np.argwhere(g != w)
            assert bad.size == 0, "%s %dx%d %s frame %d: %d bytes differ, first at (y, x, channel) %s: %d, want %d" % (
                self.fmt, self.H, self.W, self.kw, j, len(bad), bad[0], g[tuple(bad[0])], w[tuple(bad[0])])
        again = self.run(0xC3)                                    # another sentinel in the padding: the same bytes
        for g, a in zip(got, again):
            assert np.array_equal(g, a), "the padding between the rows, or around the planes, reached the output"


# ---- 1. the kernel alone
@pytest.mark.parametrize("chroma", ["nearest", "linear"])
@pytest.mark.parametrize("fmt", ["nv12", "nv21", "i420", "p010"])
def test_kernel_equals_yuv_host(fmt, chroma):
    seen = set()
    for H, W in SIZES:
        for mode in ("row", "row+3", "256"):
            for matrix, range_ in PAIRS[fmt]:
                Case(fmt, H, W, mode, seed=len(seen), matrix=matrix, range=range_, chroma=chroma).check()
                seen.add((matrix, range_))
    assert len(seen) == 2


def test_the_formats_cover_all_four_matrix_range_pairs():
    assert {p for v in PAIRS.values() for p in v} == {(m, r) for m in ("bt601", "bt709") for r in ("limited", "full")} and all(len(v) == 2 for v in PAIRS.values())


@pytest.mark.parametrize("chroma", ["nearest", "linear"])
def test_kernel_on_a_1080p_nv12_frame(chroma):
    Case("nv12", 1080, 1920, "row", seed=1, chroma=chroma).check()            # 16-byte loads and stores at the real width


@pytest.mark.parametrize("fmt", ["nv12", "nv21", "i420", "p010"])
def test_kernel_with_a_pointer_offset_by_one_element_and_several_frames(fmt):
    matrix, range_ = PAIRS[fmt][0]
    for H, W in ((5, 7), (33, 130), (35, 176), (7, 132)):
        Case(fmt, H, W, "256", shift=1, seed=3, matrix=matrix, range=range_, chroma="linear").check()
        Case(fmt, H, W, "row", shift=1, seed=4, matrix=matrix, range=range_, chroma="nearest").check()
    for n in (3, 16):
        Case(fmt, 33, 130, "256", n=n, seed=n, matrix=matrix, range=range_, chroma="linear").check()
        Case(fmt, 6, 16, "row", n=n, seed=n + 1, matrix=matrix, range=range_, chroma="nearest").check()


def test_refusals_launch_nothing():
    from countr_amd import _lib, yuv as Y
    L = _lib.yuv_lib()
    y, c = torch.zeros(4 * 6, dtype=torch.uint8, device="cuda"), torch.full((2 * 6,), 128, dtype=torch.uint8, device="cuda")
    out = torch.full((4 * 6 * 3,), 7, dtype=torch.uint8, device="cuda")
    arr = lambda t: (C.c_void_p * 1)(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.countr_yuv_to_rgb(arr(y), arr(c), None, arr(out), 1, 4, 6, 5, 6, 0, 1, 0, 0, st) < 0 and "pitch_y 5" in L.countr_yuv_last_error().decode()
    assert L.countr_yuv_to_rgb(arr(y), arr(c), arr(c), arr(out), 1, 4, 6, 6, 6, 0, 1, 0, 0, st) < 0 and "c1 must be NULL" in L.countr_yuv_last_error().decode()
    assert L.countr_yuv_to_rgb(arr(y), arr(c), None, arr(out), 1, 4, 6, 6, 6, 9, 1, 0, 0, st) < 0 and "unknown format 9" in L.countr_yuv_last_error().decode()
    with pytest.raises(_lib.CountrError, match="unknown format 9"):
        _lib.yuv_check(-1, "countr_yuv_to_rgb")
    torch.cuda.synchronize()
    assert bool((out == 7).all())
    assert L.countr_yuv_to_rgb(arr(y), arr(c), None, arr(out), 1, 4, 6, 6, 6, 0, 1, 0, 0, st) == 0
    torch.cuda.synchronize()
    assert bool((out == 0).all())                                 # (Y = 0 with neutral chroma is below black under the limited range)
    assert Y.MAX_FRAMES == 16


# ---- 2. end to end on the tiny configuration
def make_model(precision):
    import torch.nn as nn
    from countr_amd.models_mae_cross import SupervisedMAE
    p, D, depth, H, Dd, ddepth, Hd = W.CONFIGS["tiny_test"]
    m = SupervisedMAE(patch_size=p, embed_dim=D, depth=depth, num_heads=H, decoder_embed_dim=Dd, decoder_depth=ddepth, decoder_num_heads=Hd,
                      mlp_ratio=4, norm_layer=partial(nn.LayerNorm, eps=1e-6), precision=precision)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.make_state_dict("tiny_test", seed=3).items()}, strict=True)
    return m.to("cuda").eval()


@pytest.fixture(scope="module", params=["fp32", "bf16"])
def model(request):
    return make_model(request.param)


def random_frame(fmt, H, W, seed, **kw):
    from countr_amd import YuvFrame
    rs = np.random.RandomState(seed)
    planes = []
    for rows, row in rows_of(fmt, H, W):
        if fmt == "p010":
            planes.append((rs.randint(0, 1024, (rows, row // 2)) << 6).astype(np.uint16))
        else:
            planes.append(rs.randint(0, 256, (rows, row)).astype(np.uint8))
    return YuvFrame(*planes, format=fmt, **kw)


def frames_and_boxes():
    """Two frames of the shapes of tests/test_regions_gpu.py.  Frame 0: exemplars under 10 px in the resized image -> the 3 x 3 split;
    frame 1: large exemplars."""
    fr = [random_frame("nv12", 60, 90, 21), random_frame("i420", 48, 120, 22, matrix="bt601", range="full", chroma="linear")]
    boxes = [[(10, 10, 11, 11), (40, 20, 41, 21), (70, 40, 71, 41)], [(5, 5, 30, 30), (50, 10, 80, 40), (90, 8, 115, 36)]]
    return fr, boxes


def rgb_of(frames):
    from countr_amd import YuvFrame, yuv_host
    return [yuv_host(f) if isinstance(f, YuvFrame) else f for f in frames]


def same_counts(got, want):
    assert len(got) == len(want)
    for (c0, d0), (c1, d1) in zip(got, want):
        assert c0 == c1 and d0.dtype == d1.dtype and torch.equal(d0, d1)


@pytest.mark.parametrize("shots", [0, 3])
def test_count_frames_equals_the_call_on_yuv_host(model, shots):
    from countr_amd import count_frames, frames as FR
    fr, boxes = frames_and_boxes()
    boxes = boxes if shots else None
    want = count_frames(model, rgb_of(fr), boxes)
    same_counts(count_frames(model, fr, boxes), want)
    if shots:                                                     # frame 0 takes the 3 x 3 split, frame 1 does not
        crops = [cr for _c, _d, cr in FR.count_items_crops(model, FR.prepare_items("cuda", fr, boxes))]
        assert [cr is not None for cr in crops] == [True, False]
    assert any(float(d.abs().sum()) > 0 for _c, d in want)


def test_zoom_2_on_a_96_x_80_frame(model):
    from countr_amd import count_frames
    f = random_frame("nv21", 96, 80, 23, chroma="linear")
    boxes = [[(10, 10, 30, 30), (40, 20, 60, 45), (5, 50, 25, 80)]]
    want = count_frames(model, rgb_of([f]), boxes, zoom=2)
    assert tuple(want[0][1].shape) == (768, 640)
    same_counts(count_frames(model, [f], boxes, zoom=2), want)


def test_locate_regions_and_classes(model):
    from countr_amd import count_classes, count_regions, locate_frames
    fr, boxes = frames_and_boxes()
    rgb = rgb_of(fr)
    for a, b in zip(locate_frames(model, fr, boxes), locate_frames(model, rgb, boxes)):
        assert len(a) == len(b) == 4 and a[0] == b[0] and torch.equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    grid = [("grid", 2, 3)]
    for a, b in zip(count_regions(model, fr, grid, boxes), count_regions(model, rgb, grid, boxes)):
        assert a[0] == b[0] and torch.equal(a[1], b[1]) and a[2].shape == (6,) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    classes = {"things": boxes, "anything": None}
    for a, b in zip(count_classes(model, fr, classes), count_classes(model, rgb, classes)):
        assert a.names == b.names == ("things", "anything") and a.counts == b.counts
        assert all(torch.equal(x, y) for x, y in zip(a.maps, b.maps))
        assert (a.labels is None) == (b.labels is None)
        if a.labels is not None:
            assert torch.equal(a.labels, b.labels) and np.array_equal(a.won, b.won) and np.array_equal(a.total, b.total) and np.array_equal(a.area, b.area)


def test_a_mixed_call_and_a_steady_stream_allocates_no_converter_buffers(model):
    from countr_amd import YuvFrame, count_frames, frames as FR
    rgb = np.random.RandomState(31).randint(0, 256, (60, 90, 3)).astype(np.uint8)
    host = random_frame("nv12", 60, 90, 32)
    src = random_frame("nv12", 60, 90, 33, matrix="bt601", range="full", chroma="linear")
    wide_y, wide_c = torch.full((60, 256), 0x5A, dtype=torch.uint8, device="cuda"), torch.full((30, 256), 0x5A, dtype=torch.uint8, device="cuda")
    wide_y[:, :90], wide_c[:, :90] = torch.from_numpy(src.y).cuda(), torch.from_numpy(src.c0).cuda()
    dev = YuvFrame(wide_y[:, :90], wide_c[:, :90], format="nv12", matrix="bt601", range="full", chroma="linear")
    assert dev.is_cuda and dev.y.stride(0) == 256
    ten = random_frame("p010", 50, 76, 34)
    mixed = [rgb, host, dev, ten]
    want = count_frames(model, [rgb] + rgb_of([host, src, ten]))
    same_counts(count_frames(model, mixed), want)
    conv = FR.frame_prep("cuda").yuv
    before = conv.buffers()
    assert len(before) >= 2 + 2 + 3                              # two staged frames (host + device copy each), three rgb buffers
    same_counts(count_frames(model, mixed), want)
    assert conv.buffers() == before
    # the same frames on another stream: FramePrep's guard orders the reuse of the buffers
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = count_frames(model, mixed)
    side.synchronize()
    same_counts(got, want)
    same_counts(count_frames(model, mixed), want)
    assert conv.buffers() == before


def test_converter_refusals():
    from countr_amd import YuvConverter, YuvFrame, _lib
    with pytest.raises(_lib.CountrError, match="no CPU fallback"):
        YuvConverter("cpu")
    conv = YuvConverter("cuda")
    with pytest.raises(ValueError, match="a YuvFrame is required"):
        conv.convert([np.zeros((4, 4, 3), np.uint8)])
    with pytest.raises(ValueError, match="all on the host or all on one device"):
        YuvFrame(torch.zeros(4, 6, dtype=torch.uint8, device="cuda"), torch.zeros(2, 6, dtype=torch.uint8))
    seventeen = [random_frame("nv12", 6, 8, 40 + k) for k in range(17)]        # two launches: 16 + 1
    for f, t in zip(seventeen, conv.convert(seventeen)):
        assert np.array_equal(t.cpu().numpy(), rgb_of([f])[0])


# ---- 3. the demo in a fresh child process
def test_demo_zero_cli_on_a_raw_clip(tmp_path):
    from PIL import Image
    import models_mae_cross
    from countr_amd import YuvFrame, count_frames
    Wd, H = 80, 96
    size = Wd * H * 3 // 2
    raw = np.random.RandomState(5).randint(0, 256, 3 * size).astype(np.uint8)
    clip = tmp_path / "clip.yuv"
    clip.write_bytes(raw.tobytes())
    out = tmp_path / "out"
    cmd = [sys.executable, "demo_zero.py", "--yuv", "nv12:80x96", "--model_path", "", "--output_path", str(out)]
    r = subprocess.run(cmd + ["--input_path", str(clip)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = re.findall(r"^clip#(\d+): Count: (\S+) - Time: \S+$", r.stdout, re.M)
    assert [int(k) for k, _c in lines] == [0, 1, 2], r.stdout
    torch.manual_seed(0)                                          # the demo's model for --model_path ""
    m = models_mae_cross.__dict__["mae_vit_base_patch16"](norm_pix_loss="store_true", precision="bf16").to("cuda").eval()
    frames = [YuvFrame.from_buffer(raw[k * size:(k + 1) * size], Wd, H) for k in range(3)]
    want = count_frames(m, frames, normalization=False)
    assert [float(c) for _k, c in lines] == [float(c) for c, _dm in want]
    for k in range(3):
        assert Image.open(out / ("viz_clip_%d.jpg" % k)).size == (Wd, H)
    # --max_frames reads the head of the clip; a truncated clip is an error, not a shorter run
    short = tmp_path / "short.yuv"
    short.write_bytes(raw.tobytes()[:-7])
    r = subprocess.run(cmd + ["--input_path", str(short), "--no_viz"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "incomplete frame of %d bytes" % (size - 7) in r.stderr, r.stdout[-2000:] + r.stderr[-3000:]
