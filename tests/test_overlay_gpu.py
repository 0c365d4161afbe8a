"""GPU: countr_overlay_render (csrc_overlay/overlay.hip) through countr_amd.Overlay against countr_amd.overlay_host, byte for byte -- behind
the heat's two fp32 roundings the rule is integer arithmetic, so there is no tolerance -- and annotate_frames on the tiny model: counts,
maps and points are the existing entry points', the picture is overlay_host of the same inputs."""
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
OUTS = ("rgb", "nv12", "nv21", "i420")
SPACES = [(m, r) for m in ("bt601", "bt709") for r in ("limited", "full")]
GUARD = 64


def random_map(rs, mh, mw):
    """Values around the levels' range, with negatives, a NaN, an infinity-free saturating value and an exact zero."""
    m = (rs.standard_normal((mh, mw)) * 1.2).astype(np.float32)
    m[rs.randint(mh), rs.randint(mw)] = np.nan
    m[rs.randint(mh), rs.randint(mw)] = 1e6
    m[0, 0] = 0.0
    m[mh - 1, mw - 1] = -3.0
    return m


def on_device(frame, shift):
    """The frame on the device, its first byte `shift` bytes behind a 16-byte boundary."""
    buf = torch.zeros(16 + frame.size + 16, dtype=torch.uint8, device="cuda")
    view = buf[16 + shift:16 + shift + frame.size].view(frame.shape)
    view.copy_(torch.from_numpy(frame))
    assert view.data_ptr() % 16 == shift
    return view


def guarded(ov, H, W, out, n, shift):
    """Give the Overlay output buffers of our own for n frames of (H, W): each inside a larger buffer filled with a sentinel."""
    from countr_amd import overlay as O
    sizes = {"_rgb": H * W * 3, "_yuv": O.frame_bytes(out, W, H)}
    bigs = []
    for name, size in sizes.items():
        views = []
        for _ in range(n):
            big = torch.full((GUARD + size + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
            v = big[GUARD + shift:GUARD + shift + size]
            views.append(v.view(H, W, 3) if name == "_rgb" else v)
            bigs.append((big, GUARD + shift, size))
        getattr(ov, name)[(H, W)] = views
    return bigs


def unharmed(bigs):
    for big, lead, size in bigs:
        b = big.cpu().numpy()
        assert (b[:lead] == 0xA5).all() and (b[lead + size:] == 0xA5).all(), "bytes outside an output buffer were written"


def same(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s: %d bytes differ, first at %s: %d, want %d" % (what, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


# ---- 1. the kernels against the host rule
# (H, W, mh, mw, shift): both sides odd with an upscale; a downscale; a width that is a multiple of 16 on aligned pointers (the 16-byte
# loads and stores); the same with every pointer one byte behind a 16-byte boundary (element-wise); a strong downscale, whose block
# reads more of the map than it stages in LDS (the direct loads), and the same frame on either side of that threshold of 8192 map pixels
SHAPES = [(37, 53, 24, 40, 0), (19, 23, 48, 64, 0), (48, 64, 24, 40, 0), (48, 64, 24, 40, 1), (8, 40, 200, 300, 0), (8, 40, 100, 91, 0),
          (8, 40, 101, 92, 0)]


def test_the_shapes_lie_on_both_sides_of_the_staging_threshold():
    """A frame of at most 1024 x 8 pixels is one block of the composition; the block stages the map rectangle its taps span."""
    from countr_amd import overlay as O

    def rectangle(H, W, mh, mw):
        (x0, x1, _fx), (y0, y1, _fy) = O.axis_host(W, mw), O.axis_host(H, mh)
        return int((x1[-1] - x0[0] + 1) * (y1[-1] - y0[0] + 1))
    assert [rectangle(*s[:4]) for s in SHAPES[4:]] == [294 * 177, 8190, 92 * 91]
    assert all(rectangle(*s[:4]) <= 8192 for s in SHAPES[:4])


@pytest.mark.parametrize("H,W,mh,mw,shift", SHAPES)
def test_kernels_equal_overlay_host(H, W, mh, mw, shift):
    from countr_amd import Overlay, overlay_host
    rs = np.random.RandomState(H * 100 + W + shift)
    frame = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
    m = random_map(rs, mh, mw)
    pts = rs.uniform(-3, max(H, W) + 3, (9, 2))
    polys = [[(2.4, 3.6), (W - 3.0, 5.2), (W / 2.0, H - 2.5)], [(-5.0, H / 2.0), (W + 6.0, H / 2.0 + 3)]]
    lab = (rs.randint(0, 256, (9, 21)).astype(np.uint8), W - 12, H - 5)
    ov = Overlay("cuda")
    dev, dm = on_device(frame, shift), torch.from_numpy(m).cuda()
    n = 0
    for out in OUTS:
        for matrix, range_ in SPACES:
            for gain, cmap in ((3.0, "red"), ("max", "heat")):
                kw = dict(gain=gain, colormap=cmap, point_radius=1 + n % 3, out=out, matrix=matrix, range=range_)
                bigs = guarded(ov, H, W, out, 1, shift)
                got = ov.render([dev], [dm], points=[pts], regions=[polys], labels=[lab], **kw)[0]
                torch.cuda.synchronize()
                same(got, overlay_host(frame, m, points=pts, regions=polys, label=lab, **kw), "%s %s %s gain %s" % (out, matrix, range_, gain))
                unharmed(bigs)
                n += 1
    assert n == 32
    # without marks, on a map with nothing above 0 (gain "max" is then 0: the frame comes back), and with a colour table of the caller's
    flat = torch.full((mh, mw), -1.0, device="cuda")
    same(ov.render([dev], [flat], gain="max")[0], frame, "nothing above 0")
    lut = rs.randint(0, 256, (256, 4)).astype(np.uint8)
    same(ov.render([dev], [dm], gain=40.0, colormap=lut)[0], overlay_host(frame, m, gain=40.0, colormap=lut), "own table")
    lut[:, 3] = 0
    same(ov.render([dev], [dm], gain=40.0, colormap=lut)[0], frame, "all-zero alpha")
    # a 16-bit map is widened exactly
    half = torch.from_numpy(m).cuda().bfloat16()
    same(ov.render([dev], [half], gain=3.0)[0], overlay_host(frame, half.float().cpu().numpy(), gain=3.0), "bf16 map")


def test_three_frames_with_their_own_gains_and_marks_and_seventeen_frames_in_two_calls():
    from countr_amd import Overlay, overlay_host
    rs = np.random.RandomState(7)
    H, W, mh, mw = 21, 34, 12, 20
    frames = [rs.randint(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(17)]
    maps = [random_map(rs, mh, mw) for _ in range(17)]
    gains = [2.0, "max", 0.0]
    points = [rs.uniform(0, 20, (5, 2)), None, rs.uniform(0, 20, (1, 2))]
    regions = [None, [[(1, 1), (30, 4), (12, 18)]], [[(3, 3)]]]
    labels = [(rs.randint(0, 256, (4, 6)).astype(np.uint8), 2, 3), None, None]
    ov = Overlay("cuda")
    dev, dms = [torch.from_numpy(f).cuda() for f in frames], [torch.from_numpy(m).cuda() for m in maps]
    for out in ("rgb", "i420"):
        got = ov.render(dev[:3], dms[:3], gain=gains, colormap="heat", points=points, regions=regions, labels=labels, out=out)
        for k in range(3):
            same(got[k], overlay_host(frames[k], maps[k], gain=gains[k], colormap="heat", points=points[k], regions=regions[k], label=labels[k],
                                      out=out), "frame %d of three, %s" % (k, out))
    gains17 = [float(k) for k in range(17)]
    got = ov.render(dev, dms, gain=gains17, out="nv12", matrix="bt601", range="full")
    assert len(ov._packs) == 2                                      # 16 + 1
    for k in range(17):
        same(got[k], overlay_host(frames[k], maps[k], gain=gains17[k], out="nv12", matrix="bt601", range="full"), "frame %d of seventeen" % k)
    # frames of two shapes and a frame without a map in one render
    other = rs.randint(0, 256, (10, 7, 3)).astype(np.uint8)
    got = ov.render([dev[0], torch.from_numpy(other).cuda(), dev[1]], [dms[0], dms[1], None], labels=[None, None, labels[0]])
    same(got[0], overlay_host(frames[0], maps[0]), "mixed 0")
    same(got[1], overlay_host(other, maps[1]), "mixed 1")
    same(got[2], overlay_host(frames[1], None, label=labels[0]), "mixed 2, no heat")


def test_marks_at_their_limits_and_the_drawing_order():
    from countr_amd import Overlay, overlay_host
    rs = np.random.RandomState(11)
    H, W = 70, 90
    frame = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
    m = rs.uniform(0, 1, (16, 24)).astype(np.float32)
    pts = rs.uniform(-20, 110, (4096, 2))                                           # some centres outside the frame
    polys = [rs.uniform(-15, 105, (64, 2)) for _ in range(64)]
    lab = (rs.randint(0, 256, (64, 256)).astype(np.uint8), W - 40, H - 30)           # hangs over the right and bottom edges
    ov = Overlay("cuda")
    dev, dm = torch.from_numpy(frame).cuda(), torch.from_numpy(m).cuda()
    for r in (0, 16):
        got = ov.render([dev], [dm], points=[pts], point_radius=r, regions=[polys], labels=[lab])[0]
        same(got, overlay_host(frame, m, points=pts, point_radius=r, regions=polys, label=lab), "marks at the limits, r = %d" % r)
    # all three kinds on one pixel: the label under the outline under the point
    solid = (np.full((8, 8), 255, np.uint8), 10, 10)
    args = dict(labels=[solid], regions=[[[(8, 12), (20, 12)]]], points=[[(12, 12)]], point_radius=0)
    got = ov.render([dev], [dm], **args)[0].cpu().numpy()
    assert tuple(got[11, 12]) == (255, 255, 255) and tuple(got[12, 13]) == (255, 255, 0) and tuple(got[12, 12]) == (0, 255, 0)
    same(ov.render([dev], [dm], **args)[0], overlay_host(frame, m, label=solid, regions=args["regions"][0], points=[(12, 12)], point_radius=0), "order")
    # two runs of one call give the same bytes
    a = ov.render([dev], [dm], gain="max", points=[pts], regions=[polys], labels=[lab], out="nv12")[0].clone()
    b = ov.render([dev], [dm], gain="max", points=[pts], regions=[polys], labels=[lab], out="nv12")[0]
    assert torch.equal(a, b)
    with pytest.raises(ValueError, match="at most 4096 points"):
        ov.render([dev], [dm], points=[np.zeros((4097, 2))])
    with pytest.raises(ValueError, match="1..64 vertices"):
        ov.render([dev], [dm], regions=[[np.zeros((65, 2))]])
    with pytest.raises(ValueError, match="at most 64 polygons"):
        ov.render([dev], [dm], regions=[[[(1, 1)]] * 65])
    with pytest.raises(ValueError, match="at most 64 x 256"):
        ov.render([dev], [dm], labels=[(np.zeros((65, 4), np.uint8), 0, 0)])


def test_a_refused_call_launches_nothing():
    import ctypes as C
    from countr_amd import _lib
    L = _lib.overlay_lib()
    frame = torch.full((4, 6, 3), 9, dtype=torch.uint8, device="cuda")
    out = torch.full((4, 6, 3), 7, dtype=torch.uint8, device="cuda")
    m = torch.ones(2, 3, device="cuda")
    pack = torch.zeros(1088, dtype=torch.uint8, device="cuda")
    rec = (_lib.OverlayFrame * 1)()
    rec[0].rgb, rec[0].map, rec[0].out = frame.data_ptr(), m.data_ptr(), out.data_ptr()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda fmt=0, H=4: L.countr_overlay_render(rec, 1, H, 6, 2, 3, pack.data_ptr(), 1088, 2, 0, 0, fmt, 1, 0, None, st)
    assert call(fmt=9) < 0 and "unknown format 9" in L.countr_overlay_last_error().decode()
    assert call(fmt=1) < 0 and "null pointer" in L.countr_overlay_last_error().decode()           # a 4:2:0 output without its buffer
    assert call(H=0) < 0
    torch.cuda.synchronize()
    assert bool((out == 7).all())
    assert call() == 0                                              # a zero table: the frame comes back
    torch.cuda.synchronize()
    assert bool((out == 9).all())


# ---- 2. end to end on the tiny configuration (the frames of tests/test_yuv_gpu.py)
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
    hc, wc = (H + 1) // 2, (W + 1) // 2
    shapes = [(H, W)] + ([(hc, wc), (hc, wc)] if fmt == "i420" else [(hc, 2 * wc)])
    return YuvFrame(*[rs.randint(0, 256, s).astype(np.uint8) for s in shapes], format=fmt, **kw)


def frames_and_boxes():
    """Frame 0: exemplars under 10 px in the resized image -> the 3 x 3 split; frame 1: large exemplars."""
    fr = [random_frame("nv12", 60, 90, 21), random_frame("i420", 48, 120, 22, matrix="bt601", range="full", chroma="linear")]
    boxes = [[(10, 10, 11, 11), (40, 20, 41, 21), (70, 40, 71, 41)], [(5, 5, 30, 30), (50, 10, 80, 40), (90, 8, 115, 36)]]
    return fr, boxes


@pytest.mark.parametrize("shots", [0, 3])
def test_annotate_frames(model, shots):
    from countr_amd import YuvFrame, annotate_frames, count_frames, locate_frames, overlay as O, overlay_host, yuv_host
    fr, boxes = frames_and_boxes()
    boxes = boxes if shots else None
    polys = [[(5.0, 5.0), (70.5, 8.0), (40.0, 44.0)]]
    counted = count_frames(model, fr, boxes)
    located = locate_frames(model, fr, boxes)
    for out in ("rgb", "nv12"):
        got = annotate_frames(model, fr, boxes, out=out, points=True, regions=polys, gain="max", colormap="heat")
        assert len(got) == 2
        for k, (f, (c, dm, pic, pts, score)) in enumerate(zip(fr, got)):
            assert c == counted[k][0] and dm.dtype == counted[k][1].dtype and torch.equal(dm, counted[k][1])
            assert np.array_equal(pts, located[k][2]) and np.array_equal(score, located[k][3])
            H, Wd, _ = f.shape
            split = bool(shots) and k == 0                          # the frame on the 3 x 3 split: no heat, its marks
            want = overlay_host(yuv_host(f), None if split else dm.float().cpu().numpy(), gain="max", colormap="heat", points=pts, regions=polys,
                                label=O.count_label(c, Wd, H), out=out, matrix=f.matrix, range=f.range)
            same(pic, want, "frame %d %s" % (k, out))
            if split:                                               # without heat a pixel no mark touches is the frame's own
                plain = overlay_host(yuv_host(f), None)
                marked = overlay_host(yuv_host(f), None, points=pts, regions=polys, label=O.count_label(c, Wd, H))
                assert (marked != plain).any()
            if out == "nv12":                                       # a buffer YuvFrame.from_buffer accepts, straight back in
                back = YuvFrame.from_buffer(pic, Wd, H, format="nv12", matrix=f.matrix, range=f.range)
                assert back.is_cuda and back.shape == f.shape
    plainly = annotate_frames(model, fr, boxes, label=False)        # points=False: no points, no score, and nothing drawn but the heat
    for k, (c, dm, pic, pts, score) in enumerate(plainly):
        assert pts is None and score is None and c == counted[k][0]
        split = bool(shots) and k == 0
        same(pic, overlay_host(yuv_host(fr[k]), None if split else dm.float().cpu().numpy()), "heat only, frame %d" % k)


def test_annotate_frames_zoom_2_draws_from_the_768_high_map(model):
    from countr_amd import annotate_frames, count_frames, overlay as O, overlay_host, yuv_host
    f = random_frame("nv21", 96, 80, 23, chroma="linear")
    boxes = [[(10, 10, 30, 30), (40, 20, 60, 45), (5, 50, 25, 80)]]
    want = count_frames(model, [f], boxes, zoom=2)
    (c, dm, pic, pts, score), = annotate_frames(model, [f], boxes, zoom=2, points=True, out="nv21")
    assert tuple(dm.shape) == (768, 640) and c == want[0][0] and torch.equal(dm, want[0][1])
    same(pic, overlay_host(yuv_host(f), dm.float().cpu().numpy(), points=pts, label=O.count_label(c, 80, 96), out="nv21"), "zoom 2")


def test_a_steady_stream_allocates_no_buffers(model):
    from countr_amd import annotate_frames, frames as FR, overlay as O
    rgb = np.random.RandomState(31).randint(0, 256, (60, 90, 3)).astype(np.uint8)
    mixed = [rgb, random_frame("nv12", 60, 90, 32), random_frame("i420", 50, 76, 34)]
    first = [(c, pic.clone()) for c, _dm, pic, _p, _s in annotate_frames(model, mixed, points=True, out="nv12")]
    prep, ov = FR.frame_prep("cuda"), O.overlay_for("cuda")
    slots = lambda: sorted([s.dev.data_ptr() for v in prep._slots.values() for s in v] + [s.host.data_ptr() for v in prep._slots.values() for s in v])
    before = (ov.buffers(), prep.yuv.buffers(), slots())
    assert len(before[0]) >= 3 + 1 + 3 + 3 and len(before[2]) >= 2
    again = annotate_frames(model, mixed, points=True, out="nv12")
    assert (ov.buffers(), prep.yuv.buffers(), slots()) == before
    for (c0, p0), (c1, _dm, p1, _p, _s) in zip(first, again):
        assert c0 == c1 and torch.equal(p0, p1)
    side = torch.cuda.Stream()                                      # another stream: the guards order the reuse of the buffers
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = annotate_frames(model, mixed, points=True, out="nv12")
    side.synchronize()
    for (c0, p0), (c1, _dm, p1, _p, _s) in zip(first, got):
        assert c0 == c1 and torch.equal(p0, p1)
    assert (ov.buffers(), prep.yuv.buffers(), slots()) == before


def test_device_frames_is_the_front_part_of_prepare():
    from countr_amd import FramePrep, yuv_host
    prep = FramePrep("cuda")
    rgb = np.random.RandomState(3).randint(0, 256, (20, 30, 3)).astype(np.uint8)
    y = random_frame("nv12", 20, 30, 4)
    on = torch.from_numpy(rgb).cuda()
    want = [t.clone() for t in prep.prepare([rgb, y, on])]
    dev = prep.device_frames([rgb, y, on])
    assert dev[2] is on and np.array_equal(dev[0].cpu().numpy(), rgb) and np.array_equal(dev[1].cpu().numpy(), yuv_host(y))
    for a, b in zip(prep.prepare(dev), want):
        assert torch.equal(a, b)


# ---- 3. the demo in a fresh child process
def test_demo_zero_cli_writes_the_annotated_clip(tmp_path):
    import models_mae_cross
    from PIL import Image
    from countr_amd import YuvFrame, locate_frames, overlay as O, overlay_host, yuv_host
    Wd, H = 80, 96
    size = Wd * H * 3 // 2
    raw = np.random.RandomState(5).randint(0, 256, 4 * size).astype(np.uint8)
    clip = tmp_path / "clip.yuv"
    clip.write_bytes(raw.tobytes())
    cmd = [sys.executable, "demo_zero.py", "--yuv", "nv12:80x96", "--model_path", "", "--input_path", str(clip)]
    plain = subprocess.run(cmd + ["--output_path", str(tmp_path / "a"), "--no_viz"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert plain.returncode == 0, plain.stdout[-2000:] + plain.stderr[-3000:]
    ann = tmp_path / "annotated.yuv"
    r = subprocess.run(cmd + ["--output_path", str(tmp_path / "b"), "--out_yuv", str(ann) + ":i420", "--points", "--device_viz"], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    pattern = r"^(clip#\d+: Count: \S+) - Time: \S+$"
    lines = re.findall(pattern, r.stdout, re.M)
    assert len(lines) == 4 and lines == re.findall(pattern, plain.stdout, re.M)
    got = np.fromfile(ann, np.uint8)
    assert got.size == 4 * size
    torch.manual_seed(0)                                            # the demo's model for --model_path ""
    m = models_mae_cross.__dict__["mae_vit_base_patch16"](norm_pix_loss="store_true", precision="bf16").to("cuda").eval()
    frames = [YuvFrame.from_buffer(raw[k * size:(k + 1) * size], Wd, H) for k in range(4)]
    for k, (f, (c, dm, pts, _score)) in enumerate(zip(frames, locate_frames(m, frames, normalization=False))):
        want = overlay_host(yuv_host(f), dm.float().cpu().numpy(), points=pts, label=O.count_label(c, Wd, H), out="i420")
        assert np.array_equal(got[k * size:(k + 1) * size], want), "frame %d" % k
        assert Image.open(tmp_path / "b" / ("viz_clip_%d.jpg" % k)).size == (Wd, H) and (tmp_path / "b" / ("points_clip_%d.json" % k)).exists()
