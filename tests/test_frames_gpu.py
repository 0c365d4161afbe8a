"""GPU: the raw-frame path -- countr_frame_resize_u8 against PIL + ToTensor (bit for bit), countr_crop_resize_f32 against
F.interpolate on the CPU, count_frames against inference.count_images fed with host-prepared tensors, and the two demo CLIs."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

from oracle import weights as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pil_path(frame, ow, oh=384):
    """What demo_zero.load_image does to a decoded frame."""
    im = Image.fromarray(frame).resize((ow, oh), Image.BILINEAR)
    return torch.from_numpy(np.asarray(im, dtype=np.uint8).copy()).permute(2, 0, 1).float().div(255)


def make_frames(H, W, seed=0):
    rs = np.random.RandomState(seed + H * 31 + W)
    noise = rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    ramp = np.stack([xx * 255.0 / (W - 1), yy * 255.0 / (H - 1), (xx + yy) * 255.0 / (W + H - 2)], 2).astype(np.uint8)
    return noise, ramp


def raw_resize(hip, frames_dev, oh, ow, stream=None):
    """countr_frame_resize_u8 through ctypes with tables and workspace made here."""
    from countr_amd.frames import pil_tables
    H, Wd = frames_dev[0].shape[:2]
    _k, hb, hw = pil_tables(Wd, ow)
    _k, vb, vw = pil_tables(H, oh)
    hb, hw, vb, vw = (torch.from_numpy(t).cuda() for t in (hb, hw, vb, vw))
    n = len(frames_dev)
    tmp = torch.empty(n, H, ow, 3, dtype=torch.uint8, device="cuda")
    outs = [torch.full((3, oh, ow), -1.0, device="cuda") for _ in range(n)]
    torch.cuda.synchronize()
    st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
    rc = hip.countr_frame_resize_u8((C.c_void_p * n)(*[f.data_ptr() for f in frames_dev]), (C.c_void_p * n)(*[o.data_ptr() for o in outs]),
                                    n, H, Wd, oh, ow, hb.data_ptr(), hw.data_ptr(), vb.data_ptr(), vw.data_ptr(), tmp.data_ptr(), st)
    assert rc == 0, hip.countr_last_error()
    torch.cuda.synchronize()
    return outs


@pytest.mark.parametrize("W_,H_", [(1920, 1080), (640, 427), (300, 500), (1000, 384)])
def test_frame_resize_equals_pil_bit_for_bit(hip, W_, H_):
    from countr_amd.frames import FramePrep, new_width
    prep = FramePrep("cuda")
    ow = new_width(W_, H_)
    frames = list(make_frames(H_, W_))
    got = prep.prepare(frames)                                   # host frames: pinned staging + device resize, both in one launch pair
    got_dev = prep.prepare([torch.from_numpy(f).cuda() for f in frames])
    torch.cuda.synchronize()
    for f, g, gd in zip(frames, got, got_dev):
        want = pil_path(f, ow)
        assert g.shape == (1, 3, 384, ow) and g.dtype == torch.float32
        assert torch.equal(g[0].cpu(), want) and torch.equal(gd[0].cpu(), want)


def test_frame_resize_scalar_path_odd_width(hip):
    """out_w % 4 != 0 (and a frame pointer that is not 16-byte aligned): the element-wise kernels, through the raw export."""
    H_, W_, oh, ow = 200, 301, 150, 133
    for f in make_frames(H_, W_):
        want = torch.from_numpy(np.asarray(Image.fromarray(f).resize((ow, oh), Image.BILINEAR)).copy()).permute(2, 0, 1).float().div(255)
        got = raw_resize(hip, [torch.from_numpy(f).cuda()], oh, ow)[0]
        assert torch.equal(got.cpu(), want)
        buf = torch.empty(H_ * W_ * 3 + 1, dtype=torch.uint8, device="cuda")
        buf[1:].copy_(torch.from_numpy(f).cuda().view(-1))
        got = raw_resize(hip, [buf[1:].view(H_, W_, 3)], oh, ow)[0]
        assert torch.equal(got.cpu(), want)


def test_frame_resize_wide_frame_halves_the_horizontal_tile(hip):
    """2400 -> 100 columns: scale 24 and 49 taps, so 256 output pixels would stage (ceil(24 * 255) + 49 + 1) * 3 + 48 = 18 558 bytes of a
    row and the 16 384-byte staging buffer takes 128 per work item instead -- with 16-byte loads (aligned frame) and without."""
    H_, W_, oh, ow = 8, 2400, 4, 100
    for f in make_frames(H_, W_):
        want = pil_path(f, ow, oh)
        got = raw_resize(hip, [torch.from_numpy(f).cuda()], oh, ow)[0]
        assert torch.equal(got.cpu(), want)
        buf = torch.empty(H_ * W_ * 3 + 1, dtype=torch.uint8, device="cuda")
        buf[1:].copy_(torch.from_numpy(f).cuda().view(-1))
        got = raw_resize(hip, [buf[1:].view(H_, W_, 3)], oh, ow)[0]
        assert torch.equal(got.cpu(), want)


def test_frame_resize_batched_eight_and_side_stream(hip):
    from countr_amd.frames import FramePrep
    frames = [make_frames(1080, 1920, seed=k)[0] for k in range(7)] + [make_frames(1080, 1920)[1]]
    want = [pil_path(f, 672) for f in frames]
    got = raw_resize(hip, [torch.from_numpy(f).cuda() for f in frames], 384, 672)
    for g, w in zip(got, want):
        assert torch.equal(g.cpu(), w)
    prep = FramePrep("cuda")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = prep.prepare(frames)
    side.synchronize()
    for g, w in zip(got, want):
        assert torch.equal(g[0].cpu(), w)
    got = prep.prepare(frames[:3])                               # back on the default stream: waits for the side stream's use of the buffers
    torch.cuda.synchronize()
    for g, w in zip(got, want):
        assert torch.equal(g[0].cpu(), w)


CROP_TOL = 1e-4     # absolute, values in [0, 1]: three times the ulp of an fp32 source coordinate in [256, 512) (2^-15) times a neighbour
                    # difference <= 1 -- two axes plus the blend's own rounding; 40 times below one uint8 step


def test_crop_resize_matches_interpolate_on_cpu(hip):
    """The bar is F.interpolate on the CPU in fp32 within CROP_TOL; the comparison with torch's GPU result is printed, not asserted."""
    from countr_amd.frames import crop_resize, split_rects
    rs = np.random.RandomState(5)
    img = torch.from_numpy(rs.uniform(0, 1, size=(1, 3, 384, 560)).astype(np.float32))
    dev = img.cuda()
    # inclusive rectangles of 1x1, 3x40, 9x9, 37x30, 200x150 pixels, one touching the right and bottom borders, one reaching past them
    rects = [[10, 20, 10, 20], [5, 7, 7, 46], [100, 200, 108, 208], [50, 300, 86, 329], [120, 40, 319, 189], [300, 500, 383, 559],
             [350, 520, 400, 600]]
    got = crop_resize(dev, rects, 64, 64).cpu()
    assert got.shape == (len(rects), 3, 64, 64)
    for k, (y1, x1, y2, x2) in enumerate(rects):
        want = F.interpolate(img[:, :, y1:y2 + 1, x1:x2 + 1], size=(64, 64), mode="bilinear", align_corners=False)[0]
        err = (got[k] - want).abs().max().item()
        on_gpu = F.interpolate(dev[:, :, y1:y2 + 1, x1:x2 + 1], size=(64, 64), mode="bilinear", align_corners=False)[0].cpu()
        print("crop %s: max abs err %.3e (equal to torch on the GPU: %s)" % ((y1, x1, y2, x2), err, torch.equal(got[k], on_gpu)))
        assert err <= CROP_TOL, (rects[k], err)
    nine = crop_resize(dev, split_rects(384, 560), 384, 560).cpu()
    for k, (top, left, y2, x2) in enumerate(split_rects(384, 560)):
        assert (y2 - top + 1, x2 - left + 1) == (128, 186)
        want = F.interpolate(img[:, :, top:top + 128, left:left + 186], size=(384, 560), mode="bilinear", align_corners=False)[0]
        err = (nine[k] - want).abs().max().item()
        print("split crop %d: max abs err %.3e" % (k, err))
        assert err <= CROP_TOL, (k, err)
    # an output width that is not a multiple of 4: the element-wise kernel
    got = crop_resize(dev, rects[3:5], 30, 45).cpu()
    for k, (y1, x1, y2, x2) in enumerate(rects[3:5]):
        want = F.interpolate(img[:, :, y1:y2 + 1, x1:x2 + 1], size=(30, 45), mode="bilinear", align_corners=False)[0]
        assert (got[k] - want).abs().max().item() <= CROP_TOL


def _model(precision):
    import models_mae_cross
    m = models_mae_cross.mae_vit_base_patch16(precision=precision)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.make_state_dict("mae_vit_base_patch16", seed=0).items()})
    return m.to("cuda").eval()


@pytest.fixture(scope="module", params=["fp32", "bf16"])
def model(request):
    return _model(request.param)


def host_items(frames):
    """demo_zero.load_image + the hand-over of demo_zero.main, from decoded frames."""
    from countr_amd.frames import new_width
    return [(pil_path(f, new_width(f.shape[1], f.shape[0])).unsqueeze(0).cuda(), torch.Tensor([]).unsqueeze(0).cuda(), None) for f in frames]


def same(res, ref):
    assert len(res) == len(ref)
    for (c, dm), (rc, rdm) in zip(res, ref):
        assert c == rc and torch.equal(dm, rdm)


def test_count_frames_zero_shot_equals_host_prepared_path(model):
    from countr_amd import count_frames, inference
    eight = [make_frames(1080, 1920, seed=k)[0] for k in range(8)]                   # one native forward of 32 windows
    same(count_frames(model, eight, normalization=False), inference.count_images(model, host_items(eight), normalization=False))
    mixed = [make_frames(H_, W_, seed=9)[k % 2] for k, (W_, H_) in enumerate([(1920, 1080), (640, 427), (1000, 384), (640, 427), (1280, 720)])]
    same(count_frames(model, mixed), inference.count_images(model, host_items(mixed)))
    same(count_frames(model, mixed, boxes=[[]] * 5), inference.count_images(model, host_items(mixed)))      # empty box lists = zero-shot


def test_count_frames_few_shot_plumbing(model):
    from countr_amd import count_frames, frames as FR, inference
    fs = [make_frames(1080, 1920, seed=20)[0], make_frames(427, 640, seed=21)[0], make_frames(720, 1280, seed=22)[1]]
    three = [(136, 98, 173, 127), (209, 125, 242, 150), (212, 168, 258, 200)]
    for boxes in ([three] * 3, [three[:1]] * 3, [three, [], three[:1]]):
        res = count_frames(model, fs, boxes)
        items = FR.prepare_items("cuda", fs, boxes)               # the same device-made images, exemplars and rects
        for (im, ex, rects), f, bx in zip(items, fs, boxes):
            assert ex.shape == ((1, len(bx), 3, 64, 64) if bx else (1, 0))
            assert rects == (FR.scale_boxes(bx, f.shape[1], f.shape[0]) if bx else None)
        same(res, inference.count_images(model, items))
    # tiny exemplars (under 10 pixels after scaling): the 3 x 3 split, restated with the nine device-made crops
    small = [[(400, 300, 420, 318), (500, 500, 521, 520), (212, 168, 258, 200)]]
    (cnt, dm), = count_frames(model, fs[:1], small)
    (im, ex, rects), = FR.prepare_items("cuda", fs[:1], small)
    assert inference._small_exemplars(rects) == 2
    dms = inference.density_maps(model, FR.split_crops(im), [ex] * 9, 3)
    pred = sum((d.sum() / 60).item() for d in dms)
    assert cnt == inference._normalise(pred, dms[-1], rects, True) and torch.equal(dm, dms[-1])
    (cnt1, _), = count_frames(model, fs[:1], small, max_s_cnt=3)          # fewer small exemplars than max_s_cnt: no split
    (ref1, _), = inference.count_images(model, [(im, ex, rects)], max_s_cnt=3)
    assert cnt1 == ref1 and cnt1 != cnt


def test_count_frames_reuses_its_buffers(model):
    from countr_amd import count_frames
    fs = [make_frames(1080, 1920, seed=k)[0] for k in range(8)] + [make_frames(427, 640, seed=3)[0]]
    boxes = [[]] * 8 + [[(136, 98, 173, 127)]]
    res = count_frames(model, fs, boxes)
    del res
    torch.cuda.synchronize()
    first = torch.cuda.memory_allocated()
    res = count_frames(model, [f.copy() for f in fs], boxes)
    del res
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == first


def run(cmd):
    r = subprocess.run([sys.executable] + cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout


def test_demo_zero_device_prep_prints_the_same_counts(tmp_path):
    src = tmp_path / "in"
    src.mkdir()
    for k, (W_, H_) in enumerate([(1280, 720), (640, 427), (1280, 720)]):
        Image.fromarray(make_frames(H_, W_, seed=40 + k)[k % 2]).save(src / ("f%d.png" % k))
    base = ["demo_zero.py", "--input_path", str(src), "--output_path", str(tmp_path / "out"), "--model_path", "", "--no_viz"]

    def counts(out):
        return [l.split("count =")[1].split("-")[0].strip() for l in out.splitlines() if "count =" in l]
    host, dev = counts(run(base)), counts(run(base + ["--device_prep"]))
    assert len(host) == 3 and host == dev


def test_demo_cli_counts_and_writes_the_visualisation(tmp_path):
    import models_mae_cross
    from countr_amd import count_frames
    frame = make_frames(720, 1280, seed=50)[0]
    Image.fromarray(frame).save(tmp_path / "shelf.png")
    out = run(["demo.py", "--input_path", str(tmp_path / "shelf.png"), "--output_path", str(tmp_path / "out"), "--model_path", "",
               "--boxes", "136,98,173,127;209,125,242,150;212,168,258,200"])
    line, = [l for l in out.splitlines() if l.startswith("Count:")]
    assert (tmp_path / "out" / "viz_shelf.jpg").exists()
    assert Image.open(tmp_path / "out" / "viz_shelf.jpg").size == (672, 384)
    torch.manual_seed(0)                                          # the CLI's seeded random model
    m = models_mae_cross.mae_vit_base_patch16(norm_pix_loss="store_true", precision="bf16").to("cuda").eval()
    (cnt, _dm), = count_frames(m, [frame], [[(136, 98, 173, 127), (209, 125, 242, 150), (212, 168, 258, 200)]])
    assert float(line.split()[1]) == cnt


def test_count_items_is_the_front_of_count_items_crops():
    """count_items returns the first two fields of count_items_crops (one implementation): a frame on the 3 x 3 split beside a frame on
    the plain path, on the tiny configuration in fp32."""
    from functools import partial
    import torch.nn as nn
    from countr_amd import frames as FR
    from countr_amd.models_mae_cross import SupervisedMAE
    p, D, depth, H, Dd, ddepth, Hd = W.CONFIGS["tiny_test"]
    m = SupervisedMAE(patch_size=p, embed_dim=D, depth=depth, num_heads=H, decoder_embed_dim=Dd, decoder_depth=ddepth, decoder_num_heads=Hd,
                      mlp_ratio=4, norm_layer=partial(nn.LayerNorm, eps=1e-6), precision="fp32")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.make_state_dict("tiny_test", seed=3).items()}, strict=True)
    m = m.to("cuda").eval()
    fs = [np.random.RandomState(11).randint(0, 256, (60, 90, 3)).astype(np.uint8), np.random.RandomState(12).randint(0, 256, (48, 120, 3)).astype(np.uint8)]
    # frame 0: three exemplars under 10 px in the resized image -> the 3 x 3 split; frame 1: large exemplars -> the plain path
    boxes = [[(10, 10, 11, 11), (40, 20, 41, 21), (70, 40, 71, 41)], [(5, 5, 30, 30), (50, 10, 80, 40), (90, 8, 115, 36)]]
    items = FR.prepare_items("cuda", fs, boxes)
    assert [inference_small(it[2]) for it in items] == [3, 0]
    full = FR.count_items_crops(m, items)
    short = FR.count_items(m, items)
    assert len(short) == len(full) == 2 and all(len(s) == 2 and len(f) == 3 for s, f in zip(short, full))
    for (c, dm), (fc, fdm, _cr) in zip(short, full):
        assert c == fc and torch.equal(dm, fdm)
    assert len(full[0][2]) == 9 and full[0][1] is full[0][2][-1]
    assert full[1][2] is None


def inference_small(rects):
    from countr_amd import inference
    return inference._small_exemplars(rects)
