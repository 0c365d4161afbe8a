"""CPU: the host side of the raw-frame path (csrc/frames.hip, countr_amd/frames.py) -- Pillow's BILINEAR tap tables restated in the
library, the resized width and box scaling of the reference's demo.py:42-66, and the argument checks of the three exports (which
run before anything touches a GPU)."""
import ctypes as C

import numpy as np
import pytest
from PIL import Image


def _lib():
    from countr_amd import _lib
    return _lib, _lib.lib()


def _apply(src, bounds, weights):
    """One pass of Pillow's 8-bit resample along axis 0 of src [n, ...] uint8, in integer arithmetic."""
    out = np.empty((bounds.shape[0],) + src.shape[1:], np.uint8)
    for i, (first, cnt) in enumerate(bounds):
        k = weights[i, :cnt].astype(np.int64).reshape((cnt,) + (1,) * (src.ndim - 1))
        acc = (1 << 21) + (src[first:first + cnt].astype(np.int64) * k).sum(0)
        out[i] = np.clip(acc >> 22, 0, 255)
    return out


def _resize_with_tables(img, oh, ow):
    from countr_amd.frames import pil_tables
    H, W = img.shape[:2]
    _kh, hb, hw = pil_tables(W, ow)
    _kv, vb, vw = pil_tables(H, oh)
    tmp = _apply(img.transpose(1, 0, 2), hb, hw).transpose(1, 0, 2)      # horizontal pass first, into 8 bits
    return _apply(tmp, vb, vw)


def _images(H, W):
    rs = np.random.RandomState(H * 10007 + W)
    noise = rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    ramp = np.stack([(xx * 255.0 / max(W - 1, 1)), (yy * 255.0 / max(H - 1, 1)), ((xx + yy) * 255.0 / max(W + H - 2, 1))], 2).astype(np.uint8)
    return {"noise": noise, "ramp": ramp}


# (in, out) pairs of the two axes: every pair the issue lists appears as a width pair or a height pair (or both)
SIZES = [  # (W, H, out_w, out_h)
    (1920, 1080, 672, 384),
    (640, 427, 560, 384),       # upscale in neither / downscale in both; 427 -> 384
    (300, 131, 880, 384),       # 131 -> 384: upscale
    (1000, 384, 1000, 384),     # 384 -> 384: both passes are the identity
    (257, 2160, 32, 384),       # 2160 -> 384: 13 taps
    (500, 500, 224, 224),
    (427, 1080, 384, 384),
    (131, 384, 384, 672),
]


@pytest.mark.parametrize("W,H,ow,oh", SIZES)
def test_tables_reproduce_pillow_bilinear_byte_for_byte(W, H, ow, oh):
    for name, img in _images(H, W).items():
        want = np.asarray(Image.fromarray(img).resize((ow, oh), Image.BILINEAR))
        got = _resize_with_tables(img, oh, ow)
        assert got.shape == want.shape
        assert np.array_equal(got, want), "%s %dx%d -> %dx%d: %d bytes differ" % (name, W, H, ow, oh, int((got != want).sum()))


def test_table_layout_and_tap_stride():
    from countr_amd.frames import pil_tables
    for n_in, n_out, ksize in ((1920, 672, 7), (1080, 384, 7), (2160, 384, 13), (4320, 384, 25), (427, 384, 5), (131, 384, 3), (384, 384, 3)):
        k, bounds, weights = pil_tables(n_in, n_out)
        assert k == ksize == weights.shape[1] and bounds.shape == (n_out, 2)
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds[:, 1] <= k).all() and (bounds.sum(1) <= n_in).all()
        assert (weights >= 0).all() and all((weights[i, c:] == 0).all() for i, c in enumerate(bounds[:, 1]))
        assert np.abs(weights.sum(1) - (1 << 22)).max() <= k          # normalised to 1.0 up to the rounding of each tap


def test_new_width_and_box_scaling_literals():
    """demo.py:42-46 (new_W, scale factors) and :60-65 (int() truncation), worked out by hand: 1920 x 1080 -> 672 x 384, factors 0.35 and
    0.3555...; 640 x 427 -> 560 x 384 (640 / 427 * 384 = 575.55, / 16 = 35.97 -> 35), factors 0.875 and 0.8993."""
    from countr_amd.frames import new_width, scale_boxes
    assert new_width(1920, 1080) == 672 and new_width(640, 427) == 560 and new_width(300, 500) == 224 and new_width(1000, 384) == 992
    ref = [(136, 98, 173, 127), (209, 125, 242, 150), (212, 168, 258, 200)]          # demo.py:53-57
    assert scale_boxes(ref, 1920, 1080) == [[34, 47, 45, 60], [44, 73, 53, 84], [59, 74, 71, 90]]
    assert scale_boxes(ref, 640, 427) == [[88, 119, 114, 151], [112, 182, 134, 211], [151, 185, 179, 225]]
    # both corners truncate to one pixel (35.56 / 35.35 and 35.91 / 35.7): a 1 x 1 crop, the rectangle being inclusive
    assert scale_boxes([(101, 100, 102, 101)], 1920, 1080) == [[35, 35, 35, 35]]
    assert scale_boxes([(82, 101, 82, 101)], 640, 427) == [[90, 71, 90, 71]]
    # boxes that reach the last row and column of the frame land on the last row and column of the resized one
    assert scale_boxes([(1801, 1000, 1919, 1079)], 1920, 1080) == [[355, 630, 383, 671]]
    assert scale_boxes([(600, 400, 639, 426)], 640, 427) == [[359, 525, 383, 559]]


def test_exports_reject_bad_arguments_before_touching_a_gpu():
    _l, L = _lib()

    def failed(rc):
        assert rc < 0 and L.countr_last_error()
        return L.countr_last_error().decode()

    buf = (C.c_int * 64)()
    p = C.cast(buf, C.c_void_p)
    assert "countr_pil_bilinear_tables" in failed(L.countr_pil_bilinear_tables(0, 10, None, None))
    assert "countr_pil_bilinear_tables" in failed(L.countr_pil_bilinear_tables(10, -1, None, None))
    assert "both" in failed(L.countr_pil_bilinear_tables(10, 5, p, None))
    assert L.countr_pil_bilinear_tables(10, 5, None, None) == 5          # the query form: 2 * ceil(2.0) + 1

    one = (C.c_void_p * 1)(p.value)
    ok = dict(frames=one, outs=one, n=1, H=8, W=8, oh=4, ow=4, hb=p, hw=p, vb=p, vw=p, tmp=p)

    def resize(**kw):
        a = dict(ok, **kw)
        return L.countr_frame_resize_u8(a["frames"], a["outs"], a["n"], a["H"], a["W"], a["oh"], a["ow"], a["hb"], a["hw"], a["vb"], a["vw"],
                                        a["tmp"], None)
    for bad in (dict(frames=None), dict(outs=None), dict(n=0), dict(n=17), dict(hb=None), dict(vw=None), dict(tmp=None), dict(H=0),
                dict(ow=0), dict(frames=(C.c_void_p * 1)(None))):
        assert "countr_frame_resize_u8" in failed(resize(**bad)), bad
    assert "too wide" in failed(resize(W=1 << 20, ow=16))                 # the taps of one output pixel exceed the row staging

    rect = (C.c_int * 4)(0, 0, 3, 3)

    def crop(img=p, h=8, w=8, rects=rect, n=1, oh=4, ow=4, out=p):
        return L.countr_crop_resize_f32(img, h, w, rects, n, oh, ow, out, None)
    for bad in (dict(img=None), dict(out=None), dict(rects=None), dict(n=0), dict(n=17), dict(h=0), dict(ow=0)):
        assert "countr_crop_resize_f32" in failed(crop(**bad)), bad
    assert "negative" in failed(crop(rects=(C.c_int * 4)(-1, 0, 3, 3)))
    assert "empty" in failed(crop(rects=(C.c_int * 4)(8, 0, 9, 3)))       # starts below the image: nothing left after clipping
    assert "empty" in failed(crop(rects=(C.c_int * 4)(2, 5, 4, 4)))       # x2 < x1


def test_package_exports():
    import countr_amd
    from countr_amd import frames
    assert countr_amd.count_frames is frames.count_frames and countr_amd.FramePrep is frames.FramePrep


@pytest.mark.parametrize("scale, rects, normalization", [(1.0, None, True), (1.0, [[0, 0, 3, 3], [2, 2, 5, 7], [1, 0, 1, 9]], True),
                                                         (40.0, [[0, 0, 3, 3], [2, 2, 5, 7], [1, 0, 1, 9]], True),
                                                         (40.0, [[0, 0, 3, 3], [2, 2, 5, 7], [1, 0, 1, 9]], False)])
def test_split_count_is_the_references_expression(scale, rects, normalization):
    """inference.split_count on nine small maps against FSC_test_cross(few-shot).py:273-320 + 353-359 written out: the nine counts
    added in list order, the LAST map returned and read by the normalisation.  scale = 40 puts the rectangles' mean over 1.8."""
    import torch
    from countr_amd import inference
    g = torch.Generator().manual_seed(11)
    dms = [torch.rand(6, 10, generator=g) * scale * (k + 1) for k in range(9)]
    pred = 0
    for d in dms:
        pred += (d.sum() / 60).item()
    want, divided = pred, False
    if normalization and rects:
        e_cnt = 0
        for r in rects:
            e_cnt += (dms[-1][r[0]:r[2] + 1, r[1]:r[3] + 1].sum() / 60).item()
        e_cnt = e_cnt / 3
        if e_cnt > 1.8:
            want, divided = pred / e_cnt, True
    assert divided == (scale == 40.0 and normalization)
    got, dm = inference.split_count(dms, rects, normalization)
    assert got == want and dm is dms[-1]


def test_regions_one_list_for_every_frame_or_one_per_frame():
    from countr_amd import frames
    tri, quad, grid = [(0, 0), (4, 0), (0, 4)], [(1, 1), (5, 1), (5, 5), (1, 5)], ("grid", 2, 3)
    per = frames._per_frame([tri, grid], 3)
    assert len(per) == 3 and all(p == [tri, grid] for p in per)
    assert frames._per_frame([[tri], [quad, grid], []], 3) == [[tri], [quad, grid], []]
    assert frames._per_frame(iter([tri]), 2) == [[tri], [tri]]
    for bad, n in (([[tri], [quad]], 3), ([[tri], [quad], [tri]], 2)):
        with pytest.raises(ValueError, match="regions: one list for every frame, or one list per frame"):
            frames._per_frame(bad, n)
    # both users raise it: the polygons of annotate_frames and the regions of count_regions
    with pytest.raises(ValueError, match="regions: one list for every frame, or one list per frame"):
        frames._frame_polygons([[tri], [quad]], 3)
    with pytest.raises(ValueError, match="regions: one list for every frame, or one list per frame"):
        frames.frame_regions([[tri], [quad]], [(8, 8)] * 3)
    assert [len(rs) for rs in frames.frame_regions([tri, grid], [(8, 8), (6, 4)])] == [2, 2]
