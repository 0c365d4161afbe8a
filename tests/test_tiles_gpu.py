"""GPU: the two kernels of csrc_tiles/tiles.hip through TileStitcher against torch slicing and tiles_host (bit for bit), their sums within
the a-priori bound of an fp32 sum, their refusals, and count_frames / locate_frames(zoom=) end to end on the tiny model against the same
result composed from existing functions: FramePrep at the zoomed height, the band images through inference.density_maps,
inference.blend_windows over the transposed band maps.

The bound (tests/test_regions_gpu.py states it): an fp32 sum of n terms in ANY order differs from the exact sum by at most
(n - 1) u sum|v| / (1 - (n - 1) u) with u = 2^-24; the fp64 sum it is compared with has an error far below that; one ulp of the result
covers the final rounding of the comparison.  Derived, not measured."""
import json
import os
import subprocess
import sys
from functools import partial

import numpy as np
import pytest
import torch

from oracle import weights as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24

GRIDS = {"768x400": (768, 400, 128), "1152x640s256": (1152, 640, 256), "768x640": (768, 640, 128)}


def sum_bound(values):
    """The bound above for the fp32 sum of `values` (float64 array), with the ulp of the result."""
    n = values.size
    if n == 0:
        return 0.0
    return (n - 1) * U * np.abs(values).sum() / (1 - (n - 1) * U) + float(np.spacing(np.float32(abs(values.sum()))))


@pytest.fixture(scope="module")
def stitcher():
    from countr_amd import TileStitcher
    return TileStitcher("cuda")


def grid(name):
    from countr_amd import tile_starts
    hk, wk, stride = GRIDS[name]
    return hk, wk, tile_starts(hk, stride), tile_starts(wk, 128)


# ---- 1. the kernels alone
@pytest.mark.parametrize("name", ["768x400", "1152x640s256"])
def test_gather_equals_torch_slicing(stitcher, name):
    hk, wk, rows, cols = grid(name)
    tiles = [(r, c) for r in rows for c in cols]
    assert len(tiles) == {"768x400": 8, "1152x640s256": 12}[name]
    img = torch.from_numpy(np.random.RandomState(hk + wk).uniform(-1, 1, (1, 3, hk, wk)).astype(np.float32)).cuda()
    dst = torch.full((len(tiles) + 2, 3, 384, 384), 7.0, device="cuda")
    stitcher.gather(img, tiles, dst)
    for j, (r, c) in enumerate(tiles):
        assert torch.equal(dst[j], img[0, :, r:r + 384, c:c + 384]), (j, r, c)
    assert bool((dst[len(tiles):] == 7.0).all())              # the padding rows are the caller's


@pytest.mark.parametrize("name", list(GRIDS))
def test_blend_equals_tiles_host_and_sums_are_within_the_bound(stitcher, name):
    from countr_amd import tiles_host
    hk, wk, rows, cols = grid(name)
    outs = np.random.RandomState(hk * 3 + wk).uniform(-0.5, 1.0, (len(rows) * len(cols), 384, 384)).astype(np.float32)
    rects = [[0, 0, hk - 1, wk - 1], [hk - 70, wk - 40, hk + 130, wk + 600], [5, 7, 5, 7], [hk, 0, hk + 5, 9], [100, 3, 140, 501]]
    dev = torch.from_numpy(outs).cuda()
    dm, sums = stitcher.stitch(rows, cols, hk, wk, rects, outs=dev)
    want = tiles_host(outs, rows, cols, hk, wk)
    got = dm.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (hk, wk)
    assert np.array_equal(got, want)
    assert sums.dtype == np.float32 and sums.shape == (1 + len(rects),)
    d = got.astype(np.float64)
    clipped = [d, d, d[hk - 70:, wk - 40:], d[5:6, 7:8], d[:0], d[100:141, 3:min(502, wk)]]
    for k, part in enumerate(clipped):
        err, bound = abs(float(sums[k]) - part.sum()), sum_bound(part)
        print("%s sum %d: %d pixels, error %.3e, bound %.3e" % (name, k, part.size, err, bound))
        assert err <= bound, (k, err, bound)
    assert sums[3] == got[5, 7] and sums[4] == 0.0
    # a second run, and a run without rectangles, give the same bytes
    dm2, sums2 = stitcher.stitch(rows, cols, hk, wk, rects, outs=dev)
    assert torch.equal(dm2, dm) and sums2.tobytes() == sums.tobytes()
    dm3, sums3 = stitcher.stitch(rows, cols, hk, wk, outs=dev)
    assert torch.equal(dm3, dm) and sums3.tobytes() == sums[:1].tobytes()


def test_refusals_return_a_text_and_launch_nothing(stitcher):
    import ctypes as C
    from countr_amd import _lib
    T = _lib.tiles_lib()
    ints = lambda v: (C.c_int * len(v))(*v)
    err = lambda: T.countr_tiles_last_error().decode()
    img = torch.zeros(1, 3, 768, 400, device="cuda")
    wins = torch.full((66, 3, 384, 384), 7.0, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert T.countr_tile_gather(img.data_ptr(), 768, 400, ints([0] * 65), ints([0] * 65), 65, wins.data_ptr(), st) < 0 and "1..64 tiles" in err()
    assert T.countr_tile_gather(img.data_ptr(), 768, 400, ints([0, 385]), ints([0, 16]), 2, wins.data_ptr(), st) < 0 and "outside" in err()
    assert T.countr_tile_gather(img.data_ptr(), 768, 400, ints([0]), ints([32]), 1, wins.data_ptr(), st) < 0 and "outside" in err()
    with pytest.raises(_lib.CountrError, match="outside"):
        stitcher.gather(img, [(0, 0), (400, 0)], wins)
    torch.cuda.synchronize()
    assert bool((wins == 7.0).all())
    outs = torch.zeros(8, 384, 384, device="cuda")
    dm = torch.full((768, 400), 7.0, device="cuda")
    sums = torch.full((9,), 7.0, device="cuda")
    ws = torch.zeros(T.countr_tiles_workspace(768, 400), dtype=torch.uint8, device="cuda")

    def blend(rows, cols, rects=()):
        flat = [v for r in rects for v in r]
        return T.countr_tile_blend(outs.data_ptr(), len(rows), len(cols), ints(list(rows)), ints(list(cols)), 768, 400, ints(flat) if flat else None,
                                   len(rects), dm.data_ptr(), sums.data_ptr(), ws.data_ptr(), st)

    assert blend(range(65), [0, 16]) < 0 and "got 65" in err()
    assert blend([0, 128, 256, 384], [0, 16], [(0, 0, 1, 1)] * 9) < 0 and "0..8 rectangles, got 9" in err()
    assert blend([0, 128, 256, 512], [0, 16]) < 0 and "row start 3 = 512" in err()
    with pytest.raises(_lib.CountrError, match="0..8 rectangles"):
        stitcher.blend(outs, [0, 128, 256, 384], [0, 16], 768, 400, [(0, 0, 1, 1)] * 9)
    torch.cuda.synchronize()
    assert bool((dm == 7.0).all()) and bool((sums == 7.0).all())


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


FRAME = np.random.RandomState(11).randint(0, 256, (96, 80, 3)).astype(np.uint8)          # zoom 2: 768 x 640 = 4 x 3 tiles
NARROW = np.random.RandomState(12).randint(0, 256, (96, 51, 3)).astype(np.uint8)         # zoom 2: 768 x 400, the snapped column
BOXES3 = [(10, 10, 30, 30), (40, 20, 60, 45), (5, 50, 25, 80)]                           # pixels of the 80 x 96 frame; x 8 at zoom 2
NARROW3 = [(4, 10, 20, 30), (25, 20, 45, 45), (5, 50, 25, 80)]


def composed(model, frame, boxes, k, max_batch=32, band_stride=128):
    """The zoomed map from existing functions: (map [Hk, Wk], rects or None)."""
    from countr_amd import frames as FR, inference, tile_starts
    im = FR.frame_prep("cuda").prepare([frame], 384 * k)[0]
    hk, wk = im.shape[-2:]
    if boxes:
        ex, rects = FR.exemplars(im, boxes, frame.shape[1], frame.shape[0], 384 * k)
    else:
        ex, rects = torch.zeros(1, 0, device="cuda"), None
    rows = tile_starts(hk, band_stride)
    bands = [im[:, :, r:r + 384, :].contiguous() for r in rows]
    S = ex.shape[1] if ex.nelement() > 0 else 0
    maps = inference.density_maps(model, bands, [ex] * len(rows), S, max_batch)
    dm = inference.blend_windows(torch.stack([m.clone() for m in maps]).transpose(1, 2), rows, hk, wk).t().contiguous()
    return dm, rects


def check_count(cnt, dm, rects, normalization=True):
    """cnt against inference._normalise's formulas on the map in float64: count = S / 60, divided by e_cnt = (the rectangles' sums / 60,
    added) / 3 where e_cnt > 1.8.  The fp32 path rounds S and every rectangle sum within sum_bound, every / 60 within one relative u,
    so |cnt - want| <= |want| (rel S + rel e_cnt + 2 u), taken with a factor 1.01 for the second-order terms."""
    d = dm.double().cpu().numpy()
    want = d.sum() / 60
    rel = sum_bound(d) / abs(d.sum()) + U
    if normalization and rects:
        parts = [d[r[0]:r[2] + 1, r[1]:r[3] + 1] for r in rects]
        e_cnt = sum(p.sum() / 60 for p in parts) / 3
        e_err = sum(sum_bound(p) / 60 + abs(p.sum()) / 60 * U for p in parts) / 3
        assert abs(e_cnt - 1.8) > e_err, "the rule's threshold lies inside the rounding of e_cnt: choose other data"
        if e_cnt > 1.8:
            want /= e_cnt
            rel += e_err / e_cnt + U
    print("count %.6f, float64 %.6f, error %.3e, bound %.3e" % (cnt, want, abs(cnt - want), 1.01 * rel * abs(want)))
    assert abs(cnt - want) <= 1.01 * rel * abs(want)


@pytest.mark.parametrize("shots", [0, 3])
def test_zoom_2_equals_the_composition_from_existing_functions(model, shots):
    from countr_amd import count_frames
    boxes = BOXES3 if shots else None
    want, rects = composed(model, FRAME, boxes, 2)
    assert want.shape == (768, 640) and (rects is None) == (shots == 0)
    (cnt, dm), = count_frames(model, [FRAME], [boxes] if shots else None, zoom=2)          # 12 tiles: one forward of 16
    assert isinstance(cnt, float) and dm.dtype == torch.float32 and torch.equal(dm, want)
    check_count(cnt, dm, rects)
    (cnt_plain, dm_plain), = count_frames(model, [FRAME], [boxes] if shots else None, normalization=False, zoom=2)
    assert torch.equal(dm_plain, want)
    check_count(cnt_plain, dm_plain, rects, normalization=False)
    # chunks of 8 and 4 tiles: two forwards of their own buckets
    want8, _ = composed(model, FRAME, boxes, 2, max_batch=8)
    (_c, dm8), = count_frames(model, [FRAME], [boxes] if shots else None, max_batch=8, zoom=2)
    assert torch.equal(dm8, want8)
    # three chunks of 4: consecutive chunks of one bucket (the encoder look-ahead where the precision has one)
    want4, _ = composed(model, FRAME, boxes, 2, max_batch=4)
    (_c, dm4), = count_frames(model, [FRAME], [boxes] if shots else None, max_batch=4, zoom=2)
    assert torch.equal(dm4, want4)
    # three bands instead of four
    want256, _ = composed(model, FRAME, boxes, 2, band_stride=256)
    (c256, dm256), = count_frames(model, [FRAME], [boxes] if shots else None, zoom=2, band_stride=256)
    assert torch.equal(dm256, want256)
    check_count(c256, dm256, rects)
    # 768 x 400: two columns, the second snapped to 16
    nboxes = NARROW3 if shots else None
    wantn, rectsn = composed(model, NARROW, nboxes, 2)
    assert wantn.shape == (768, 400)
    (cn, dmn), = count_frames(model, [NARROW], [nboxes] if shots else None, zoom=2)
    assert torch.equal(dmn, wantn)
    check_count(cn, dmn, rectsn)


# ---- 3. zoom=1 and "auto"
def test_zoom_1_is_the_existing_path_and_auto_takes_each_frame_where_it_belongs(model):
    from countr_amd import count_frames, frames as FR, locate_frames
    from test_regions_gpu import BOXES, FRAMES
    base = count_frames(model, FRAMES, BOXES)
    one = count_frames(model, FRAMES, BOXES, zoom=1)
    for (c0, d0), (c1, d1) in zip(base, one):
        assert c0 == c1 and torch.equal(d0, d1)
    loc0 = locate_frames(model, FRAMES, BOXES)
    loc1 = locate_frames(model, FRAMES, BOXES, zoom=1)
    for a, b in zip(loc0, loc1):
        assert len(a) == len(b) == 4 and a[0] == b[0] and torch.equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    # frame 0: exemplars of 2 px, 6 px at zoom 1 (the 3 x 3 path there) and 12 px at zoom 2; frame 1: large exemplars
    assert FR.frame_zooms(FRAMES, BOXES, "auto") == [2, 1]
    crops = [cr for _c, _d, cr in FR.count_items_crops(model, FR.prepare_items("cuda", FRAMES, BOXES))]
    assert [cr is not None for cr in crops] == [True, False]
    auto = count_frames(model, FRAMES, BOXES, zoom="auto")
    assert tuple(auto[0][1].shape) == (768, 1152)
    want, rects = composed(model, FRAMES[0], BOXES[0], 2)
    assert torch.equal(auto[0][1], want)                       # the tile path, not the nine crops
    check_count(auto[0][0], auto[0][1], rects)
    (c1, d1), = count_frames(model, FRAMES[1:], BOXES[1:])
    assert auto[1][0] == c1 and torch.equal(auto[1][1], d1)
    # zoom_max = 1 leaves nothing to choose
    assert FR.frame_zooms(FRAMES, BOXES, "auto", zoom_max=1) == [1, 1]


# ---- 4. locate_frames(zoom=2)
def test_locate_at_zoom_2(model):
    from countr_amd import frames as FR, locate_frames
    Wd, H = FRAME.shape[1], FRAME.shape[0]
    planted = [(100, 50, 3.0), (400, 333, 2.0), (700, 600, 1.0)]                # (cy, cx, height), far apart
    dm = torch.zeros(768, 640, device="cuda")
    for cy, cx, v in planted:
        dm[cy - 1:cy + 2, cx - 1:cx + 2] = v / 2
        dm[cy, cx] = v
    (pts, score, total), = FR.locate_maps([(3.0, dm)], [(Wd, H)], new_h=768)
    assert total == 3 and pts.shape == (3, 2)
    x, y = FR.frame_points([p[0] for p in planted], [p[1] for p in planted], Wd, H, 640, new_h=768)
    assert np.allclose(pts[:, 0], x, atol=1e-4) and np.allclose(pts[:, 1], y, atol=1e-4)
    assert not np.allclose(pts[:, 1], FR.frame_points([p[0] for p in planted], [p[1] for p in planted], Wd, H, 640)[1], atol=1e-2)
    (cnt, dmz, p2, s2), = locate_frames(model, [FRAME], zoom=2)
    assert tuple(dmz.shape) == (768, 640)
    (p3, s3, _t), = FR.locate_maps([(cnt, dmz)], [(Wd, H)], new_h=768)
    assert np.array_equal(p2, p3) and np.array_equal(s2, s3)
    if len(p2):
        assert p2[:, 0].min() >= -0.5 and p2[:, 0].max() <= Wd - 0.5 and p2[:, 1].min() >= -0.5 and p2[:, 1].max() <= H - 0.5
    with pytest.raises(ValueError, match="regions"):
        locate_frames(model, [FRAME], zoom=2, regions=[[(0, 0), (10, 0), (10, 10)]])


# ---- 5. the demo in a fresh child process
def test_demo_zero_cli_with_zoom(tmp_path):
    import re
    from PIL import Image
    src = tmp_path / "a.png"
    Image.fromarray(np.random.RandomState(5).randint(0, 255, size=(96, 80, 3)).astype(np.uint8)).save(src)

    def run(extra, out):
        r = subprocess.run([sys.executable, "demo_zero.py", "--input_path", str(src), "--output_path", str(out), "--model_path", "", "--points"] + extra,
                           cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        m = re.search(r"^Count: (\S+) - Time: \S+$", r.stdout, re.M)
        assert m, r.stdout
        pts = json.load(open(out / "points_a.json"))
        assert set(pts) == {"count", "total_peaks", "points"} and pts["count"] == float(m.group(1))
        for x, y, _s in pts["points"]:
            assert -0.5 <= x <= 79.5 and -0.5 <= y <= 95.5
        return Image.open(out / "viz_a.jpg").size

    assert run(["--zoom", "2"], tmp_path / "z2") == (640, 768)           # drawn from the zoomed image and map
    assert run([], tmp_path / "z1") == (80, 96)                          # without the flag: resized back to the input size, as before


def test_demo_cli_with_zoom_auto(tmp_path):
    """demo.py --zoom auto: 2-px exemplars in a 90 x 60 image are under 10 px at zoom 1 and 12 px at zoom 2, so the image is counted at
    zoom 2 and its picture has the zoomed size."""
    import re
    from PIL import Image
    src = tmp_path / "b.png"
    Image.fromarray(np.random.RandomState(6).randint(0, 255, size=(60, 90, 3)).astype(np.uint8)).save(src)
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, "demo.py", "--input_path", str(src), "--output_path", str(out), "--model_path", "", "--points", "--zoom", "auto",
                        "--boxes", "10,10,11,11;40,20,41,21;70,40,71,41"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    m = re.search(r"^Count: (\S+) - Time: \S+$", r.stdout, re.M)
    assert m, r.stdout
    pts = json.load(open(out / "points_b.json"))
    assert pts["count"] == float(m.group(1))
    for x, y, _s in pts["points"]:
        assert -0.5 <= x <= 89.5 and -0.5 <= y <= 59.5
    assert Image.open(out / "viz_b.jpg").size == (1152, 768)
