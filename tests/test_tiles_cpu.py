"""CPU: the rule of count_frames(zoom=k) as countr_amd/tiles.py and countr_amd/frames.py state it on the host -- tile starts, zoomed
sizes, scaled boxes, the auto rule, and tiles_host against a per-pixel statement of the stitching written here with coverage masks
(tiles_host itself is two applications of inference.blend_windows and never looks at a mask)."""
import numpy as np
import pytest

from countr_amd import frames, inference, tiles


def test_tile_starts_are_the_references_window_starts_at_stride_128():
    for w in range(16, 3073, 16):
        assert tiles.tile_starts(w, 128) == inference.window_starts(w), w
    assert tiles.tile_starts(640) == inference.window_starts(640)


def test_tile_starts_pins():
    assert tiles.tile_starts(768, 128) == [0, 128, 256, 384]
    assert tiles.tile_starts(768, 192) == [0, 192, 384]
    assert tiles.tile_starts(768, 256) == [0, 256, 384]
    assert tiles.tile_starts(768, 384) == [0, 384]
    assert tiles.tile_starts(400, 128) == [0, 16]
    assert tiles.tile_starts(300, 128) == []
    # every list is a full cover: begins at 0, increases, leaves no gap, ends at size - 384
    for size in (384, 400, 768, 1152, 1536, 2720):
        for stride in tiles.BAND_STRIDES:
            s = tiles.tile_starts(size, stride)
            assert s[0] == 0 and s[-1] == size - 384 and all(0 < b - a <= 384 for a, b in zip(s, s[1:])), (size, stride, s)


def brute_force(outs, rows, cols, hk, wk):
    """The rule pixel by pixel: inside a band, a pixel that an earlier tile of the band covered becomes old / 2 + new / 2, else it is the
    new tile's; the bands enter the frame's map by the same rule, in band order.  Coverage is kept as masks."""
    outs = outs.reshape(len(rows), len(cols), 384, 384)
    dm = np.zeros((hk, wk), np.float32)
    seen = np.zeros((hk, wk), bool)
    two = np.float32(2)
    for b, rb in enumerate(rows):
        band = np.zeros((384, wk), np.float32)
        band_seen = np.zeros((384, wk), bool)
        for k, s in enumerate(cols):
            old = band_seen[:, s:s + 384]
            band[:, s:s + 384] = np.where(old, band[:, s:s + 384] / two + outs[b, k] / two, outs[b, k])
            band_seen[:, s:s + 384] = True
        assert band_seen.all()
        old = seen[rb:rb + 384]
        dm[rb:rb + 384] = np.where(old, dm[rb:rb + 384] / two + band / two, band)
        seen[rb:rb + 384] = True
    assert seen.all()
    return dm


@pytest.mark.parametrize("hk,wk,stride", [(768, 400, 128), (768, 640, 256), (1152, 400, 192)])
def test_tiles_host_equals_the_rule_pixel_by_pixel(hk, wk, stride):
    rows, cols = tiles.tile_starts(hk, stride), tiles.tile_starts(wk, 128)
    outs = np.random.RandomState(hk + wk + stride).uniform(-0.5, 1.0, (len(rows) * len(cols), 384, 384)).astype(np.float32)
    got = tiles.tiles_host(outs, rows, cols, hk, wk)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (hk, wk)
    assert np.array_equal(got, brute_force(outs, rows, cols, hk, wk))
    # a pixel three tiles deep on both axes is not the plain mean: the sequential rule weighs the last tile 1/2
    import torch
    assert torch.equal(tiles.tiles_host(torch.from_numpy(outs), rows, cols, hk, wk), torch.from_numpy(got))


def test_zoomed_sizes_and_scaled_boxes():
    assert tiles.zoomed_size(3840, 2160, 1) == (384, 672) and frames.new_width(3840, 2160) == 672
    assert tiles.zoomed_size(3840, 2160, 2) == (768, 1360)         # 1365.33 -> 85 sixteens
    assert tiles.zoomed_size(3840, 2160, 3) == (1152, 2048)
    assert tiles.zoomed_size(3840, 2160, 4) == (1536, 2720)        # 2730.67 -> 170 sixteens
    assert tiles.zoomed_size(80, 96, 2) == (768, 640) and tiles.zoomed_size(51, 96, 2) == (768, 400)
    for k in (1, 2, 3, 4):
        assert tiles.zoomed_size(1920, 1080, k)[1] == frames.new_width(1920, 1080, 384 * k)
    # sh = 768 / 2160 = 0.3556, sw = 1360 / 3840 = 0.3542: (100, 200, 119, 219) -> y 71.1 .. 77.9, x 35.4 .. 42.1, truncated
    assert frames.scale_boxes([(100, 200, 119, 219)], 3840, 2160, 768) == [[71, 35, 77, 42]]
    # the same box at the default height: sh = 0.1778, sw = 0.175
    assert frames.scale_boxes([(100, 200, 119, 219)], 3840, 2160) == [[35, 17, 38, 20]] == frames.scale_boxes([(100, 200, 119, 219)], 3840, 2160, 384)
    # 80 x 96 at k = 2: both factors are 8
    assert frames.scale_boxes([(10, 11, 30, 31)], 80, 96, 768) == [[88, 80, 248, 240]]


def test_points_and_placement_at_a_zoomed_height():
    x, y = frames.frame_points([0.0, 767.0], [0.0, 639.0], 80, 96, 640, new_h=768)
    assert np.allclose(x, [0.5 / 8 - 0.5, 639.5 / 8 - 0.5]) and np.allclose(y, [0.5 / 8 - 0.5, 767.5 / 8 - 0.5])
    assert frames.frame_points(3.0, 5.0, 1920, 1080, 672) == frames.frame_points(3.0, 5.0, 1920, 1080, 672, new_h=384)
    ax, bx, ay, by = frames.map_placement(80, 96, 640, new_h=768)
    assert (ax, ay) == (0.125, 0.125) and bx == by == 0.5 / 8 - 0.5
    assert frames.map_placement(1920, 1080, 672) == frames.map_placement(1920, 1080, 672, 384)


def test_auto_rule():
    # 768 x 768 frame: the factor is k / 2.  A 16-px box is 8 px at 1 (small) and 16 px at 2
    mid = [(100, 100, 116, 116), (200, 200, 216, 216), (300, 300, 316, 316)]
    tiny = [(100, 100, 101, 101)] * 3
    assert inference._small_exemplars(frames.scale_boxes(mid, 768, 768, 384)) == 3
    assert inference._small_exemplars(frames.scale_boxes(mid, 768, 768, 768)) == 0
    assert tiles.auto_zoom(mid, 768, 768) == 2
    assert tiles.auto_zoom(mid, 768, 768, zoom_max=1) == 1
    assert tiles.auto_zoom(tiny, 768, 768) == 3 and tiles.auto_zoom(tiny, 768, 768, zoom_max=4) == 4      # small at every k: zoom_max
    assert tiles.auto_zoom(None, 768, 768) == 1 and tiles.auto_zoom([], 768, 768) == 1
    big = [(100, 100, 200, 200)] * 3
    assert tiles.auto_zoom(big, 768, 768) == 1
    # one small exemplar of three: max_s_cnt = 1 zooms, max_s_cnt = 2 does not
    mixed = [mid[0], big[0], big[0]]
    assert tiles.auto_zoom(mixed, 768, 768, max_s_cnt=1) == 2 and tiles.auto_zoom(mixed, 768, 768, max_s_cnt=2) == 1
    shapes = [np.zeros((768, 768, 3), np.uint8)] * 3
    assert frames.frame_zooms(shapes, [mid, tiny, None], "auto") == [2, 3, 1]
    assert frames.frame_zooms(shapes, None, "auto") == [1, 1, 1] and frames.frame_zooms(shapes, None, 3) == [3, 3, 3]


def test_arguments_are_checked():
    tiles.check_zoom(1), tiles.check_zoom(4), tiles.check_zoom("auto", 4, 384)
    for bad in (0, 5, 2.0, "2", True, None):
        with pytest.raises(ValueError):
            tiles.check_zoom(bad)
    with pytest.raises(ValueError):
        tiles.check_zoom(2, 5)
    with pytest.raises(ValueError):
        tiles.check_zoom(2, 3, 100)


def test_normalised_count_is_normalises_formula():
    sums = np.array([6000.0, 300.0, 360.0, 420.0], np.float32)
    rects = [[0, 0, 1, 1]] * 3
    assert tiles.normalised_count(sums, None) == 100.0 == tiles.normalised_count(sums, rects, normalization=False)
    assert tiles.normalised_count(sums, rects) == 100.0 / ((5.0 + 6.0 + 7.0) / 3)
    assert tiles.normalised_count(np.array([6000.0, 30.0, 36.0, 42.0], np.float32), rects) == 100.0        # e_cnt = 0.6 <= 1.8


def test_package_exports():
    import countr_amd
    assert countr_amd.tile_starts is tiles.tile_starts and countr_amd.tiles_host is tiles.tiles_host
    assert countr_amd.TileStitcher is tiles.TileStitcher
