"""CPU: the peak rule's host statement (countr_amd/peaks.py: peaks_host), the host-only workspace export, the ABI listing of the two
new exports, and the coordinate mappings of locate_frames."""
import numpy as np

from countr_amd import _lib, peaks
from countr_amd.peaks import peaks_host


def test_header_names_are_exported_by_both_libraries():
    names = _lib.exported_symbols()
    assert "countr_peaks_workspace" in names and "countr_density_peaks" in names
    for variant in ("", "f16"):
        L = _lib.lib(variant)
        assert L.countr_version() == 9 == _lib.ABI_VERSION
        missing = [n for n in names if not hasattr(L, n)]
        assert not missing, (variant, missing)


def test_peaks_workspace_is_host_only_and_checks_its_arguments():
    L = _lib.lib()
    assert L.countr_peaks_workspace(1, 1, 1, 1) > 0
    small, large = L.countr_peaks_workspace(8, 384, 1360, 4096), L.countr_peaks_workspace(16, 384, 1360, 4096)
    assert 0 < small < large
    # at least the ballot masks (8 bytes per 64-pixel row segment) and the raster-order records
    assert small >= 8 * 384 * 22 * 8 + 8 * 4096 * 24
    for bad in ((0, 384, 400, 64), (17, 384, 400, 64), (4, 384, 400, 0), (4, 384, 400, 8193), (4, 0, 400, 64), (4, 384, 0, 64)):
        assert L.countr_peaks_workspace(*bad) < 0, bad
        assert L.countr_last_error()


def test_constant_map_has_one_peak_at_the_origin():
    total, recs = peaks_host(np.full((5, 7), 0.75, np.float32), radius=1, threshold=0.0, rel_threshold=0.1, cap=16)
    assert total == 1 and recs.shape == (1, 6)
    y, x, score, cy, cx, mass = recs[0]
    assert (y, x) == (0, 0) and score == np.float32(0.75)
    assert abs(cy - 0.5) < 1e-12 and abs(cx - 0.5) < 1e-12              # the clipped 2 x 2 window's centre
    assert abs(mass - 4 * 0.75 / 60) < 1e-12


def test_all_zero_map_and_nan():
    total, recs = peaks_host(np.zeros((6, 9), np.float32), radius=2)
    assert total == 0 and recs.shape == (0, 6)
    d = np.zeros((9, 9), np.float32)
    d[2, 2], d[6, 6] = np.nan, 1.0
    total, recs = peaks_host(d, radius=1)
    assert total == 1 and tuple(recs[0, :2]) == (6, 6)                   # the NaN neither wins the maximum nor is a peak
    total, _ = peaks_host(np.full((3, 3), np.nan, np.float32), radius=1)
    assert total == 0


def test_two_equal_maxima_r2_keeps_the_lower_idx_r1_keeps_both():
    """Two equal maxima spanning three pixels (two apart): inside each other's window at r = 2, outside at r = 1."""
    for a, b in (((3, 4), (3, 6)), ((2, 2), (4, 3)), ((4, 6), (2, 4))):
        d = np.zeros((8, 12), np.float32)
        d[a] = d[b] = 1.5
        lo, hi = sorted((a, b))
        total, recs = peaks_host(d, radius=2)
        assert total == 1 and tuple(recs[0, :2]) == lo
        total, recs = peaks_host(d, radius=1)
        assert total == 2 and [tuple(r[:2]) for r in recs] == [lo, hi]               # equal scores: idx ascending
    e = np.zeros((7, 12), np.float32)
    e[3, 4] = e[3, 7] = 2.0                                               # a distance of three: r = 3 reaches, r = 2 does not
    assert peaks_host(e, radius=2)[0] == 2
    total, recs = peaks_host(e, radius=3)
    assert total == 1 and tuple(recs[0, :2]) == (3, 4)


def test_plateau_yields_its_first_pixel_unless_something_higher_is_in_reach():
    d = np.zeros((7, 12), np.float32)
    d[3, 4:8] = 2.0
    d[4, 3:6] = 2.0                                                       # an L-shaped plateau; (3, 4) is its first pixel in raster order
    total, recs = peaks_host(d, radius=2)
    assert total == 1 and tuple(recs[0, :2]) == (3, 4)
    d[1, 5] = 3.0                                                         # higher and within reach of (3, 4): the plateau's first pixel is out,
    total, recs = peaks_host(d, radius=2)                                 # and no other plateau pixel takes its place
    assert total == 1 and tuple(recs[0, :2]) == (1, 5)


def test_corner_maxima_use_clipped_windows():
    d = np.full((9, 9), 0.01, np.float32)
    for k, (y, x) in enumerate(((0, 0), (0, 8), (8, 0), (8, 8))):
        d[y, x] = 1.0 + k
    total, recs = peaks_host(d, radius=3, rel_threshold=0.2)
    assert total == 4
    assert [tuple(r[:2]) for r in recs] == [(8, 8), (8, 0), (0, 8), (0, 0)]           # score descending
    y, x, score, cy, cx, mass = recs[-1]                                 # (0, 0): a 4 x 4 window
    s = 1.0 + 15 * float(np.float32(0.01))
    want = 4 * (1 + 2 + 3) * float(np.float32(0.01)) / s                 # rows 1..3 of the window, four background pixels each
    assert abs(mass - s / 60) < 1e-12 and abs(cy - want) < 1e-12 and abs(cx - want) < 1e-12


def test_cap_keeps_the_raster_first_and_orders_them_by_score():
    d = np.zeros((20, 20), np.float32)
    spots = [((2, 3), 1.0), ((2, 15), 3.0), ((9, 9), 2.0), ((15, 4), 5.0), ((16, 16), 4.0)]
    for (y, x), v in spots:
        d[y, x] = v
    total, recs = peaks_host(d, radius=2, cap=3)
    assert total == 5 and recs.shape == (3, 6)
    assert [tuple(r[:2]) for r in recs] == [(2, 15), (9, 9), (2, 3)] and recs[:, 2].tolist() == [3.0, 2.0, 1.0]
    total, recs = peaks_host(d, radius=2, cap=8)
    assert total == 5 and recs[:, 2].tolist() == [5.0, 4.0, 3.0, 2.0, 1.0]


def test_rel_threshold_one_keeps_only_the_maximum():
    d = np.zeros((12, 30), np.float32)
    d[3, 3], d[3, 20], d[9, 10] = 2.0, 2.0, np.nextafter(np.float32(2.0), np.float32(0))
    total, recs = peaks_host(d, radius=2, rel_threshold=1.0)
    assert total == 2 and [tuple(r[:2]) for r in recs] == [(3, 3), (3, 20)]
    assert peaks_host(d, radius=2, rel_threshold=0.5)[0] == 3
    assert peaks_host(d, radius=2, threshold=2.0)[0] == 0                 # v > threshold is strict


def test_bad_arguments_raise():
    d = np.ones((4, 4), np.float32)
    for kw in ({"radius": 0}, {"radius": 9}, {"threshold": -1.0}, {"rel_threshold": 1.5}, {"cap": 0}, {"cap": 8193}):
        try:
            peaks_host(d, **kw)
        except ValueError:
            continue
        raise AssertionError(kw)
    assert peaks.MAX_MAPS == _lib.PEAKS_MAX_MAPS == 16


def test_frame_mapping_sends_the_centre_to_the_centre():
    from countr_amd.frames import NEW_H, frame_points, new_width
    for W, H in ((200, 120), (1920, 1080), (301, 500)):
        nw = new_width(W, H)
        x, y = frame_points((NEW_H - 1) / 2, (nw - 1) / 2, W, H, nw)
        assert abs(x - (W - 1) / 2) < 1e-9 and abs(y - (H - 1) / 2) < 1e-9
        x, y = frame_points(np.array([-0.5, NEW_H - 0.5]), np.array([-0.5, nw - 0.5]), W, H, nw)       # the outer pixel edges
        assert np.allclose(x, [-0.5, W - 0.5]) and np.allclose(y, [-0.5, H - 0.5])
        assert x.dtype == np.float64


def test_split_crop_mapping_lands_inside_its_rectangle():
    from countr_amd.frames import crop_points, split_rects
    for h, w in ((384, 640), (384, 560), (385, 1001)):
        rects = split_rects(h, w)
        for k, (top, left, bottom, right) in enumerate(rects):
            cy, cx = crop_points((h - 1) / 2, (w - 1) / 2, k, h, w)
            assert top <= cy <= bottom and left <= cx <= right, (k, cy, cx)
            assert abs(cy - (top + bottom) / 2) < 1e-9 and abs(cx - (left + right) / 2) < 1e-9
        cy, cx = crop_points(-0.5, -0.5, 8, h, w)                         # the crop's outer corner = the rectangle's
        assert abs(cy - (rects[8][0] - 0.5)) < 1e-9 and abs(cx - (rects[8][1] - 0.5)) < 1e-9


def test_keep_count_rule():
    from countr_amd.frames import _keep_count
    assert _keep_count(10, 3.49, "count") == 3 and _keep_count(10, 3.5, "count") == 4 and _keep_count(2, 7.0, "count") == 2
    assert _keep_count(10, -2.0, "count") == 0 and _keep_count(10, 0.2, "count") == 0 and _keep_count(10, -2.0, "all") == 10
