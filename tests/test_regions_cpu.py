"""CPU: the rule of the regional counts as countr_amd/regions.py restates it in numpy (regions_host is the GPU tests' yardstick), GAME
read off grid cells, and the placements frames.py composes for the 3 x 3 path."""
import numpy as np
import pytest

from countr_amd import frames, regions
from countr_amd.regions import game_grid, game_levels, grid_dot_counts, regions_host

IDENT = (1.0, 0.0, 1.0, 0.0)


def one(map, regs, placement=IDENT):
    return regions_host([map], [placement], [regs])[0]


def test_rectangles_and_a_right_triangle_by_hand():
    d = np.ones((10, 12), np.float32)
    # [1.5, 5.5) x [2.5, 6.5): columns 2..5, rows 3..6
    mass, area, total = one(d, [[(1.5, 2.5), (5.5, 2.5), (5.5, 6.5), (1.5, 6.5)]])
    assert area.tolist() == [16] and mass.tolist() == [16.0] and total == 120.0
    # corners ON centres: an edge's lower end is in, its upper end is out, on both axes -> columns 2..4, rows 3..5
    assert one(d, [[(2, 3), (5, 3), (5, 6), (2, 6)]])[1].tolist() == [9]
    # right triangle (0, 0), (8, 0), (0, 8) shifted by -0.5: row y holds the centres x < 7.5 - y - ... = 8 - y columns minus the diagonal's own
    tri = one(d, [[(-0.5, -0.5), (7.5, -0.5), (-0.5, 7.5)]])[1][0]
    by_hand = sum(sum(1 for x in range(12) if x + 0.5 < 8 - (y + 0.5)) for y in range(10))       # centres strictly under the hypotenuse
    assert tri == by_hand == 28
    d = np.arange(120, dtype=np.float32).reshape(10, 12)
    mass, area, _t = one(d, [[(1.5, 2.5), (5.5, 2.5), (5.5, 6.5), (1.5, 6.5)]])
    assert mass[0] == d[3:7, 2:6].sum() and area[0] == 16


def test_two_polygons_that_tile_a_rectangle_share_no_pixel():
    rs = np.random.RandomState(0)
    d = rs.uniform(-1, 1, (24, 40)).astype(np.float32)
    rect = [(3, 2), (31, 2), (31, 20), (3, 20)]
    lower, upper = [(3, 2), (31, 2), (31, 20)], [(3, 2), (31, 20), (3, 20)]      # the diagonal passes through centres
    x, y = regions.centres(d.shape, IDENT)
    a, b, r = (regions.inside_polygon(x, y, np.asarray(p, np.float64)) for p in (lower, upper, rect))
    assert not (a & b).any() and ((a | b) == r).all() and a.any() and b.any()
    mass, area, _t = one(d, [lower, upper, rect])
    assert area[0] + area[1] == area[2] == 28 * 18 and abs(mass[0] + mass[1] - mass[2]) < 1e-9


def test_outside_orientation_and_concave():
    rs = np.random.RandomState(1)
    d = rs.uniform(0, 1, (16, 16)).astype(np.float32)
    mass, area, total = one(d, [[(40, 40), (50, 40), (45, 50)], [(-30, -5), (-20, -5), (-20, 30)]])
    assert mass.tolist() == [0.0, 0.0] and area.tolist() == [0, 0] and total == d.astype(np.float64).sum()
    poly = [(1.2, 0.7), (13.1, 2.2), (9.4, 14.6), (2.3, 11.9)]
    cw, ccw = one(d, [poly]), one(d, [poly[::-1]])
    assert cw[1][0] == ccw[1][0] > 0 and cw[0][0] == ccw[0][0]
    # a concave L: [0.5, 10.5) x [0.5, 4.5) plus [0.5, 4.5) x [4.5, 12.5)
    L = [(0.5, 0.5), (10.5, 0.5), (10.5, 4.5), (4.5, 4.5), (4.5, 12.5), (0.5, 12.5)]
    mass, area, _t = one(d, [L])
    want = d[1:5, 1:11].astype(np.float64).sum() + d[5:13, 1:5].astype(np.float64).sum()
    assert area[0] == 40 + 32 and abs(mass[0] - want) < 1e-9
    # hanging over the frame: only the part on the map counts
    assert one(d, [[(-5, -5), (3.5, -5), (3.5, 3.5), (-5, 3.5)]])[1][0] == 16


def test_grid_cells_partition_and_ties_go_up():
    rs = np.random.RandomState(2)
    d = rs.uniform(0, 1, (33, 130)).astype(np.float32)
    for gy, gx in ((1, 1), (3, 5), (8, 8), (16, 16)):
        mass, area, total = one(d, [regions.frame_grid(130, 33, gy, gx)])
        assert mass.shape == (gy * gx,) and area.sum() == d.size and abs(mass.sum() - total) < 1e-9
    # boundaries exactly on centres: ys[i] <= y < ys[i + 1] puts the centre into the upper cell
    mass, area, _t = one(np.ones((6, 6), np.float32), [("grid", [0, 3, 5], [0, 2, 5])])
    assert area.tolist() == [3 * 2, 3 * 3, 2 * 2, 2 * 3]          # row 5 and column 5 lie ON the last boundary: outside
    # a placement: a 3 x 4 map that covers a 6 x 8 frame, centres at 2 c + 0.5
    mass, area, _t = one(np.ones((3, 4), np.float32), [regions.frame_grid(8, 6, 3, 2)], (2.0, 0.5, 2.0, 0.5))
    assert area.tolist() == [2] * 6
    assert regions.point_regions([(0.5, 0.5), (7.4, 5.4), (9, 9)], [[(100, 100), (101, 100), (101, 101)], regions.frame_grid(8, 6, 3, 2)]).tolist() == [1, 6, -1]


def test_game_grid_and_levels():
    _g, ys, xs = game_grid(384, 640, 3)
    assert ys.tolist() == [k * 48 - 0.5 for k in range(9)] and xs.tolist() == [k * 80 - 0.5 for k in range(9)]
    _g, ys, xs = game_grid(384, 400, 0)
    assert ys.tolist() == [-0.5, 383.5] and xs.tolist() == [-0.5, 399.5]
    # a coarser level's boundaries are every other boundary of the finer one, bit for bit
    assert game_grid(384, 1360, 2)[2].tolist() == game_grid(384, 1360, 3)[2][::2].tolist()
    rs = np.random.RandomState(3)
    for trial in range(5):
        h, w = 384, 16 * int(rs.randint(24, 60))
        d = (rs.uniform(0, 1, (h, w)) * 60 * 40 / (h * w)).astype(np.float32)
        dots = np.stack([rs.randint(0, w, 37), rs.randint(0, h, 37)], 1).astype(np.float32)
        grid = game_grid(h, w, 3)
        mass, _a, total = one(d, [grid])
        cells = grid_dot_counts(dots, grid)
        assert cells.sum() == 37
        game = game_levels(mass.reshape(8, 8) / 60, cells)
        assert abs(game[0] - abs(total / 60 - 37)) < 1e-9                    # GAME(0) = |pred - gt|
        assert all(game[l] <= game[l + 1] + 1e-9 for l in range(3))           # the triangle inequality
        for l in range(3):                                                   # and each level equals its own grid's
            m_l = one(d, [game_grid(h, w, l)])[0].reshape(1 << l, 1 << l) / 60
            assert abs(np.abs(m_l - grid_dot_counts(dots, game_grid(h, w, l))).sum() - game[l]) < 1e-9
    with pytest.raises(ValueError):
        game_levels(np.zeros((3, 3)), np.zeros((3, 3)))


def test_crop_placements_put_every_centre_inside_its_rectangle():
    for W, H, h, w in ((90, 60, frames.NEW_H, frames.new_width(90, 60)), (1920, 1080, frames.NEW_H, frames.new_width(1920, 1080)), (48, 24, 24, 48)):
        base = frames.map_placement(W, H, w) if h == frames.NEW_H else (1.0, 0.0, 1.0, 0.0)
        for k, (top, left, bottom, right) in enumerate(frames.split_rects(h, w)):
            x, y = regions.centres((h, w), frames.crop_placement(k, h, w, base))
            # the crop's rectangle covers [left - 0.5, right + 0.5) x [top - 0.5, bottom + 0.5) in pixels of the image it was cut from
            x_lo, x_hi = base[0] * (left - 0.5) + base[1], base[0] * (right + 0.5) + base[1]
            y_lo, y_hi = base[2] * (top - 0.5) + base[3], base[2] * (bottom + 0.5) + base[3]
            assert (x > x_lo).all() and (x < x_hi).all() and (y > y_lo).all() and (y < y_hi).all()
            assert (np.diff(x) > 0).all() and (np.diff(y) > 0).all()
            if h == frames.NEW_H:      # the composition is crop_points followed by frame_points, up to rounding
                cy, _cx = frames.crop_points(np.arange(h), np.zeros(h), k, h, w)
                _cy, cx = frames.crop_points(np.zeros(w), np.arange(w), k, h, w)
                assert np.allclose(x, frames.frame_points(np.zeros(w), cx, W, H, w)[0], rtol=0, atol=1e-9)
                assert np.allclose(y, frames.frame_points(cy, np.zeros(h), W, H, w)[1], rtol=0, atol=1e-9)
        # and an unsplit map's placement IS frame_points at the pixel centres, up to rounding; the identity when nothing is resized
        if h == frames.NEW_H:
            x, y = regions.centres((h, w), base)
            assert np.allclose(x, frames.frame_points(np.zeros(w), np.arange(w), W, H, w)[0], rtol=0, atol=1e-9)
    assert frames.map_placement(640, 384, 640) == (1.0, 0.0, 1.0, 0.0)


def test_the_split_paths_count_identity():
    """A partition of the frame summed over the nine crop maps = the sum of the nine maps / 60, which is the split path's count."""
    rs = np.random.RandomState(4)
    h, w, W, H = 24, 48, 48, 24
    nine = [rs.uniform(0, 1, (h, w)).astype(np.float32) for _ in range(9)]
    places = [frames.crop_placement(k, h, w, (1.0, 0.0, 1.0, 0.0)) for k in range(9)]
    (mass, area, total), = regions_host(nine, places, [[regions.frame_grid(W, H, 4, 4)]])
    count = sum(float(m.astype(np.float64).sum()) / 60 for m in nine)
    assert area.sum() == 9 * h * w and abs(mass.sum() / 60 - count) < 1e-9 and abs(total / 60 - count) < 1e-9
    # each crop adds to the cells its rectangle touches only: crop 0 is the top-left third
    (m0, a0, _t), = regions_host(nine[:1], places[:1], [[regions.frame_grid(W, H, 3, 3)]])
    assert a0.tolist() == [h * w] + [0] * 8
    # two sets in one call, maps assigned by set_of_map
    a, b = regions_host(nine[:2], [(1.0, 0.0, 1.0, 0.0)] * 2, [[regions.frame_grid(W, H, 1, 1)], [regions.frame_grid(W, H, 2, 2)]], [1, 0])
    assert abs(a[0][0] - nine[1].astype(np.float64).sum()) < 1e-9 and abs(b[0].sum() - nine[0].astype(np.float64).sum()) < 1e-9


def test_region_summer_chunks_calls_by_the_headers_limits():
    tri, grid = np.zeros((3, 2)), game_grid(8, 8, 1)
    chunks = regions.RegionSummer._chunks
    # 17 sets of one map: 16 maps a call
    assert [len(c) for c in chunks([[tri]] * 17, [[k] for k in range(17)])] == [16, 1]
    # a set's nine maps stay together: 9 + 9 > 16
    assert chunks([[tri], [tri]], [list(range(9)), list(range(9, 18))]) == [[(0, 0, 1)], [(1, 0, 1)]]
    # 70 polygons and 3 grids of one set: two pieces over the same maps, in two calls (64 + 6 polygons > 64)
    assert chunks([[tri] * 70 + [grid] * 3], [[0]]) == [[(0, 0, 64)], [(0, 64, 73)]]
    # 17 grids: 16 a call
    assert chunks([[grid] * 17], [[0]]) == [[(0, 0, 16)], [(0, 16, 17)]]
    # polygons of several sets share a call up to 64
    assert [len(c) for c in chunks([[tri] * 30] * 3, [[0], [1], [2]])] == [2, 1]
    with pytest.raises(ValueError, match="spans 17 maps"):
        chunks([[tri]], [list(range(17))])
    assert (regions.MAX_MAPS, regions.MAX_POLYGONS, regions.MAX_VERTICES, regions.MAX_CELLS) == (16, 64, 64, 256)
