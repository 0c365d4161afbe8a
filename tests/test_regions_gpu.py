"""GPU: countr_region_sums (csrc_ext/regions.hip) through the C ABI against regions_host -- areas exactly, masses within the a-priori
bound of an fp32 sum -- RegionSummer's chunking and refusals, and count_regions / locate_frames(regions=) end to end on the tiny model.

The bound: an fp32 sum of n terms in ANY order differs from the exact sum by at most (n - 1) u sum|v| / (1 - (n - 1) u) with u = 2^-24,
which n 2^-24 sum|v| covers for every n here; regions_host sums in float64, whose own error is far below that; one ulp of the result
covers the final rounding of the comparison.  Derived, not measured."""
from functools import partial

import numpy as np
import pytest
import torch

from oracle import weights as W

pytestmark = pytest.mark.gpu

IDENT = (1.0, 0.0, 1.0, 0.0)
SCALE = (1080 / 384, 0.5 * 1080 / 384 - 0.5, 1080 / 384, 0.5 * 1080 / 384 - 0.5)      # a 384-high map of a 1080p frame
SIZES = [(5, 7), (24, 40), (33, 130)]


def make_map(h, w, seed):
    return np.random.RandomState(seed).uniform(-0.5, 1.0, (h, w)).astype(np.float32)       # negative densities are summed as they are


def extent(shape, placement):
    """(x0, y0, x1, y1): what an [h, w] map with this placement covers."""
    ax, bx, ay, by = placement
    return (bx - 0.5 * ax, by - 0.5 * ay, bx + (shape[1] - 0.5) * ax, by + (shape[0] - 0.5) * ay)


def star(n, seed):
    rs = np.random.RandomState(seed)
    ang = np.sort(rs.uniform(0, 2 * np.pi, n))
    rad = np.where(np.arange(n) % 2 == 0, 0.48, 0.2) * rs.uniform(0.8, 1.0, n)
    return np.stack([0.5 + rad * np.cos(ang), 0.5 + rad * np.sin(ang)], 1)


# polygons in units of the frame ([0, 1]^2 = the frame), scaled by polygons(): a triangle, the 64-vertex limit, a concave polygon, one
# hanging over two edges, one outside, one covering everything, two that tile a rectangle along its diagonal
UNIT = [
    [(0.1, 0.15), (0.9, 0.3), (0.35, 0.95)],
    star(64, 7),
    [(0.05, 0.05), (0.8, 0.05), (0.8, 0.4), (0.4, 0.4), (0.4, 0.9), (0.05, 0.9)],
    [(0.6, -0.3), (1.4, -0.3), (1.4, 0.5), (0.6, 0.5)],
    [(1.5, 1.5), (2.5, 1.5), (2.0, 2.5)],
    [(-1, -1), (2, -1), (2, 2), (-1, 2)],
    [(0.125, 0.25), (0.875, 0.25), (0.875, 0.75)],
    [(0.125, 0.25), (0.875, 0.75), (0.125, 0.75)],
]


def polygons(ext):
    x0, y0, x1, y1 = ext
    return [np.asarray(p, np.float64) * (x1 - x0, y1 - y0) + (x0, y0) for p in UNIT]


def grids(ext):
    x0, y0, x1, y1 = ext
    return [("grid", y0 + np.arange(g + 1) * (y1 - y0) / g, x0 + np.arange(g + 1) * (x1 - x0) / g) for g in (1, 8, 16)]


@pytest.fixture(scope="module")
def summer():
    from countr_amd.regions import RegionSummer
    return RegionSummer("cuda")


def check(summer, maps, places, som, sets):
    """One RegionSummer.sum against regions_host: areas equal, masses and totals within the bound.  -> the GPU's results."""
    from countr_amd.regions import regions_host
    got = summer.sum([torch.from_numpy(m).cuda() for m in maps], places, som, sets)
    want = regions_host(maps, places, sets, som, members=True)
    assert len(got) == len(want) == len(sets)
    u = 2.0 ** -24
    for s, ((mass, area, total), (wm, wa, wt, wabs, tabs)) in enumerate(zip(got, want)):
        assert mass.dtype == np.float32 and area.dtype == np.int32 and mass.shape == area.shape == wm.shape
        assert np.array_equal(area, wa), (s, area, wa)
        bound = wa * u * wabs + np.spacing(np.abs(wm).astype(np.float32))
        err = np.abs(mass.astype(np.float64) - wm)
        print("set %d: %d slots, worst mass error / bound %.3f" % (s, len(wm), (err / np.maximum(bound, 1e-300)).max() if len(wm) else 0))
        assert (err <= bound).all(), (s, err, bound)
        npix = sum(m.size for m, k in zip(maps, som) if k == s)
        assert abs(float(total) - wt) <= npix * u * tabs + np.spacing(np.float32(abs(wt)))
    return got


@pytest.mark.parametrize("placement", [IDENT, SCALE], ids=["identity", "1080p"])
@pytest.mark.parametrize("h,w", SIZES)
def test_polygons_and_grids_equal_the_host_rule(summer, h, w, placement):
    m = make_map(h, w, h * w)
    ext = extent((h, w), placement)
    (mass, area, total), = check(summer, [m], [placement], [0], [polygons(ext) + grids(ext)])
    assert area[4] == 0 and mass[4] == 0 and area[5] == h * w                 # outside; covering everything
    for at, cells in ((8, 1), (9, 64), (73, 256)):                            # every grid partitions the map
        assert area[at:at + cells].sum() == h * w


def test_two_polygons_that_tile_a_rectangle(summer):
    m = make_map(24, 40, 1)
    lower, upper, rect = [(3, 2), (31, 2), (31, 20)], [(3, 2), (31, 20), (3, 20)], [(3, 2), (31, 2), (31, 20), (3, 20)]
    (mass, area, _t), = check(summer, [m], [IDENT], [0], [[lower, upper, rect]])
    assert area[0] + area[1] == area[2] == 28 * 18 and min(area[:2]) > 0


def test_nine_crop_maps_add_into_one_frame(summer):
    from countr_amd import frames, regions
    h, w = 24, 48
    nine = [make_map(h, w, 100 + k) for k in range(9)]
    places = [frames.crop_placement(k, h, w, IDENT) for k in range(9)]
    ext = (-0.5, -0.5, w - 0.5, h - 0.5)
    (mass, area, total), = check(summer, nine, places, [0] * 9, [polygons(ext) + [regions.frame_grid(w, h, 4, 4)]])
    assert area[5] == 9 * h * w and area[8:].sum() == 9 * h * w
    assert abs(float(mass[8:].astype(np.float64).sum()) - float(total)) <= 9 * h * w * 2.0 ** -24 * sum(np.abs(m).sum() for m in nine) * 2


def test_sixteen_maps_seventeen_maps_and_two_sets_with_their_own_regions(summer):
    maps = [make_map(*SIZES[k % 3], 200 + k) for k in range(17)]
    sets = []
    for k, m in enumerate(maps):
        ext = extent(m.shape, IDENT)
        sets.append(polygons(ext)[k % 3:k % 3 + 3] + grids(ext)[k % 2:k % 2 + 1])
    check(summer, maps[:16], [IDENT] * 16, list(range(16)), sets[:16])
    got = check(summer, maps, [IDENT] * 17, list(range(17)), sets)             # 17 maps: two calls of the export
    one = check(summer, maps[16:], [IDENT], [0], sets[16:])
    assert all(np.array_equal(a, b) for a, b in zip(got[16], one[0]))
    # two sets with different region lists in one call, three and two maps each, maps interleaved; a set without maps gets zeros
    ext = extent((33, 130), SCALE)
    five = [make_map(33, 130, 300 + k) for k in range(5)]
    res = check(summer, five, [SCALE] * 5, [0, 1, 0, 1, 0], [polygons(ext)[:2], grids(ext)[1:2] + polygons(ext)[2:3], grids(ext)[:1]])
    assert res[2][1].tolist() == [0] and res[2][0].tolist() == [0.0] and float(res[2][2]) == 0.0


def test_one_region_and_sixty_four_and_more(summer):
    rs = np.random.RandomState(5)
    m = make_map(33, 130, 6)
    tri = lambda: rs.uniform(-10, 140, (3, 2)) * (1.0, 0.3)
    check(summer, [m], [IDENT], [0], [[tri()]])
    check(summer, [m], [IDENT], [0], [[tri() for _ in range(64)]])
    check(summer, [m], [IDENT], [0], [[star(64, k) * (130, 33) - 0.5 for k in range(20)]])     # 1280 vertices: two LDS groups
    got = check(summer, [m], [IDENT], [0], [[tri() for _ in range(70)] + grids(extent(m.shape, IDENT))])      # more than a call's 64
    assert got[0][0].shape == (70 + 1 + 64 + 256,)


def test_second_run_and_side_stream_give_the_same_bytes(summer):
    maps = [torch.from_numpy(make_map(33, 130, 400 + k)).cuda() for k in range(3)]
    ext = extent((33, 130), IDENT)
    args = (maps, [IDENT] * 3, [0, 0, 1], [polygons(ext) + grids(ext), grids(ext)[1:]])
    a = summer.sum(*args)
    b = summer.sum(*args)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = summer.sum(*args)
    torch.cuda.synchronize()
    for x, y, z in zip(a, b, c):
        for k in range(3):
            assert np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes() == np.asarray(z[k]).tobytes()


def test_malformed_input_is_refused_with_a_text(summer):
    from countr_amd._lib import CountrError
    m = torch.from_numpy(make_map(5, 7, 0)).cuda()
    sum1 = partial(summer.sum, [m], [IDENT], [0])
    for bad, text in (([[(0, 0), (3, 3)]], "3..64 vertices"),
                      ([np.zeros((65, 2))], "3..64 vertices"),
                      ([("grid", [0, 2, 2], [0, 4])], "strictly increasing"),
                      ([("grid", [0, 4], [3, 1])], "strictly increasing"),
                      ([("grid", np.arange(18), np.arange(17))], "at most 256 cells"),
                      ([[(0, 0), (3, np.nan), (1, 4)]], "not finite")):
        with pytest.raises(CountrError, match=text):
            sum1([bad])
    with pytest.raises(CountrError, match="ax > 0"):
        summer.sum([m], [(-1.0, 0.0, 1.0, 0.0)], [0], [[[(0, 0), (3, 0), (3, 3)]]])
    with pytest.raises(ValueError, match="spans 17 maps"):
        summer.sum([m] * 17, [IDENT] * 17, [0] * 17, [[[(0, 0), (3, 0), (3, 3)]]])
    with pytest.raises(ValueError):
        summer.sum([m.double()], [IDENT], [0], [[[(0, 0), (3, 0), (3, 3)]]])
    (mass, area, _t), = sum1([[[(-0.5, -0.5), (6.5, -0.5), (6.5, 4.5), (-0.5, 4.5)]]])      # and the summer works after the refusals
    assert area.tolist() == [35]


# ---- end to end on the tiny configuration, fp32
@pytest.fixture(scope="module")
def model():
    import torch.nn as nn
    from countr_amd.models_mae_cross import SupervisedMAE
    p, D, depth, H, Dd, ddepth, Hd = W.CONFIGS["tiny_test"]
    m = SupervisedMAE(patch_size=p, embed_dim=D, depth=depth, num_heads=H, decoder_embed_dim=Dd, decoder_depth=ddepth, decoder_num_heads=Hd,
                      mlp_ratio=4, norm_layer=partial(nn.LayerNorm, eps=1e-6), precision="fp32")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.make_state_dict("tiny_test", seed=3).items()}, strict=True)
    return m.to("cuda").eval()


FRAMES = [np.random.RandomState(11).randint(0, 256, (60, 90, 3)).astype(np.uint8), np.random.RandomState(12).randint(0, 256, (48, 120, 3)).astype(np.uint8)]
# frame 0: exemplars under 10 px in the resized image -> the 3 x 3 path; frame 1: large exemplars
BOXES = [[(10, 10, 11, 11), (40, 20, 41, 21), (70, 40, 71, 41)], [(5, 5, 30, 30), (50, 10, 80, 40), (90, 8, 115, 36)]]
POLYS = [[(10.5, 5.5), (60.5, 5.5), (60.5, 40.5), (10.5, 40.5)], [(0, 0), (80, 10), (30, 45)], [(-20, -20), (200, -20), (200, 200), (-20, 200)]]


@pytest.mark.parametrize("shots", [0, 3])
def test_count_regions_end_to_end(model, shots):
    from countr_amd import count_frames, count_regions, frames as FR, inference, locate_frames, regions
    boxes = BOXES if shots else None
    regs = POLYS + [("grid", 4, 4)]
    ref = count_frames(model, FRAMES, boxes)
    res = count_regions(model, FRAMES, regs, boxes)
    items = FR.prepare_items("cuda", FRAMES, boxes)
    crops = [cr for _c, _dm, cr in FR.count_items_crops(model, items)]
    assert [cr is not None for cr in crops] == ([True, False] if shots else [False, False])
    u = 2.0 ** -24
    for f, ((cnt, dm, rc, ra), (c0, dm0), cr) in enumerate(zip(res, ref, crops)):
        assert cnt == c0 and torch.equal(dm, dm0)                              # count_frames' bit for bit
        Wd, H = FRAMES[f].shape[1], FRAMES[f].shape[0]
        h, w = dm.shape
        pl = FR.map_placement(Wd, H, w)
        maps = [m.float().cpu().numpy() for m in (cr if cr is not None else [dm])]
        places = [FR.crop_placement(k, h, w, pl) for k in range(9)] if cr is not None else [pl]
        per = FR.frame_regions(regs, [(Wd, H)])[0]
        (wm, wa, wt, wabs, tabs), = regions.regions_host(maps, places, [per], members=True)
        assert rc.dtype == np.float32 and ra.dtype == np.int32 and rc.shape == ra.shape == (3 + 16,)
        assert np.array_equal(ra, wa) and ra[2] == len(maps) * h * w and ra[3:].sum() == len(maps) * h * w
        # region_counts = scale * mass / 60 with scale = count / (total / 60): the bound of mass and of total, carried through
        npix = len(maps) * h * w
        scale = cnt / (wt / 60) if wt > 0 else 1.0
        want = scale * wm / 60
        rel_t = npix * u * tabs / abs(wt) if wt else 0.0
        bound = abs(scale) / 60 * (wa * u * wabs + np.spacing(np.abs(wm).astype(np.float32))) + np.abs(want) * 2 * rel_t + np.spacing(np.abs(want).astype(np.float32))
        err = np.abs(rc.astype(np.float64) - want)
        print("frame %d (%d maps): count %.4f, total / 60 %.4f, worst error / bound %.3f" % (f, len(maps), cnt, wt / 60, (err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all()
        # the 4 x 4 grid partitions the frame, so its cells sum to count: sum(mass), the kernel's total and the forward's own fp32 sum of
        # the same pixels (count = that sum / 60, times the normalisation that scale carries) are each within n 2^-24 sum|v| of the exact
        # sum, so two differences of two of them are within 4 n 2^-24 sum|v|; plus the rounding of the sixteen float32 results and of count
        part = float(rc[3:].astype(np.float64).sum())
        assert abs(part - cnt) <= abs(scale) / 60 * 4 * npix * u * tabs + float(np.spacing(np.abs(rc[3:])).sum()) + np.spacing(np.float32(abs(cnt))), (part, cnt)
    # region_maps: (count, map, crops) entries with crops None give what (count, map) entries with an explicit crops list give, from raw
    # regions or from frame_regions' result
    triples = FR.count_items_crops(model, items)
    sizes = [(f.shape[1], f.shape[0]) for f in FRAMES]
    explicit = FR.region_maps([t[:2] for t in triples], sizes, crops, regs)
    for other in (FR.region_maps(triples, sizes, None, regs), FR.region_maps(triples, sizes, None, FR.frame_regions(regs, sizes))):
        for (rc, ra), (rc2, ra2), (_c, _d, rc0, ra0) in zip(explicit, other, res):
            assert np.array_equal(rc, rc2) and np.array_equal(ra, ra2) and np.array_equal(rc, rc0) and np.array_equal(ra, ra0)
    loc = locate_frames(model, FRAMES, boxes)
    both = locate_frames(model, FRAMES, boxes, regions=regs)
    for (cnt, dm, pts, score), got, (_c, _d, rc, _ra), frame in zip(loc, both, res, FRAMES):
        assert len(got) == 6 and got[0] == cnt and torch.equal(got[1], dm) and np.array_equal(got[2], pts) and np.array_equal(got[3], score)
        assert np.array_equal(got[4], rc)
        per = FR.frame_regions(regs, [(frame.shape[1], frame.shape[0])])[0]
        idx = got[5]
        assert idx.dtype == np.int32 and idx.shape == (len(pts),) and np.array_equal(idx, regions.point_regions(pts, per))
        assert ((idx >= 0) & (idx <= 2)).all()                                 # POLYS[2] covers the frame: no point is left to the grid
