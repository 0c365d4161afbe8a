"""CPU: the rule of include/countr_hip_overlay.h as countr_amd.overlay_host restates it -- the 4:2:0 coefficient table against the float
matrices and through the existing decoder rule on all 2^24 colours, the heat, the integer upsampling against torch's bilinear, the blend's
division, and discs and lines against a brute-force restatement."""
from fractions import Fraction

import numpy as np
import pytest

from countr_amd import overlay as O
from countr_amd import overlay_host

KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
CONFIGS = [(m, r) for m in ("bt601", "bt709") for r in ("full", "limited")]


def planes_gb():
    g, b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    return g, b


def test_the_table_is_the_header_s():
    assert O.COEFFICIENTS == {("bt601", "full"): (77, 150, 29, 0, -43, -85, 128, 128, -107, -21),
                              ("bt601", "limited"): (66, 129, 25, 16, -38, -74, 112, 112, -94, -18),
                              ("bt709", "full"): (54, 184, 18, 0, -29, -99, 128, 128, -116, -12),
                              ("bt709", "limited"): (47, 157, 16, 16, -26, -86, 112, 112, -102, -10)}
    for (matrix, range_), (yr, yg, yb, yoff, ur, ug, ub, vr, vg, vb) in O.COEFFICIENTS.items():
        kr, kb = KR_KB[matrix]
        ys, cs = (1.0, 1.0) if range_ == "full" else (219.0 / 255, 224.0 / 255)
        rnd = lambda v: int(np.floor(256 * v + 0.5))
        assert (yr, yb) == (rnd(ys * kr), rnd(ys * kb)) and yr + yg + yb == (256 if range_ == "full" else 220)
        assert (ur, ub) == (rnd(-cs * kr / (2 * (1 - kb))), rnd(cs * 0.5)) and ur + ug + ub == 0
        assert (vr, vb) == (rnd(cs * 0.5), rnd(-cs * kb / (2 * (1 - kr)))) and vr + vg + vb == 0


@pytest.mark.parametrize("matrix,range_", CONFIGS)
def test_the_coefficients_against_the_float_matrix_on_all_2_24_triples(matrix, range_):
    yr, yg, yb, yoff, ur, ug, ub, vr, vg, vb = O.COEFFICIENTS[(matrix, range_)]
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    ys, cs, y0 = (1.0, 1.0, 0.0) if range_ == "full" else (219.0 / 255, 224.0 / 255, 16.0)
    g, b = planes_gb()
    worst, lo, hi = 0, [255] * 3, [0] * 3
    for r in range(256):
        got = (((yr * r + yg * g + yb * b + 128) >> 8) + yoff,
               np.clip(((ur * r + ug * g + ub * b + 128) >> 8) + 128, 0, 255), np.clip(((vr * r + vg * g + vb * b + 128) >> 8) + 128, 0, 255))
        y = kr * r + kg * g + kb * b
        want = (y0 + ys * y, 128 + cs * (b - y) / (2 * (1 - kb)), 128 + cs * (r - y) / (2 * (1 - kr)))
        for k in range(3):
            worst = max(worst, int(np.abs(got[k] - np.clip(np.floor(want[k] + 0.5), 0, 255)).max()))
            lo[k], hi[k] = min(lo[k], int(got[k].min())), max(hi[k], int(got[k].max()))
    assert worst <= 1
    if range_ == "limited":
        assert 16 <= lo[0] and hi[0] <= 235 and all(16 <= v for v in lo[1:]) and all(v <= 240 for v in hi[1:])
    else:
        assert 0 <= min(lo) and max(hi) <= 255


@pytest.mark.parametrize("matrix,range_", CONFIGS)
def test_the_round_trip_through_the_decoder_rule_on_all_2_24_colours(matrix, range_):
    """overlay_host(out="nv12") -> YuvFrame.from_buffer -> yuv_host(chroma="nearest") on frames of uniform 2 x 2 blocks, one frame per red
    value: at most 3 a channel (2 for BT.601 full), more than 2 on under 1e-4 of the pixels."""
    from countr_amd import YuvFrame, yuv_host
    g, b = planes_gb()
    worst, over, total = 0, 0, 0
    for r in range(256):
        blocks = np.stack([np.full_like(g, r), g, b], -1).astype(np.uint8)                # [256, 256, 3]
        frame = np.repeat(np.repeat(blocks, 2, 0), 2, 1)                                  # [512, 512, 3]
        buf = overlay_host(frame, None, out="nv12", matrix=matrix, range=range_)
        back = yuv_host(YuvFrame.from_buffer(buf, 512, 512, format="nv12", matrix=matrix, range=range_, chroma="nearest"))
        d = np.abs(back.astype(np.int32) - frame.astype(np.int32)).max(-1)
        worst = max(worst, int(d.max()))
        over += int((d > 2).sum())
        total += d.size
    assert total == 4 << 24
    assert worst <= (2 if (matrix, range_) == ("bt601", "full") else 3)
    assert over / total < 1e-4


def test_zero_alpha_or_zero_gain_returns_the_frame():
    rs = np.random.RandomState(0)
    frame = rs.randint(0, 256, (13, 17, 3)).astype(np.uint8)
    m = rs.uniform(0, 3, (5, 9)).astype(np.float32)
    lut = rs.randint(0, 256, (256, 4)).astype(np.uint8)
    lut[:, 3] = 0
    assert np.array_equal(overlay_host(frame, m, colormap=lut), frame)
    for cmap in ("red", "heat"):
        assert np.array_equal(overlay_host(frame, m, gain=0.0, colormap=cmap), frame)
    assert np.array_equal(overlay_host(frame, None), frame)
    assert np.array_equal(overlay_host(frame, -m, gain="max"), frame)                     # nothing above 0: the gain is 0


def test_the_heat():
    m = np.array([[-1.0, 0.0, 0.4999, 0.5, 1.0, 254.4, 254.5, 255.0, 1e9, np.nan, np.inf, -np.inf]], np.float32)
    assert O.heat_host(m, 1.0).tolist() == [[0, 0, 0, 1, 1, 254, 255, 255, 255, 0, 255, 0]]
    assert O.heat_host(m, 0.0).tolist() == [[0] * 9 + [0, 0, 0]]                          # (inf x 0 is a NaN: 0)
    assert O.gain_host(np.array([[0.5, -2.0, np.nan, 4.0]], np.float32), "max") == np.float32(255.0) / np.float32(4.0)
    assert O.gain_host(np.array([[-1.0, 0.0, np.nan]], np.float32), "max") == 0.0
    # one multiply and one add, each rounded to fp32: not an fma
    a, g = np.float32(1.0000001), np.float32(3.0000002)
    assert O.heat_host(np.array([[a]]), g)[0, 0] == int(np.floor(np.float32(np.float32(a * g) + np.float32(0.5))))
    assert O.colormap_table("red")[77].tolist() == [255, 0, 0, 77]
    assert O.colormap_table("heat")[[0, 50, 100, 200, 255]].tolist() == [[0, 0, 0, 0], [150, 0, 0, 100], [255, 45, 0, 200], [255, 255, 90, 255],
                                                                        [255, 255, 255, 255]]


@pytest.mark.parametrize("H,W,mh,mw", [(7, 9, 3, 4), (5, 5, 40, 33), (1, 1, 1, 1), (33, 2, 2, 70), (16, 16, 16, 16)])
def test_a_constant_map_gives_a_constant_heat(H, W, mh, mw):
    for q in (0, 1, 137, 255):
        assert (O.upsample_host(np.full((mh, mw), q), H, W) == q).all()


def test_a_map_of_the_frame_s_size_is_sampled_exactly():
    rs = np.random.RandomState(1)
    for H, W in ((6, 11), (1, 5), (17, 1)):
        q = rs.randint(0, 256, (H, W))
        assert np.array_equal(O.upsample_host(q, H, W), q)
        for size in (H, W):
            i0, _i1, fr = O.axis_host(size, size)
            assert np.array_equal(i0, np.arange(size)) and (fr == 0).all()


@pytest.mark.parametrize("H,W,mh,mw", [(37, 53, 24, 40), (19, 23, 48, 64), (108, 192, 24, 43), (9, 200, 30, 7)])
def test_the_upsampling_against_torch_s_bilinear(H, W, mh, mw):
    """The 8-bit weights are the only difference.  A weight is cut to a multiple of 1 / 256, so it is short by ex < 1 / 256 along x and
    ey < 1 / 256 along y, and the level moves by at most ex dx + ey dy + ex ey |q00 - q01 - q10 + q11| with dx, dy the largest step
    between neighbouring map levels along the axis; the one rounding at the end adds 0.5.  A heat whose neighbours differ by at most 63
    a side -- a density map is smooth -- therefore stays within 0.5 + 2 x 63 / 256 + 126 / 65536 < 1 level: the bound asserted.  On white
    noise (steps up to 255) the same reasoning gives 0.5 + 2 x 255 / 256 + 510 / 65536 < 2.5; 1.44 is what this noise reaches."""
    import torch
    rs = np.random.RandomState(H + W)
    ref = lambda q: torch.nn.functional.interpolate(torch.from_numpy(q).double()[None, None], size=(H, W), mode="bilinear",
                                                    align_corners=False)[0, 0].numpy()
    walk = lambda n: np.cumsum(rs.randint(-63, 64, n))
    smooth = np.clip(128 + walk(mh)[:, None] + walk(mw)[None, :], 0, 255)                  # (clipping keeps every step within 63)
    assert np.abs(np.diff(smooth, axis=0)).max() <= 63 and np.abs(np.diff(smooth, axis=1)).max() <= 63 and np.ptp(smooth) > 100
    got = O.upsample_host(smooth, H, W)
    assert np.abs(got - ref(smooth)).max() <= 1.0
    noise = rs.randint(0, 256, (mh, mw))
    got = O.upsample_host(noise, H, W)
    assert np.abs(got - ref(noise)).max() < 2.5
    assert got.min() >= 0 and got.max() <= 255


def test_the_blend_s_division_on_its_whole_domain():
    v = np.arange(255 * 255 + 1)                                                          # frame (255 - a) + colour a
    assert np.array_equal(O.div255(v + 127), (v + 127) // 255)
    assert np.array_equal(O.div255(np.arange(65536)), np.arange(65536) // 255)
    frame = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, 2)
    for a in (0, 1, 128, 254, 255):
        lut = np.tile(np.array([[10, 200, 255, a]], np.uint8), (256, 1))
        got = O.blend_host(frame, np.zeros((16, 16), np.int64), lut)
        for c, colour in enumerate((10, 200, 255)):
            want = [int(Fraction(int(p) * (255 - a) + colour * a + 127, 255)) for p in frame[..., c].ravel()]      # (int() floors: all >= 0)
            assert got[..., c].ravel().tolist() == want


def brute_line(x0, y0, x1, y1):
    dx, dy = x1 - x0, y1 - y0
    n = max(abs(dx), abs(dy))
    if n == 0:
        return {(x0, y0)}
    rdiv = lambda a: (2 * a + n) // (2 * n)                                                # python integers: exact, floors
    return {(x0 + rdiv(i * dx), y0 + rdiv(i * dy)) for i in range(n + 1)}


def painted(rgb, color):
    ys, xs = np.nonzero((rgb == np.array(color, np.uint8)).all(-1))
    return set(zip(xs.tolist(), ys.tolist()))


def test_lines_against_a_brute_force_restatement():
    H, W = 20, 30
    blank = np.zeros((H, W, 3), np.uint8)
    inside = lambda pts: {(x, y) for x, y in pts if 0 <= x < W and 0 <= y < H}
    cases = {"horizontal": (3, 5, 25, 5), "vertical": (7, 18, 7, 2), "diagonal": (2, 2, 15, 15), "shallow": (1, 4, 28, 9), "steep back": (20, 19, 16, 0),
             "both ends outside": (-10, -4, 45, 27), "wholly outside": (40, 3, 60, 9)}
    for name, (x0, y0, x1, y1) in cases.items():
        got = painted(overlay_host(blank, None, regions=[[(x0, y0), (x1, y1)]]), O.REGION_COLOR)
        assert got == inside(brute_line(x0, y0, x1, y1)) | inside(brute_line(x1, y1, x0, y0)), name      # (two vertices: the edge and its way back)
        assert (len(got) == 0) == (name == "wholly outside")
    assert len(painted(overlay_host(blank, None, regions=[[(3, 5), (25, 5)]]), O.REGION_COLOR)) == 23
    # a shallow edge steps once per column and moves in y by exactly round-half-up of the exact line
    for i, x in enumerate(range(1, 29)):
        y = Fraction(4) + Fraction(i * 5, 27)
        assert (x, int(np.floor(y + Fraction(1, 2)))) in brute_line(1, 4, 28, 9)
    # a polygon with a single vertex is one pixel; a triangle is its three edges; vertices round as floor(v + 0.5)
    assert painted(overlay_host(blank, None, regions=[[(4.4, 6.5)]]), O.REGION_COLOR) == {(4, 7)}
    tri = [(2, 3), (25, 6), (11, 17)]
    want = brute_line(2, 3, 25, 6) | brute_line(25, 6, 11, 17) | brute_line(11, 17, 2, 3)
    assert painted(overlay_host(blank, None, regions=[tri], region_color=(1, 2, 3)), (1, 2, 3)) == want
    assert O.round_coords([(-0.5, 0.49), (2.5, -1.51)]).tolist() == [[0, 0], [3, -2]]


def test_discs_against_a_brute_force_restatement():
    H, W = 24, 24
    blank = np.zeros((H, W, 3), np.uint8)
    assert painted(overlay_host(blank, None, points=[(5, 6)], point_radius=0), O.POINT_COLOR) == {(5, 6)}
    for r in (1, 2, 5, 16):
        for cx, cy in ((12, 11), (0, 0), (23, 25), (-4, 30)):
            want = {(x, y) for x in range(W) for y in range(H) if (x - cx) ** 2 + (y - cy) ** 2 <= r * r}
            assert painted(overlay_host(blank, None, points=[(cx, cy)], point_radius=r), O.POINT_COLOR) == want, (r, cx, cy)
    with pytest.raises(ValueError, match="point_radius is 0..16"):
        overlay_host(blank, None, points=[(1, 1)], point_radius=17)
    with pytest.raises(ValueError, match="-1048576 .. 1048576"):
        overlay_host(blank, None, points=[(3e6, 1)])


def test_the_label_blends_towards_white_and_is_clipped():
    frame = np.full((10, 12, 3), 100, np.uint8)
    patch = np.array([[0, 255, 128], [64, 0, 255]], np.uint8)
    got = overlay_host(frame, None, label=(patch, 10, 9))                                 # hangs over the right and bottom edges
    assert got[9, 10].tolist() == [100] * 3 and got[9, 11].tolist() == [255] * 3
    assert (got[:9] == 100).all() and (got[9, :10] == 100).all()
    got = overlay_host(frame, None, label=(patch, 0, 0))
    assert got[0, 2].tolist() == [(100 * 127 + 255 * 128 + 127) // 255] * 3 and got[1, 0].tolist() == [(100 * 191 + 255 * 64 + 127) // 255] * 3
    p = O.label_patch("12.345")
    assert p.dtype == np.uint8 and 1 <= p.shape[0] <= 64 and 1 <= p.shape[1] <= 256 and p.max() > 128 and p[-1].any() and p[:, -1].any()


def test_the_marks_are_drawn_in_order_and_the_output_formats_hold_the_same_picture():
    rs = np.random.RandomState(2)
    frame = rs.randint(0, 256, (11, 13, 3)).astype(np.uint8)                              # both sides odd: the last chroma sample replicates the edge
    m = rs.uniform(0, 2, (4, 6)).astype(np.float32)
    solid = (np.full((5, 5), 255, np.uint8), 2, 2)
    kw = dict(label=solid, regions=[[(0, 4), (12, 4)]], points=[(4, 4)], point_radius=0)
    rgb = overlay_host(frame, m, **kw)
    assert rgb[3, 4].tolist() == [255, 255, 255] and rgb[4, 5].tolist() == [255, 255, 0] and rgb[4, 4].tolist() == [0, 255, 0]
    bufs = {out: overlay_host(frame, m, out=out, **kw) for out in ("nv12", "nv21", "i420")}
    n, hc, wc = 11 * 13, 6, 7
    assert all(b.shape == (n + 2 * hc * wc,) and b.dtype == np.uint8 for b in bufs.values())
    assert O.frame_bytes("nv12", 13, 11) == n + 2 * hc * wc and O.frame_bytes("rgb", 13, 11) == 3 * n
    u, v = bufs["i420"][n:n + hc * wc], bufs["i420"][n + hc * wc:]
    assert np.array_equal(bufs["nv12"][n:].reshape(-1, 2), np.stack([u, v], 1)) and np.array_equal(bufs["nv21"][n:].reshape(-1, 2), np.stack([v, u], 1))
    assert np.array_equal(bufs["nv12"][:n], bufs["i420"][:n])
    yr, yg, yb, yoff, ur, ug, ub = O.COEFFICIENTS[("bt709", "limited")][:7]
    p = rgb.astype(int)
    assert bufs["i420"][n - 1] == ((yr * p[10, 12, 0] + yg * p[10, 12, 1] + yb * p[10, 12, 2] + 128) >> 8) + yoff
    s = [(4 * p[10, 12, c] + 2) >> 2 for c in range(3)]                                   # the corner block: one pixel, replicated
    assert u[-1] == min(255, max(0, ((ur * s[0] + ug * s[1] + ub * s[2] + 128) >> 8) + 128))
    s = [(p[0, 0, c] + p[0, 1, c] + p[1, 0, c] + p[1, 1, c] + 2) >> 2 for c in range(3)]
    assert u[0] == min(255, max(0, ((ur * s[0] + ug * s[1] + ub * s[2] + 128) >> 8) + 128))
    with pytest.raises(ValueError, match="out is one of"):
        overlay_host(frame, m, out="p010")
