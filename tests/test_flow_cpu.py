"""CPU: the rule of include/countr_hip_flow.h as countr_amd.flow_host restates it -- its edges one by one, and synthetic scenes with known
answers (blob_scene: Gaussian density blobs on textured patches that cross a vertical line at a fractional x, one at an integer x and a
tilted one, in both directions; the truth is every object's first and last centre, and every object crosses completely).

The scenes' bound is 3 % of the true crossings, forward and backward.  flow_host's own figures on the committed seeds (printed by the
tests): fast scene within 1.7 %, slow scene within 0.9 % at interval 4 and 6.1 % off at interval 1."""
import numpy as np
import pytest

from countr_amd import flow as F

IDENT = (1.0, 0.0, 1.0, 0.0)


def noise(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w)).astype(np.uint8)


def smooth(h, w, seed):
    """A texture without flat spots whose SAD grows steadily around a match: low-pass noise, stretched to the byte range."""
    rs = np.random.RandomState(seed)
    a = rs.uniform(0, 1, (h + 8, w + 8))
    k = np.ones(5) / 5
    for ax in (0, 1):
        a = np.apply_along_axis(lambda v: np.convolve(v, k, "same"), ax, a)
    a = a[4:-4, 4:-4]
    return np.floor(255 * (a - a.min()) / (a.max() - a.min())).astype(np.uint8)


def window_sad(cur, old, j, i, oy, ox):
    """S(o) of one cell, pixel by pixel with the clamp written out."""
    h, w = cur.shape
    s = 0
    for py in range(8 * j - 4, 8 * j + 12):
        for px in range(8 * i - 4, 8 * i + 12):
            c = int(cur[min(max(py, 0), h - 1), min(max(px, 0), w - 1)])
            e = int(old[min(max(py + oy, 0), h - 1), min(max(px + ox, 0), w - 1)])
            s += abs(c - e)
    return s


@pytest.mark.parametrize("dx,dy", [(0, 0), (3, 0), (0, -2), (-4, 4), (1, -3)])
def test_translation_gives_the_backward_offset(dx, dy):
    old = noise(64, 96, 5)
    cur = np.roll(old, (dy, dx), (0, 1))                                           # cur(p) = old(p - d): the content moved by d
    V = F.motion_host(cur, old, search=4, min_gain=256)
    assert V.dtype == np.int16 and V.shape == (8, 12, 2)
    assert (V[1:-1, 1:-1] == (-16 * dx, -16 * dy)).all()                          # an exact match has S0 = 0 and f = 0 ... on both axes
    # ... because white noise has S- and S+ within 1/16 of each other; the border cells see the wrap of np.roll


def test_flat_frames_give_zero_motion():
    a, b = np.full((32, 48), 100, np.uint8), np.full((32, 48), 107, np.uint8)
    for cur, old in ((a, a), (a, b)):                                              # every S(o) is equal: the tie order picks o = 0
        assert not F.motion_host(cur, old, search=4, min_gain=0).any()
    assert F.candidates(2)[:5] == [(0, 0), (-1, 0), (0, -1), (0, 1), (1, 0)]


def test_min_gain_on_both_sides_of_its_threshold():
    old = smooth(32, 48, 3)
    cur = np.roll(old, (0, 2), (0, 1))
    S = F.sad_host(cur, old, 4).astype(np.int64)
    gain = int(S[4, 4, 1, 2] - S[4, 2, 1, 2])                                      # S(0) - S(best) of cell (1, 2), best = (0, -2)
    assert gain > 0 and S[:, :, 1, 2].min() == S[4, 2, 1, 2]
    moved = F.motion_host(cur, old, 4, min_gain=gain)[1, 2]
    assert moved[0] // 16 in (-2, -3) and abs(moved[0] + 32) <= 8                  # S(0) - S(best) < min_gain is false: it moves
    assert (F.motion_host(cur, old, 4, min_gain=gain + 1)[1, 2] == 0).all()        # ... and true: at rest, no sub-pixel part either
    assert (F.motion_host(cur, old, 4, min_gain=0)[1, 2] == moved).all()


def test_clamping_at_the_image_edge():
    cur, old = noise(16, 16, 1), noise(16, 16, 2)                                  # two cells a side: every window hangs over an edge
    S = F.sad_host(cur, old, 3)
    assert S.shape == (7, 7, 2, 2) and S.dtype == np.uint32
    for j, i, oy, ox in [(0, 0, -3, -3), (0, 1, 3, -1), (1, 0, 0, 0), (1, 1, 3, 3), (1, 1, -2, 1), (0, 0, 1, 2)]:
        assert S[oy + 3, ox + 3, j, i] == window_sad(cur, old, j, i, oy, ox)
    V = F.motion_host(cur, old, 3, 0)
    assert V.shape == (2, 2, 2) and (np.abs(V) <= 16 * 3 + 8).all()


def test_sub_pixel_part_stays_within_half_a_pixel():
    assert F._subpel(100, 100, 300) == -8 and F._subpel(300, 100, 100) == 8        # floor(-15 / 2), floor(17 / 2)
    assert F._subpel(100, 100, 100) == 0 and F._subpel(50, 100, 60) == 0           # den <= 0
    assert F._subpel(300, 100, 300) == 0 and F._subpel(250, 100, 300) == -2        # floor(0.5), floor(-600 / 400)
    for seed in range(4):
        old = smooth(48, 64, seed)
        cur = np.roll(smooth(48, 64, seed), (1, -2), (0, 1)) if seed % 2 else smooth(48, 64, seed + 10)
        r = 4
        S = F.sad_host(cur, old, r).astype(np.int64)
        order = F.candidates(r)
        pick = np.stack([S[oy + r, ox + r] for oy, ox in order]).argmin(0)
        best = np.array(order)[pick][..., ::-1]                                    # (x, y)
        V = F.motion_host(cur, old, r, 0).astype(np.int64)
        f = V - 16 * best
        assert f.min() >= -8 and f.max() <= 8
        edge = np.abs(best) == r
        assert (f[edge] == 0).all()                                                # a neighbour outside the search square: no fit


@pytest.mark.parametrize("band", [2, 8])
def test_band_takes_exactly_w_columns_at_an_integer_x(band):
    h, w = 16, 64
    M = np.ones((h, w), np.float32)
    V = np.zeros((2, 8, 2), np.int16)
    V[..., 0] = -16                                                                # every cell's content moved by +1 px along x
    line = [(30.0, -0.5, 30.0, 15.5)]                                              # t covers rows 0 .. 15: 0 <= t < len2 is half-open too
    flux, total, n, ab, tabs = F.flux_host(M, V, IDENT, line, band, 1, members=True)
    assert total == h * w == tabs
    # e = (0, 16): the normal (-ey, ex) points to -x, so a move to +x is backward
    assert n.tolist() == [[0, band * h]] and flux[0, 0] == 0
    assert abs(flux[0, 1] - h / 60) < 1e-6                                         # band columns x h rows x 1 / band / 60
    cols = [x for x in range(w) if F.flux_host(np.eye(1, w, x, dtype=np.float32).repeat(h, 0), V, IDENT, line, band)[0][0, 1] > 0]
    assert cols == list(range(30 - band // 2 + 1, 30 + band // 2 + 1))            # -hw <= cr < hw with cr = -16 (x - 30): x in (30 - w/2, 30 + w/2]
    # the rows: a line that ends at y = 7.5 takes rows 0 .. 7
    _f, _t, n2, _a, _b = F.flux_host(M, V, IDENT, [(30.0, -0.5, 30.0, 7.5)], band, 1, members=True)
    assert n2.tolist() == [[0, band * 8]]
    # reversed, the same pixels count forward
    assert F.flux_host(M, V, IDENT, [(30.0, 15.5, 30.0, -0.5)], band, 1, members=True)[2].tolist() == [[band * h, 0]]


def test_zero_length_line_counts_nothing():
    M = np.ones((16, 32), np.float32)
    V = np.full((2, 4, 2), -16, np.int16)
    flux, _t, n, _a, _b = F.flux_host(M, V, IDENT, [(10.0, 5.0, 10.0, 5.0), (10.0, -1.0, 10.0, 20.0)], 4, 1, members=True)
    assert flux[0].tolist() == [0, 0] and n[0].tolist() == [0, 0] and n[1, 1] == 4 * 16


def test_interval_scales_the_move_and_the_history_counts_nothing():
    M = np.ones((16, 32), np.float32)
    V = np.full((2, 4, 2), -32, np.int16)
    f1 = F.flux_host(M, V, IDENT, [(10.0, -1.0, 10.0, 20.0)], 4, 1)[0]
    f2 = F.flux_host(M, V, IDENT, [(10.0, -1.0, 10.0, 20.0)], 4, 2)[0]
    assert f1[0, 1] > 0 and abs(f1[0, 1] - 2 * f2[0, 1]) < 1e-12
    lumas, maps, lines, _truth = F.blob_scene(h=32, w=64, objects=2, frames=6)
    for s in (1, 3):
        out, fc = F.flow_host(lumas, maps, lines=lines, interval=s)
        assert [o[0] is None for o in out] == [True] * s + [False] * (6 - s)
        assert fc.frames == 6 and fc.counted == 6 - s and fc.line_counts.shape == (3, 2)
    # a frame without a frame map counts nothing, and its luma still is the next frame's earlier luma
    gap = list(maps)
    gap[2] = None
    out, fc = F.flow_host(lumas, gap, lines=lines, interval=1)
    full, _ = F.flow_host(lumas, maps, lines=lines, interval=1)
    assert out[2][0] is None and fc.counted == 4 and np.array_equal(out[3][1], full[3][1]) and np.array_equal(out[3][0], full[3][0])
    # counts carry the test-time normalisation: scale = count / (total / 60)
    _o, scaled = F.flow_host(lumas, maps, lines=lines, counts=[2 * float(m.astype(np.float64).sum()) / 60 for m in maps])
    assert np.allclose(scaled.line_counts, 2 * F.flow_host(lumas, maps, lines=lines)[1].line_counts, rtol=1e-12)


def test_luma_recovers_the_resized_bytes():
    rgb = np.random.RandomState(0).randint(0, 256, (3, 8, 16)).astype(np.uint8)
    image = rgb.astype(np.float32) / np.float32(255)                               # ToTensor
    want = (77 * rgb[0].astype(int) + 150 * rgb[1].astype(int) + 29 * rgb[2].astype(int) + 128) >> 8
    assert np.array_equal(F.luma_host(image), want) and np.array_equal(F.luma_host(image[None]), want)
    every = np.arange(256, dtype=np.uint8)
    assert np.array_equal(F.luma_host(F.image_of_luma(every.reshape(16, 16))), every.reshape(16, 16))


def worst(fc, truth):
    err = np.abs(fc.line_counts - truth) / truth
    return float(err.max())


@pytest.mark.parametrize("seed,noise_sigma", [(0, 0.0), (1, 0.0), (0, 2.0)])
def test_known_answers_fast_scene(seed, noise_sigma):
    lumas, maps, lines, truth = F.blob_scene(h=96, w=192, objects=5, frames=60, speed=(1.0, 3.0), seed=seed, noise=noise_sigma)
    assert truth.min() >= 2 and (truth.sum(1) == 5).all()                          # every object crosses every line, both directions occur
    _out, fc = F.flow_host(lumas, maps, lines=lines, search=4, interval=1, band=8.0)
    print("seed %d noise %g: truth %s, flux %s, worst %.4f" % (seed, noise_sigma, truth.tolist(), np.round(fc.line_counts, 4).tolist(), worst(fc, truth)))
    assert worst(fc, truth) <= 0.03


def test_known_answers_slow_scene_needs_the_interval():
    lumas, maps, lines, truth = F.blob_scene(h=96, w=192, objects=5, frames=220, speed=(0.25, 0.6), seed=0)
    assert truth.min() >= 2 and (truth.sum(1) == 5).all()
    _o, at4 = F.flow_host(lumas, maps, lines=lines, search=4, interval=4, band=8.0)
    _o, at1 = F.flow_host(lumas, maps, lines=lines, search=4, interval=1, band=8.0)
    print("slow scene: truth %s, interval 4 %s worst %.4f, interval 1 %s worst %.4f"
          % (truth.tolist(), np.round(at4.line_counts, 4).tolist(), worst(at4, truth), np.round(at1.line_counts, 4).tolist(), worst(at1, truth)))
    assert worst(at4, truth) <= 0.03
    assert worst(at1, truth) > worst(at4, truth)


def test_settings_are_checked():
    for bad in (dict(search=0), dict(search=17), dict(interval=0), dict(interval=9), dict(min_gain=-1), dict(band=0.0), dict(band=float("nan"))):
        with pytest.raises(ValueError):
            F.flow_host([], [], lines=[], **bad)
    with pytest.raises(ValueError):
        F.flow_host([], [], lines=[(0, 0, 1, 1)] * 17)
    with pytest.raises(ValueError):
        F.motion_host(np.zeros((12, 16), np.uint8), np.zeros((12, 16), np.uint8))
