"""CPU: the rule of include/countr_hip_draw.h as countr_amd/draw.py restates it -- the font, draw_host against an independent per-pixel
statement (greatest key over per-mark masks), the overlay's edge and point rules, clipping -- and the host side of an annotated clip:
Trails on a lane scene, clip_marks."""
import numpy as np
import pytest

from countr_amd import draw, overlay, tracks
from countr_amd.draw import Marks, Trails, clip_marks, draw_host

DIGITS = """
.###. ..#.. .###. ##### ...#. ##### ..##. ##### .###. .###.
#...# .##.. #...# ...#. ..##. #.... .#... ....# #...# #...#
#..## ..#.. ....# ..#.. .#.#. ####. #.... ...#. #...# #...#
#.#.# ..#.. ...#. ...#. #..#. ....# ####. ..#.. .###. .####
##..# ..#.. ..#.. ....# ##### ....# #...# .#... #...# ....#
#...# ..#.. .#... #...# ...#. #...# #...# .#... #...# ...#.
.###. .###. ##### .###. ...#. .###. .###. .#... .###. .##..
"""


def test_font_glyphs_are_distinct_and_digits_are_what_is_written_here():
    f = draw.font()
    assert f.shape == (95, 7) and f.dtype == np.uint8 and f.max() < 32
    assert not f[0].any() and all(f[g].any() for g in range(1, 95))
    assert len({f[g].tobytes() for g in range(95)}) == 95
    art = np.array([[c == "#" for c in row.replace(" ", ".")] for row in DIGITS.strip().splitlines()])         # [7, 59]
    box = draw.text_mask_host(b"0123456789", 1)
    assert box.shape == (8, 60) and not box[7].any() and not box[:, 59].any()
    assert np.array_equal(box[:7, :59], art)
    # through draw_host: foreground on the glyph, background on the rest of the cells, nothing outside them
    frame = np.full((12, 64, 3), 7, np.uint8)
    out = draw_host(frame, Marks().text(2, 3, "0123456789", 1, (255, 255, 255), (1, 2, 3)))
    assert np.array_equal((out[3:11, 2:62] == 255).all(2), box) and np.array_equal((out[3:11, 2:62] == (1, 2, 3)).all(2), ~box)
    rest = np.ones((12, 64), bool)
    rest[3:11, 2:62] = False
    assert (out[rest] == 7).all()
    # without a background only the glyph is written; an unknown byte is '?'
    out = draw_host(frame, Marks().text(2, 3, "0123456789", 1, (255, 255, 255)))
    assert np.array_equal((out[3:11, 2:62] == 255).all(2), box) and ((out == 7).all(2) | (out == 255).all(2)).all()
    assert np.array_equal(draw.text_mask_host(bytes([7, 200, 127]), 1), draw.text_mask_host(b"???", 1))


@pytest.mark.parametrize("s", [2, 3, 8])
def test_scale_is_pixel_replication(s):
    one = draw.text_mask_host(b"Ag%7~", 1)
    assert np.array_equal(draw.text_mask_host(b"Ag%7~", s), np.kron(one, np.ones((s, s), bool)))
    frame = np.zeros((8 * s + 3, 30 * s + 5, 3), np.uint8)
    a = draw_host(np.zeros((11, 35, 3), np.uint8), Marks().text(2, 1, "Ag%7~", 1, (9, 8, 7), (1, 1, 1)))
    b = draw_host(frame, Marks().text(2, 1, "Ag%7~", s, (9, 8, 7), (1, 1, 1)))
    assert np.array_equal(b[1:1 + 8 * s, 2:2 + 30 * s], np.kron(a[1:9, 2:32], np.ones((s, s, 1), np.uint8)))


def random_marks(rs, H, W, n=12):
    m = Marks()
    for _ in range(n):
        m.segment(rs.randint(-10, W + 10, 2), rs.randint(-10, W + 10, 2), rs.randint(0, 9), rs.randint(0, 256, 3))
        m.disc(rs.randint(-10, W + 10, 2), rs.randint(0, 17), rs.randint(0, 256, 3))
        text = bytes(rs.randint(20, 140, rs.randint(0, 8)).astype(np.uint8))
        m.text(rs.randint(-20, W), rs.randint(-10, H), text, rs.randint(1, 4), rs.randint(0, 256, 3), rs.randint(0, 256, 3) if rs.rand() < 0.5 else None)
    return m


def brute_force(frame, marks):
    """The rule, pixel by pixel: a mask and a colour plane per mark from the header's words, the greatest key wins."""
    H, W, _ = frame.shape
    f = draw.font()
    segments, discs, texts = marks.arrays()
    yy, xx = np.mgrid[0:H, 0:W]
    layers = []                                                     # (mask [H, W], colours [H, W] as 0xRRGGBB) in key order
    for x0, y0, x1, y1, w, c in segments.tolist():
        dx, dy = x1 - x0, y1 - y0
        n = max(abs(dx), abs(dy))
        mask = np.zeros((H, W), bool)
        for i in range(n + 1):
            cx = x0 + ((2 * i * dx + n) // (2 * n) if n else 0)
            cy = y0 + ((2 * i * dy + n) // (2 * n) if n else 0)
            mask |= (xx - cx) ** 2 + (yy - cy) ** 2 <= w * w
        layers.append((mask, np.full((H, W), c)))
    for cx, cy, r, c in discs.tolist():
        layers.append(((xx - cx) ** 2 + (yy - cy) ** 2 <= r * r, np.full((H, W), c)))
    for rec in texts:
        x, y, s, fg, bg, n = rec[:6].tolist()
        raw = rec[6:].view(np.uint8)[:n]
        u, v = xx - x, yy - y
        cell = (u >= 0) & (u < 6 * s * n) & (v >= 0) & (v < 8 * s)
        k, gc, gr = np.clip(u // (6 * s), 0, max(n - 1, 0)), (u % (6 * s)) // s, np.clip(v // s, 0, 7)
        glyph = np.array([b if 32 <= b <= 126 else 63 for b in raw] + [32], np.int64)[k if n else 0 * k] - 32
        rows = np.concatenate([f, np.zeros((95, 1), np.uint8)], 1)[glyph, gr]
        fore = cell & (gc < 5) & (((rows >> np.clip(4 - gc, 0, 7)) & 1) == 1)
        layers.append((fore | (cell & (bg >= 0)), np.where(fore, fg, bg)))
    out = frame.copy()
    key = np.zeros((H, W), np.int64)
    col = np.zeros((H, W), np.int64)
    for k, (mask, colours) in enumerate(layers):
        key[mask], col[mask] = k + 1, colours[mask]
    won = key > 0
    out[won] = np.stack([(col >> 16) & 255, (col >> 8) & 255, col & 255], -1)[won]
    return out


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_draw_host_equals_the_per_pixel_rule(seed):
    rs = np.random.RandomState(seed)
    frame = rs.randint(0, 256, (37, 53, 3)).astype(np.uint8)
    marks = random_marks(rs, 37, 53)
    got = draw_host(frame, marks)
    assert np.array_equal(got, brute_force(frame, marks)) and (got != frame).any()
    for out, mx, rg in (("nv12", "bt709", "limited"), ("i420", "bt601", "full")):
        assert np.array_equal(draw_host(frame, marks, out, mx, rg), overlay.rgb_to_yuv_host(got, out, mx, rg))
        assert len(draw_host(frame, marks, out, mx, rg)) == overlay.frame_bytes(out, 53, 37)
    assert np.array_equal(draw_host(frame, None), frame) and np.array_equal(draw_host(frame, Marks()), frame)


def test_thin_segments_and_discs_are_the_overlay_s_edges_and_points():
    rs = np.random.RandomState(4)
    frame = rs.randint(0, 256, (37, 53, 3)).astype(np.uint8)
    edges = rs.randint(-8, 60, (9, 4))
    edges[0, 2:] = edges[0, :2]                                     # a segment of length zero
    want = frame.copy()
    overlay.draw_edges_host(want, edges, (10, 200, 30))
    assert np.array_equal(draw_host(frame, Marks().segments(edges[:, :2], edges[:, 2:], 0, (10, 200, 30))), want)
    centres = rs.randint(-8, 60, (7, 2))
    for r in (0, 1, 5, 16):
        want = frame.copy()
        overlay.draw_points_host(want, centres, r, (1, 2, 250))
        assert np.array_equal(draw_host(frame, Marks().discs(centres, r, (1, 2, 250))), want)


def test_clipping_and_the_ends_of_the_coordinate_range():
    frame = np.random.RandomState(5).randint(0, 256, (37, 53, 3)).astype(np.uint8)
    far = 1 << 20
    outside = (Marks().segment((-30, -5), (-9, 60), 8, (1, 1, 1)).segment((far, far), (far, -far), 8, (1, 1, 1)).disc((70, 54), 16, (2, 2, 2))
               .disc((-far, far), 16, (2, 2, 2)).text(53, 0, "out", 8, (3, 3, 3), (4, 4, 4)).text(-far, -far, "out", 8, (3, 3, 3), (4, 4, 4))
               .text(far, far, "x" * 32, 8, (3, 3, 3), (4, 4, 4)).text(0, -64, "above", 8, (3, 3, 3), (4, 4, 4)))
    assert np.array_equal(draw_host(frame, outside), frame)
    partly = (Marks().segment((-far, -far), (far, far), 1, (9, 9, 9)).segment((-4, 30), (10, 40), 8, (8, 8, 8)).disc((52, 0), 16, (7, 7, 7))
              .text(40, 30, "Wg", 8, (6, 6, 6), (5, 5, 5)))
    got = draw_host(frame, partly)
    assert np.array_equal(got, brute_force_clipped(frame, partly)) and (got[0, 0] == 9).all() and (got[36, 36] == 9).all()
    assert (got[36, 52] == 5).all() or (got[36, 52] == 6).all()
    for bad in (lambda: Marks().segment((far + 1, 0), (0, 0)), lambda: Marks().disc((0, -far - 1)), lambda: Marks().text(far + 1, 0, "a"),
                lambda: Marks().segment((0, 0), (1, 1), 9), lambda: Marks().disc((0, 0), 17), lambda: Marks().text(0, 0, "a", 0),
                lambda: Marks().text(0, 0, "a", 9), lambda: Marks().text(0, 0, "a" * 33), lambda: Marks().disc((0, 0), 1, (256, 0, 0)),
                lambda: Marks().disc((np.nan, 0))):
        with pytest.raises(ValueError):
            bad()


def brute_force_clipped(frame, marks):
    """brute_force with the long diagonal's centres cut to those near the frame (the others cover nothing of it)."""
    segments, discs, texts = marks.arrays()
    H, W, _ = frame.shape
    short = Marks()
    for x0, y0, x1, y1, w, c in segments.tolist():
        if abs(x0) == 1 << 20:
            assert (x0, y0, x1, y1) == (-(1 << 20),) * 2 + (1 << 20,) * 2      # the diagonal: centre i is (x0 + i, y0 + i)
            x0, y0, x1, y1 = -20, -20, max(H, W) + 20, max(H, W) + 20
        short.segment((x0, y0), (x1, y1), w, ((c >> 16) & 255, (c >> 8) & 255, c & 255))
    short._discs, short._texts = [discs], [texts]
    return brute_force(frame, short)


def test_trails_on_a_lane_scene():
    length = 5
    pts, _owners, line, _truth = tracks.lane_scene(K=12, frames=20, seed=3)
    steps, _st = tracks.tracks_host(pts, max_dist=12.0, lines=[line])
    pts.append(np.zeros((0, 2), np.float32))                        # and empty frames behind the clip, until every trail has gone
    steps += [(np.zeros(0, np.int32), np.zeros(0, np.uint32), steps[-1][2])] * (length + 2)
    pts += [pts[-1]] * (length + 1)
    trails = Trails(length)
    seen, last, history = {}, {}, {}
    for f, (p, (ids, _ev, _s)) in enumerate(zip(pts, steps), 1):
        ids = np.concatenate([ids, [-1]])                           # a point without a track: no trail
        p = np.concatenate([p, [[1.0, 2.0]]])
        for q, i in zip(p[:-1], ids[:-1].tolist()):
            seen[i] = seen.get(i, 0) + 1
            last[i] = f
            history.setdefault(i, []).append(q.astype(np.float64))
        tid, xy, n = trails.update(p, ids)
        assert -1 not in tid and np.array_equal(tid, np.sort(tid)) and xy.shape == (len(tid), length, 2)
        # every id seen within the last `length` frames has a trail, and no other
        assert tid.tolist() == sorted(i for i in last if f - last[i] <= length)
        lines = trails.polylines()
        for i, k in zip(tid.tolist(), n.tolist()):
            assert k == min(seen[i], length) == len(lines[i])
            assert np.array_equal(lines[i], np.asarray(history[i][-k:]))
    assert len(seen) >= 12 and max(seen.values()) > length and len(trails.ids) == 0
    with pytest.raises(ValueError):
        Trails(0)


def test_clip_marks_tallies_hit_colour_and_scene_anchoring():
    pts, _owners, line, _truth = tracks.lane_scene(K=10, frames=14, seed=1)
    lines = [line, (0.0, 300.0, 10.0, 300.0)]
    steps, _st = tracks.tracks_host(pts, max_dist=12.0, lines=lines)
    trails, hits = Trails(4), 0
    for p, (ids, ev, summary) in zip(pts, steps):
        tr = trails.update(p, ids)
        live = (tr[0].copy(), tr[1].copy(), tr[2].copy())
        m = clip_marks(p, ids, ev, summary, ["gate", "far"], lines, 9.26, size=(400, 220), trails=live)
        seg, disc, text = m.arrays()
        # trails first (half-width s - 1 = 0), then the two lines (half-width s = 1)
        assert len(seg) == int((live[2] - 1).sum()) + 2 and (seg[:-2, 4] == 0).all() and (seg[-2:, 4] == 1).all()
        crossed = bool((ev & 0x00010001).any())
        hits += crossed
        assert seg[-2, 5] == (0xffffff if crossed else 0x00ffff) and seg[-1, 5] == 0x00ffff
        assert np.array_equal(seg[-2, :4], overlay.round_coords([line[:2], line[2:]]).ravel())
        # a disc per point in its track's colour, a tag per tracked point
        assert len(disc) == len(p) and (disc[:, 2] == 2).all()
        assert disc[:, 3].tolist() == [(r << 16) | (g << 8) | b for r, g, b in (draw.track_color(i) for i in ids)]
        words = [bytes(t[6:].view(np.uint8)[:t[5]]).decode() for t in text]
        assert words[:len(p)] == ["%d" % i for i in ids]
        assert words[len(p):] == ["gate %d/%d" % (summary[8], summary[9]), "far 0/0", "count 9.3", "tracks %d" % summary[0], "total %d" % summary[2]]
        assert (text[len(p):, 4] == 0x202020).all() and (text[:len(p), 4] == -1).all()
        # under a camera the trails and the lines move against the camera, the points stay
        C = np.array([3.25, -7.5])
        sm = clip_marks(p, ids, ev, summary, ["gate", "far"], lines, 9.26, C, size=(400, 220), trails=live)
        sseg, sdisc, stext = sm.arrays()
        assert np.array_equal(sdisc, disc) and np.array_equal(stext[:len(p)], text[:len(p)])
        want = np.concatenate([overlay.round_coords(live[1][t, j] - C) for t in range(len(live[0])) for j in range(4 - live[2][t], 4)]
                              or [np.zeros((0, 2), np.int64)])
        ends = np.concatenate([sseg[:-2, 0:2], sseg[:-2, 2:4]])
        assert {tuple(v) for v in ends.tolist()} <= {tuple(v) for v in want.tolist()}
        assert np.array_equal(sseg[-2, :4], overlay.round_coords([np.asarray(line[:2]) - C, np.asarray(line[2:]) - C]).ravel())
    assert 0 < hits < len(pts) and int(steps[-1][2][8] + steps[-1][2][9]) > 0
    # the options, and the size of the marks
    bare = clip_marks(pts[-1], steps[-1][0], steps[-1][1], steps[-1][2], ["gate", "far"], lines, 1.0, size=(1920, 1080), tags=False, tally=False, hud=False)
    seg, disc, text = bare.arrays()
    assert len(text) == 0 and (seg[:, 4] == 2).all() and (disc[:, 2] == 4).all()
    assert [draw.mark_scale(h) for h in (60, 809, 810, 1080, 2160)] == [1, 1, 2, 2, 4] and draw.mark_scale(1080, 3) == 3
    assert draw.track_color(-1) == (128, 128, 128) and draw.track_color(17) == draw.PALETTE[1] and len(set(draw.PALETTE)) == 16
