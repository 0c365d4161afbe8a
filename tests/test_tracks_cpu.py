"""CPU: the tracking rule itself (include/countr_hip_tracks.h), as countr_amd.tracks_host restates it -- the yardstick the GPU tests hold
csrc_tracks/tracks.hip to.  Known answers on synthetic scenes: no accuracy claim is made or tested."""
import numpy as np
import pytest

from countr_amd import match_host, tracks_host
from countr_amd import tracks as TR

f32 = np.float32


def run(frames, **kw):
    kw.setdefault("max_dist", 8)
    return tracks_host([np.asarray(f, f32).reshape(-1, 2) for f in frames], **kw)


def test_one_frame_gives_ids_in_order():
    pts = np.random.RandomState(0).uniform(0, 1000, (37, 2)).astype(f32)
    (ids, events, summary), = run([pts])[0]
    assert ids.dtype == np.int32 and events.dtype == np.uint32 and summary.dtype == np.int32 and summary.shape == (40,)
    assert ids.tolist() == list(range(37)) and not events.any()
    assert summary[:8].tolist() == [37, 37, 0, 0, 37, 0, 0, 1] and not summary[8:].any()
    res, st = run([np.zeros((0, 2))])
    assert res[0][0].shape == (0,) and res[0][2][:8].tolist() == [0, 0, 0, 0, 0, 0, 0, 1] and st["id"].shape == (0,)


def test_every_step_s_association_is_match_host_on_the_predictions():
    frames, _own, line, _truth = TR.lane_scene(K=40, frames=10, seed=3)
    st = None
    for D in frames:
        before = TR.empty_state() if st is None else st
        p = np.stack([before["x"] + before["vx"], before["y"] + before["vy"]], 1).astype(f32).reshape(-1, 2)
        match, _d2 = match_host(D, p, 8)
        (ids, _ev, summary), = (got := tracks_host([D], max_dist=8, lines=[line], state=st))[0]
        st = got[1]
        hit = match >= 0
        assert np.array_equal(ids[hit], before["id"][match[hit]]) and summary[3] == hit.sum()
        assert np.array_equal(ids[~hit], before["started"] + np.arange((~hit).sum()))          # births in index order
        # the tracks stay in ascending id order
        assert np.all(np.diff(st["id"]) > 0)


def test_velocity_update_in_fp32():
    # dyadic values: exact by hand.  v = 0 + 0.5 (1.5 - 0) = 0.75; p = 2.25; v = 0.75 + 0.5 (3.25 - 2.25) = 1.25
    res, st = run([[(0, 0)], [(1.5, 0)], [(3.25, -1)]], min_hits=1)
    assert st["vx"].tolist() == [1.25] and st["vy"].tolist() == [-0.5] and st["x"].tolist() == [3.25] and st["lx"].tolist() == [3.25]
    assert st["hits"].tolist() == [3] and st["missed"].tolist() == [0] and [r[0].tolist() for r in res] == [[0]] * 3
    # values that round: every operation once, in fp32, in the written order
    beta, d1, d2 = f32(0.3), f32(1.1), f32(2.7)
    v1 = f32(f32(0) + f32(beta * f32(d1 - f32(0))))
    p2 = f32(d1 + v1)
    v2 = f32(v1 + f32(beta * f32(d2 - p2)))
    _res, st = run([[(0, 5)], [(d1, 5)], [(d2, 5)]], beta=0.3)
    assert st["vx"][0] == v2 and st["vx"].dtype == f32 and st["vy"][0] == 0
    # a coasting track takes its prediction and keeps v
    _res, st = run([[(0, 5)], [(d1, 5)], [(d2, 5)], []], beta=0.3)
    assert st["x"][0] == f32(d2 + v2) and st["vx"][0] == v2 and st["lx"][0] == d2 and st["missed"].tolist() == [1]


@pytest.mark.parametrize("max_missed", [0, 1, 2, 255])
def test_max_missed_edges(max_missed):
    gaps = min(max_missed, 3)
    # a still object seen, then `gaps` empty frames, then seen again: it survives; one empty frame more and it is gone
    res, st = run([[(5, 5)]] + [[]] * gaps + [[(5, 5)]], max_missed=max_missed)
    assert res[-1][0].tolist() == [0] and st["started"] == 1
    if max_missed < 255:
        res, st = run([[(5, 5)]] + [[]] * (max_missed + 1) + [[(5, 5)]], max_missed=max_missed)
        assert res[-1][0].tolist() == [1] and st["started"] == 2 and st["id"].tolist() == [1]
        assert res[max_missed + 1][2][:8].tolist() == [0, 1, 0, 0, 0, 1, 0, max_missed + 2]          # died on the step that passed the limit
        assert res[max_missed][2][5] == 0


@pytest.mark.parametrize("min_hits", [1, 2, 3])
def test_min_hits_edges(min_hits):
    res, st = run([[(5, 5)]] * 5, min_hits=min_hits)
    assert [int(r[2][2]) for r in res] == [int(k + 1 >= min_hits) for k in range(5)]      # confirmed once, when hits reaches min_hits
    assert st["confirmed"] == 1 and st["hits"].tolist() == [5]
    with pytest.raises(ValueError):
        run([[(5, 5)]], min_hits=0)
    with pytest.raises(ValueError):
        run([[(5, 5)]], min_hits=256)
    with pytest.raises(ValueError):
        run([[(5, 5)]], max_missed=256)
    with pytest.raises(ValueError):
        run([[(5, 5)]], max_dist=0)
    with pytest.raises(ValueError):
        run([[(5, 5)]], beta=1.5)
    with pytest.raises(ValueError):
        run([[(5, 5)]], lines=[(0, 0, 1, 1)] * 17)


LINE = (10.0, 0.0, 10.0, 20.0)          # side 1 is x <= 10: a move that ends there is "forward"


def counts_of(frames, lines=(LINE,), **kw):
    res, st = run(frames, lines=lines, max_dist=20, **kw)
    return [int(r[1][0]) if len(r[1]) else 0 for r in res], st["counts"][:len(lines)].tolist()


def test_crossings_both_directions_and_on_the_line_counts_once():
    assert counts_of([[(13, 5)], [(8, 5)]]) == ([0, 1], [[1, 0]])                        # forward: bit 0
    assert counts_of([[(8, 5)], [(13, 5)]]) == ([0, 1 << 16], [[0, 1]])                  # backward: bit 16
    # landing exactly on the line is side 1: right -> on counts forward, on -> left counts nothing
    assert counts_of([[(14, 5)], [(10, 5)], [(6, 5)]]) == ([0, 1, 0], [[1, 0]])
    # left -> on counts nothing, on -> right counts backward: once again
    assert counts_of([[(6, 5)], [(10, 5)], [(14, 5)]]) == ([0, 0, 1 << 16], [[0, 1]])
    # two lines: bits 0 and 1 / 16 and 17
    two = (LINE, (12.0, 0.0, 12.0, 20.0))
    assert counts_of([[(14, 5)], [(8, 5)], [(14, 5)]], two) == ([0, 3, 3 << 16], [[1, 1], [1, 1]])


def test_what_counts_nothing():
    # beyond the segment's end (the segment spans y 0 .. 20)
    assert counts_of([[(13, 25)], [(8, 25)]]) == ([0, 0], [[0, 0]])
    assert counts_of([[(13, 19)], [(8, 24)]]) == ([0, 0], [[0, 0]])                      # crosses the line's extension at y = 21.4
    # a zero-length line, a zero-length move
    assert counts_of([[(13, 5)], [(8, 5)]], ((10.0, 5.0, 10.0, 5.0),)) == ([0, 0], [[0, 0]])
    assert counts_of([[(10, 5)], [(10, 5)], [(10, 5)]]) == ([0, 0, 0], [[0, 0]])
    # a coasting step: the estimate passes the line, no detection does; the next matched move (13 -> 5) counts once
    ev, counts = counts_of([[(19, 5)], [(16, 5)], [(13, 5)], [], [(5, 5)]])
    assert ev[:3] == [0, 0, 0] and ev[4] == 1 and counts == [[1, 0]]


def test_capacity_and_dropped():
    grid = np.stack(np.meshgrid(np.arange(64), np.arange(64)), -1).reshape(-1, 2).astype(f32) * 100
    far = grid[:10] + f32(50)
    # 4090 live tracks, four of them coasting: six of the ten far-away detections start a track, four are dropped
    res, st = run([grid[:4090], np.concatenate([grid[:4086], far])], max_dist=8)
    ids, _ev, summary = res[1]
    assert ids[:4086].tolist() == list(range(4086)) and ids[4086:].tolist() == [4090, 4091, 4092, 4093, 4094, 4095, -1, -1, -1, -1]
    assert summary[:8].tolist() == [4096, 4096, 0, 4086, 6, 0, 4, 2] and st["dropped"] == 4 and st["id"].shape == (4096,)
    assert np.all(np.diff(st["id"]) > 0)
    # at capacity every unmatched detection is dropped, and the counter adds up over steps
    res, st = run([np.concatenate([grid[:4086], far])], max_dist=8, state=st)
    assert res[0][0][4086:].tolist() == [4090, 4091, 4092, 4093, 4094, 4095, -1, -1, -1, -1] and res[0][2][:8].tolist() == [4096, 4096, 4086, 4092, 0, 0, 8, 3]          # (the 4086 seen three times are confirmed)
    # a death frees its slot on the same step: the survivors are counted first
    res, st = run([grid, np.concatenate([grid[3:], far[:3]])], max_dist=8, max_missed=0)
    assert res[1][0][-3:].tolist() == [4096, 4097, 4098] and res[1][2][:8].tolist() == [4096, 4099, 0, 4093, 3, 3, 0, 2]
    assert st["id"][:2].tolist() == [3, 4] and st["id"][-3:].tolist() == [4096, 4097, 4098]


def test_non_finite_detections():
    pts = np.array([(5, 5), (np.nan, 7), (9, np.inf), (40, 40), (-np.inf, np.nan)], f32)
    res, st = run([pts, pts])
    for ids, ev, summary in res:
        assert ids.tolist() == [0, -1, -1, 1, -1] and not ev.any() and summary[6] == 0
    assert st["started"] == 2 and st["dropped"] == 0 and st["hits"].tolist() == [2, 2]


def test_a_run_split_in_two_equals_one_run():
    frames, _own, line, _truth = TR.lane_scene(K=30, frames=12, seed=5)
    kw = dict(max_dist=8, lines=[line], max_missed=1, min_hits=2, beta=0.4)
    whole, st = tracks_host(frames, **kw)
    head, mid = tracks_host(frames[:5], **kw)
    snapshot = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in mid.items()}
    tail, end = tracks_host(frames[5:], state=mid, **kw)
    assert TR.states_equal(mid, snapshot)                                                # the state handed in is left unchanged
    assert TR.states_equal(end, st)
    for (a, b, c), (d, e, f) in zip(whole, head + tail):
        assert np.array_equal(a, d) and np.array_equal(b, e) and np.array_equal(c, f)


def test_known_answer_scene():
    """70 objects on lanes 20 px apart, 2..6 px/frame either way, jitter under 0.5 px, shuffled detections, drop-outs of at most 2
    frames and none in the first 3, 24 frames, max_dist = 8, one vertical line."""
    frames, owners, line, truth = TR.lane_scene(K=70, frames=24, seed=0)
    assert len(frames) == 24 and all(len(f) == 70 for f in frames[:3]) and min(len(f) for f in frames) < 70
    gone = np.ones((24, 70), bool)
    for f, who in enumerate(owners):
        gone[f, who] = False
    assert gone.any() and not (gone[:-2] & gone[1:-1] & gone[2:]).any()                  # at most 2 consecutive drop-outs
    assert any(not np.array_equal(a, np.sort(a)) for a in owners)                        # shuffled
    res, st = tracks_host(frames, max_dist=8, lines=[line])
    assert st["started"] == st["confirmed"] == 70 and st["dropped"] == 0 and st["id"].shape == (70,)
    assert truth == (20, 10) and st["counts"][0].tolist() == list(truth) and not st["counts"][1:].any()
    track_of = {}
    for (ids, _ev, _s), who in zip(res, owners):                                         # an object keeps its id through the clip
        for i, k in zip(ids.tolist(), who.tolist()):
            assert track_of.setdefault(k, i) == i
    assert sorted(track_of.values()) == list(range(70))
    counts = TR.clip_counts(res[-1][2], 1)
    assert counts[:3] == (70, 70, 0) and counts.line_counts.tolist() == [[20, 10]] and counts.live == 70
