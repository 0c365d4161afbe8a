"""GPU: countr_tracks_step (csrc_tracks/tracks.hip) through ctypes and through countr_amd.Tracker against countr_amd.tracks_host: ids,
events, summary and the downloaded state are EQUAL after every step, bit for bit -- minima, integer scans and written-out fp32 / fp64
arithmetic leave no tolerance.  Then count_clip on the tiny model against locate_frames + tracks_host, and the demo's --track."""
import ctypes as C
import functools
import json
import os
import re
import subprocess
import sys
from functools import partial

import numpy as np
import pytest
import torch

from oracle import weights as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
PAD, SENTINEL = 16, 0x5A5A5A5A          # 32-bit words between all output slices, and what they hold


# ---- the scenes
@functools.lru_cache(maxsize=None)
def scene(name):
    """-> dict(frames, max_dist, max_missed, min_hits, beta, lines)."""
    from countr_amd import tracks as TR
    kw = dict(max_dist=8.0, max_missed=2, min_hits=3, beta=0.5, lines=())
    rs = np.random.RandomState(11)
    if name == "empties_and_one":          # empty frames at the start and in the middle, a single point
        z = np.zeros((0, 2), f32)
        pt = lambda x, y: np.array([(x, y)], f32)
        frames = [z, z, pt(5, 5), pt(7, 6), z, pt(12, 7), z, z, z, pt(13, 7), z]
        kw.update(lines=[(9.5, 0.0, 9.5, 20.0)], min_hits=2)
    elif name == "lanes70":                # crosses the 64-lane wave boundary
        frames, _own, line, _truth = TR.lane_scene(K=70, frames=24, seed=0)
        kw.update(lines=[line])
    elif name == "lattice":                # integer coordinates: many d2 tie, the (d2, i, j) order decides
        g = np.stack(np.meshgrid(np.arange(12), np.arange(11)), -1).reshape(-1, 2).astype(f32) * 2
        frames = [g[rs.permutation(len(g))] + f32(k) * np.array([1, (k % 2)], f32) for k in range(5)]
        frames[3] = frames[3][:100]
        kw.update(max_dist=2.0, lines=[(6.0, -1.0, 6.0, 30.0), (-1.0, 7.0, 40.0, 7.0), (3.0, 3.0, 3.0, 3.0)], max_missed=1, min_hits=1)
    elif name == "ladder":                 # one round per pair (tests/test_match_cpu.py): tracks from frame 0, detections in frame 1
        xs = np.concatenate([[0.0], np.cumsum(1.0 + 0.01 * np.arange(63))])
        zero = np.zeros(32)
        frames = [np.stack([xs[0::2][::-1], zero], 1).astype(f32), np.stack([xs[1::2][::-1], zero], 1).astype(f32)]
        kw.update(max_dist=1000.0, lines=[(30.0, -5.0, 30.0, 5.0)])
    elif name == "non_finite":
        frames = [rs.uniform(0, 60, (90, 2)).astype(f32) for _ in range(4)]
        for k, fr in enumerate(frames):
            fr[3 + k, 0], fr[17, 1], fr[40 + k] = np.nan, np.inf, (-np.inf, np.nan)
        frames[2][60, 0] = 1e30
        kw.update(max_dist=5.0, lines=[(30.0, 0.0, 30.0, 60.0)], max_missed=0)
    elif name == "capacity":               # 4096 live tracks, then 10 far-away detections that are dropped; then deaths and compaction
        g = np.stack(np.meshgrid(np.arange(64), np.arange(64)), -1).reshape(-1, 2).astype(f32) * 100
        frames = [g, np.concatenate([g[rs.permutation(4096)][:4086] + f32(1), g[:10] + f32(50)]), g[5:], g[5:][::-1]]
        kw.update(max_dist=8.0, max_missed=1, lines=[(3100.5, -10.0, 3100.5, 7000.0)])
    elif name.startswith("mixed_"):        # different N including 0, different lines and different parameters
        k = int(name.split("_")[1])
        n = [0, 1, 63, 64, 65, 130, 257, 5][k % 8]
        pts = rs.uniform(0, 120, (n, 2))
        vel = rs.uniform(-3, 3, (n, 2))
        frames = []
        for f in range(4):
            keep = rs.rand(n) > 0.15
            cur = (pts + vel * f + rs.uniform(-0.3, 0.3, (n, 2)))[keep]
            frames.append(cur[rs.permutation(len(cur))].astype(f32))
        if k % 5 == 2:
            frames[1] = np.zeros((0, 2), f32)
        kw.update(max_dist=[4.0, 6.5, 30.0][k % 3], max_missed=k % 3, min_hits=1 + k % 4, beta=[0.0, 0.25, 0.5, 1.0][k % 4],
                  lines=[(10.0 * (j + 1) + k, -5.0, 10.0 * (j + 1), 130.0) for j in range(k % 5)] + ([(0.0, 60.0, 120.0, 61.0)] if k % 2 else []))
    else:
        raise KeyError(name)
    kw["frames"] = frames
    return kw


@functools.lru_cache(maxsize=None)
def want(name):
    """The host rule, step by step: [(ids, events, summary, state after the step), ...]."""
    from countr_amd import tracks_host
    sc = dict(scene(name))
    frames, st, out = sc.pop("frames"), None, []
    for D in frames:
        (r,), st = tracks_host([D], state=st, **sc)
        out.append(r + (st,))
    return out


# ---- 1. the export through ctypes
def run_abi(names, stream=None):
    """The scenes as the trackers of ONE call per frame; the states start as garbage and go through countr_tracks_reset.  Every output
    slice lies between sentinel pads.  -> per scene and step (ids, events, summary, state); the bytes of the whole output buffer."""
    from countr_amd import _lib
    from countr_amd import tracks as TR
    L = _lib.tracks_lib()
    scs = [scene(n) for n in names]
    n = len(scs)
    steps = max(len(sc["frames"]) for sc in scs)
    where, words, floats = {}, PAD, 0
    for s, sc in enumerate(scs):
        for f, D in enumerate(sc["frames"]):
            N = len(D)
            where[s, f] = (floats, words, words + N + PAD, words + 2 * (N + PAD))
            floats += 2 * N
            words += 2 * (N + PAD) + TR.SUMMARY_INTS + PAD
    host = np.concatenate([np.asarray(D, f32).reshape(-1) for sc in scs for D in sc["frames"]] + [np.zeros(2, f32)])
    lines_host = np.zeros((n, 16, 4), f32)
    for s, sc in enumerate(scs):
        lines_host[s, :len(sc["lines"])] = np.asarray(sc["lines"], f32).reshape(-1, 4)
    pts, lines = torch.from_numpy(host).cuda(), torch.from_numpy(lines_host).cuda()
    out = torch.full((words,), SENTINEL, dtype=torch.int32, device="cuda")
    states = torch.full((n, TR.STATE_BYTES), 0xAB, dtype=torch.uint8, device="cuda")
    ws_bytes = L.countr_tracks_workspace(n, max(len(D) for sc in scs for D in sc["frames"]))
    assert ws_bytes > 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    st = C.c_void_p(stream.cuda_stream) if stream is not None else None
    ptrs = (C.c_void_p * n)(*[states[s].data_ptr() for s in range(n)])
    _lib.tracks_check(L.countr_tracks_reset(ptrs, n, st), "countr_tracks_reset")
    recs = (_lib.TracksStream * 16)()
    got = [[] for _ in scs]
    for f in range(steps):
        live = [s for s, sc in enumerate(scs) if f < len(sc["frames"])]
        for k, s in enumerate(live):
            sc, d = scs[s], recs[k]
            N = len(sc["frames"][f])
            fo, io, eo, so = where[s, f]
            d.state, d.summary = states[s].data_ptr(), out.data_ptr() + 4 * so
            d.points, d.ids, d.events = (pts.data_ptr() + 4 * fo, out.data_ptr() + 4 * io, out.data_ptr() + 4 * eo) if N else (None, None, None)
            d.lines, d.L, d.N = (lines[s].data_ptr() if len(sc["lines"]) else None), len(sc["lines"]), N
            d.max_dist, d.beta, d.max_missed, d.min_hits = sc["max_dist"], sc["beta"], sc["max_missed"], sc["min_hits"]
        _lib.tracks_check(L.countr_tracks_step(recs, len(live), ws.data_ptr(), st), "countr_tracks_step")
        (stream or torch.cuda.current_stream()).synchronize()
        raw, o = states.cpu().numpy(), out.cpu().numpy()
        for s in live:
            N = len(scs[s]["frames"][f])
            _fo, io, eo, so = where[s, f]
            got[s].append((o[io:io + N].copy(), o[eo:eo + N].view(np.uint32).copy(), o[so:so + TR.SUMMARY_INTS].copy(),
                           TR.state_from_bytes(raw[s].tobytes())))
    o = out.cpu().numpy()
    used = np.zeros(words, bool)
    for (s, f), (_fo, io, eo, so) in where.items():
        N = len(scs[s]["frames"][f])
        used[io:io + N] = used[eo:eo + N] = used[so:so + TR.SUMMARY_INTS] = True
    assert (o[~used].view(np.uint32) == SENTINEL).all() and (~used).sum() >= PAD * (3 * len(where) + 1)
    return got, o.tobytes()


def compare(names, got):
    from countr_amd import tracks as TR
    for name, steps in zip(names, got):
        ref = want(name)
        assert len(steps) == len(ref)
        for f, ((ids, ev, summary, st), (wi, we, ws, wst)) in enumerate(zip(steps, ref)):
            assert ids.dtype == wi.dtype and np.array_equal(ids, wi), (name, f)
            assert ev.dtype == we.dtype and np.array_equal(ev, we), (name, f)
            assert np.array_equal(summary, ws), (name, f, summary[:8], ws[:8])
            assert TR.states_equal(st, wst), (name, f)


SCENES = ["empties_and_one", "lanes70", "lattice", "ladder", "non_finite", "capacity"]
MIXED = ["mixed_%d" % k for k in range(16)]


@pytest.mark.parametrize("name", SCENES)
def test_kernel_equals_the_host_rule_after_every_step(name):
    compare([name], run_abi([name])[0])


def test_the_scenes_hold_what_they_are_for():
    from countr_amd.match import match_rounds_host
    lad = scene("ladder")["frames"]
    assert match_rounds_host(lad[1], lad[0], 1000.0)[2] == 32                                # a round per pair
    ref = want("lattice")
    st0 = ref[0][3]
    D = scene("lattice")["frames"][1]
    d2 = ((D[:, None, :] - np.stack([st0["x"], st0["y"]], 1)[None]) ** 2).sum(-1)
    assert ((d2 == d2.min(1, keepdims=True)).sum(1) > 1).sum() > 50                           # many detections with tied nearest tracks
    assert ref[-1][2][8:12].min() > 0 and not ref[-1][2][12:].any()                           # lines that are crossed both ways; the zero-length one never
    cap = want("capacity")
    assert cap[0][2][:8].tolist() == [4096, 4096, 0, 0, 4096, 0, 0, 1]
    assert cap[1][2][:8].tolist() == [4096, 4096, 0, 4086, 0, 0, 10, 2] and cap[1][0][-10:].tolist() == [-1] * 10
    assert cap[3][2][5] >= 5 and cap[3][2][0] < 4096 and cap[3][3]["id"][0] > 0               # deaths, and the compaction behind them
    nf = want("non_finite")
    assert all((r[0] == -1).sum() >= 3 for r in nf) and nf[-1][2][6] == 0
    lanes = want("lanes70")[-1][2]
    assert lanes[:3].tolist() == [70, 70, 70] and lanes[8:10].tolist() == [20, 10]
    assert any(len(scene(n)["lines"]) == 0 for n in MIXED) and any(len(scene(n)["lines"]) == 5 for n in MIXED)
    assert any(int(want(n)[-1][2][8:].sum()) > 0 for n in MIXED)


def test_sixteen_trackers_in_one_call_and_two_runs_give_the_same_bytes():
    got, raw = run_abi(MIXED)
    compare(MIXED, got)
    again, raw2 = run_abi(MIXED)
    assert raw == raw2
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other, raw3 = run_abi(MIXED, stream=side)
    assert raw3 == raw
    compare(MIXED, other)


# ---- 2. the Tracker
def tracker_for(sc, **kw):
    from countr_amd import Tracker
    return Tracker("cuda", max_dist=sc["max_dist"], max_missed=sc["max_missed"], min_hits=sc["min_hits"], beta=sc["beta"], lines=sc["lines"], **kw)


def same_steps(got, ref):
    assert len(got) == len(ref)
    for (ids, ev, summary), r in zip(got, ref):
        assert ids.dtype == np.int32 and ev.dtype == np.uint32 and summary.dtype == np.int32
        assert np.array_equal(ids, r[0]) and np.array_equal(ev, r[1]) and np.array_equal(summary, r[2])


@pytest.mark.parametrize("name", ["empties_and_one", "lanes70", "lattice"])
def test_tracker_run_reset_split_and_streams(name):
    from countr_amd import tracks as TR
    sc, ref = scene(name), want(name)
    t = tracker_for(sc)
    same_steps(t.run(sc["frames"]), ref)
    assert TR.states_equal(t.state(), ref[-1][3])
    assert t.run([]) == []
    # a clip run as two calls equals one call; reset() starts over
    t.reset()
    assert TR.states_equal(t.state(), TR.empty_state())
    cut = len(sc["frames"]) // 2
    same_steps(t.run(sc["frames"][:cut]) + t.run(sc["frames"][cut:]), ref)
    assert TR.states_equal(t.state(), ref[-1][3])
    # a run on a non-default stream equals a run on the default stream, and the buffers did not grow
    sizes = (t._ws.numel(), t._pts.numel(), t._out.numel())
    side = torch.cuda.Stream()
    t.reset()
    with torch.cuda.stream(side):
        same_steps(t.run(sc["frames"]), ref)
    more, _st = TR.tracks_host(sc["frames"][:1], state=ref[-1][3], **{k: v for k, v in sc.items() if k != "frames"})
    same_steps(t.run(sc["frames"][:1]), more)                      # back on the default stream: the call waits for the side stream's event
    assert (t._ws.numel(), t._pts.numel(), t._out.numel()) == sizes


def test_seventeen_trackers_are_chunked():
    from countr_amd import Tracker, _lib
    from countr_amd import tracks as TR
    sc = dict(scene("lanes70"))
    frames = sc["frames"]
    per = [[fr[(np.arange(len(fr)) + 3 * s) % len(fr)][:len(fr) - s] for fr in frames[:6 + s % 3]] for s in range(17)]      # different N, different lengths
    per[5] = []
    t = tracker_for(sc, streams=17)
    got = t.run(per)
    kw = {k: v for k, v in sc.items() if k != "frames"}
    for s in range(17):
        ref, st = TR.tracks_host(per[s], **kw)
        same_steps(got[s], ref)
        assert TR.states_equal(t.state(s), st)
    with pytest.raises(ValueError, match="17 streams"):
        t.run(per[:16])
    with pytest.raises(_lib.CountrError, match="no CPU fallback"):
        Tracker("cpu", max_dist=1.0)


# ---- 3. count_clip on the tiny configuration
@pytest.fixture(scope="module")
def model():
    import torch.nn as nn
    from countr_amd.models_mae_cross import SupervisedMAE
    p, D, depth, H, Dd, ddepth, Hd = W.CONFIGS["tiny_test"]
    m = SupervisedMAE(patch_size=p, embed_dim=D, depth=depth, num_heads=H, decoder_embed_dim=Dd, decoder_depth=ddepth, decoder_num_heads=Hd,
                      mlp_ratio=4, norm_layer=partial(nn.LayerNorm, eps=1e-6), precision="fp32")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.make_state_dict("tiny_test", seed=3).items()}, strict=True)
    return m.to("cuda").eval()


def nv12_frames(n, H=60, Wd=90, seed=7):
    from countr_amd import YuvFrame
    rs = np.random.RandomState(seed)
    return [YuvFrame(rs.randint(0, 256, (H, Wd)).astype(np.uint8), rs.randint(0, 256, ((H + 1) // 2, 2 * ((Wd + 1) // 2))).astype(np.uint8),
                     format="nv12") for _ in range(n)]


def check_clip(model, frames, boxes, group, **kw):
    from countr_amd import ClipCounts, count_clip, locate_frames, tracks_host
    lines = [(45.0, -1.0, 45.0, 61.0), (-1.0, 30.0, 91.0, 30.0)]
    trk = dict(max_dist=25.0, max_missed=1, min_hits=2, beta=0.5)
    peak = dict(radius=3, rel_threshold=0.05)
    got, clip = count_clip(model, frames, boxes, lines=lines, group=group, **trk, **peak, **kw)
    assert len(got) == len(frames) and isinstance(clip, ClipCounts)
    ref = []
    for g0 in range(0, len(frames), group):
        ref += locate_frames(model, frames[g0:g0 + group], boxes[g0:g0 + group] if boxes is not None else None, **peak)
    for a, b in zip(got, ref):
        assert len(a) == 6 and a[0] == b[0] and torch.equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    steps, st = tracks_host([b[2] for b in ref], lines=lines, **trk)
    for a, (ids, ev, _s) in zip(got, steps):
        assert np.array_equal(a[4], ids) and np.array_equal(a[5], ev) and a[4].dtype == np.int32 and a[5].dtype == np.uint32
    assert clip[:3] == (st["started"], st["confirmed"], st["dropped"]) and clip.live == len(st["id"])
    assert clip.line_counts.shape == (2, 2) and np.array_equal(clip.line_counts, st["counts"][:2])
    assert sum(len(b[2]) for b in ref) > 0 and st["started"] > 0
    return got, clip, st


def test_count_clip_on_host_rgb_frames(model):
    from countr_amd import Tracker, count_clip, tracks_host
    rs = np.random.RandomState(3)
    frames = [rs.randint(0, 256, (60, 90, 3)).astype(np.uint8) for _ in range(5)]
    boxes = [[(5, 5, 30, 30), (50, 10, 80, 40), (20, 30, 45, 55)]] * 5
    got, clip, st = check_clip(model, frames, boxes, 2)
    check_clip(model, frames, None, 8)
    # tracker=: the live-stream case -- two calls continue one tracker and equal one call
    t = Tracker("cuda", max_dist=25.0, max_missed=1, min_hits=2, lines=[(45.0, -1.0, 45.0, 61.0), (-1.0, 30.0, 91.0, 30.0)])
    peak = dict(radius=3, rel_threshold=0.05)
    a, _c = count_clip(model, frames[:2], boxes[:2], max_dist=25.0, group=2, tracker=t, **peak)
    b, clip2 = count_clip(model, frames[2:], boxes[2:], max_dist=25.0, group=2, tracker=t, summaries=True, **peak)
    for x, y in zip(a + b, got):
        assert np.array_equal(x[4], y[4]) and np.array_equal(x[5], y[5])
    assert clip2[:3] == clip[:3] and np.array_equal(clip2.line_counts, clip.line_counts) and clip2.live == clip.live
    assert b[-1][6].shape == (40,) and b[-1][6][7] == 5
    with pytest.raises(ValueError, match="the lines are its own"):
        count_clip(model, frames[:1], max_dist=25.0, tracker=t, lines=[])
    empty, none = count_clip(model, [], max_dist=3.0)
    assert empty == [] and none[:3] == (0, 0, 0) and none.live == 0 and none.line_counts.shape == (0, 2)


def test_count_clip_on_yuv_frames(model):
    frames = nv12_frames(4)
    check_clip(model, frames, None, 3)


def test_shared_exemplars_equal_count_items_on_the_shared_crop_items(model):
    from countr_amd import count_clip, frames as FR
    clip = nv12_frames(3, seed=9)
    bx = [(10, 10, 11, 11), (40, 20, 41, 21), (70, 40, 71, 41)]            # under 10 px: with rectangles these would take the 3 x 3 split
    got, _c = count_clip(model, clip, (1, bx), max_dist=10.0, group=2)
    crops = FR.cut_exemplars("cuda", clip[1], bx)
    assert tuple(crops.shape) == (1, 3, 3, 64, 64)
    items = FR.shared_exemplar_items("cuda", clip, crops)
    assert all(r is None and ex is crops for _im, ex, r in items)
    ref = FR.count_items(model, items[:2]) + FR.count_items(model, items[2:])
    for a, (c, dm) in zip(got, ref):
        assert a[0] == c and torch.equal(a[1], dm)
    # and they differ from the per-frame form, which cuts each frame's own crops
    own = FR.count_items(model, FR.prepare_items("cuda", clip, [bx] * 3))
    assert any(not torch.equal(a[1], dm) for a, (_c2, dm) in zip(got, own))
    with pytest.raises(ValueError, match="names a frame of the call"):
        count_clip(model, clip, (3, bx), max_dist=10.0)


# ---- 4. the demo in a fresh child process
def test_demo_zero_track_on_a_raw_clip(tmp_path):
    from PIL import Image
    Wd, H = 80, 96
    size = Wd * H * 3 // 2
    raw = np.random.RandomState(5).randint(0, 256, 3 * size).astype(np.uint8)
    clip = tmp_path / "clip.yuv"
    clip.write_bytes(raw.tobytes())
    lines = tmp_path / "lines.json"
    lines.write_text(json.dumps({"gate": [[40, -1], [40, 97]], "mid": [[-1, 48], [81, 48]]}))
    out = tmp_path / "out"
    cmd = [sys.executable, "demo_zero.py", "--yuv", "nv12:80x96", "--model_path", "", "--output_path", str(out), "--input_path", str(clip),
           "--track", "--track_dist", "30", "--lines_json", str(lines), "--track_hits", "2", "--group_images", "2"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    rows = re.findall(r"^clip#(\d+): Count: (\S+) - Time: \S+ - tracks: (\d+) - crossed: (\{.*\})$", r.stdout, re.M)
    assert [int(k) for k, _c, _t, _x in rows] == [0, 1, 2], r.stdout
    crossed = [json.loads(x) for _k, _c, _t, x in rows]
    assert all(list(c) == ["gate", "mid"] for c in crossed)
    doc = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{"clip"')][-1])
    assert doc == json.load(open(out / "tracks_clip.json")) and list(doc["clip"]) == ["started", "confirmed", "lines"]
    assert doc["clip"]["lines"] == {n: [sum(c[n][0] for c in crossed), sum(c[n][1] for c in crossed)] for n in ("gate", "mid")}
    ids = []
    for k in range(3):
        pj = json.load(open(out / ("points_clip_%d.json" % k)))
        assert len(pj["ids"]) == len(pj["points"]) and float(rows[k][1]) == pj["count"]
        ids += pj["ids"]
        assert Image.open(out / ("viz_clip_%d.jpg" % k)).size == (Wd, H)
    assert doc["clip"]["started"] == max(ids + [-1]) + 1 and doc["clip"]["confirmed"] <= doc["clip"]["started"]
    assert int(rows[-1][2]) <= doc["clip"]["started"]
    # --track needs --yuv and --track_dist
    r = subprocess.run(cmd[:-8] + ["--track"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--track is for --yuv and needs --track_dist" in r.stderr
