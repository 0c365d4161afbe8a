"""GPU: csrc_cam/cam.hip against countr_amd.cam's host rule -- records, flags and compensated fields byte for byte (all of it is integer
arithmetic) -- FlowCounter(camera="translation") against flow_host(camera=...), count_flow and count_clip with a camera on the tiny
model, and demo_zero.py --flow --camera translation.

The flux bound is tests/test_flow_gpu.py's, derived there: the device and flow_host sum the SAME fp32 terms v, the device in fp32 in a
fixed order, the host in float64, so they differ by at most n u sum|v| plus one ulp of the result, u = 2^-24.  The camera changes the
field and the placement that form the terms, identically on both sides, and nothing about the sums."""
import ctypes as C
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
U = 2.0 ** -24
GUARD = 0x5A


def smooth(h, w, seed):
    rs = np.random.RandomState(seed)
    a = rs.uniform(0, 1, (h // 4 + 3, w // 4 + 3))
    a = np.kron(a, np.ones((4, 4)))
    k = np.ones(7) / 7
    for ax in (0, 1):
        a = np.apply_along_axis(lambda v: np.convolve(v, k, "same"), ax, a)
    a = a[4:4 + h, 4:4 + w]
    return np.floor(255 * (a - a.min()) / (a.max() - a.min())).astype(np.uint8)


def translated(h, w, n, seed, step):
    """n lumas cut from one smooth texture, the cut moving by `step` = (dx, dy) >= 0 per frame."""
    dx, dy = step
    big = smooth(h + dy * n, w + dx * n, seed)
    return [np.ascontiguousarray(big[dy * t:dy * t + h, dx * t:dx * t + w]) for t in range(n)]


def pairs(h, w, n, kind, seed=0):
    """n (field, luma) pairs.  motion: a panned texture with a flat block and motion_host's fields; any: every int16, noise lumas with
    flat cells; equal: one offset everywhere; edge: offsets of +-264 and +-265."""
    from countr_amd import flow as F
    rs = np.random.RandomState(seed + h + w)
    if kind == "motion":
        lumas = translated(h, w, n + 1, seed + 1, (2, 1))
        for L in lumas:
            L[h // 4:h // 2, w // 4:w // 2] = 90                                    # flat cells that rest, whatever the camera does
        return [F.motion_host(lumas[t + 1], lumas[t], 4, 256) for t in range(n)], lumas[1:]
    lumas = []
    for t in range(n):
        L = rs.randint(0, 256, (h, w)).astype(np.uint8)
        L[:h // 2, :8 * ((w // 8 + 1) // 2)] //= 64                                 # cells around min_texture = 128 on both sides
        lumas.append(L)
    shape = (n, h // 8, w // 8, 2)
    if kind == "any":
        V = rs.randint(-32768, 32768, shape).astype(np.int16)
        V[rs.uniform(size=shape[:3]) < 0.5] = rs.randint(-40, 41, 2)               # half of the cells agree; a few rest
        V[rs.uniform(size=shape[:3]) < 0.1] = 0
    elif kind == "equal":
        V = np.empty(shape, np.int16)
        V[...] = (-37, 264)
    else:
        V = rs.choice(np.array([-265, -264, 264, 265], np.int16), shape)
    return list(V), lumas


def device_rule(fields, lumas, in_place=False, settings=(128, 8, 16)):
    """countr_cam_estimate and _compensate on n <= 16 pairs through the C ABI, every output followed by guard bytes -> (records, flags,
    compensated fields) as numpy arrays."""
    from countr_amd import _lib
    L = _lib.cam_lib()
    n, (h, w) = len(fields), lumas[0].shape
    cells = (h // 8) * (w // 8)
    dl = [torch.from_numpy(l).cuda() for l in lumas]
    df = [torch.from_numpy(np.concatenate([f.reshape(-1), np.full(8, 0x5A5A, np.int16)])).cuda() for f in fields]
    do = df if in_place else [torch.full((2 * cells + 8,), 0x5A5A, dtype=torch.int16, device="cuda") for _ in fields]
    rec = torch.full((8 * n + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    flags = torch.full((n * cells + 64,), GUARD, dtype=torch.uint8, device="cuda")
    ws = torch.empty(L.countr_cam_workspace(n, h, w), dtype=torch.uint8, device="cuda").fill_(0xFF)      # the call clears it itself
    arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.cam_check(L.countr_cam_estimate(arr(df), arr(dl), rec.data_ptr(), flags.data_ptr(), n, h, w, *settings, ws.data_ptr(), st), "estimate")
    _lib.cam_check(L.countr_cam_compensate(arr(df), rec.data_ptr(), flags.data_ptr(), arr(do), n, h, w, st), "compensate")
    torch.cuda.synchronize()
    rec, flags, out = rec.cpu().numpy(), flags.cpu().numpy(), [o.cpu().numpy() for o in do]
    assert (rec[8 * n:] == 0x5A5A5A5A).all() and (flags[n * cells:] == GUARD).all()  # bytes beyond the outputs are untouched
    assert all((o[2 * cells:] == 0x5A5A).all() for o in out)
    if not in_place:
        assert all(np.array_equal(d.cpu().numpy()[:2 * cells], f.reshape(-1)) for d, f in zip(df, fields))
    return rec[:8 * n].reshape(n, 8), flags[:n * cells].reshape(n, h // 8, w // 8), np.stack([o[:2 * cells].reshape(h // 8, w // 8, 2) for o in out])


def host_rule(fields, lumas, settings=(128, 8, 16)):
    from countr_amd import cam
    rec, flags, out = [], [], []
    for V, L in zip(fields, lumas):
        r, f = cam.estimate_host(V, L, *settings)
        rec.append(r)
        flags.append(f)
        out.append(cam.compensate_host(V, r, f))
    return np.stack(rec), np.stack(flags), np.stack(out)


@pytest.mark.parametrize("h,w,n,kind", [
    (16, 24, 1, "motion"),               # six cells: under min_voters
    (16, 24, 2, "equal"),
    (96, 192, 16, "motion"),
    (96, 192, 3, "edge"),
    (384, 64, 2, "any"),                 # 48 cell rows of eight cells
    (384, 296, 2, "motion"),             # 37 cells a row: not a multiple of a wave, two rounds of a block's columns
    (384, 296, 1, "any"),
    (384, 296, 1, "equal"),
])
def test_estimate_and_compensate_equal_the_host_rule(h, w, n, kind):
    fields, lumas = pairs(h, w, n, kind)
    want = host_rule(fields, lumas)
    got = device_rule(fields, lumas)
    for a, b, what in zip(got, want, ("records", "flags", "fields")):
        assert a.dtype == b.dtype and np.array_equal(a, b), (what, np.argwhere(a != b)[:5])
    again = device_rule(fields, lumas, in_place=True)                              # two runs give the same bytes, in place too
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    rec = want[0]
    print("%s %dx%d: g %s voters %s inliers %s valid %s" % (kind, h, w, rec[:, :2].tolist(), rec[:, 2].tolist(), rec[:, 3].tolist(), rec[:, 4].tolist()))
    if (h, w) == (16, 24):
        assert not rec[:, 4].any() and (rec[:, 2] <= 6).all()
    elif kind == "motion":
        assert rec[:, 4].all() and (np.abs(rec[:, :2] - (32, 16)) <= 8).all()        # the cut moves by (2, 1) px a frame
        flat = want[1] == 0
        assert flat.any() and (want[2][flat] == 0).all(-1).any()                   # a flat cell that rests stays at rest
    elif kind == "equal":
        assert rec[:, 4].all() and (rec[:, :2] == (-37, 264)).all() and (rec[:, 2] == rec[:, 3]).all()
    elif kind == "edge":
        assert rec[:, 2].min() > 0 and (rec[:, 2] < rec[:, 5]).all()              # +-265 did not vote


def test_other_settings_and_the_validity_edges_on_the_device():
    from countr_amd import cam
    L = np.random.RandomState(1).randint(0, 256, (32, 64)).astype(np.uint8)

    def field_of(offsets):
        V = np.full((4, 8, 2), 9999, np.int16)
        V.reshape(-1, 2)[:len(offsets)] = offsets
        return V
    half = field_of([(0, 0)] * 8 + [(100 + 20 * k, 0) for k in range(8)])           # 2 * inliers == n
    fewer = field_of([(0, 0)] * 7 + [(-100, 0)] + [(100 + 20 * k, 0) for k in range(8)])
    sat = field_of([(-32768, 32767), (32767, -32768)] + [(264, -264)] * 16)
    fields = [half, fewer, field_of([(33, 7)] * 16), field_of([(33, 7)] * 15), sat, field_of([(16 * k, -16 * k) for k in (1, 2, 3, 4)])]
    got, want = device_rule(fields, [L] * 6), host_rule(fields, [L] * 6)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    assert got[0][:, 4].tolist() == [1, 0, 1, 0, 1, 0] and got[0][4, :2].tolist() == [264, -264] and got[2][4, 0, 0].tolist() == [-32768, 32767]
    for settings in ((0, 0, 1), (32640, 528, 4), (5000, 16, 4)):
        got, want = device_rule(fields, [L] * 6, settings=settings), host_rule(fields, [L] * 6, settings)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), settings


@pytest.mark.parametrize("n", [1, 17])
def test_camera_estimator_chunks(n):
    from countr_amd import CameraEstimator
    fields, lumas = pairs(96, 192, n, "any", seed=n)
    est = CameraEstimator("cuda")
    got = est.run([torch.from_numpy(f).cuda() for f in fields], [torch.from_numpy(l).cuda() for l in lumas])
    want = host_rule(fields, lumas)
    assert all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(got, want))
    with pytest.raises(ValueError, match="one shape"):
        est.run([torch.zeros(2, 3, 2, dtype=torch.int16, device="cuda")], [torch.zeros(16, 24, dtype=torch.uint8, device="cuda")])


@pytest.fixture(scope="module")
def scene():
    from countr_amd import cam, flow as F
    lumas, maps, lines, _truth, _c = cam.pan_scene(frames=20, seed=0, pan=(1.3, 0.4), jitter=0.3)
    host = {}
    for s in (1, 4):
        fields = [None if t < s else F.motion_host(lumas[t], lumas[t - s], 6, 256) for t in range(20)]
        host[s] = (fields,) + F.flow_host(lumas, maps, lines=lines, search=6, interval=s, band=8.0, fields=fields, camera="translation")
    return lumas, maps, lines, host


@pytest.mark.parametrize("interval", [1, 4])
def test_flow_counter_with_a_camera_equals_flow_host(scene, interval):
    from countr_amd import cam, flow as F
    lumas, maps, lines, host = scene
    fields, want, counts, path = host[interval]
    images = [torch.from_numpy(F.image_of_luma(l)).cuda() for l in lumas]           # 20 frames: a chunk of 16 and one of 4
    dmaps = [torch.from_numpy(m).cuda() for m in maps]
    kw = dict(lines=lines, search=6, interval=interval, band=8.0)
    fc = F.FlowCounter("cuda", camera="translation", **kw)
    got = fc.run(images, dmaps, [(192, 96)] * 20, motion=True)
    mine = fc.camera_path()
    assert mine.path.dtype == np.int64 and np.array_equal(mine.path, path.path) and np.array_equal(mine.records, path.records)
    # at interval 4 the pan alone is 5.2 +- 1.2 px: one frame leaves the search of 6 and the host rule loses it -- a lost frame in the middle
    assert mine.lost == path.lost == {1: 0, 4: 1}[interval] and np.abs(mine.path[-1]).sum() > 0
    _rec, _path, comp = cam.camera_host(lumas, fields, interval)
    worst, acc = 0.0, np.zeros((3, 2))
    for t, ((flux, mv, total), (wflux, wmv, wtotal)) in enumerate(zip(got, want)):
        assert (mv is None) == (t < interval) and (flux is None) == (t < interval)
        if mv is None:
            continue
        assert np.array_equal(mv, wmv) and np.array_equal(mv, fields[t])            # motion=True still returns the raw field
        _f, _t, n, ab, tabs = F.flux_host(maps[t], comp[t], cam.shifted_placement(path.path[t], fc.placement), lines, 8.0, interval, members=True)
        assert np.array_equal(_f, wflux)
        bound = n * U * ab + np.spacing(np.abs(wflux).astype(np.float32))
        err = np.abs(flux.astype(np.float64) - wflux)
        assert flux.dtype == np.float32 and (err <= bound).all(), (t, err, bound)
        assert abs(total - wtotal) <= maps[t].size * U * tabs + np.spacing(np.float32(abs(wtotal)))
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        acc += flux.astype(np.float64)
    assert np.array_equal(fc.counts().line_counts, acc) and fc.counts().counted == counts.counted
    print("interval %d: worst flux error / bound %.3f, end of path %s, counts %s" % (interval, worst, (mine.path[-1] / 16).tolist(), np.round(acc, 4).tolist()))
    # camera=None is the path without the feature: the same bytes whether the argument is given or not, and flow_host's without a camera
    plain = F.FlowCounter("cuda", **kw).run(images, dmaps, [(192, 96)] * 20, motion=True)
    none = F.FlowCounter("cuda", camera=None, **kw)
    off = none.run(images, dmaps, [(192, 96)] * 20, motion=True)
    hoff, _c = F.flow_host(lumas, maps, lines=lines, search=6, interval=interval, band=8.0, fields=fields)
    differs = False
    for (f1, m1, t1), (f2, m2, t2), (f3, _m3, _t3), (_hf, hm, _ht) in zip(plain, off, got, hoff):
        assert (f1 is None and f2 is None) or (f1.tobytes() == f2.tobytes() and m1.tobytes() == m2.tobytes() and t1 == t2)
        if f1 is not None:
            assert np.array_equal(m1, hm)
            differs |= f1.tobytes() != f3.tobytes()
    assert differs and none._cam is None
    with pytest.raises(ValueError, match="camera=None"):
        none.camera_path()
    with pytest.raises(ValueError, match="camera is None or one of"):
        F.FlowCounter("cuda", lines=lines, camera="zoom")


# ---- count_flow and count_clip on the tiny configuration, fp32
@pytest.fixture(scope="module")
def model():
    import torch.nn as nn
    from countr_amd.models_mae_cross import SupervisedMAE
    p, D, depth, H, Dd, ddepth, Hd = W.CONFIGS["tiny_test"]
    m = SupervisedMAE(patch_size=p, embed_dim=D, depth=depth, num_heads=H, decoder_embed_dim=Dd, decoder_depth=ddepth, decoder_num_heads=Hd,
                      mlp_ratio=4, norm_layer=partial(nn.LayerNorm, eps=1e-6), precision="fp32")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.make_state_dict("tiny_test", seed=3).items()}, strict=True)
    return m.to("cuda").eval()


LINES = [(72.0, -1.0, 72.0, 97.0), (-1.0, 48.0, 145.0, 48.0)]
FLOW = dict(search=5, interval=1, min_gain=256)
TRK = dict(max_dist=25.0, max_missed=1, min_hits=2, beta=0.5)
PEAK = dict(radius=3, rel_threshold=0.05)


def rgb_clip(n, H=96, Wd=144, seed=1):
    """Frames cut from one smooth texture, the cut moving by 1 px of the frame (4 px of the map) per frame: a pan."""
    planes = [translated(H, Wd, n, seed + c, (1, 0)) for c in range(3)]
    return [np.ascontiguousarray(np.stack([planes[c][t] for c in range(3)], -1)) for t in range(n)]


def nv12_clip(n, H=96, Wd=144, seed=2):
    from countr_amd import YuvFrame
    ys = translated(H, Wd, n, seed, (1, 0))                                        # (grey chroma: noise that does not pan would hide the pan)
    return [YuvFrame(y, np.full((H // 2, Wd), 128, np.uint8), format="nv12") for y in ys]


def check_camera(model, frames, group):
    """count_flow and count_clip with camera="translation" against the camera-less calls (count, map and points bit for bit) and against
    camera_host on the prepared images' lumas (C_t; ids and events of tracks_host on the host-shifted points)."""
    from countr_amd import cam, count_clip, count_flow, flow as F, frames as FR, tracks_host
    n = len(frames)
    on, con = count_flow(model, frames, lines=LINES, group=group, motion=True, camera="translation", **FLOW)
    off, coff = count_flow(model, frames, lines=LINES, group=group, motion=True, **FLOW)
    images = []
    for g0 in range(0, n, group):
        images += [im.cpu().numpy() for im, _ex, _r in FR.prepare_items("cuda", frames[g0:g0 + group], None)]
    lumas = [F.luma_host(im) for im in images]
    s = FLOW["interval"]
    fields = [None if t < s else F.motion_host(lumas[t], lumas[t - s], FLOW["search"], FLOW["min_gain"]) for t in range(n)]
    rec, path, _comp = cam.camera_host(lumas, fields, s)
    pl = FR.map_placement(144, 96, 576)
    where = [cam.position(path[t], pl) for t in range(n)]
    assert rec[s:, 4].all() and (np.abs(rec[s:, :2] - (64, 0)) <= 8).all()          # 1 px of the frame a frame = 4 map px
    for t, (a, b) in enumerate(zip(on, off)):
        assert len(a) == 5 and len(b) == 4 and a[0] == b[0] and torch.equal(a[1], b[1]) and np.array_equal(a[3], b[3])
        assert np.array_equal(a[3], fields[t] if fields[t] is not None else np.zeros((48, 72, 2), np.int16))
        assert a[4].dtype == np.float64 and a[4].tobytes() == where[t].tobytes(), (t, a[4], where[t])
    assert con.counted == coff.counted and not np.array_equal(con.line_counts, coff.line_counts)
    # the background is all there is, and against the scene it rests: an inlier keeps at most tol = 8 of its 64, so most of the flux goes
    assert np.abs(con.line_counts).sum() < 0.5 * np.abs(coff.line_counts).sum()
    got, clip = count_clip(model, frames, lines=LINES, group=group, camera="translation", **TRK, **PEAK, **FLOW)
    ref, _c = count_clip(model, frames, lines=LINES, group=group, **TRK, **PEAK)
    for t, (a, b) in enumerate(zip(got, ref)):
        assert len(a) == 7 and len(b) == 6 and a[0] == b[0] and torch.equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
        assert a[6].tobytes() == where[t].tobytes()
    shifted = [(b[2].astype(np.float64) + c).astype(np.float32) for b, c in zip(ref, where)]
    steps, st = tracks_host(shifted, lines=LINES, **TRK)
    for a, (ids, ev, _s) in zip(got, steps):
        assert np.array_equal(a[4], ids) and np.array_equal(a[5], ev)
    assert clip[:3] == (st["started"], st["confirmed"], st["dropped"]) and np.array_equal(clip.line_counts, st["counts"][:2])
    assert sum(len(b[2]) for b in ref) > 0
    print("group %d: camera ends at %s px, flux with %s, without %s" % (group, where[-1].tolist(), np.round(con.line_counts, 4).tolist(),
                                                                      np.round(coff.line_counts, 4).tolist()))


def test_count_flow_and_count_clip_with_a_camera_on_host_rgb_frames(model):
    from countr_amd import FlowCounter, count_clip, count_flow
    frames = rgb_clip(4)
    check_camera(model, frames, 3)
    with pytest.raises(ValueError, match="and so is the camera"):
        count_flow(model, frames[:1], lines=None, counter=FlowCounter("cuda", lines=LINES), camera="translation")
    with pytest.raises(ValueError, match="line-less FlowCounter with a camera"):
        count_clip(model, frames[:1], max_dist=5.0, counter=FlowCounter("cuda", lines=()))


def test_count_flow_and_count_clip_with_a_camera_on_yuv_frames(model):
    check_camera(model, nv12_clip(4), 8)


# ---- the demo in a fresh child process
def test_demo_zero_flow_with_a_camera_on_a_raw_clip(tmp_path):
    Wd, H = 80, 96
    ys = translated(H, Wd, 4, 3, (1, 0))
    raw = b"".join(y.tobytes() + np.full(Wd * H // 2, 128, np.uint8).tobytes() for y in ys)
    clip = tmp_path / "clip.yuv"
    clip.write_bytes(raw)
    lines = tmp_path / "lines.json"
    lines.write_text(json.dumps({"gate": [[40, -1], [40, 97]]}))
    out = tmp_path / "out"
    cmd = [sys.executable, "demo_zero.py", "--yuv", "nv12:80x96", "--model_path", "", "--output_path", str(out), "--input_path", str(clip),
           "--no_viz", "--group_images", "3", "--flow", "--lines_json", str(lines), "--flow_search", "6", "--camera", "translation"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    rows = re.findall(r"^clip#(\d+): Count: (\S+) - Time: \S+ - flux: (.*) - cam: (\[.*\])$", r.stdout, re.M)
    assert [int(k) for k, _c, _x, _w in rows] == [0, 1, 2, 3], r.stdout
    cams = [json.loads(w) for _k, _c, _x, w in rows]
    assert cams[0] == [0.0, 0.0] and all(abs(c[0] - t) <= 0.5 and abs(c[1]) <= 0.5 for t, c in enumerate(cams))      # 1 px a frame along x
    doc = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{"clip"')][-1])
    assert doc == json.load(open(out / "flow_clip.json")) and list(doc) == ["clip", "camera"] and list(doc["clip"]["flux"]) == ["gate"]
    assert doc["camera"] == {"end": cams[-1], "lost": 0}
    r = subprocess.run(cmd[:-7] + ["--camera", "translation"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--camera is for --flow or --track" in r.stderr
