"""GPU: countr_density_peaks (csrc/peaks.hip) against peaks_host through the C ABI, PeakFinder's buffer reuse, locate_frames against
count_frames + peaks_host + the documented mappings, and the --points flag of the two demo CLIs.

Bars: y, x, score, total and the order are EQUAL.  cy / cx within 1e-3 pixel: each of the two sums has <= 289 fp32 terms of magnitude
<= 8 w, so its relative error is <= 289 * 2^-24 ~ 1.7e-5 and the quotient's absolute error <= 8 * 2 * 1.7e-5 ~ 3e-4.  mass within 1e-4
relative (the same sum, once)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from oracle import weights as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -7.0
CENTROID_TOL, MASS_RTOL = 1e-3, 1e-4


def seeded_map(h, w, seed):
    """1-40 Gaussians (sigma 1-3, amplitude 0.2-3) + uniform noise of +-0.02 (negative values occur) + a constant plateau patch."""
    rs = np.random.RandomState(seed * 7919 + h * 131 + w)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    d = np.zeros((h, w), np.float64)
    for _ in range(rs.randint(1, 41)):
        cy, cx, sg, amp = rs.uniform(0, h), rs.uniform(0, w), rs.uniform(1, 3), rs.uniform(0.2, 3)
        d += amp * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * sg * sg))
    d += rs.uniform(-0.02, 0.02, size=(h, w))
    py, px = rs.randint(0, h), rs.randint(0, w)
    d[py:py + 5, px:px + 7] = d[py:py + 5, px:px + 7].max() + 0.25        # a plateau: exactly one peak, its first pixel
    return d.astype(np.float32)


def run_kernel(hip, maps, r, thr=0.0, rel=0.1, cap=256, stream=None):
    """countr_density_peaks through ctypes on device maps, into fresh sentinel-filled buffers -> (rc, totals int32 [n], recs [n, cap, 6])."""
    from countr_amd import _lib
    n = len(maps)
    descs = (_lib.PeakMap * max(n, 1))()
    for j, m in enumerate(maps):
        descs[j].map, descs[j].h, descs[j].w = m.data_ptr(), m.shape[0], m.shape[1]
    ws_bytes = hip.countr_peaks_workspace(min(max(n, 1), 16), max(m.shape[0] for m in maps), max(m.shape[1] for m in maps), min(max(cap, 1), 8192))
    assert ws_bytes > 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    totals = torch.full((max(n, 1),), -3, dtype=torch.int32, device="cuda")
    recs = torch.full((max(n, 1), max(cap, 1), 6), SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
    rc = hip.countr_density_peaks(descs, n, r, thr, rel, cap, totals.data_ptr(), recs.data_ptr(), ws.data_ptr(), st)
    (stream or torch.cuda.current_stream()).synchronize()
    return rc, totals.cpu().numpy(), recs.cpu().numpy()


def compare(name, d, total, recs, r, thr, rel, cap):
    """One map's kernel output against peaks_host: prints the figures, then asserts the bars of the module docstring."""
    from countr_amd.peaks import peaks_host
    want_total, want = peaks_host(d, r, thr, rel, cap)
    kept = min(want_total, cap)
    got = recs[:kept].astype(np.float64)
    rest = recs[kept:]
    cerr = float(np.abs(got[:, 3:5] - want[:, 3:5]).max()) if kept and total == want_total else float("nan")
    merr = float((np.abs(got[:, 5] - want[:, 5]) / want[:, 5]).max()) if kept and total == want_total else float("nan")
    print("%s: total %d (host %d), kept %d, centroid err %.3e px, mass rel err %.3e" % (name, total, want_total, kept, cerr, merr))
    assert total == want_total
    assert np.array_equal(got[:, :3], want[:, :3]), name                 # y, x, score and the order
    assert (rest == SENTINEL).all(), name                                 # entries behind the kept ones are untouched
    if kept:
        assert cerr <= CENTROID_TOL and merr <= MASS_RTOL, (name, cerr, merr)
    return want_total


@pytest.mark.parametrize("h,w,r", [(1, 1, 1), (3, 5, 8), (16, 17, 1), (33, 65, 4), (64, 130, 8), (384, 400, 4)])
def test_kernel_equals_the_host_rule(hip, h, w, r):
    d = seeded_map(h, w, seed=r)
    rc, totals, recs = run_kernel(hip, [torch.from_numpy(d).cuda()], r)
    assert rc == 0, hip.countr_last_error()
    total = compare("%dx%d r=%d" % (h, w, r), d, int(totals[0]), recs[0], r, 0.0, 0.1, 256)
    assert total >= 1                                                     # the plateau patch at least
    # the same map with both thresholds at work, and with none (every positive local maximum of the noise)
    for thr, rel in ((0.5, 0.5), (0.0, 0.0)):
        rc, totals, recs = run_kernel(hip, [torch.from_numpy(d).cuda()], r, thr, rel, cap=2048)
        assert rc == 0, hip.countr_last_error()
        compare("%dx%d r=%d thr=%g rel=%g" % (h, w, r, thr, rel), d, int(totals[0]), recs[0], r, thr, rel, 2048)


def test_unaligned_view_takes_the_element_path(hip):
    d = seeded_map(33, 65, seed=11)
    buf = torch.empty(33 * 65 + 1, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[1:].view(33, 65)
    view.copy_(torch.from_numpy(d))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    rc, totals, recs = run_kernel(hip, [view], 4)
    assert rc == 0, hip.countr_last_error()
    compare("offset view", d, int(totals[0]), recs[0], 4, 0.0, 0.1, 256)
    rc, totals_a, recs_a = run_kernel(hip, [torch.from_numpy(d).cuda()], 4)
    assert np.array_equal(totals, totals_a) and recs.tobytes() == recs_a.tobytes()


def test_sixteen_mixed_maps_equal_sixteen_single_calls(hip):
    shapes = [(1, 1), (3, 5), (16, 17), (33, 65), (64, 130), (40, 200), (7, 300), (129, 64), (65, 63), (32, 64), (31, 129), (100, 100),
              (2, 2), (90, 257), (64, 128), (50, 70)]
    ds = [seeded_map(h, w, seed=20 + k) for k, (h, w) in enumerate(shapes)]
    dev = [torch.from_numpy(d).cuda() for d in ds]
    rc, totals, recs = run_kernel(hip, dev, 3, cap=64)
    assert rc == 0, hip.countr_last_error()
    for k, d in enumerate(ds):
        compare("map %d %s" % (k, shapes[k]), d, int(totals[k]), recs[k], 3, 0.0, 0.1, 64)
        rc, t1, r1 = run_kernel(hip, [dev[k]], 3, cap=64)
        assert rc == 0 and t1[0] == totals[k] and r1[0].tobytes() == recs[k].tobytes(), k


def test_cap_keeps_the_raster_first_eight(hip):
    from countr_amd.peaks import peaks_host
    rs = np.random.RandomState(5)
    d = rs.uniform(-0.02, 0.02, size=(90, 110)).astype(np.float32)
    spots = [(4 + 17 * (k // 4) + int(rs.randint(0, 3)), 6 + 26 * (k % 4) + int(rs.randint(0, 5))) for k in range(20)]
    for (y, x), v in zip(spots, rs.permutation(20)):
        d[y, x] = 1.0 + 0.125 * v
    rc, totals, recs = run_kernel(hip, [torch.from_numpy(d).cuda()], 4, cap=8)
    assert rc == 0, hip.countr_last_error()
    assert totals[0] == 20 == compare("cap 8 of 20", d, int(totals[0]), recs[0], 4, 0.0, 0.1, 8)
    first8 = sorted(spots, key=lambda p: p[0] * 110 + p[1])[:8]
    assert sorted((int(y), int(x)) for y, x in recs[0, :8, :2]) == sorted(first8)
    assert (np.diff(recs[0, :8, 2]) < 0).all()
    assert peaks_host(d, 4, 0.0, 0.1, 8)[0] == 20


def test_more_peaks_than_one_list_pass_and_than_the_largest_cap(hip):
    """Every other pixel of every other row is a peak at r = 1.  At 640 x 1024 a block of the write launch owns 20 rows = 320 row segments
    (two scan chunks) with 5120 peaks, 4096 of them in its first chunk (two passes of its 2048-entry list); 163 840 peaks in all against
    cap = 8192 (eight staging rounds of the rank launch), with ties in the score."""
    h, w = 640, 1024
    rs = np.random.RandomState(9)
    d = np.zeros((h, w), np.float32)
    vals = 1.0 + rs.permutation(320 * 512).astype(np.float32) / 262144.0
    vals[rs.randint(0, 8192, 600)] = 1.25                                 # ties among the kept: idx ascending decides
    d[0::2, 0::2] = vals.reshape(320, 512)
    rc, totals, recs = run_kernel(hip, [torch.from_numpy(d).cuda()], 1, cap=8192)
    assert rc == 0, hip.countr_last_error()
    assert compare("dense", d, int(totals[0]), recs[0], 1, 0.0, 0.1, 8192) == 320 * 512


def test_constant_and_all_zero_maps(hip):
    const = np.full((40, 70), 0.5, np.float32)
    zero = np.zeros((40, 70), np.float32)
    rc, totals, recs = run_kernel(hip, [torch.from_numpy(const).cuda(), torch.from_numpy(zero).cuda()], 2, cap=16)
    assert rc == 0, hip.countr_last_error()
    assert totals.tolist() == [1, 0]
    compare("constant", const, 1, recs[0], 2, 0.0, 0.1, 16)
    compare("zero", zero, 0, recs[1], 2, 0.0, 0.1, 16)
    assert recs[0, 0, :3].tolist() == [0.0, 0.0, 0.5]


def test_second_run_and_side_stream_give_the_same_bytes(hip):
    ds = [seeded_map(64, 130, seed=31), seeded_map(33, 65, seed=32)]
    dev = [torch.from_numpy(d).cuda() for d in ds]
    rc, t0, r0 = run_kernel(hip, dev, 4, 0.0, 0.0, cap=1024)
    rc2, t1, r1 = run_kernel(hip, dev, 4, 0.0, 0.0, cap=1024)
    assert rc == 0 and rc2 == 0 and np.array_equal(t0, t1) and r0.tobytes() == r1.tobytes()
    side = torch.cuda.Stream()
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream())
    side.wait_event(ev)
    rc3, t2, r2 = run_kernel(hip, dev, 4, 0.0, 0.0, cap=1024, stream=side)
    assert rc3 == 0 and np.array_equal(t0, t2) and r0.tobytes() == r2.tobytes()


@pytest.mark.parametrize("kw", [{"r": 0}, {"r": 9}, {"thr": -1.0}, {"n": 17}])
def test_bad_arguments_are_errors_not_launches(hip, kw):
    d = torch.from_numpy(seeded_map(16, 17, seed=1)).cuda()
    maps = [d] * kw.get("n", 1)
    rc, totals, recs = run_kernel(hip, maps, kw.get("r", 2), kw.get("thr", 0.0), cap=8)
    assert rc < 0
    assert hip.countr_last_error()
    assert (totals == -3).all() and (recs == SENTINEL).all()


def test_peak_finder_reuses_its_buffers(hip):
    from countr_amd import PeakFinder
    from countr_amd.peaks import peaks_host
    ds = [seeded_map(h, w, seed=40 + k) for k, (h, w) in enumerate([(64, 130)] * 17 + [(33, 65)])]          # two chunks
    dev = [torch.from_numpy(d).cuda() for d in ds]
    pf = PeakFinder("cuda")
    res = pf.find(dev, radius=3, max_points=128)
    assert len(res) == 18
    for d, pk in zip(ds, res):
        total, want = peaks_host(d, 3, 0.0, 0.1, 128)
        assert pk.total == total and pk.yx.dtype == np.int32 and pk.yx.shape == (min(total, 128), 2) and pk.centroid.dtype == np.float32
        assert np.array_equal(pk.yx, want[:, :2].astype(np.int32)) and np.array_equal(pk.score, want[:, 2].astype(np.float32))
        assert np.abs(pk.centroid - want[:, 3:5]).max() <= CENTROID_TOL
        assert (np.abs(pk.mass - want[:, 5]) <= MASS_RTOL * want[:, 5] + 1e-7).all()
    del res
    torch.cuda.synchronize()
    first = torch.cuda.memory_allocated()
    res = pf.find(dev, radius=3, max_points=128)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == first                         # the results live on the host
    assert res[0].total == peaks_host(ds[0], 3, 0.0, 0.1, 128)[0]


# ---- locate_frames
@pytest.fixture(scope="module")
def model():
    import models_mae_cross
    m = models_mae_cross.mae_vit_base_patch16(precision="bf16")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.make_state_dict("mae_vit_base_patch16", seed=0).items()})
    return m.to("cuda").eval()


def make_frame(H, Wd, seed):
    rs = np.random.RandomState(seed)
    return rs.randint(0, 256, size=(H, Wd, 3)).astype(np.uint8)


def host_points(dm, Wd, H):
    """peaks_host on a returned map, through the documented mapping -> (points (x, y) float64 [P, 2], score, total)."""
    from countr_amd.frames import frame_points
    from countr_amd.peaks import peaks_host
    total, recs = peaks_host(dm.float().cpu().numpy(), 4, 0.0, 0.1, 4096)
    x, y = frame_points(recs[:, 3], recs[:, 4], Wd, H, dm.shape[1])
    return np.stack([x, y], 1), recs[:, 2], total


def test_locate_frames_zero_shot(model):
    from countr_amd import count_frames, locate_frames
    fs = [make_frame(120, 200, 60), make_frame(120, 200, 61)]
    ref = count_frames(model, fs)
    res = locate_frames(model, fs)
    by_count = locate_frames(model, fs, keep="count")
    assert len(res) == 2
    for (cnt, dm, pts, score), (rc, rdm), (c2, dm2, p2, s2) in zip(res, ref, by_count):
        assert cnt == rc and torch.equal(dm, rdm) and dm.shape == (384, 640)
        assert c2 == rc and torch.equal(dm2, rdm)
        want, wscore, total = host_points(dm, 200, 120)
        print("zero-shot: count %.3f, %d peaks" % (cnt, total))
        assert total > 0                                                  # (a random-weight map has positive bumps: the test is not vacuous)
        assert pts.dtype == np.float32 and pts.shape == (min(total, 4096), 2) and score.shape == (len(pts),)
        assert np.array_equal(score, wscore.astype(np.float32))
        assert np.abs(pts - want).max() <= 1e-3
        keep = min(len(pts), max(0, int(np.floor(cnt + 0.5))))
        assert len(p2) == keep and np.array_equal(p2, pts[:keep]) and np.array_equal(s2, score[:keep])


def test_locate_frames_few_shot_takes_the_three_by_three_path(model):
    from countr_amd import frames as FR, inference, locate_frames
    from countr_amd.peaks import peaks_host
    f = make_frame(120, 200, 62)
    boxes = [[(50, 40, 52, 42), (100, 60, 102, 62), (150, 90, 152, 92)]]
    (cnt, dm, pts, score), = locate_frames(model, [f], boxes)
    (rc, rdm), = FR.count_frames(model, [f], boxes)
    assert cnt == rc and torch.equal(dm, rdm)
    (im, ex, rects), = FR.prepare_items("cuda", [f], boxes)
    assert inference._small_exemplars(rects) == 3                         # under 10 px after scaling: the 3 x 3 path
    dms = inference.density_maps(model, FR.split_crops(im), [ex] * 9, 3)
    assert torch.equal(dms[-1], dm)
    h, w = dm.shape
    rows = []
    for k, m in enumerate(dms):
        _t, recs = peaks_host(m.float().cpu().numpy(), 4, 0.0, 0.1, 4096)
        cy, cx = FR.crop_points(recs[:, 3], recs[:, 4], k, h, w)
        x, y = FR.frame_points(cy, cx, 200, 120, w)
        rows += [(-np.float32(s), k, int(yy) * w + int(xx), px, py) for s, yy, xx, px, py in zip(recs[:, 2], recs[:, 0], recs[:, 1], x, y)]
    rows.sort(key=lambda t: t[:3])                                        # (score descending, crop, idx)
    print("few-shot 3 x 3: count %.3f, %d peaks over nine crops" % (cnt, len(rows)))
    assert len(rows) > 0 and len(pts) == len(rows)
    assert np.array_equal(score, np.array([-t[0] for t in rows], np.float32))
    assert np.abs(pts - np.array([[t[3], t[4]] for t in rows])).max() <= 1e-3
    assert (pts[:, 0] > -0.5).all() and (pts[:, 0] < 199.5).all() and (pts[:, 1] > -0.5).all() and (pts[:, 1] < 119.5).all()
    # locate_maps: (count, map, crops) entries without crops= give what (count, map) entries with an explicit crops list give
    (p1, s1, t1), = FR.locate_maps([(cnt, dm)], [(200, 120)], [dms])
    (p2, s2, t2), = FR.locate_maps([(cnt, dm, dms)], [(200, 120)])
    (p3, _s3, t3), = FR.locate_maps([(cnt, dm, dms)], [(200, 120)], [None])          # an explicit crops= wins: the last crop's map alone
    assert np.array_equal(p1, pts) and np.array_equal(p2, p1) and np.array_equal(s2, s1) and t2 == t1 and np.array_equal(s1, score)
    (p4, _s4, t4), = FR.locate_maps([(cnt, dm)], [(200, 120)])
    assert np.array_equal(p3, p4) and t3 == t4 and t4 <= t1


# ---- the CLIs
def run(cmd):
    r = subprocess.run([sys.executable] + cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout


def count_line(out):
    line, = [l for l in out.splitlines() if l.startswith("Count:")]
    return line.split(" - Time:")[0]


def test_demo_zero_points(tmp_path):
    Image.fromarray(make_frame(120, 200, 70)).save(tmp_path / "shelf.jpg", quality=95)
    base = ["demo_zero.py", "--input_path", str(tmp_path / "shelf.jpg"), "--model_path", "", "--no_viz"]
    out = run(base + ["--output_path", str(tmp_path / "a"), "--points"])
    js = json.loads((tmp_path / "a" / "points_shelf.json").read_text())
    assert set(js) == {"count", "total_peaks", "points"}
    assert js["count"] == float(count_line(out).split()[1])
    assert len(js["points"]) == min(js["total_peaks"], 4096)
    assert all(len(p) == 3 and -0.5 <= p[0] <= 199.5 and -0.5 <= p[1] <= 119.5 for p in js["points"])
    assert not list((tmp_path / "a").glob("viz_*"))
    plain = run(base + ["--output_path", str(tmp_path / "b")])
    assert not list((tmp_path / "b").glob("points_*.json"))
    assert count_line(plain) == count_line(out)


def test_demo_points_writes_json_and_a_dotted_picture(tmp_path):
    Image.fromarray(make_frame(120, 200, 71)).save(tmp_path / "shelf.png")
    out = run(["demo.py", "--input_path", str(tmp_path / "shelf.png"), "--output_path", str(tmp_path / "out"), "--model_path", "",
               "--boxes", "40,30,90,70", "--points", "--points_keep", "count"])
    js = json.loads((tmp_path / "out" / "points_shelf.json").read_text())
    assert js["count"] == float(count_line(out).split()[1])
    assert len(js["points"]) == min(js["total_peaks"], 4096, max(0, int(np.floor(js["count"] + 0.5))))
    assert Image.open(tmp_path / "out" / "viz_shelf.jpg").size == (200, 120)
