"""GPU: countr_match_points (csrc/match.hip) against match_host through the C ABI, PointMatcher's chunking and buffer reuse, the peak
finder + matcher on maps with a known answer, and FSC_test_cross.py --localize on synthetic images.

Bars: match, match_d2 (bit for bit) and counts are EQUAL to match_host's -- kernel and host round every operation of d2 alike and take
the same minima, so no tolerance applies."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M_SENTINEL, D_SENTINEL, C_SENTINEL = -77, -7.0, -3
PAD = 5                     # sentinel elements between the slices of two sets


def ladder():
    """32 preds and 32 gts interleaved on a line with gaps 1, 1.01, 1.02, ...: one pair per round (tests/test_match_cpu.py)."""
    xs = np.concatenate([[0.0], np.cumsum(1.0 + 0.01 * np.arange(63))])
    z = np.zeros(32)
    return np.stack([xs[1::2][::-1], z], 1).astype(np.float32), np.stack([xs[0::2][::-1], z], 1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    """A named set -> (pred, gt, max_dist, host match, host d2): the host answer is computed once and shared."""
    from countr_amd.match import match_host
    rs = np.random.RandomState(sum(map(ord, name)) * 31 + 7)
    f = lambda n, w, h: (rs.uniform(0, 1, (n, 2)) * [w, h]).astype(np.float32)
    if name == "one":
        pred, gt, md = np.array([[3.0, 4.0]], np.float32), np.array([[0.0, 0.0]], np.float32), 5.0
    elif name == "no_pred":
        pred, gt, md = np.zeros((0, 2), np.float32), f(5, 20, 20), 8.0
    elif name == "no_gt":
        pred, gt, md = f(5, 20, 20), np.zeros((0, 2), np.float32), 8.0
    elif name == "counter_example":
        pred, gt, md = np.array([[1, 0], [4, 0], [17, 0]], np.float32), np.array([[0, 0], [10, 0]], np.float32), 100.0
    elif name == "uniform_17_33":
        pred, gt, md = f(17, 40, 30), f(33, 40, 30), 6.0
    elif name == "lattice_64_64":
        pred, gt, md = rs.randint(0, 12, (64, 2)).astype(np.float32), rs.randint(0, 12, (64, 2)).astype(np.float32), 4.0
    elif name == "field_300_257":
        pred, gt, md = f(300, 700, 384), f(257, 700, 384), 8.0
    elif name == "all_pairs_1024_1000":
        pred, gt, md = f(1024, 700, 384), f(1000, 700, 384), 1000.0
    elif name == "ladder":
        pred, gt = ladder()
        md = 1000.0
    elif name == "nan_and_far":
        pred, gt, md = f(40, 30, 30), f(50, 30, 30), 3.0
        pred[3, 0], pred[11, 1], gt[7, 1], gt[20, 0] = np.nan, np.inf, np.nan, 1e30
    elif name.startswith("edge_"):
        # integer lattice, sizes that straddle the 64-candidate chunk and the 32-bit mask word on both sides: thousands of tied
        # distances, so the masked rescan and the (d2, i, j) tie-break run at every boundary (4 to 9 rounds in match_rounds_host)
        P, G = map(int, name.split("_")[1:])
        edge = np.random.RandomState(1000 * P + G)
        pred = edge.randint(0, 12, (P, 2)).astype(np.float32)
        gt, md = edge.randint(0, 12, (G, 2)).astype(np.float32), 4.0
    elif name.startswith("mixed_"):
        k = int(name.split("_")[1])
        P, G = [(0, 0), (1, 0), (0, 3), (70, 65), (129, 200), (33, 31), (5, 500), (260, 9)][k % 8]
        pred, gt, md = f(P, 90, 60), f(G, 90, 60), [2.5, 7.0, 200.0][k % 3]
    else:
        raise KeyError(name)
    m, d2 = match_host(pred, gt, md)
    for a in (pred, gt, m, d2):
        a.setflags(write=False)
    return pred, gt, md, m, d2


def run_kernel(hip, names, stream=None):
    """countr_match_points through ctypes on the named sets, into fresh sentinel-filled buffers whose slices lie PAD elements apart
    -> (match, match_d2, counts, offsets) as numpy arrays."""
    from countr_amd import _lib
    n = len(names)
    descs = (_lib.MatchSet * max(n, 1))()
    keep, offsets, at = [], [], PAD
    for k, name in enumerate(names):
        pred, gt, md, _m, _d = case(name)
        dp, dg = torch.from_numpy(pred.copy()).cuda(), torch.from_numpy(gt.copy()).cuda()
        keep += [dp, dg]
        descs[k].pred, descs[k].gt = (dp.data_ptr() if len(pred) else None), (dg.data_ptr() if len(gt) else None)
        descs[k].P, descs[k].G, descs[k].max_dist, descs[k].offset = len(pred), len(gt), md, at
        offsets.append(at)
        at += len(pred) + PAD
    ws_bytes = hip.countr_match_workspace(n, max(len(case(x)[0]) for x in names), max(len(case(x)[1]) for x in names))
    assert ws_bytes > 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    match = torch.full((at,), M_SENTINEL, dtype=torch.int32, device="cuda")
    d2 = torch.full((at,), D_SENTINEL, dtype=torch.float32, device="cuda")
    counts = torch.full((n + 2,), C_SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    st = stream or torch.cuda.current_stream()
    rc = hip.countr_match_points(descs, n, match.data_ptr(), d2.data_ptr(), counts.data_ptr(), ws.data_ptr(), C.c_void_p(st.cuda_stream))
    st.synchronize()
    assert rc == 0, hip.countr_last_error()
    return match.cpu().numpy(), d2.cpu().numpy(), counts.cpu().numpy(), offsets


def compare(names, match, d2, counts, offsets):
    """Every named set's slice equals the host answer, and everything outside the slices kept its sentinel."""
    inside = np.zeros(match.shape[0], bool)
    for k, (name, off) in enumerate(zip(names, offsets)):
        _pred, _gt, _md, want_m, want_d2 = case(name)
        P = len(want_m)
        got_m, got_d2 = match[off:off + P], d2[off:off + P]
        inside[off:off + P] = True
        print("%s: P %d, matched %d (host %d), differing match %d, differing d2 bits %d" % (
            name, P, counts[k], int((want_m >= 0).sum()), int((got_m != want_m).sum()),
            int((got_d2.view(np.uint32) != want_d2.view(np.uint32)).sum())))
        assert np.array_equal(got_m, want_m), name
        assert np.array_equal(got_d2.view(np.uint32), want_d2.view(np.uint32)), name          # bit for bit, +inf included
        assert counts[k] == int((want_m >= 0).sum()), name
    assert (match[~inside] == M_SENTINEL).all() and (d2[~inside] == D_SENTINEL).all()
    assert (counts[len(names):] == C_SENTINEL).all()


SHAPES = ["one", "no_pred", "no_gt", "counter_example", "uniform_17_33", "lattice_64_64", "field_300_257", "all_pairs_1024_1000",
          "ladder", "nan_and_far", "edge_63_65", "edge_64_64", "edge_65_63", "edge_127_129", "edge_128_128", "edge_129_127"]


@pytest.mark.parametrize("name", SHAPES)
def test_kernel_equals_the_host_rule(hip, name):
    compare([name], *run_kernel(hip, [name]))


def test_the_ladder_needs_a_round_per_pair(hip):
    """What a capped round loop gets wrong: 32 rounds in the host's rounds form, and the kernel still equals the greedy matching."""
    from countr_amd.match import match_rounds_host
    pred, gt, md, want_m, _d2 = case("ladder")
    assert match_rounds_host(pred, gt, md)[2] == 32 and (want_m == np.arange(32)).all()
    match, _d, counts, offsets = run_kernel(hip, ["ladder"])
    assert counts[0] == 32 and np.array_equal(match[offsets[0]:offsets[0] + 32], want_m)


MIXED = ["mixed_%d" % k for k in range(16)]


def test_sixteen_sets_in_one_call(hip):
    compare(MIXED, *run_kernel(hip, MIXED))


def test_two_calls_give_identical_bytes_and_a_side_stream_works(hip):
    names = ["lattice_64_64", "field_300_257", "mixed_4", "all_pairs_1024_1000"]
    a = run_kernel(hip, names)
    b = run_kernel(hip, names)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = run_kernel(hip, names, stream=side)
    for other in (b, c):
        for x, y in zip(a[:3], other[:3]):
            assert x.tobytes() == y.tobytes()
    compare(names, *c)


def check_matcher(matcher, names):
    got = matcher.match([case(x)[:3] for x in names])
    assert len(got) == len(names)
    for name, (m, d2, cnt) in zip(names, got):
        _p, _g, _md, want_m, want_d2 = case(name)
        assert m.dtype == np.int32 and d2.dtype == np.float32
        assert np.array_equal(m, want_m) and np.array_equal(d2.view(np.uint32), want_d2.view(np.uint32)), name
        assert cnt == int((want_m >= 0).sum()), name


def test_point_matcher_chunks_seventeen_sets(hip):
    from countr_amd.match import PointMatcher, point_matcher
    check_matcher(PointMatcher("cuda"), MIXED + ["uniform_17_33"])
    assert point_matcher("cuda") is point_matcher("cuda:%d" % torch.cuda.current_device())
    assert PointMatcher("cuda").match([]) == []


def test_point_matcher_reuses_its_buffers(hip):
    from countr_amd.match import PointMatcher
    pm = PointMatcher("cuda")
    check_matcher(pm, ["counter_example"])
    check_matcher(pm, ["field_300_257", "all_pairs_1024_1000", "no_pred"])
    ptrs = (pm._ws.data_ptr(), pm._pts.data_ptr(), pm._out.data_ptr(), pm._pts_host.data_ptr(), pm._out_host.data_ptr())
    check_matcher(pm, ["counter_example", "no_gt"])
    check_matcher(pm, ["field_300_257"])
    assert ptrs == (pm._ws.data_ptr(), pm._pts.data_ptr(), pm._out.data_ptr(), pm._pts_host.data_ptr(), pm._out_host.data_ptr())
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        check_matcher(pm, ["lattice_64_64"])
    check_matcher(pm, ["uniform_17_33"])
    try:
        pm.match([(np.zeros((3, 3), np.float32), np.zeros((1, 2), np.float32), 4.0)])
    except ValueError:
        pass
    else:
        raise AssertionError("a [3, 3] point array was accepted")


def lattice_map(h, w, seed):
    """Gaussians (sigma 2, amplitude 0.5-3) on a 24-pixel lattice, each centre jittered by +-4 pixels -> (map fp32 [h, w], dots (x, y))."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    d, dots = np.zeros((h, w), np.float64), []
    for ky in range(h // 24):
        for kx in range(w // 24):
            cy, cx = 12 + 24 * ky + rs.uniform(-4, 4), 12 + 24 * kx + rs.uniform(-4, 4)
            d += rs.uniform(0.5, 3) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * 2.0 ** 2))
            dots.append((cx, cy))
    return d.astype(np.float32), np.array(dots, np.float32)


@pytest.mark.parametrize("h,w", [(96, 128), (384, 400)])
def test_peaks_and_matcher_recover_a_known_lattice(hip, h, w):
    """Every dot is found once and nothing else: P == G == TP at max_dist 1, each matched distance <= 0.25 pixel (the centroid of a
    sigma-2 Gaussian over the 9 x 9 window lies within 0.10 pixel of its centre on the host; the GPU centroid differs from the
    host's by <= 1e-3)."""
    from countr_amd.match import PointMatcher, localization_metrics
    from countr_amd.peaks import PeakFinder
    d, dots = lattice_map(h, w, seed=h + w)
    pk = PeakFinder("cuda").find([torch.from_numpy(d).cuda()], radius=4, threshold=0.0, rel_threshold=0.1)[0]
    points = np.stack([pk.centroid[:, 1], pk.centroid[:, 0]], 1).astype(np.float32)           # (cx, cy) -> (x, y)
    (m, d2, cnt), = PointMatcher("cuda").match([(points, dots, 1.0)])
    row = localization_metrics(d2, len(points), len(dots), [1.0])[0]
    worst = float(np.sqrt(d2[np.isfinite(d2)].max())) if cnt else float("nan")
    print("%d x %d: P %d, G %d, TP %d, worst matched distance %.4f px" % (h, w, len(points), len(dots), row["tp"], worst))
    assert len(dots) == (h // 24) * (w // 24)
    assert len(points) == len(dots) == row["tp"] == cnt
    assert sorted(m.tolist()) == list(range(len(dots)))
    assert worst <= 0.25
    assert row["precision"] == 1.0 and row["recall"] == 1.0 and row["f1"] == 1.0


def _cli(args):
    r = subprocess.run([sys.executable, "FSC_test_cross.py", "--resume", "", "--synthetic", "3"] + args, cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout.splitlines()


def test_cli_localize():
    """FSC_test_cross.py --synthetic 3 --localize prints a line per image and the run's localization line, whose micro figures are the
    sums of the per-image lines; without the flag nothing of it is printed and the counts are the same."""
    out = _cli(["--localize"])
    plain = _cli([])
    per_image = [json.loads(l.split(": localization: ", 1)[1]) for l in out if ": localization: " in l]
    assert len(per_image) == 3
    summary = [json.loads(l) for l in out if l.startswith("{") and '"localization"' in l]
    assert len(summary) == 1
    loc = summary[0]["localization"]
    assert loc["images"] == 3 and loc["radius"] == 4 and loc["rel_threshold"] == 0.1 and loc["keep"] == "all"
    assert list(loc["dist"]) == ["4", "8", "16"]
    for lab in ("4", "8", "16"):
        tp = sum(im["dist"][lab]["tp"] for im in per_image)
        P, G = sum(im["points"] for im in per_image), sum(im["dots"] for im in per_image)
        col = loc["dist"][lab]
        assert (col["tp"], col["pred"], col["gt"], col["images"]) == (tp, P, G, 3)
        prec, rec = (tp / P if P else 0.0), (tp / G if G else 0.0)
        assert abs(col["precision"] - prec) < 1e-12 and abs(col["recall"] - rec) < 1e-12
        assert abs(col["f1"] - (2 * prec * rec / (prec + rec) if prec + rec else 0.0)) < 1e-12
        assert abs(col["macro_f1"] - sum(im["dist"][lab]["f1"] for im in per_image) / 3) < 1e-12
        for im in per_image:
            assert im["dist"][lab]["tp"] <= min(im["points"], im["dots"])
    assert [im["dist"]["4"]["tp"] <= im["dist"]["8"]["tp"] <= im["dist"]["16"]["tp"] for im in per_image] == [True] * 3
    # the dots are --report's draws: as many as the image's gt_cnt
    counts = [l for l in out if "pred_cnt" in l]
    assert [im["dots"] for im in per_image] == [int(float(l.split("gt_cnt:")[1].split(",")[0])) for l in counts]
    # without the flag
    assert not [l for l in plain if "localization" in l]
    assert counts == [l for l in plain if "pred_cnt" in l] and len(counts) == 3
    m1 = [json.loads(l) for l in out if l.startswith("{") and '"MAE"' in l]
    m0 = [json.loads(l) for l in plain if l.startswith("{") and '"MAE"' in l]
    assert len(m1) == len(m0) == 1 and set(m1[0]) == set(m0[0])
    assert all(m1[0][k] == m0[0][k] for k in m1[0] if k != "mean_infer_time_s")         # (a wall-clock measurement differs between runs)
