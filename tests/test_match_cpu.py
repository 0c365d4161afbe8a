"""CPU: the matching rule's host statement (countr_amd/match.py: match_host), its two properties (locally dominant rounds, prefix),
the metrics and their totals, the ABI listing and argument checks of the two new exports, and the evaluation CLI's new flags."""
import ctypes as C

import numpy as np

from countr_amd import _lib, match
from countr_amd.match import LocalizationTotals, localization_metrics, match_host, match_rounds_host

INF = np.float32(np.inf)


def line(xs):
    return np.array([[x, 0.0] for x in xs], np.float32)


def test_counter_example_of_the_proposal_shortcut():
    """gt at x = 0, 10; pred at x = 1, 4, 17: greedy takes (0, 0) at d2 1, then (1, 1) at 36; pred 2 (d2 49 to gt 1) stays unmatched.
    "Each pred proposes to its best gt" would leave gt 1 to pred 2, its only proposer."""
    m, d2 = match_host(line([1, 4, 17]), line([0, 10]), 100.0)
    assert m.tolist() == [0, 1, -1] and m.dtype == np.int32
    assert d2.tolist() == [1.0, 36.0, np.inf] and d2.dtype == np.float32
    m2, d22, rounds = match_rounds_host(line([1, 4, 17]), line([0, 10]), 100.0)
    assert m2.tolist() == [0, 1, -1] and d22.tolist() == [1.0, 36.0, np.inf] and rounds == 2


def test_duplicates_the_lower_index_wins():
    m, d2 = match_host([[5, 5], [5, 5]], [[5, 6]], 3.0)
    assert m.tolist() == [0, -1] and d2.tolist() == [1.0, np.inf]
    m, d2 = match_host([[5, 6]], [[5, 5], [5, 5]], 3.0)                  # and the lower gt index
    assert m.tolist() == [0] and d2.tolist() == [1.0]


def test_boundary_is_inclusive():
    m, d2 = match_host([[0, 0]], [[3, 4]], 5.0)
    assert m.tolist() == [0] and d2.tolist() == [25.0]
    m, d2 = match_host([[0, 0]], [[3, 4]], 4.999)
    assert m.tolist() == [-1] and d2.tolist() == [np.inf]


def test_a_nan_point_matches_nothing():
    m, d2 = match_host([[np.nan, 1.0], [2.0, 2.0], [np.inf, 0.0]], [[2.0, 2.5], [0.0, 1.0]], 50.0)
    assert m.tolist() == [-1, 0, -1] and d2.tolist() == [np.inf, 0.25, np.inf]
    m, _ = match_host([[2.0, 2.0]], [[np.nan, np.nan], [2.0, 3.0]], 50.0)
    assert m.tolist() == [1]


def test_empty_sides():
    m, d2 = match_host(np.zeros((0, 2), np.float32), [[1, 2]], 4.0)
    assert m.shape == (0,) and d2.shape == (0,) and m.dtype == np.int32 and d2.dtype == np.float32
    m, d2 = match_host([[1, 2], [3, 4]], np.zeros((0, 2), np.float32), 4.0)
    assert m.tolist() == [-1, -1] and d2.tolist() == [np.inf, np.inf]
    m, d2 = match_host([], [], 4.0)
    assert m.shape == (0,) and d2.shape == (0,)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        try:
            match_host([[0, 0]], [[0, 0]], bad)
        except ValueError:
            continue
        raise AssertionError(bad)


def seeded_sets():
    """Uniform sets and integer-lattice sets (many exact ties), sizes <= 40."""
    rs = np.random.RandomState(20261018)
    for k in range(60):
        P, G = int(rs.randint(0, 41)), int(rs.randint(0, 41))
        if k % 2:
            yield rs.randint(0, 7, (P, 2)).astype(np.float32), rs.randint(0, 7, (G, 2)).astype(np.float32)
        else:
            yield rs.uniform(0, 12, (P, 2)).astype(np.float32), rs.uniform(0, 12, (G, 2)).astype(np.float32)


def test_locally_dominant_rounds_equal_the_greedy_matching():
    for pred, gt in seeded_sets():
        for md in (100.0, 1.5):
            m, d2 = match_host(pred, gt, md)
            mr, d2r, _rounds = match_rounds_host(pred, gt, md)
            assert np.array_equal(m, mr) and np.array_equal(d2, d2r)
            hit = m >= 0
            assert len(set(m[hit].tolist())) == int(hit.sum())          # one to one
            assert (d2[hit] <= np.float32(md) * np.float32(md)).all() and (d2[~hit] == INF).all()


def test_prefix_property():
    """The matching under the smaller bound is the part of the larger bound's matching whose d2 is within the smaller bound."""
    for pred, gt in seeded_sets():
        big, big_d2 = match_host(pred, gt, 100.0)
        small, small_d2 = match_host(pred, gt, 1.5)
        keep = big_d2 <= np.float32(1.5) * np.float32(1.5)
        assert np.array_equal(small, np.where(keep, big, -1))
        assert np.array_equal(small_d2, np.where(keep, big_d2, INF))


def test_ladder_takes_one_round_per_pair():
    """pred k and gt k interleaved on a line with growing gaps: only the leftmost remaining pair is ever locally dominant."""
    gaps = 1.0 + 0.01 * np.arange(63)
    xs = np.concatenate([[0.0], np.cumsum(gaps)])
    pred, gt = line(xs[1::2][::-1]), line(xs[0::2][::-1])               # right to left: gt 31, pred 31, ..., gt 0 | the smallest gap first
    m, d2, rounds = match_rounds_host(pred, gt, 1000.0)
    mh, d2h = match_host(pred, gt, 1000.0)
    assert rounds == 32 and np.array_equal(m, mh) and np.array_equal(d2, d2h) and (m == np.arange(32)).all()


def test_metrics_on_hand_computed_numbers():
    d2 = np.array([1.0, 16.0, 25.0, np.inf, 100.0], np.float32)         # distances 1, 4, 5, -, 10
    rows = localization_metrics(d2, P=5, G=8, dists=[4, 5, 16])
    assert [r["dist"] for r in rows] == [4.0, 5.0, 16.0] and [r["tp"] for r in rows] == [2, 3, 4]
    assert rows[0]["precision"] == 2 / 5 and rows[0]["recall"] == 2 / 8
    assert abs(rows[0]["f1"] - 2 * 0.4 * 0.25 / 0.65) < 1e-12 and abs(rows[0]["mean_dist"] - 2.5) < 1e-12
    assert abs(rows[2]["mean_dist"] - 5.0) < 1e-12 and rows[2]["precision"] == 0.8 and rows[2]["recall"] == 0.5
    zero = localization_metrics(np.zeros(0, np.float32), 0, 0, [4])[0]
    assert zero == {"dist": 4.0, "tp": 0, "precision": 0.0, "recall": 0.0, "f1": 0.0, "mean_dist": 0.0}
    none = localization_metrics(np.full(3, np.inf, np.float32), 3, 0, [4])[0]
    assert none["tp"] == 0 and none["precision"] == 0.0 and none["recall"] == 0.0 and none["f1"] == 0.0
    # the boundary is the kernel's: d2 <= fl(dist * dist) in fp32
    edge = np.float32(4.999) * np.float32(4.999)
    assert localization_metrics(np.array([edge, np.nextafter(edge, INF)], np.float32), 2, 2, [4.999])[0]["tp"] == 1


def test_totals_micro_and_macro():
    t = LocalizationTotals()
    assert t.summary() == {}
    a = localization_metrics(np.array([1.0, 1.0, np.inf, np.inf], np.float32), 4, 2, [4])[0]         # tp 2: p 0.5, r 1, f1 2/3
    b = localization_metrics(np.array([np.inf], np.float32), 1, 5, [4])[0]                            # tp 0: f1 0
    c = localization_metrics(np.zeros(0, np.float32), 0, 0, [4])[0]                                   # nothing at all
    for row, P, G in ((a, 4, 2), (b, 1, 5), (c, 0, 0)):
        t.add("4", row, P, G)
    t.add("box", a, 4, 2)
    s = t.summary()
    assert s["4"]["images"] == 3 and (s["4"]["tp"], s["4"]["pred"], s["4"]["gt"]) == (2, 5, 7)
    assert s["4"]["precision"] == 2 / 5 and s["4"]["recall"] == 2 / 7
    assert abs(s["4"]["f1"] - 2 * (2 / 5) * (2 / 7) / (2 / 5 + 2 / 7)) < 1e-12
    assert abs(s["4"]["macro_f1"] - (2 / 3) / 3) < 1e-12
    assert s["box"]["images"] == 1 and abs(s["box"]["macro_f1"] - 2 / 3) < 1e-12
    z = LocalizationTotals()
    z.add("4", c, 0, 0)
    assert z.summary()["4"] == {"images": 1, "tp": 0, "pred": 0, "gt": 0, "precision": 0.0, "recall": 0.0, "f1": 0.0, "macro_f1": 0.0}


def test_match_set_layout_version_and_limits():
    assert C.sizeof(_lib.MatchSet) == 32
    for variant in ("", "f16"):
        L = _lib.lib(variant)
        assert L.countr_version() == 9 == _lib.ABI_VERSION and all(hasattr(L, n) for n in ("countr_match_workspace", "countr_match_points"))
    assert match.MAX_SETS == _lib.MATCH_MAX_SETS == 16


def test_workspace_is_host_only_and_checks_its_arguments():
    L = _lib.lib()
    assert L.countr_match_workspace(1, 0, 0) > 0
    assert 0 < L.countr_match_workspace(8, 140, 1000) < L.countr_match_workspace(16, 8192, 8192)
    for bad in ((0, 10, 10), (17, 10, 10), (4, 8193, 10), (4, 10, 8193), (4, -1, 10)):
        assert L.countr_match_workspace(*bad) < 0, bad
        assert L.countr_last_error()


def test_match_points_rejects_bad_arguments_before_any_launch():
    """Every call below must fail in the argument checks: this test runs without a GPU, and the pointers are not memory."""
    L = _lib.lib()
    fake = 1 << 20                                                       # non-null, 16-byte aligned, never dereferenced
    sets = (_lib.MatchSet * 17)()

    def call(n=1, P=4, G=4, md=8.0, pred=fake, gt=fake, offset=0, out=fake):
        for d in sets:
            d.pred, d.gt, d.P, d.G, d.max_dist, d.offset = fake, fake, 1, 1, 1.0, 0
        sets[0].pred, sets[0].gt, sets[0].P, sets[0].G, sets[0].max_dist, sets[0].offset = pred, gt, P, G, md, offset
        return L.countr_match_points(sets, n, out, fake, fake, fake, None)

    for kw in ({"n": 0}, {"n": 17}, {"n": -1}, {"P": 8193}, {"G": 8193}, {"P": -1}, {"md": 0.0}, {"md": -2.0}, {"md": float("nan")},
               {"md": float("inf")}, {"pred": None}, {"gt": None}, {"pred": fake + 4}, {"offset": -1}, {"out": None}):
        rc = call(**kw)
        assert rc != 0, kw
        text = L.countr_last_error()
        assert text and b"countr_match_points" in text, kw


def test_parser_has_the_new_flags_with_their_defaults():
    import FSC_test_cross as cli
    a = cli.get_args_parser().parse_args([])
    assert a.localize is False and a.localize_dist == "4,8,16" and a.localize_box_scale == 0
    assert a.points_radius == 4 and a.points_rel_threshold == 0.1 and a.points_keep == "all"
    a = cli.get_args_parser().parse_args(["--localize", "--localize_dist", "2,6.5", "--localize_box_scale", "0.5", "--points_radius", "3",
                                          "--points_rel_threshold", "0.2", "--points_keep", "count"])
    assert a.localize and cli.localize_distances(a.localize_dist) == [2.0, 6.5] and a.localize_box_scale == 0.5
    assert (a.points_radius, a.points_rel_threshold, a.points_keep) == (3, 0.2, "count")
    import inspect
    from countr_amd import frames
    sig = inspect.signature(frames.locate_frames).parameters                 # the defaults are locate_frames' own
    assert sig["radius"].default == 4 and sig["rel_threshold"].default == 0.1 and sig["keep"].default == "all"
    assert cli.box_distance([(0, 0, 9, 19), (0, 0, 29, 19)], 0.5) == 0.5 * (10 + 20) / 2 and cli.box_distance([], 0.5) is None
    assert cli.box_distance([(0, 0, 9, 19)], 0.0) is None
    for bad in ("", "4,-1", "0", "nan"):
        try:
            cli.localize_distances(bad)
        except ValueError:
            continue
        raise AssertionError(bad)


def test_test_dots_scales_as_the_test_resize(tmp_path):
    from PIL import Image
    from countr_amd.data import fsc147
    Image.new("RGB", (500, 300)).save(tmp_path / "7.jpg")
    anno = {"7.jpg": {"points": [[0.0, 0.0], [250.5, 100.25], [499.0, 299.0]]}, "8.jpg": {"points": []}}
    dots = fsc147.test_dots(anno, str(tmp_path), "7.jpg")
    new_w = 16 * int((500 / 300 * 384) / 16)
    want = np.array(anno["7.jpg"]["points"]) * np.array([new_w / 500, 384 / 300])
    assert dots.dtype == np.float32 and dots.shape == (3, 2) and np.allclose(dots, want, rtol=1e-6)
    Image.new("RGB", (300, 300)).save(tmp_path / "8.jpg")
    assert fsc147.test_dots(anno, str(tmp_path), "8.jpg").shape == (0, 2)


def test_cli_lines_and_csv_columns(capsys):
    """print_localization: a line per image, the run's line from the sums, and the results.csv columns (an image without exemplar
    rectangles has empty `box` cells and is left out of that column's totals)."""
    import json
    import FSC_test_cross as cli
    args = cli.get_args_parser().parse_args(["--localize", "--localize_dist", "4,8", "--localize_box_scale", "0.5"])
    a = localization_metrics(np.array([1.0, 49.0, np.inf], np.float32), 3, 4, [4, 8, 6.0])
    b = localization_metrics(np.array([4.0], np.float32), 1, 1, [4, 8])
    header, cells = cli.print_localization(args, [4.0, 8.0], ["a.jpg", "b.jpg"], [(3, 4, a, ["4", "8", "box"]), (1, 1, b, ["4", "8"])])
    assert header == ["points", "dots", "tp_4", "precision_4", "recall_4", "tp_8", "precision_8", "recall_8", "tp_box", "precision_box", "recall_box"]
    assert cells["a.jpg"] == [3, 4, 1, "0.3333", "0.2500", 2, "0.6667", "0.5000", 1, "0.3333", "0.2500"]
    assert cells["b.jpg"] == [1, 1, 1, "1.0000", "1.0000", 1, "1.0000", "1.0000", "", "", ""]
    out = capsys.readouterr().out.splitlines()
    assert len(out) == 3 and out[0].startswith("a.jpg: localization: ") and out[1].startswith("b.jpg: localization: ")
    assert json.loads(out[0].split(": localization: ", 1)[1])["dist"]["box"]["dist"] == 6.0
    loc = json.loads(out[2])["localization"]
    assert loc["images"] == 2 and (loc["dist"]["4"]["tp"], loc["dist"]["4"]["pred"], loc["dist"]["4"]["gt"]) == (2, 4, 5)
    assert loc["dist"]["box"]["images"] == 1 and loc["dist"]["8"]["tp"] == 3
