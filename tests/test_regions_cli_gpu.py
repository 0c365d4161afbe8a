"""GPU: the command-line side of the regional counts -- FSC_test_cross.py --game and demo_zero.py / demo.py --regions_json -- run as a
user would run them (subprocesses, the randomly initialised model)."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(cmd):
    r = subprocess.run([sys.executable] + cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout.splitlines()


def test_game_on_synthetic_images(monkeypatch, capsys):
    argv = ["--resume", "", "--synthetic", "3", "--precision", "fp32"]
    out = run(["FSC_test_cross.py"] + argv + ["--game", "3"])
    plain = run(["FSC_test_cross.py"] + argv)
    # without --game: the lines of a plain run (the last one carries a time)
    timed = lambda lines: [l for l in lines if "mean_infer_time_s" not in l]
    assert timed(plain) == [l for l in timed(out) if ": game: " not in l and not l.startswith('{"GAME"')]
    assert len([l for l in plain if "pred_cnt" in l]) == 3 and not any("game" in l.lower() for l in plain)
    per = [json.loads(l.split(": game: ")[1]) for l in out if ": game: " in l]
    assert [l.split(":")[0] for l in out if ": game: " in l] == ["synthetic_%d" % k for k in range(3)]
    assert len(per) == 3 and all(list(g) == ["0", "1", "2", "3"] for g in per)
    final, = [json.loads(l) for l in out if l.startswith('{"GAME"')]
    assert final["images"] == 3 and list(final["GAME"]) == ["0", "1", "2", "3"]
    mae = json.loads([l for l in out if l.startswith('{"MAE"')][0])["MAE"]
    errs = [float(re.search(r"error:\s*([-0-9.]+)", l).group(1)) for l in out if "pred_cnt" in l]
    # The bound.  An image's cells are scale * mass / 60 with scale = count / (total / 60) (1 when total <= 0), so their sum is
    # count * sum(mass) / total, or sum(mass) / 60 against count = the forward's own fp32 sum / 60.  sum(mass), total and the forward's
    # sum are fp32 sums of the same n pixels, each within n 2^-24 sum|v| of the exact sum (tests/test_regions_gpu.py); two differences
    # of two of them: |sum of cells - count| <= |count| * 4 n 2^-24 sum|v| / |total|, plus the rounding of the 64 float32 cells (half
    # an ulp each).  sum|v| / |total| is read off the very maps the run sums: the same run in this process, with frames.region_maps
    # recording them.
    import FSC_test_cross
    from countr_amd import frames
    seen = []
    inner = frames.region_maps

    def recording(results, sizes, crops, regions):
        got = inner(results, sizes, crops, regions)
        for (count, dm), cr, (cells, _area) in zip(results, crops, got):
            maps = [m.double() for m in (cr if cr is not None else [dm])]
            n, sabs, tot = sum(m.numel() for m in maps), sum(float(m.abs().sum()) for m in maps), sum(float(m.sum()) for m in maps)
            seen.append(abs(count) * 4 * n * 2.0 ** -24 * sabs / abs(tot) + float(np.spacing(np.abs(cells)).sum()) / 2)
        return got

    monkeypatch.setattr(frames, "region_maps", recording)
    FSC_test_cross.main(FSC_test_cross.get_args_parser().parse_args(argv + ["--game", "3"]))
    here = capsys.readouterr().out.splitlines()
    assert [l for l in here if ": game: " in l or l.startswith('{"GAME"')] == [l for l in out if ": game: " in l or l.startswith('{"GAME"')]
    assert len(seen) == 3
    print("GAME", final["GAME"], "MAE", mae, "per-image bounds", seen)
    assert abs(final["GAME"]["0"] - mae) <= sum(seen) / 3 + 1e-12 * max(mae, 1.0)        # (the mean of three fp64 figures)
    for g, e, b in zip(per, errs, seen):
        assert abs(g["0"] - e) <= b + 5e-4                                     # (the error is printed with three decimals)
        assert all(g[str(l)] <= g[str(l + 1)] + 1e-9 for l in range(3))        # the triangle inequality, up to the fp64 sums' rounding
    assert all(final["GAME"][str(l)] <= final["GAME"][str(l + 1)] + 1e-9 for l in range(3))


def test_game_with_report_and_localize(tmp_path):
    out = run(["FSC_test_cross.py", "--resume", "", "--synthetic", "3", "--precision", "fp32", "--game", "2", "--report", "--localize",
               "--output_dir", str(tmp_path)])
    rows = (tmp_path / "results.csv").read_text().splitlines()
    head = rows[0].split(",")
    assert head[:3] == ["time", "name", "prediction"] and head[-3:] == ["game_0", "game_1", "game_2"] and "points" in head
    per = {l.split(":")[0]: json.loads(l.split(": game: ")[1]) for l in out if ": game: " in l}
    for row in rows[1:]:
        cells = row.split(",")
        assert [float(v) for v in cells[-3:]] == [float("%.4f" % per[cells[1]][str(l)]) for l in range(3)]


def test_demos_regions_json(tmp_path):
    rs = np.random.RandomState(80)
    Image.fromarray(rs.randint(0, 256, size=(120, 200, 3)).astype(np.uint8)).save(tmp_path / "lot.png")
    named = {"left": [[-0.5, -0.5], [99.5, -0.5], [99.5, 119.5], [-0.5, 119.5]], "right": [[99.5, -0.5], [199.5, -0.5], [199.5, 119.5], [99.5, 119.5]],
             "bay": [[20, 30], [80, 25], [90, 100], [30, 90]]}
    (tmp_path / "regions.json").write_text(json.dumps(named))
    # demo.py's boxes are under 10 px in the resized image: the 3 x 3 path, nine maps of 384 x 640 add into the regions
    for script, extra, maps in (("demo_zero.py", [], 1), ("demo.py", ["--boxes", "40,30,42,32;90,60,92,62", "--points"], 9)):
        base = [script, "--input_path", str(tmp_path / "lot.png"), "--model_path", "", "--precision", "fp32"] + extra
        outdir = tmp_path / ("out_" + script)
        out = run(base + ["--output_path", str(outdir), "--regions_json", str(tmp_path / "regions.json")])
        js = json.loads((outdir / "regions_lot.json").read_text())
        assert set(js) == {"count", "regions"} and list(js["regions"]) == list(named)
        assert all(set(v) == {"count", "area"} and np.isfinite(v["count"]) for v in js["regions"].values())
        count_line, = [l for l in out if l.startswith("Count:")]
        assert js["count"] == float(count_line.split()[1])
        assert [l.split()[1].rstrip(":") for l in out if l.startswith("  region ")] == list(named)
        a = {k: v["area"] for k, v in js["regions"].items()}
        assert a["left"] + a["right"] == maps * 384 * 640 and 0 < a["bay"] < min(a["left"], a["right"])
        # one map: the frame's midline x = 99.5 is the map's (column 319.5).  Nine crop maps: a crop is 640 // 3 = 213 image columns upscaled
        # to 640; the left and right crops fall wholly on one side, and a middle crop's column cx lies at image column
        # 213 + (cx + 0.5) 213 / 640 - 0.5, left of 319.5 iff cx + 0.5 < 107 * 640 / 213 = 321.502: 322 columns left, 318 right, in 3 maps
        assert a["left"] - a["right"] == (0 if maps == 1 else 3 * 384 * (322 - 318))
        assert Image.open(outdir / "viz_lot.jpg").size == (200, 120)
        assert ("--points" in extra) == (outdir / "points_lot.json").exists()
        # without the flag: the same count, no regions file, no region lines
        plain = run(base + ["--output_path", str(outdir) + "_plain", "--no_viz"])
        assert [l for l in plain if l.startswith("Count:")][0].split(" - Time:")[0] == count_line.split(" - Time:")[0]
        assert not list((tmp_path / (outdir.name + "_plain")).glob("regions_*")) and not [l for l in plain if l.startswith("  region ")]
