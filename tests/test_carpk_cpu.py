"""CPU: the host restatements of the CARPK scripts (countr_amd/data/carpk.py) against tests/golden/carpk.npz -- recorded from the
reference's own loop bodies by tools/oracle/make_golden_carpk.py --, the devkit loader, the random streams and the C prototypes."""
import os
import random

import numpy as np
import pytest
import torch

from countr_amd.data import carpk as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 2e-5          # the oracle pins' bar for floats (tests/test_oracle_golden.py)


def toy_model(window, boxes, shot_num):
    """The stand-in model of tools/oracle/make_golden_carpk.py, restated."""
    gain = 0.2 + 0.4 * boxes[:, :shot_num].mean()
    return window.mean(1) * gain


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "carpk.npz"))
    offs = np.concatenate([[0], np.cumsum(g["nboxes"])])
    toffs = np.concatenate([[0], np.cumsum(g["ntarget"])])
    cases = []
    for k, seed in enumerate(g["seeds"]):
        cases.append({"seed": int(seed), "boxes": g["boxes"][offs[k]:offs[k + 1]].tolist(), "cells": g["cells"][k],
                      "pred_cnt": float(g["pred_cnt"][k]), "e_cnt": float(g["e_cnt"][k]), "n_over": int(g["n_over"][k]),
                      "starts": g["starts"][k].tolist(), "target_cells": g["target_cells"][toffs[k]:toffs[k + 1]].tolist(),
                      "target_sum": float(g["target_sum"][k]), "after_test": float(g["after_test"][k]),
                      "after_train": g["after_train"][k].tolist(), "train_idx": int(g["train_idx"][k])})
    return int(g["stream_seed"]), cases


def close(a, b):
    return abs(a - b) <= REL * abs(b)


def test_golden_covers_both_branches_with_margins(golden):
    _s, cases = golden
    assert len(cases) >= 4
    assert any(c["n_over"] >= 1 for c in cases)
    assert any(c["e_cnt"] <= 0.5 for c in cases) and any(c["e_cnt"] > 0.5 for c in cases)
    assert min(np.abs(c["cells"] - 1.224).min() for c in cases) > 1e-3
    assert min(abs(c["e_cnt"] - 0.5) for c in cases) > 1e-3


def test_test_path_reproduces_the_reference(golden):
    """prepare_host -> stitch -> count_rule_host on the seeded samples: integers exact, floats within 2e-5 relative."""
    _s, cases = golden
    for c in cases:
        item = D.synthetic_item(c["seed"])
        assert item["boxes"] == c["boxes"]
        image, ex = D.prepare_host(item["images"], [D.box_rect(b) for b in item["boxes"][:2]])
        assert image.shape == (1, 3, 384, 683) and ex.shape == (1, 2, 3, 64, 64)
        dm, starts = D.stitch_host(toy_model, image, ex, 2)
        assert starts == c["starts"] == [0, 128, 256, 299]
        pred, st = D.count_rule_host(dm.numpy(), D.script_rects(item["boxes"]))
        assert st["n_over"] == c["n_over"]
        assert (st["e_cnt"] <= 0.5) == (c["e_cnt"] <= 0.5)
        assert st["cells"].shape == (24, 42)
        assert np.all(np.abs(st["cells"] - c["cells"]) <= REL * np.abs(c["cells"]))
        assert close(st["e_cnt"], c["e_cnt"]) and close(pred, c["pred_cnt"]), (c["seed"], pred, c["pred_cnt"], st["e_cnt"], c["e_cnt"])


def test_script_rects_follow_the_scripts_slicing():
    """Line :238 slices a [1, 1, 384, 683] tensor: the whole map for a box at x = y = 0, nothing otherwise -- against torch slicing."""
    dm = torch.arange(384 * 683, dtype=torch.float32).reshape(384, 683) / 1e5
    for box in ([0, 0, 50, 40], [0, 3, 50, 40], [2, 0, 50, 40], [100, 200, 60, 30], [0, 0, 0, 0]):
        want = torch.sum(dm[None, None][int(box[0]):int(box[0] + box[2] + 1), int(box[1]):int(box[1] + box[3] + 1)] / 60).item()
        _p, st = D.count_rule_host(dm.numpy(), D.script_rects([box, [5, 5, 5, 5]]))
        assert abs(2 * st["e_cnt"] - want) <= REL * abs(want)


def test_count_rule_host_clips_rectangles_and_drops_trailing_columns():
    rs = np.random.RandomState(3)
    dm = rs.uniform(0, 0.5, size=(32, 40)).astype(np.float32)
    pred, st = D.count_rule_host(dm, [[30, 38, 10, 10], [32, 0, 4, 4]])      # one clipped by the map, one wholly outside
    assert st["cells"].shape == (2, 2)
    assert close(st["total"], float(dm[:, :32].astype(np.float64).sum() / 60))
    assert close(st["e_cnt"], float(dm[30:, 38:].astype(np.float64).sum() / 60) / 2)
    assert close(pred, st["total"] - st["n_over"] + (2 if st["e_cnt"] <= 0.5 else 0))


def test_train_target_reproduces_the_reference(golden):
    _s, cases = golden
    for c in cases:
        boxes = c["boxes"]
        assert sorted(D.train_cells(boxes)) == [tuple(v) for v in c["target_cells"]]
        gt = D.train_target_host(boxes)
        assert gt.shape == (384, 384) and gt.dtype == np.float32
        assert close(float(gt.astype(np.float64).sum()), c["target_sum"])
    # a centre right of column 720 is dropped, duplicates collapse
    assert D.train_cells([[700, 10, 60, 20], [10, 10, 20, 20], [10, 10, 21, 21], [11, 11, 20, 20]]) == [(10, 10), (11, 11)]


def test_random_streams_stay_in_step(golden):
    stream_seed, cases = golden
    for c in cases:
        random.seed(stream_seed + c["seed"])
        assert D.test_draws(len(c["boxes"])) == (0, 1)
        assert random.random() == c["after_test"]
        random.seed(stream_seed + c["seed"])
        np.random.seed(stream_seed + c["seed"])
        assert D.train_draw(len(c["boxes"])) == c["train_idx"]
        assert D.train_mask_draw().shape == (384, 384)
        assert [random.random(), float(np.random.random_sample())] == c["after_train"]


def test_devkit_loader(tmp_path):
    from PIL import Image
    for d in ("Images", "Annotations", "ImageSets"):
        (tmp_path / d).mkdir()
    rs = np.random.RandomState(0)
    frames, names = {}, ["20160331_NTU_00001", "20160331_NTU_00002", "20161225_TPZ_00003"]
    for k, name in enumerate(names):
        frames[name] = rs.randint(0, 256, size=(36 + k, 64, 3)).astype(np.uint8)
        Image.fromarray(frames[name]).save(tmp_path / "Images" / (name + ".png"))
        (tmp_path / "Annotations" / (name + ".txt")).write_text("".join("%d %d %d %d 1\n" % (3 + j, 4 + j, 20 + 2 * j, 14 + j) for j in range(k + 2)))
    (tmp_path / "ImageSets" / "train.txt").write_text("\n".join(names[:2]) + "\n")
    (tmp_path / "ImageSets" / "test.txt").write_text(names[2] + "\n")
    assert D.available(str(tmp_path), "train") and not D.available(str(tmp_path), "val")
    train, test = D.Devkit(str(tmp_path), "train"), D.Devkit(str(tmp_path), "test")
    assert len(train) == 2 and len(test) == 1
    for ds, sel in ((train, names[:2]), (test, names[2:])):
        for k, name in enumerate(sel):
            it = ds[k]
            assert it["name"] == name and it["images"].dtype == np.uint8 and np.array_equal(it["images"], frames[name])
            nb = names.index(name) + 2
            assert it["boxes"] == [[3 + j, 4 + j, 17 + j, 10] for j in range(nb)]      # w = x2 - x1, h = y2 - y1
