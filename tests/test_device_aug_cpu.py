"""CPU: the host half of the device augmentation (countr_amd/data/fsc147.py: recipe_train, TrainData(device_aug=True)) against the host
transforms it must agree with, and the numpy restatement of the device's normal stream (include/countr_hip.h) that the GPU test
compares the kernels with."""
import argparse
import random

import numpy as np
import pytest
import torch

from oracle import weights as W
from oracle.philox import philox4x32_10


# ---------------------------------------------------------------------------------------------------------------------------------
# the normal stream of countr_aug_normal / countr_aug_jitter, restated: conversions in float32 as on the device, log / sin / cos in
# float64
# ---------------------------------------------------------------------------------------------------------------------------------
def normal_stream(seed, counter, n):
    """z[0..n) of stream (seed, counter) -> float64 [n]."""
    g = np.arange((n + 3) // 4, dtype=np.uint32)
    ctr = np.stack([g, np.ones_like(g), np.full_like(g, counter & 0xFFFFFFFF), np.full_like(g, (counter >> 32) & 0xFFFFFFFF)], axis=-1)
    r = philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    z = np.empty((len(g), 4), np.float64)
    for k in (0, 2):
        u1 = ((r[:, k] >> np.uint32(9)) + np.uint32(1)).astype(np.float32) * np.float32(2.0 ** -23)
        t = (r[:, k + 1] >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -23)           # 2 u2
        rad = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
        z[:, k] = rad * np.cos(np.pi * t.astype(np.float64))
        z[:, k + 1] = rad * np.sin(np.pi * t.astype(np.float64))
    return z.reshape(-1)[:n]


NOISE_SEED = 0          # the statistics below hold for this seed (checked here, on the restatement itself)


def test_normal_stream_restatement_statistics():
    n = 3 * 512 * 768
    z = normal_stream(NOISE_SEED, 5, n)
    x = 0.1 * z
    assert np.isfinite(x).all()
    assert abs(x.mean()) <= 5 * 0.1 / np.sqrt(n), x.mean()
    assert abs(x.var() - 0.01) <= 5 * 0.01 * np.sqrt(2.0 / n), x.var()
    # another counter or another seed is another stream; the same pair repeats
    assert np.array_equal(normal_stream(NOISE_SEED, 5, 4096), z[:4096])
    assert not np.array_equal(normal_stream(NOISE_SEED, 6, 4096), z[:4096])
    assert not np.array_equal(normal_stream(NOISE_SEED + 1, 5, 4096), z[:4096])


# ---------------------------------------------------------------------------------------------------------------------------------
# recipes
# ---------------------------------------------------------------------------------------------------------------------------------
class LoggedRandom:
    """random.Random(seed) behind the two methods the transforms use, with a log of every draw."""

    def __init__(self, seed):
        self.r = random.Random(seed)
        self.log = []

    def random(self):
        v = self.r.random()
        self.log.append(("random", v))
        return v

    def randint(self, a, b):
        v = self.r.randint(a, b)
        self.log.append(("randint", v))
        return v


def aug_args(root):
    W.write_aug_dataset(str(root))
    return argparse.Namespace(data_path=str(root), anno_file="anno.json", data_split_file="split.json", im_dir="images",
                              class_file="classes.txt", seed=0)


@pytest.fixture(scope="module")
def aug_ds(tmp_path_factory):
    from countr_amd.data import fsc147 as D
    random.seed(3)
    return D.TrainData(aug_args(tmp_path_factory.mktemp("aug")), split="train", do_aug=True, device_aug=True)


def item_of(ds, idx):
    im_id = ds.img[idx]
    anno = ds.annotations[im_id]
    dots = np.array(anno["points"])
    rects = [[b[0][1], b[0][0], b[2][1], b[2][0]] for b in anno["box_examples_coordinates"]]
    return ds.open_image(im_id), rects, dots, im_id


@pytest.fixture()
def dot_maps(monkeypatch):
    """The inputs of scipy.ndimage.gaussian_filter while the fixture lives: the host transforms' dot maps before the filter."""
    from scipy import ndimage
    seen, orig = [], ndimage.gaussian_filter

    def spy(a, *args, **kw):
        seen.append(np.array(a, copy=True))
        return orig(a, *args, **kw)
    monkeypatch.setattr(ndimage, "gaussian_filter", spy)
    return seen


SEEDS = (0, 1, 2, 3)


def test_recipe_agrees_with_host_transform(aug_ds, dot_maps):
    from scipy import ndimage
    from countr_amd.data import fsc147 as D
    kinds, flips, cases = set(), set(), 0
    for seed in SEEDS:
        for idx in range(len(aug_ds)):
            image, rects, dots, im_id = item_of(aug_ds, idx)
            rec = D.recipe_train(image, rects, dots, im_id, aug_ds, do_aug=True, rng=random.Random(1000 * seed + idx),
                                 nprng=np.random.RandomState(seed), noise_counter=idx)
            lr = LoggedRandom(1000 * seed + idx)
            del dot_maps[:]
            ref = D.transform_train_aug(image, rects, dots, im_id, aug_ds, rng=lr, nprng=np.random.RandomState(77),
                                        params=rec.get("params") or D.AugParams(np.random.RandomState(1)))
            host_mosaic, host_flip = lr.log[0][1] < 0.25, lr.log[1][1] > 0.5
            assert (rec["kind"] == "mosaic") == host_mosaic and rec["flip"] == host_flip and rec["m_flag"] == ref["m_flag"]
            assert tuple(rec["frame"].shape) == (image.size[1], image.size[0], 3) and rec["frame"].dtype == torch.uint8
            assert (rec["new_h"], rec["new_w"]) == D.flex_resize(image.size[1], image.size[0])
            assert rec["n_dots"] == len(dots) and rec["im_id"] == im_id
            sh, sw = rec["new_h"] / image.size[1], rec["new_w"] / image.size[0]
            img_t = D.to_tensor(image.resize((rec["new_w"], rec["new_h"]), 2))          # 2 = PIL BILINEAR
            assert list(rec["rects"]) == list(D.exemplar_crops(img_t, rects, sh, sw)[1])
            host_dots = dot_maps[-1]                     # the map the final filter of transform_train_aug saw
            assert host_dots.shape == (384, 384)
            cells = np.asarray(rec["cells"]).reshape(-1, 2)
            assert len(set(map(tuple, cells.tolist()))) == len(cells)
            assert set(map(tuple, cells.tolist())) == set(map(tuple, np.argwhere(host_dots != 0).tolist()))
            if host_mosaic:
                assert torch.equal(rec["image"], ref["image"])
                dens = torch.from_numpy(ndimage.gaussian_filter(rec["dens"].numpy(), sigma=(1, 1), order=0) * 60)
                assert torch.equal(dens, ref["gt_density"])
                assert "params" not in rec
                kinds.add("mosaic%d" % rec["m_flag"])
            else:
                assert (rec["start_w"], rec["start_h"]) == (lr.log[2][1], lr.log[3][1]) and len(lr.log) == 4
                assert rec["noise_counter"] == idx
                kinds.add("aug")
            flips.add(host_flip)
            cases += 1
    assert kinds == {"aug", "mosaic0", "mosaic1"} and flips == {False, True}, (kinds, flips)


def test_plain_recipe_agrees_with_host_transform(aug_ds, dot_maps):
    from countr_amd.data import fsc147 as D
    for seed in SEEDS[:2]:
        for idx in range(len(aug_ds)):
            image, rects, dots, im_id = item_of(aug_ds, idx)
            rec = D.recipe_train(image, rects, dots, im_id, aug_ds, do_aug=False, rng=random.Random(50 * seed + idx))
            lr = LoggedRandom(50 * seed + idx)
            del dot_maps[:]
            ref = D.transform_train_noaug(image, rects, dots, rng=lr)
            assert rec["kind"] == "plain" and rec["m_flag"] == 0 and (rec["start_h"], rec["start_w"]) == (0, lr.log[1][1])
            cells = np.asarray(rec["cells"]).reshape(-1, 2)
            assert set(map(tuple, cells.tolist())) == set(map(tuple, np.argwhere(dot_maps[-1] != 0).tolist()))
            assert ref["gt_density"].shape == (384, 384)


def test_noise_counters(aug_ds):
    n = len(aug_ds)
    seen = {}
    for epoch in (0, 1, 2):
        aug_ds.set_epoch(epoch)
        for idx in range(n):
            c = aug_ds.noise_counter(idx)
            assert c not in seen, (epoch, idx, seen[c])
            seen[c] = (epoch, idx)
    aug_ds.set_epoch(1)
    assert [aug_ds.noise_counter(i) for i in range(n)] == [c for c, (e, _i) in sorted(seen.items()) if e == 1]
    # the recipe carries the counter of its (epoch, index)
    random.seed(11)
    got = [aug_ds[i] for i in range(n)]
    assert all(r["noise_counter"] == aug_ds.noise_counter(i) for i, r in enumerate(got) if r["kind"] == "aug")
    aug_ds.set_epoch(0)


def test_default_dataset_is_unchanged(aug_ds, tmp_path):
    """Without device_aug (and for the val split with it) TrainData returns the tensors it always returned."""
    from countr_amd.data import fsc147 as D
    args = aug_args(tmp_path / "d")
    item = D.TrainData(args, split="train", do_aug=False)[0]
    assert len(item) == 7 and item[0].shape == (3, 384, 384)
    item = D.TrainData(args, split="val", do_aug=False, device_aug=True)[0]
    assert len(item) == 7 and item[0].shape == (3, 384, 384)


def test_recipes_collate_through_a_dataloader(aug_ds):
    from countr_amd.data import fsc147 as D
    dl = torch.utils.data.DataLoader(aug_ds, batch_size=3, shuffle=False, num_workers=2, collate_fn=D.collate_recipes, drop_last=True)
    batches = list(dl)
    assert len(batches) == 2 and all(isinstance(b, list) and len(b) == 3 for b in batches)
    recs = [r for b in batches for r in b]
    assert len({tuple(r["frame"].shape) for r in recs}) > 1                  # frames of different sizes in one batch
    assert [r["im_id"] for r in recs] == list(aug_ds.img)
    assert all(r["frame"].dtype == torch.uint8 and r["kind"] in ("aug", "mosaic") and len(r["rects"]) == 3 for r in recs)
