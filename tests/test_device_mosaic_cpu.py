"""CPU: the host half of the device mosaic (countr_amd/data/fsc147.py: mosaic_plan, recipe_train(device_mosaic=True)) against the host
transform it must agree with draw for draw and cell for cell, the argument checks of countr_aug_mosaic (which run before anything
touches a GPU), and the hand-over of mosaic_dev recipes through a DataLoader."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from test_device_aug_cpu import LoggedRandom, aug_args, item_of

SEEDS = (0, 1, 2, 3)


@pytest.fixture(scope="module")
def aug_ds(tmp_path_factory):
    from countr_amd.data import fsc147 as D
    random.seed(3)
    return D.TrainData(aug_args(tmp_path_factory.mktemp("mos")), split="train", do_aug=True, device_aug=True, device_mosaic=True)


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


def host_mosaic_draws(log, ds, im_id, self_branch):
    """The draws of fsc147.mosaic() out of a LoggedRandom log (after the mosaic and the flip coin) ->
    bl, [(source id, length, start_w, start_h)] x 4, number of log entries used."""
    vals = [v for _k, v in log[2:]]
    bl, k, quads = vals[0], 1, []
    if self_branch:
        for _ in range(4):
            quads.append((im_id,) + tuple(vals[k:k + 3]))
            k += 3
    else:
        gt_pos = vals[k + 1]
        k += 2
        for q in range(4):
            src = im_id
            if q != gt_pos:
                src = ds.train_set[vals[k]]
                k += 1
            quads.append((src,) + tuple(vals[k:k + 3]))
            k += 3
    return bl, quads, k + 2


def same_recipe(a, b):
    assert sorted(a) == sorted(b)
    for key in a:
        x, y = a[key], b[key]
        if isinstance(x, torch.Tensor):
            assert torch.equal(x, y), key
        elif isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and np.array_equal(x, y), key
        elif key == "params":
            assert vars(x) == vars(y)
        elif key == "frames":
            assert len(x) == len(y) and all(torch.equal(p, q) for p, q in zip(x, y))
        else:
            assert x == y, key


def test_mosaic_dev_recipe_agrees_with_host_transform(aug_ds, dot_maps):
    from countr_amd.data import fsc147 as D
    kinds = set()
    for seed in SEEDS:
        for idx in range(len(aug_ds)):
            image, rects, dots, im_id = item_of(aug_ds, idx)
            rng = random.Random(1000 * seed + idx)
            rec = D.recipe_train(image, rects, dots, im_id, aug_ds, do_aug=True, rng=rng, nprng=np.random.RandomState(seed),
                                 noise_counter=idx, device_mosaic=True)
            lr = LoggedRandom(1000 * seed + idx)
            del dot_maps[:]
            ref = D.transform_train_aug(image, rects, dots, im_id, aug_ds, rng=lr, nprng=np.random.RandomState(77),
                                        params=rec.get("params") or D.AugParams(np.random.RandomState(1)))
            host_mosaic = lr.log[0][1] < 0.25
            assert rng.getstate() == lr.r.getstate()
            if not host_mosaic:
                plain = D.recipe_train(image, rects, dots, im_id, aug_ds, do_aug=True, rng=random.Random(1000 * seed + idx),
                                       nprng=np.random.RandomState(seed), noise_counter=idx)
                assert rec["kind"] == "aug"
                same_recipe(rec, plain)
                kinds.add("aug")
                continue
            assert rec["kind"] == "mosaic_dev" and "image" not in rec and "dens" not in rec and "params" not in rec
            assert rec["m_flag"] == ref["m_flag"] and rec["flip"] == (lr.log[1][1] > 0.5)
            assert rec["m_flag"] == (0 if len(dots) >= 70 else 1)
            bl, quads, used = host_mosaic_draws(lr.log, aug_ds, im_id, self_branch=len(dots) >= 70)
            assert used == len(lr.log)
            assert rec["bl"] == bl and len(rec["pieces"]) == 4
            frames, ids = rec["frames"], rec["frame_ids"]
            assert ids[0] == im_id and len(set(ids)) == len(ids) == len(frames) and rec["frame"] is frames[0]
            for (k, nh, nw, start_h, start_w, length), (src, h_len, h_sw, h_sh) in zip(rec["pieces"], quads):
                assert (ids[k], length, start_w, start_h) == (src, h_len, h_sw, h_sh)
                fr = frames[k]
                assert fr.dtype == torch.uint8 and fr.ndim == 3 and fr.shape[2] == 3
                assert torch.equal(fr, torch.from_numpy(np.array(aug_ds.open_image(src), dtype=np.uint8)))
                assert (nh, nw) == D.flex_resize(fr.shape[0], fr.shape[1])
                assert 0 <= start_h <= nh - length and 0 <= start_w <= nw - length
            assert (rec["new_h"], rec["new_w"]) == D.flex_resize(image.size[1], image.size[0])
            assert rec["n_dots"] == len(dots) and rec["im_id"] == im_id and len(rec["rects"]) == 3
            host_dots = dot_maps[-1]                     # the map the final filter of transform_train_aug saw
            assert host_dots.shape == (384, 384)
            cells = np.asarray(rec["cells"])
            assert cells.dtype == np.int32 and cells.ndim == 2 and cells.shape[1] == 2
            assert len(set(map(tuple, cells.tolist()))) == len(cells)
            assert set(map(tuple, cells.tolist())) == set(map(tuple, np.argwhere(host_dots != 0).tolist()))
            kinds.add("mosaic%d" % rec["m_flag"])
    assert kinds == {"aug", "mosaic0", "mosaic1"}, kinds


def test_default_recipe_is_unchanged(aug_ds, tmp_path):
    from countr_amd.data import fsc147 as D
    seen = 0
    for seed in SEEDS[:2]:
        for idx in range(len(aug_ds)):
            image, rects, dots, im_id = item_of(aug_ds, idx)
            rec = D.recipe_train(image, rects, dots, im_id, aug_ds, do_aug=True, rng=random.Random(1000 * seed + idx),
                                 nprng=np.random.RandomState(seed), noise_counter=idx)
            off = D.recipe_train(image, rects, dots, im_id, aug_ds, do_aug=True, rng=random.Random(1000 * seed + idx),
                                 nprng=np.random.RandomState(seed), noise_counter=idx, device_mosaic=False)
            same_recipe(rec, off)
            assert rec["kind"] in ("aug", "mosaic")
            if rec["kind"] == "mosaic":
                assert rec["image"].shape == (3, 384, 384) and rec["dens"].shape == (384, 384) and "frames" not in rec
                seen += 1
    assert seen > 0
    # the switch belongs to the augmented recipe loader
    args = aug_args(tmp_path / "d")
    for kw in (dict(do_aug=True, device_aug=False), dict(do_aug=False, device_aug=True)):
        with pytest.raises(ValueError, match="device_mosaic"):
            D.TrainData(args, split="train", device_mosaic=True, **kw)
    assert D.TrainData(args, split="train", do_aug=True, device_aug=True).device_mosaic is False


def test_mosaic_export_and_argument_checks():
    """countr_aug_mosaic is declared, present in both libraries, and refuses every bad argument before it touches a GPU."""
    from countr_amd import _lib
    assert _lib.ABI_VERSION == 9
    assert "countr_aug_mosaic" in _lib.exported_symbols()
    L = _lib.lib()
    assert hasattr(_lib.lib("f16"), "countr_aug_mosaic") and L.countr_version() == 9
    assert C.sizeof(_lib.MosaicPiece) == 32 and C.sizeof(_lib.MosaicImage) == 136       # the layout of include/countr_hip.h
    raw = (C.c_char * 256)()
    p = (C.addressof(raw) + 15) & ~15          # host memory: no check dereferences it, and no case below gets as far as a launch

    def table(n=1, **kw):
        t = (_lib.MosaicImage * max(n, 1))()
        for m in t:
            m.bl, m.row = 15, 0
            for q in m.piece:
                q.src, q.h, q.w, q.start_h, q.start_w, q.length = p, 400, 640, 10, 20, 250
        for name, v in kw.items():
            if name in ("bl", "row"):
                setattr(t[0], name, v)
            else:
                setattr(t[0].piece[2], name, v)
        return t

    def failed(rc):
        assert rc < 0 and L.countr_last_error()
        return L.countr_last_error().decode()

    for n in (0, -1, 33):
        assert "countr_aug_mosaic" in failed(L.countr_aug_mosaic(table(n), n, p, 4, None)), n
    assert "countr_aug_mosaic" in failed(L.countr_aug_mosaic(None, 1, p, 4, None))
    assert "countr_aug_mosaic" in failed(L.countr_aug_mosaic(table(), 1, None, 4, None))
    assert "countr_aug_mosaic" in failed(L.countr_aug_mosaic(table(), 1, p + 4, 4, None))
    assert "countr_aug_mosaic" in failed(L.countr_aug_mosaic(table(), 1, p, 0, None))
    for bad in (dict(bl=9), dict(bl=21), dict(length=0), dict(length=401), dict(h=300, length=301, start_h=0), dict(start_h=151),
                dict(start_w=391), dict(start_h=-1), dict(start_w=-1), dict(src=None), dict(row=-1), dict(row=4), dict(h=0), dict(w=-3)):
        assert "countr_aug_mosaic" in failed(L.countr_aug_mosaic(table(**bad), 1, p, 4, None)), bad
    # the last piece of the last image is checked like the first
    t = table(3)
    t[2].piece[3].start_w = 640 - 250 + 1
    assert "countr_aug_mosaic" in failed(L.countr_aug_mosaic(t, 3, p, 4, None))


class _Seeded(torch.utils.data.Dataset):
    """A TrainData whose item idx is drawn from random.seed(seeds[idx]), in a worker as in the parent."""

    def __init__(self, ds, seeds):
        self.ds, self.seeds = ds, seeds

    def __len__(self):
        return len(self.ds)

    def __getitem__(self, idx):
        random.seed(self.seeds[idx])
        return self.ds[idx]


def test_mosaic_dev_recipes_collate_through_a_dataloader(aug_ds):
    from countr_amd.data import fsc147 as D
    seeds = [next(s for s in range(100 * idx, 100 * idx + 100) if random.Random(s).random() < 0.25) for idx in range(len(aug_ds))]
    ds = _Seeded(aug_ds, seeds)
    dl = torch.utils.data.DataLoader(ds, batch_size=3, shuffle=False, num_workers=2, collate_fn=D.collate_recipes, drop_last=True)
    batches = list(dl)
    assert len(batches) == 2 and all(isinstance(b, list) and len(b) == 3 for b in batches)
    recs = [r for b in batches for r in b]
    assert [r["kind"] for r in recs] == ["mosaic_dev"] * 6 and {r["m_flag"] for r in recs} == {0, 1}
    assert max(len(r["frames"]) for r in recs) > 1
    for idx, r in enumerate(recs):
        same_recipe(r, ds[idx])
        assert all(f.dtype == torch.uint8 for f in r["frames"]) and torch.equal(r["frame"], r["frames"][0])
        assert isinstance(r["cells"], np.ndarray) and r["cells"].dtype == np.int32
        assert all(isinstance(v, int) for p in r["pieces"] for v in p) and isinstance(r["bl"], int)
