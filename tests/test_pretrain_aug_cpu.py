"""CPU: the host side of the device pretraining transform (csrc/pretrain_aug.hip, countr_amd/pretrain_aug.py, fsc147.recipe_pretrain)
-- Pillow's BICUBIC tap tables restated in the library, the whole chain (BILINEAR to multiples of 16, crop, BICUBIC to 384 x 384, flip,
ToTensor) applied in numpy from those tables against fsc147.transform_pretrain, the draw stream of the recipe, the recipe dataset and
the argument checks of the exports (which run before anything touches a GPU).  Every comparison is exact equality."""
import argparse
import ctypes as C
import json
import random

import numpy as np
import pytest
import torch
from PIL import Image

BILINEAR, BICUBIC = 0, 1


def _lib():
    from countr_amd import _lib
    return _lib, _lib.lib()


def _apply(src, bounds, weights):
    """One pass of Pillow's 8-bit resample along axis 0 of src [n, ...] uint8, in integer arithmetic (an arithmetic shift: the bicubic
    lobes can make a sum negative)."""
    out = np.empty((bounds.shape[0],) + src.shape[1:], np.uint8)
    for i, (first, cnt) in enumerate(bounds):
        k = weights[i, :cnt].astype(np.int64).reshape((cnt,) + (1,) * (src.ndim - 1))
        acc = (1 << 21) + (src[first:first + cnt].astype(np.int64) * k).sum(0)
        out[i] = np.clip(acc >> 22, 0, 255)
    return out


def _resize(img, oh, ow, filt, skip_equal=True):
    """Pillow's two-pass resize from the library's tables: horizontal into 8 bits, then vertical; Pillow skips a pass of equal sizes."""
    from countr_amd.frames import pil_filter_tables
    H, W = img.shape[:2]
    if not (skip_equal and W == ow):
        _k, hb, hw = pil_filter_tables(filt, W, ow)
        img = _apply(img.transpose(1, 0, 2), hb, hw).transpose(1, 0, 2)
    if not (skip_equal and H == oh):
        _k, vb, vw = pil_filter_tables(filt, H, oh)
        img = _apply(img, vb, vw)
    return img


def _images(H, W):
    rs = np.random.RandomState(H * 10007 + W)
    noise = rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    ramp = np.stack([(xx * 255.0 / max(W - 1, 1)), (yy * 255.0 / max(H - 1, 1)), ((xx + yy) * 255.0 / max(W + H - 2, 1))], 2).astype(np.uint8)
    return {"noise": noise, "ramp": ramp}


# every axis pair in -> 384 of the list (27, 257, 383, 384, 534, 918, 2) appears as a width pair and as a height pair
BICUBIC_FRAMES = [(27, 257), (257, 27), (383, 384), (384, 383), (534, 918), (918, 534), (2, 384), (384, 2)]      # (W, H)


@pytest.mark.parametrize("W,H", BICUBIC_FRAMES)
def test_bicubic_tables_reproduce_pillow_byte_for_byte(W, H):
    for name, img in _images(H, W).items():
        want = np.asarray(Image.fromarray(img).resize((384, 384), Image.BICUBIC))
        got = _resize(img, 384, 384, BICUBIC, skip_equal=False)      # (the 384 -> 384 tables are applied: they must be the identity)
        assert got.shape == want.shape
        assert np.array_equal(got, want), "%s %dx%d: %d bytes differ" % (name, W, H, int((got != want).sum()))


def test_table_layout_filters_and_bad_arguments():
    from countr_amd.frames import pil_filter_tables, pil_tables
    for n_in, ksize in ((2, 5), (27, 5), (257, 5), (383, 5), (384, 5), (534, 7), (918, 11)):
        k, bounds, weights = pil_filter_tables(BICUBIC, n_in, 384)
        assert k == ksize == weights.shape[1] and bounds.shape == (384, 2)
        assert k == 2 * int(np.ceil(2.0 * max(n_in / 384, 1.0))) + 1
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds[:, 1] <= k).all() and (bounds.sum(1) <= n_in).all()
        assert all((weights[i, c:] == 0).all() for i, c in enumerate(bounds[:, 1]))
        assert np.abs(weights.sum(1) - (1 << 22)).max() <= k          # normalised to 1.0 up to the rounding of each tap
    assert (pil_filter_tables(BICUBIC, 27, 384)[2] < 0).any()         # the negative lobes are there
    _k, b, w = pil_filter_tables(BICUBIC, 384, 384)                   # equal sizes: the identity
    assert (w.sum(1) == 1 << 22).all() and all(w[i, i - b[i, 0]] == 1 << 22 for i in range(384))
    for n_in, n_out in ((1920, 672), (1080, 384), (2160, 384), (427, 384), (131, 384), (384, 384), (53, 48), (37, 32), (1, 7)):
        k0, b0, w0 = pil_tables(n_in, n_out)
        k1, b1, w1 = pil_filter_tables(BILINEAR, n_in, n_out)
        assert k0 == k1 and np.array_equal(b0, b1) and np.array_equal(w0, w1)

    _l, L = _lib()

    def failed(rc):
        assert rc < 0 and L.countr_last_error()
        return L.countr_last_error().decode()

    buf = (C.c_int * 64)()
    p = C.cast(buf, C.c_void_p)
    assert "countr_pil_tables" in failed(L.countr_pil_tables(2, 10, 5, None, None))
    assert "countr_pil_tables" in failed(L.countr_pil_tables(-1, 10, 5, None, None))
    assert "countr_pil_tables" in failed(L.countr_pil_tables(1, 0, 10, None, None))
    assert "countr_pil_tables" in failed(L.countr_pil_tables(1, 10, -1, None, None))
    assert "countr_pil_tables" in failed(L.countr_pil_tables(0, 1 << 30, 1, None, None))
    assert "both" in failed(L.countr_pil_tables(1, 10, 5, p, None))
    assert L.countr_pil_tables(1, 10, 5, None, None) == 9             # the query form: 2 * ceil(2 * 2.0) + 1
    assert L.countr_pil_tables(0, 10, 5, None, None) == 5


def test_group_layout_and_descriptor_checks():
    """countr_pretrain_aug_layout and the checks the three descriptor exports share; no case gets as far as a launch."""
    from countr_amd import pretrain_aug as P
    _l, L = _lib()
    assert C.sizeof(_l.PretrainImage) == 40 and _l.PRETRAIN_MAX_IMAGES == 16 and L.countr_version() == 9
    assert hasattr(_l.lib("f16"), "countr_pretrain_aug") and "countr_pretrain_aug_tables" in _l.exported_symbols()
    raw = (C.c_char * 256)()
    p = (C.addressof(raw) + 15) & ~15          # host memory: no check dereferences it
    ok = [(p, 37, 53, (3, 5, 20, 30), True), (p, 800, 1100, (0, 0, 800, 1088), False)]
    stride, ints, nbytes, offs = P.layout(P.descriptors(ok))
    assert stride == 2 * int(np.ceil(2 * 1088 / 384)) + 1 == 13        # the widest crop of the group sets the stride
    outs = [[48, 32, 384, 384], [1088, 800, 384, 384]]
    flat = [o for s in outs for o in s]
    assert [o for s in offs for o in s] == [int(v) for v in np.concatenate([[0], np.cumsum([n * (2 + stride) for n in flat])[:-1]])]
    assert ints == sum(n * (2 + stride) for n in flat)
    pad = lambda n: (n + 15) & ~15
    assert nbytes == sum(pad(H * W16 * 3) + pad(H16 * W16 * 3) + pad(ch * 384 * 3)
                         for H, W16, H16, ch in ((37, 48, 32, 20), (800, 1088, 800, 800)))

    def failed(rc):
        assert rc < 0 and L.countr_last_error()
        return L.countr_last_error().decode()

    sizes = (C.c_int64 * 128)()
    one = (p, 64, 64, (0, 0, 64, 64), False)
    for bad in ([], [one] * 17, [(p, 15, 64, (0, 0, 1, 1), False)], [(p, 64, 15, (0, 0, 1, 1), False)], [(p, 64, 70, (0, 0, 64, 65), False)],
                [(p, 70, 64, (1, 0, 64, 64), False)], [(p, 64, 64, (-1, 0, 4, 4), False)], [(p, 64, 64, (0, 0, 0, 4), False)]):
        t = P.descriptors(bad) if bad else (_l.PretrainImage * 1)()
        assert "countr_pretrain_aug_layout" in failed(L.countr_pretrain_aug_layout(t, len(bad), sizes)), bad
        assert "countr_pretrain_aug_tables" in failed(L.countr_pretrain_aug_tables(t, len(bad), p, None)), bad
        assert "countr_pretrain_aug" in failed(L.countr_pretrain_aug(t, len(bad), p, p, p, 32, None)), bad
    t = P.descriptors([one])
    assert "countr_pretrain_aug_layout" in failed(L.countr_pretrain_aug_layout(t, 1, None))
    assert "countr_pretrain_aug_tables" in failed(L.countr_pretrain_aug_tables(t, 1, None, None))
    for args in ((None, p, p, 1), (p, None, p, 1), (p, p, None, 1), (p, p + 4, p, 1), (p, p, p + 4, 1)):
        assert "required" in failed(L.countr_pretrain_aug(t, 1, args[0], args[1], args[2], args[3], None)), args
    assert "row" in failed(L.countr_pretrain_aug(t, 1, p, p, p, 0, None))
    assert "null frame" in failed(L.countr_pretrain_aug(P.descriptors([(None, 64, 64, (0, 0, 64, 64), False)]), 1, p, p, p, 1, None))
    two = P.descriptors([one, one])
    two[1].row = 0
    assert "one destination row" in failed(L.countr_pretrain_aug(two, 2, p, p, p, 2, None))


def numpy_chain(recipe):
    """transform_pretrain from a recipe, in numpy, with the library's tables: what the device path computes."""
    fr = recipe["frame"].numpy()
    H, W = fr.shape[:2]
    img = _resize(fr, 16 * (H // 16), 16 * (W // 16), BILINEAR)
    i, j, ch, cw = recipe["crop"]
    img = _resize(img[i:i + ch, j:j + cw], 384, 384, BICUBIC)
    if recipe["flip"]:
        img = img[:, ::-1]
    return torch.from_numpy(np.ascontiguousarray(img)).permute(2, 0, 1).float().div(255.0)


CHAIN_FRAMES = [(37, 53), (384, 512), (384, 583), (800, 1100), (16, 400), (400, 17)]      # (H, W)


@pytest.mark.parametrize("H,W", CHAIN_FRAMES)
def test_numpy_chain_equals_transform_pretrain(H, W):
    from countr_amd.data import fsc147 as D
    image = Image.fromarray(_images(H, W)["noise"])
    flips = set()
    for seed in range(4):
        rec = D.recipe_pretrain(image, random.Random(seed))
        want = D.transform_pretrain(image, random.Random(seed))
        i, j, ch, cw = rec["crop"]
        assert 0 <= i and 0 <= j and 1 <= ch and 1 <= cw and i + ch <= 16 * (H // 16) and j + cw <= 16 * (W // 16)
        assert rec["frame"].dtype == torch.uint8 and tuple(rec["frame"].shape) == (H, W, 3)
        assert torch.equal(numpy_chain(rec), want), (H, W, seed, rec["crop"], rec["flip"])
        flips.add(rec["flip"])
    if min(H, W) < 32:      # ten failed draws, then the aspect-ratio fallback: the central crop over the whole short side
        assert (ch, cw) == ((16, 21) if H == 16 else (21, 16))
    assert flips <= {True, False}


def test_recipe_consumes_the_draws_of_the_transform():
    from countr_amd.data import fsc147 as D
    for H, W in CHAIN_FRAMES[:3] + CHAIN_FRAMES[4:]:
        image = Image.fromarray(_images(H, W)["ramp"])
        for seed in range(3):
            a, b = random.Random(seed), random.Random(seed)
            D.recipe_pretrain(image, a)
            D.transform_pretrain(image, b)
            assert a.getstate() == b.getstate(), (H, W, seed)
    with pytest.raises(ValueError):                # Pillow refuses the resize to a zero size with the same exception type
        D.recipe_pretrain(Image.fromarray(_images(15, 40)["ramp"]), random.Random(0))
    with pytest.raises(ValueError):
        D.transform_pretrain(Image.fromarray(_images(15, 40)["ramp"]), random.Random(0))


@pytest.fixture(scope="module")
def fake_fsc(tmp_path_factory):
    root = tmp_path_factory.mktemp("fsc_pre")
    (root / "images_384_VarV2").mkdir()
    names = []
    for k, (w, h) in enumerate([(120, 90), (64, 100), (53, 37)]):
        name = "%d.png" % k
        Image.fromarray(_images(h, w)["noise"]).save(root / "images_384_VarV2" / name)
        names.append(name)
    json.dump({n: {"points": [], "box_examples_coordinates": []} for n in names}, open(root / "annotation_FSC147_384.json", "w"))
    json.dump({"train": names, "val": [], "test": []}, open(root / "Train_Test_Val_FSC_147.json", "w"))
    return argparse.Namespace(data_path=str(root), anno_file="annotation_FSC147_384.json",
                              data_split_file="Train_Test_Val_FSC_147.json", im_dir="images_384_VarV2")


def test_recipe_dataset_collate_and_package_export(fake_fsc):
    import countr_amd
    from countr_amd import pretrain_aug
    from countr_amd.data import fsc147 as D
    assert countr_amd.PretrainAug is pretrain_aug.PretrainAug
    ds = D.PretrainData(fake_fsc, device_aug=True)
    host = D.PretrainData(fake_fsc)
    host.img = list(ds.img)
    assert len(ds) == 3 and ds.device_aug and not host.device_aug
    sizes = {"0.png": (90, 120), "1.png": (100, 64), "2.png": (37, 53)}
    for idx in range(3):
        random.seed(11 + idx)
        rec = ds[idx]
        random.seed(11 + idx)
        want = host[idx]                            # the default dataset still returns the finished tensor, from the same draws
        assert set(rec) == {"frame", "crop", "flip"} and tuple(rec["frame"].shape) == sizes[ds.img[idx]] + (3,)
        assert want.shape == (3, 384, 384) and torch.equal(numpy_chain(rec), want)
    loader = torch.utils.data.DataLoader(ds, batch_size=2, num_workers=0, collate_fn=D.collate_pretrain_recipes, drop_last=True)
    batches = list(loader)
    assert len(batches) == 1 and isinstance(batches[0], list) and len(batches[0]) == 2 and all(set(r) == {"frame", "crop", "flip"} for r in batches[0])
    with pytest.raises(countr_amd._lib.CountrError):
        pretrain_aug.PretrainAug("cpu")            # no host fallback
