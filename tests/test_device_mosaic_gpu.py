"""GPU: countr_aug_mosaic (csrc/mosaic.hip) through ctypes against fsc147.mosaic() with injected draws, then DeviceAug.batch and the CLI
with mosaic_dev recipes on the six-image dataset.  Bars (issue "build the mosaic samples in HIP"): 1e-4 max abs over ALL pixels for
the mosaic image -- the bar every stage of the device augmentation carries against its host function (TOL of test_device_aug_gpu.py)
-- 1e-4 for the exemplars, 1e-5 x max for the density; everything the host mosaic path also computes must come out bit for bit.
Measured on an MI355X (profiles/device_aug.txt): kernel 1.4e-5 worst over five mosaics, DeviceAug.batch mosaic images 7.2e-6."""
import ctypes as C
import json
import os
import random
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from oracle import weights as W
from test_device_aug_cpu import NOISE_SEED, aug_args, item_of
from test_device_aug_gpu import frame, params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4


class Draws:
    """The two methods mosaic() draws with, fed from a list; a value outside the bounds mosaic() asks for is a mistake of the test."""

    def __init__(self, values):
        self.values = list(values)

    def randint(self, a, b):
        v = self.values.pop(0)
        assert isinstance(v, int) and a <= v <= b, (a, v, b)
        return v

    def random(self):
        v = self.values.pop(0)
        assert isinstance(v, float)
        return v


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def mosaic_cases():
    """[(bl, [clean fp32 frame [3, h, w]], [(frame index, length, start_w, start_h)] x 4, host image)]: three self mosaics of one
    frame each (385 x 389, 384 x 461, 512 x 768) and two cross mosaics of four different frames, bl 10 / 15 / 20, lengths 150, 250
    and 384 (on 384-high frames too), starts at 0 and at new - length."""
    from PIL import Image
    from countr_amd.data import fsc147 as D
    cases = []
    dots = np.random.RandomState(0).uniform(2, 380, (80, 2))              # >= 70 dots: the self branch
    for bl, (h, w), quads in (
            (10, (385, 389), [(150, 0, 0), (250, 389 - 250, 385 - 250), (384, 5, 1), (150, 239, 235)]),
            (15, (384, 461), [(384, 0, 0), (384, 77, 0), (250, 0, 134), (150, 311, 234)]),
            (20, (512, 768), [(384, 384, 128), (150, 0, 362), (250, 518, 0), (201, 333, 77)])):
        img = frame(h, w, 3 * h + bl)
        host, _dens, m_flag = D.mosaic(img, dots, 1.0, 1.0, "own", None, Draws([bl] + [v for q in quads for v in q]))
        assert m_flag == 0
        cases.append((bl, [img], [(0,) + q for q in quads], host))
    # cross mosaics: the own frame in quadrant gt_pos, three foreign images decoded, flex_resize'd and PIL-resized by mosaic() itself
    foreign = {"f%d" % k: W.make_fsc_item(30 + k, w, h)[0] for k, (w, h) in enumerate([(461, 384), (768, 512), (1030, 680), (640, 400)])}
    ids = sorted(foreign)
    ctx = types.SimpleNamespace(train_set=ids, annotations={i: {"points": [[5.0, 5.0]]} for i in ids},
                                class_dict=dict({i: ["a"] for i in ids}, own=["b"]), open_image=lambda i: foreign[i])
    clean = {}
    for i, im in foreign.items():
        th, tw = D.flex_resize(im.size[1], im.size[0])
        clean[i] = D.to_tensor(im.resize((tw, th), Image.BILINEAR)).contiguous()
    few = dots[:20]                                                        # < 70 dots: the cross branch
    for bl, (h, w), gt_pos, quads in (
            (20, (400, 640), 1, [(0, 384, 64, 0), (None, 250, 390, 150), (1, 384, 384, 128), (2, 250, 0, 0)]),
            (10, (385, 389), 3, [(3, 250, 390, 0), (1, 300, 17, 212), (0, 384, 0, 0), (None, 384, 5, 1)])):
        own = frame(h, w, 11 * bl)
        draws, frames, index, pieces = [bl, 0.9, gt_pos], [own], {}, []
        for q, (t, length, start_w, start_h) in enumerate(quads):
            assert (t is None) == (q == gt_pos)
            if t is not None:
                draws.append(t)
                if t not in index:
                    index[t] = len(frames)
                    frames.append(clean[ids[t]])
            draws += [length, start_w, start_h]
            pieces.append((0 if t is None else index[t], length, start_w, start_h))
        host, _dens, m_flag = D.mosaic(own, few, 1.0, 1.0, "own", ctx, Draws(draws))
        assert m_flag == 1 and len(frames) == 4
        cases.append((bl, frames, pieces, host))
    return cases


def test_mosaic_kernel_against_host(hip):
    from countr_amd import _lib
    cases = mosaic_cases()
    assert {c[0] for c in cases} == {10, 15, 20} and {p[1] for c in cases for p in c[2]} >= {150, 250, 384}
    n = len(cases)
    tab = (_lib.MosaicImage * n)()
    keep = []
    for j, (bl, frames, pieces, _host) in enumerate(cases):
        dev = [f.cuda() for f in frames]
        keep.append(dev)
        tab[j].bl, tab[j].row = bl, n - 1 - j                      # rows in another order than the table's
        for q, (k, length, start_w, start_h) in zip(tab[j].piece, pieces):
            q.src, q.h, q.w = dev[k].data_ptr(), dev[k].shape[1], dev[k].shape[2]
            q.start_h, q.start_w, q.length = start_h, start_w, length
    out = torch.full((n + 1, 3, 384, 384), -7.0, device="cuda")   # one row more than the table names: it must stay as it is
    _lib.check(hip.countr_aug_mosaic(tab, n, out.data_ptr(), n + 1, stream()), "countr_aug_mosaic")
    got = out.cpu()
    worst = 0.0
    for j, (bl, frames, pieces, host) in enumerate(cases):
        err = (got[n - 1 - j] - host).abs().max().item()
        print("mosaic case %d (bl %d, %d frames, own frame %d x %d): max abs %.3e over all pixels"
              % (j, bl, len(frames), frames[0].shape[1], frames[0].shape[2], err))
        worst = max(worst, err)
    print("countr_aug_mosaic max abs against fsc147.mosaic %.3e" % worst)
    assert worst <= TOL
    assert torch.isfinite(got[:n]).all() and got[:n].min().item() >= 0.0 and got[:n].max().item() <= 1.0
    assert (got[n] == -7.0).all()
    # a second launch on the same descriptors: the same bits
    again = torch.full_like(out, -7.0)
    _lib.check(hip.countr_aug_mosaic(tab, n, again.data_ptr(), n + 1, stream()), "countr_aug_mosaic")
    assert torch.equal(again.cpu(), got)
    # a crop that leaves its frame is refused, not launched
    tab[0].piece[1].start_w += 1
    assert hip.countr_aug_mosaic(tab, n, out.data_ptr(), n + 1, stream()) != 0
    assert "countr_aug_mosaic" in hip.countr_last_error().decode()


# ---------------------------------------------------------------------------------------------------------------------------------
# DeviceAug on the six-image dataset
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def aug_ds(tmp_path_factory):
    from countr_amd.data import fsc147 as D
    random.seed(3)
    return D.TrainData(aug_args(tmp_path_factory.mktemp("mos")), split="train", do_aug=True, device_aug=True, device_mosaic=True)


def todays_launches(recs):
    """What DeviceAug.batch launches for up to 32 recipes without mosaic_dev: two per distinct frame shape for the resize, three for
    the jitter / blur chain when a recipe is augmented, window + exemplars + density."""
    return 2 * len({tuple(r["frame"].shape) for r in recs}) + (3 if any(r["kind"] == "aug" for r in recs) else 0) + 3


def test_device_aug_mosaic_dev_recipes(hip, aug_ds):
    from countr_amd import DeviceAug
    from countr_amd.data import fsc147 as D
    da = DeviceAug("cuda", batch=6, noise_seed=NOISE_SEED)
    da_host = DeviceAug("cuda", batch=6, noise_seed=NOISE_SEED)
    recs, hrecs, refs, noise = [], [], [], []
    for seed in (0, 1):
        for idx in range(len(aug_ds)):
            image, rects, dots, im_id = item_of(aug_ds, idx)
            kw = dict(do_aug=True, params=params((idx + seed) % 6), noise_counter=idx)
            rec = D.recipe_train(image, rects, dots, im_id, aug_ds, rng=random.Random(1000 * seed + idx), device_mosaic=True, **kw)
            hrecs.append(D.recipe_train(image, rects, dots, im_id, aug_ds, rng=random.Random(1000 * seed + idx), **kw))
            ref = D.transform_train_aug(image, rects, dots, im_id, aug_ds, rng=random.Random(1000 * seed + idx),
                                        nprng=np.random.RandomState(40 + idx), params=params((idx + seed) % 6))
            nz = np.random.RandomState(40 + idx).normal(0, 0.1, (3, rec["new_h"], rec["new_w"])) if rec["kind"] == "aug" else None
            recs.append(rec); refs.append(ref); noise.append(nz)
    assert {r["kind"] for r in recs} == {"aug", "mosaic_dev"} and {r["kind"] for r in hrecs} == {"aug", "mosaic"}
    assert {r["m_flag"] for r in recs if r["kind"] == "mosaic_dev"} == {0, 1}
    worst_m = worst_a = 0.0
    with_mosaic = 0
    for b0 in (0, 6):
        imgs, boxes, gt, flags = da.batch(recs[b0:b0 + 6], noise=noise[b0:b0 + 6])
        launches = da.launches
        himgs, hboxes, hgt, hflags = da_host.batch(hrecs[b0:b0 + 6], noise=noise[b0:b0 + 6])
        assert flags == hflags
        assert torch.equal(gt, hgt) and torch.equal(boxes, hboxes)
        for i in range(6):
            rec, ref = recs[b0 + i], refs[b0 + i]
            assert flags[i] == ref["m_flag"]
            err = (imgs[i].cpu() - ref["image"]).abs().max().item()
            if rec["kind"] == "mosaic_dev":
                worst_m = max(worst_m, err)
            else:
                worst_a = max(worst_a, err)
                assert torch.equal(imgs[i], himgs[i])
            assert (boxes[i].cpu() - ref["boxes"]).abs().max().item() <= TOL
            assert (gt[i].cpu() - ref["gt_density"]).abs().max().item() <= 1e-5 * max(ref["gt_density"].max().item(), 1e-30)
        # the budget: today's count, one mosaic launch, two per distinct frame shape over all uploaded frames
        batch = recs[b0:b0 + 6]
        shapes = {tuple(f.shape) for r in batch for f in (r["frames"] if r["kind"] == "mosaic_dev" else [r["frame"]])}
        if any(r["kind"] == "mosaic_dev" for r in batch):
            assert launches == todays_launches(batch) - 2 * len({tuple(r["frame"].shape) for r in batch}) + 1 + 2 * len(shapes)
            assert launches <= 7 + 1 + 2 * len(shapes), (launches, len(shapes))
            with_mosaic += 1
        else:                                                # (the six recipes of seed 1 are all augmented)
            assert launches == todays_launches(batch)
        assert da_host.launches == todays_launches(hrecs[b0:b0 + 6]) <= 7 + 2 * len({tuple(r["frame"].shape) for r in batch})
    print("DeviceAug.batch with mosaic_dev recipes: mosaic images max abs %.3e, augmented images %.3e against transform_train_aug"
          % (worst_m, worst_a))
    assert worst_m <= TOL and worst_a <= TOL and with_mosaic > 0
    # steady state: the same recipes give the same bits, and no workspace grows from the second call on
    a = da.batch(recs[:6])
    size = da.workspace_bytes()
    b = da.batch(recs[:6])
    c = da.batch(recs[:6])
    assert all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(a[:3], b[:3], c[:3]))
    assert da.workspace_bytes() == size
    assert 0 <= a[0].min().item() and a[0].max().item() <= 1
    # a batch without mosaic_dev recipes launches what it launches today, on a DeviceAug that has served mosaic_dev batches too
    da.batch(hrecs[:6])
    assert da.launches == todays_launches(hrecs[:6])
    only_aug = [r for r in recs if r["kind"] == "aug"][:4]
    da.batch(only_aug)
    assert da.launches == todays_launches(only_aug)


def _cli(root, out, extra):
    cmd = [sys.executable, "FSC_finetune_cross.py", "--data_path", root, "--anno_file", "anno.json", "--data_split_file", "split.json",
           "--im_dir", "images", "--class_file", "classes.txt", "--batch_size", "2", "--epochs", "1", "--warmup_epochs", "0",
           "--num_workers", "2", "--output_dir", out, "--resume", "", "--log_every", "1", "--blr", "1e-3"] + extra
    return subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)


def test_finetune_cli_with_device_mosaic(tmp_path):
    root = str(tmp_path / "data")
    W.write_aug_dataset(root)
    out = str(tmp_path / "ft")
    r = _cli(root, out, ["--device_aug", "--device_mosaic"])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 3 and all(np.isfinite(l["loss"]) for l in lines)          # 6 images / batch 2, 1 epoch
    assert os.path.exists(os.path.join(out, "checkpoint__finetuning_last.pth"))
    # the switch alone is refused with a message, before anything is loaded
    for extra in (["--device_mosaic"], ["--device_aug", "--device_mosaic", "--no_do_aug"]):
        r = _cli(root, str(tmp_path / "no"), extra)
        assert r.returncode != 0 and "--device_mosaic needs --device_aug and --do_aug" in r.stderr
        assert not os.path.exists(str(tmp_path / "no"))
