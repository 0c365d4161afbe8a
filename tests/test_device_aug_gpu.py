"""GPU: the augmentation kernels of csrc/augment.hip through ctypes, each against the host function of countr_amd/data/fsc147.py it
restates, then DeviceAug.batch and the CLI flag on the six-image dataset.  Bars (issue "train-time augmentation as HIP kernels"):
1e-4 max abs for the fp32 image kernels (the project's bar, tests/test_frames_gpu.py), 1e-5 x max for the density, 1e-5 for 0.1 z."""
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
from test_device_aug_cpu import NOISE_SEED, aug_args, item_of, normal_stream

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4

SIZES = [(512, 768), (384, 461), (672, 1024), (400, 640), (385, 389)]       # (h, w); 640 x 400 is a size flex_resize leaves as it is
ORDERS = [(1, 0, 2, 3), (3, 1, 0, 2), (0, 3, 1, 2), (2, 0, 3, 1), (0, 1, 3, 2), (2, 3, 0, 1)]   # contrast (1) and hue (3) in all four places


def params(k):
    """Six fixed AugParams: order k of ORDERS, the other draws spread over their ranges."""
    rs = np.random.RandomState(100 + k)
    u = lambda lo, hi: float(rs.uniform(lo, hi))
    return types.SimpleNamespace(order=list(ORDERS[k]), brightness=u(0.75, 1.25), contrast=u(0.85, 1.15), saturation=u(0.85, 1.15),
                                 hue=u(-0.15, 0.15), sigma=(0.1, 2.0, 0.7, 1.3, 0.4, 1.7)[k], rotate=u(-15, 15), scale=u(0.8, 1.2),
                                 shear=u(-10, 10), tx=u(-0.2, 0.2), ty=u(-0.2, 0.2))


def frame(h, w, seed):
    """noise plus ramp, [3, h, w] fp32 in [0, 1]"""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.stack([xx / w, yy / h, ((xx * 3 + yy * 5) % 256) / 255.0]) * 0.7 + rs.uniform(0, 0.3, (3, h, w))
    return torch.from_numpy(a.astype(np.float32))


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def cases():
    return [(h, w, k) for i, (h, w) in enumerate(SIZES) for k in range(6) if i < 4 or k < 2]      # 26 images, one table


def test_jitter_and_blur_against_host(hip):
    from countr_amd import _lib
    from countr_amd.data import fsc147 as D
    from countr_amd.device_aug import fill_params
    cs = cases()
    src = [frame(h, w, 10 * k + h) for h, w, k in cs]
    dsrc = [t.cuda() for t in src]
    jit = [torch.empty_like(t) for t in dsrc]
    blr = [torch.empty_like(t) for t in dsrc]
    tab = (_lib.AugImage * len(cs))()
    for d, (h, w, k), s, j, b in zip(tab, cs, dsrc, jit, blr):
        d.src, d.jit, d.blr, d.h, d.w = s.data_ptr(), j.data_ptr(), b.data_ptr(), h, w
        fill_params(d, h, w, params(k))
    partials = torch.empty(hip.countr_aug_partials_floats(len(cs)), device="cuda")
    _lib.check(hip.countr_aug_jitter(tab, len(cs), 0, partials.data_ptr(), stream()), "countr_aug_jitter")
    _lib.check(hip.countr_aug_blur(tab, len(cs), stream()), "countr_aug_blur")
    torch.cuda.synchronize()
    worst_j = worst_b = 0.0
    for (h, w, k), s, j, b in zip(cs, src, jit, blr):
        pr = params(k)
        ref = D.color_jitter(s, pr.order, pr.brightness, pr.contrast, pr.saturation, pr.hue)
        worst_j = max(worst_j, (j.cpu() - ref).abs().max().item())
        # the blur is compared on the device's own jitter output: one stage at a time
        worst_b = max(worst_b, (b.cpu() - D.gaussian_blur(j.cpu(), (7, 9), pr.sigma)).abs().max().item())
    print("jitter max abs %.3e, blur max abs %.3e" % (worst_j, worst_b))
    assert worst_j <= TOL and worst_b <= TOL
    # a second run gives the same bits (fixed-order mean)
    first = [j.clone() for j in jit]
    _lib.check(hip.countr_aug_jitter(tab, len(cs), 0, partials.data_ptr(), stream()), "countr_aug_jitter")
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, jit))


def test_warp_flip_crop_against_host(hip):
    from countr_amd import _lib
    from countr_amd.data import fsc147 as D
    from countr_amd.device_aug import fill_params
    cs = cases()
    src = [frame(h, w, 7 * k + w) for h, w, k in cs]
    dsrc = [t.cuda() for t in src]
    tab = (_lib.AugImage * len(cs))()
    rs = random.Random(5)
    for i, (d, (h, w, k), s) in enumerate(zip(tab, cs, dsrc)):
        fill_params(d, h, w, params(k))
        d.win, d.win_h, d.win_w, d.win_mode = s.data_ptr(), h, w, 1
        d.flip = i % 2
        d.start_h, d.start_w = ((0, 0), (h - 384, w - 384), (rs.randint(0, h - 384), rs.randint(0, w - 384)))[i % 3]
    out = torch.empty(len(cs), 3, 384, 384, device="cuda")
    _lib.check(hip.countr_aug_window(tab, len(cs), out.data_ptr(), stream()), "countr_aug_window")
    got = out.cpu()
    worst, excluded, total = 0.0, 0, 0
    for i, ((h, w, k), s) in enumerate(zip(cs, src)):
        pr, d = params(k), tab[i]
        M = D.affine_matrix(h, w, pr.rotate, pr.scale, pr.shear, pr.tx, pr.ty)
        ref = D.warp_affine(s, M)
        if d.flip:
            ref = ref.flip(-1)
        ref = ref[:, d.start_h:d.start_h + 384, d.start_w:d.start_w + 384]
        # float64 source coordinates of the window's pixels: a pixel may be left out only within 1e-6 of an edge of the source
        a = list(d.affine)
        yy, xx = np.mgrid[d.start_h:d.start_h + 384, d.start_w:d.start_w + 384].astype(np.float64)
        if d.flip:
            xx = w - 1 - xx
        sy, sx = a[2] + yy * a[0] + xx * a[1], a[5] + yy * a[3] + xx * a[4]
        near = (np.minimum(np.abs(sy), np.abs(sy - (h - 1))) < 1e-6) | (np.minimum(np.abs(sx), np.abs(sx - (w - 1))) < 1e-6)
        excluded += int(near.sum())
        total += near.size
        diff = (got[i] - ref).abs().numpy()
        diff[:, near] = 0
        worst = max(worst, float(diff.max()))
    print("warp max abs %.3e, %d of %d pixels excluded" % (worst, excluded, total))
    assert excluded <= 1e-4 * total
    assert worst <= TOL
    # copy mode: the plain crop
    for d in tab:
        d.win_mode, d.flip = 0, 0
    _lib.check(hip.countr_aug_window(tab, len(cs), out.data_ptr(), stream()), "countr_aug_window")
    got = out.cpu()
    assert all(torch.equal(got[i], s[:, tab[i].start_h:tab[i].start_h + 384, tab[i].start_w:tab[i].start_w + 384]) for i, s in enumerate(src))
    # a window outside the image is refused, not launched
    tab[0].start_w = tab[0].win_w - 383
    assert hip.countr_aug_window(tab, 1, out.data_ptr(), stream()) != 0


def test_density_against_scipy(hip):
    from scipy import ndimage
    from countr_amd import _lib
    rs = np.random.RandomState(4)
    sets = [rs.randint(0, 384, (300, 2)),
            np.array([[r, c] for r in (0, 1, 2, 3, 380, 381, 382, 383) for c in (0, 1, 2, 3, 190, 380, 381, 382, 383)]),       # the outermost four
            np.array([[100, 100], [100, 100], [100, 101], [101, 100], [102, 102], [0, 0], [383, 383], [0, 383]]),              # overlapping
            np.zeros((0, 2), np.int64),
            rs.randint(0, 384, (3000, 2))]
    flat = np.concatenate([(s[:, 0] << 16 | s[:, 1]).astype(np.int32) for s in sets])
    cells = torch.from_numpy(flat).cuda()
    tab = (_lib.AugImage * len(sets))()
    k = 0
    for d, s in zip(tab, sets):
        d.cell_off, d.cell_cnt = k, len(s)
        k += len(s)
    out = torch.empty(len(sets), 384, 384, device="cuda")
    _lib.check(hip.countr_aug_density(tab, len(sets), cells.data_ptr(), len(flat), out.data_ptr(), stream()), "countr_aug_density")
    got = out.cpu().numpy()
    for i, s in enumerate(sets):
        m = np.zeros((384, 384), np.float32)
        m[s[:, 0], s[:, 1]] = 1
        ref = ndimage.gaussian_filter(m, sigma=(1, 1), order=0) * 60
        n_cells = len(set(map(tuple, s.tolist())))
        err = np.abs(got[i] - ref).max()
        print("density set %d: max abs %.3e (max of map %.3f), sum / 60 = %.6f for %d cells" % (i, err, ref.max(), got[i].sum() / 60, n_cells))
        assert err <= 1e-5 * max(ref.max(), 1e-30) or (n_cells == 0 and err == 0)
        assert abs(got[i].astype(np.float64).sum() / 60 - n_cells) <= 1e-3


def test_device_noise_against_restatement(hip):
    from countr_amd import _lib
    n = 3 * 512 * 768
    out = torch.empty(n + 3, device="cuda")
    st = stream()
    _lib.check(hip.countr_aug_normal(out.data_ptr(), n, 0.1, NOISE_SEED, 5, st), "countr_aug_normal")
    a = out[:n].cpu().numpy()
    ref = 0.1 * normal_stream(NOISE_SEED, 5, n)
    err = np.abs(a - ref).max()
    print("0.1 z: max abs against the restatement %.3e" % err)
    assert err <= 1e-5
    _lib.check(hip.countr_aug_normal(out.data_ptr(), n, 0.1, NOISE_SEED, 5, st), "countr_aug_normal")
    assert np.array_equal(out[:n].cpu().numpy(), a)
    _lib.check(hip.countr_aug_normal(out.data_ptr(), n, 0.1, NOISE_SEED, 6, st), "countr_aug_normal")
    b = out[:n].cpu().numpy()
    assert not np.array_equal(b, a) and np.abs(b - 0.1 * normal_stream(NOISE_SEED, 6, n)).max() <= 1e-5
    _lib.check(hip.countr_aug_normal(out.data_ptr(), 1001, 0.1, NOISE_SEED, (7 << 32) | 9, st), "countr_aug_normal")       # n % 4 != 0, high counter word
    assert np.abs(out[:1001].cpu().numpy() - 0.1 * normal_stream(NOISE_SEED, (7 << 32) | 9, 1001)).max() <= 1e-5
    # the jitter draws the same stream per image, on the 16-byte path (plane % 4 == 0) and on the element-wise one
    for h, w in ((384, 461), (385, 389)):
        src = torch.full((3, h, w), 0.5, device="cuda")
        jit = torch.empty_like(src)
        tab = (_lib.AugImage * 1)()
        tab[0].src, tab[0].jit, tab[0].h, tab[0].w, tab[0].noise_mode, tab[0].counter = src.data_ptr(), jit.data_ptr(), h, w, 1, 11
        partials = torch.empty(hip.countr_aug_partials_floats(1), device="cuda")
        _lib.check(hip.countr_aug_jitter(tab, 1, NOISE_SEED, partials.data_ptr(), st), "countr_aug_jitter")
        ref = np.clip(0.5 + 0.1 * normal_stream(NOISE_SEED, 11, 3 * h * w), 0, 1).reshape(3, h, w)
        assert np.abs(jit.cpu().numpy() - ref).max() <= 1e-5


# ---------------------------------------------------------------------------------------------------------------------------------
# DeviceAug on the six-image dataset
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def aug_ds(tmp_path_factory):
    from countr_amd.data import fsc147 as D
    random.seed(3)
    return D.TrainData(aug_args(tmp_path_factory.mktemp("aug")), split="train", do_aug=True, device_aug=True)


def test_device_aug_plain_recipes(hip, aug_ds):
    from countr_amd import DeviceAug
    from countr_amd.data import fsc147 as D
    da = DeviceAug("cuda", batch=6, noise_seed=NOISE_SEED)
    recs, refs = [], []
    for idx in range(len(aug_ds)):
        image, rects, dots, im_id = item_of(aug_ds, idx)
        recs.append(D.recipe_train(image, rects, dots, im_id, aug_ds, do_aug=False, rng=random.Random(idx)))
        refs.append(D.transform_train_noaug(image, rects, dots, rng=random.Random(idx)))
    imgs, boxes, gt, flags = da.batch(recs)
    assert imgs.shape == (6, 3, 384, 384) and boxes.shape == (6, 3, 3, 64, 64) and gt.shape == (6, 384, 384) and flags == [0] * 6
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in (imgs, boxes, gt))
    for i, ref in enumerate(refs):
        assert torch.equal(imgs[i].cpu(), ref["image"])
        assert (boxes[i].cpu() - ref["boxes"]).abs().max().item() <= TOL
        assert (gt[i].cpu() - ref["gt_density"]).abs().max().item() <= 1e-5 * max(ref["gt_density"].max().item(), 1e-30)


def test_device_aug_augmented_and_mosaic_recipes(hip, aug_ds):
    from countr_amd import DeviceAug
    from countr_amd.data import fsc147 as D
    da = DeviceAug("cuda", batch=6, noise_seed=NOISE_SEED)
    recs, refs, noise = [], [], []
    for seed in (0, 1):
        for idx in range(len(aug_ds)):
            image, rects, dots, im_id = item_of(aug_ds, idx)
            rec = D.recipe_train(image, rects, dots, im_id, aug_ds, do_aug=True, rng=random.Random(1000 * seed + idx),
                                 params=params((idx + seed) % 6), noise_counter=idx)
            ref = D.transform_train_aug(image, rects, dots, im_id, aug_ds, rng=random.Random(1000 * seed + idx),
                                        nprng=np.random.RandomState(40 + idx), params=params((idx + seed) % 6))
            # the explicit noise is that RandomState's first draw
            nz = np.random.RandomState(40 + idx).normal(0, 0.1, (3, rec["new_h"], rec["new_w"])) if rec["kind"] == "aug" else None
            recs.append(rec); refs.append(ref); noise.append(nz)
    assert {r["kind"] for r in recs} == {"aug", "mosaic"}
    worst = 0.0
    outs = []
    for b0 in (0, 6):
        imgs, boxes, gt, flags = da.batch(recs[b0:b0 + 6], noise=noise[b0:b0 + 6])
        outs.append((imgs, boxes, gt))
        for i in range(6):
            rec, ref = recs[b0 + i], refs[b0 + i]
            assert flags[i] == ref["m_flag"]
            if rec["kind"] == "mosaic":
                assert torch.equal(imgs[i].cpu(), ref["image"])
            else:
                worst = max(worst, (imgs[i].cpu() - ref["image"]).abs().max().item())
            assert (boxes[i].cpu() - ref["boxes"]).abs().max().item() <= TOL
            assert (gt[i].cpu() - ref["gt_density"]).abs().max().item() <= 1e-5 * max(ref["gt_density"].max().item(), 1e-30)
    print("whole chain (explicit noise) max abs against transform_train_aug %.3e" % worst)
    assert worst <= TOL
    # outputs of consecutive calls are fresh tensors
    ptrs = [t.data_ptr() for o in outs for t in o]
    assert len(set(ptrs)) == len(ptrs)
    # same recipes, same noise seed (the generator): the same bits, and no workspace growth from the second call on
    a = da.batch(recs[:6])
    size = da.workspace_bytes()
    b = da.batch(recs[:6])
    c = da.batch(recs[:6])
    assert all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(a[:3], b[:3], c[:3]))
    assert da.workspace_bytes() == size
    assert da.launches <= 7 + 2 * len({tuple(r["frame"].shape) for r in recs[:6]})
    other = DeviceAug("cuda", batch=6, noise_seed=NOISE_SEED + 1).batch(recs[:6])
    assert not torch.equal(other[0], a[0])
    # the generated noise has the documented statistics on an image: x - clean over the unclamped interior is ~N(0, 0.01)
    assert torch.isfinite(a[0]).all() and 0 <= a[0].min().item() and a[0].max().item() <= 1


def test_chain_through_the_exports_with_explicit_noise(hip):
    """Resize -> jitter (explicit noise) -> blur -> warp / flip / crop through ctypes against transform_train_aug on frames whose resized
    sizes cover 768 x 512, 461 x 384 (element-wise path in the blur), 1024 x 672 and the unchanged 640 x 400."""
    from PIL import Image
    from countr_amd import _lib
    from countr_amd.data import fsc147 as D
    from countr_amd.device_aug import fill_params
    worst = 0.0
    for k, (w, h) in enumerate([(768, 512), (432, 360), (1024, 672), (640, 400), (770, 515), (1030, 680)]):
        image, rects, dots = W.make_fsc_item(20 + k, w, h)
        seed = next(s for s in range(100) if random.Random(s).random() >= 0.25)           # not a mosaic
        pr = params(k)
        ref = D.transform_train_aug(image, rects, dots, "x", None, rng=random.Random(seed), nprng=np.random.RandomState(k), params=pr)
        rng = random.Random(seed)
        rng.random()
        flip = rng.random() > 0.5
        nh, nw = D.flex_resize(h, w)
        start_w, start_h = rng.randint(0, nw - 384), rng.randint(0, nh - 384)
        clean = D.to_tensor(image.resize((nw, nh), Image.BILINEAR)).contiguous().cuda()          # (to_tensor's result is a permuted view)
        nz = torch.from_numpy(np.random.RandomState(k).normal(0, 0.1, (3, nh, nw)).astype(np.float32)).cuda()
        jit, blr = torch.empty_like(clean), torch.empty_like(clean)
        out = torch.empty(1, 3, 384, 384, device="cuda")
        tab = (_lib.AugImage * 1)()
        d = tab[0]
        d.src, d.jit, d.blr, d.noise, d.h, d.w, d.noise_mode = clean.data_ptr(), jit.data_ptr(), blr.data_ptr(), nz.data_ptr(), nh, nw, 2
        fill_params(d, nh, nw, pr)
        d.win, d.win_h, d.win_w, d.win_mode, d.flip, d.start_h, d.start_w = blr.data_ptr(), nh, nw, 1, int(flip), start_h, start_w
        partials = torch.empty(hip.countr_aug_partials_floats(1), device="cuda")
        _lib.check(hip.countr_aug_jitter(tab, 1, 0, partials.data_ptr(), stream()), "countr_aug_jitter")
        _lib.check(hip.countr_aug_blur(tab, 1, stream()), "countr_aug_blur")
        _lib.check(hip.countr_aug_window(tab, 1, out.data_ptr(), stream()), "countr_aug_window")
        err = (out[0].cpu() - ref["image"]).abs().max().item()
        print("chain %d x %d -> %d x %d: max abs %.3e" % (w, h, nw, nh, err))
        worst = max(worst, err)
    assert worst <= TOL


def _cli(root, out, extra):
    cmd = [sys.executable, "FSC_finetune_cross.py", "--data_path", root, "--anno_file", "anno.json", "--data_split_file", "split.json",
           "--im_dir", "images", "--class_file", "classes.txt", "--batch_size", "2", "--epochs", "2", "--warmup_epochs", "0",
           "--num_workers", "2", "--output_dir", out, "--resume", "", "--log_every", "1", "--blr", "1e-3", "--device_aug"] + extra
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout


@pytest.mark.parametrize("extra", [[], ["--no_do_aug"]], ids=["do_aug", "no_do_aug"])
def test_finetune_cli_with_device_aug(tmp_path, extra):
    root = str(tmp_path / "data")
    W.write_aug_dataset(root)
    out = str(tmp_path / "ft")
    log = _cli(root, out, extra)
    lines = [json.loads(l) for l in log.splitlines() if l.startswith("{")]
    assert len(lines) == 6 and all(np.isfinite(l["loss"]) for l in lines)          # 6 images / batch 2, 2 epochs
    assert os.path.exists(os.path.join(out, "checkpoint__finetuning_last.pth"))
