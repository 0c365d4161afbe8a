"""GPU: the pretraining transform on the device (csrc/pretrain_aug.hip, countr_amd/pretrain_aug.py) against its oracle,
fsc147.transform_pretrain (Pillow BILINEAR to multiples of 16, crop, Pillow BICUBIC to 384 x 384, flip, ToTensor): the tables the device
computes against countr_pil_tables, the images of mixed batches, the grouping, unaligned frames, workspace reuse, the hand-over to
PretrainStep on its stream and the CLI flag.  Every comparison is exact equality."""
import json
import math
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = [(37, 53), (384, 512), (384, 583), (800, 1100), (16, 400), (400, 17)]      # (H, W)


def _image(H, W, salt=0):
    rs = np.random.RandomState(H * 10007 + W + salt)
    return Image.fromarray(rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8))


class Scripted:
    """A stand-in for random.Random that makes random_resized_crop_params return a chosen crop on its first attempt and the flip coin
    fall as chosen: transform_pretrain itself stays the oracle for crops its own distribution (20 % of the area at least) never draws."""

    def __init__(self, H16, W16, crop, flip):
        i, j, ch, cw = crop
        self.uniforms = [cw * ch / float(H16 * W16), math.log(cw / float(ch))]
        self.ints = [i, j]
        self.coin = 0.25 if flip else 0.75

    def uniform(self, a, b):
        return self.uniforms.pop(0)

    def randint(self, a, b):
        v = self.ints.pop(0)
        assert a <= v <= b
        return v

    def random(self):
        return self.coin


def _seed_with_flip(image, want, start):
    from countr_amd.data import fsc147 as D
    seed = start
    while D.recipe_pretrain(image, random.Random(seed))["flip"] != want:
        seed += 1
    return seed


@pytest.fixture(scope="module")
def mixed():
    """(recipes, expected [16, 3, 384, 384]) of the mixed batch: all six frame sizes, flips half and half, and three scripted crops."""
    from countr_amd.data import fsc147 as D
    scripted = {6: ((37, 53), (5, 7, 20, 3), True),              # a crop 3 px wide
                7: ((384, 583), (0, 0, 384, 576), False),        # ch = H16, cw = W16: the whole 16-multiple frame
                8: ((800, 1100), (500, 688, 300, 400), False)}    # touches the right and the bottom edge of the 800 x 1088 frame
    recipes, want = [], []
    for k in range(16):
        if k in scripted:
            (H, W), crop, flip = scripted[k]
            image = _image(H, W, salt=k)
            mk = lambda: Scripted(16 * (H // 16), 16 * (W // 16), crop, flip)
            rec = D.recipe_pretrain(image, mk())
            assert rec["crop"] == crop and rec["flip"] == flip
            want.append(D.transform_pretrain(image, mk()))
        else:
            H, W = FRAMES[k % 6]
            image = _image(H, W, salt=k)
            seed = _seed_with_flip(image, k % 2 == 1, 100 * k)
            rec = D.recipe_pretrain(image, random.Random(seed))
            want.append(D.transform_pretrain(image, random.Random(seed)))
        recipes.append(rec)
    assert sum(r["flip"] for r in recipes) == 8
    assert {tuple(r["frame"].shape[:2]) for r in recipes} == set(FRAMES)
    return recipes, torch.stack(want)


@pytest.fixture(scope="module")
def small():
    """(recipes, expected) of 18 frames of 37 x 53: two groups."""
    from countr_amd.data import fsc147 as D
    images = [_image(37, 53, salt=1000 + k) for k in range(18)]
    return ([D.recipe_pretrain(im, random.Random(k)) for k, im in enumerate(images)],
            torch.stack([D.transform_pretrain(im, random.Random(k)) for k, im in enumerate(images)]))


def _differing(got, want):
    return "%d of %d values differ, rows %s" % (int((got != want).sum()), want.numel(),
                                                sorted(set((got != want).nonzero()[:, 0].tolist())))


def test_device_tables_equal_the_host_tables_bit_for_bit(hip):
    from countr_amd import pretrain_aug as P
    from countr_amd.frames import pil_filter_tables
    aug = P.PretrainAug("cuda")
    dummy = torch.zeros(64, dtype=torch.uint8, device="cuda").data_ptr()      # the table kernel reads no frame
    sizes = [(37, 53, 20, 3), (384, 512, 384, 384), (384, 583, 384, 576), (800, 1100, 300, 400), (16, 400, 16, 21), (400, 17, 21, 16),
             (37, 53, 32, 2), (800, 1100, 800, 1088), (384, 583, 100, 2), (400, 17, 400, 16), (16, 400, 1, 384), (37, 53, 27, 48),
             (384, 512, 257, 383), (800, 1100, 534, 918), (384, 583, 383, 385), (17, 31, 16, 16)]      # (H, W, ch, cw)
    table = P.descriptors([(dummy, H, W, (0, 0, ch, cw), False) for H, W, ch, cw in sizes])
    tabs, stride, offs = aug.tables(table)
    tabs = tabs.cpu().numpy()
    assert stride == 13                                                      # 1088 -> 384: 2 ceil(2 * 1088 / 384) + 1
    seen = set()
    for s, (H, W, ch, cw) in enumerate(sizes):
        for a, (filt, n_in, n_out) in enumerate(((0, W, 16 * (W // 16)), (0, H, 16 * (H // 16)), (1, cw, 384), (1, ch, 384))):
            k, bounds, weights = pil_filter_tables(filt, n_in, n_out)
            o = offs[s][a]
            got_b = tabs[o:o + 2 * n_out].reshape(n_out, 2)
            got_w = tabs[o + 2 * n_out:o + (2 + stride) * n_out].reshape(n_out, stride)
            assert np.array_equal(got_b, bounds), (s, a, n_in, n_out)
            assert np.array_equal(got_w[:, :k], weights) and (got_w[:, k:] == 0).all(), (s, a, n_in, n_out, int((got_w[:, :k] != weights).sum()))
            seen.add((filt, n_in, n_out))
    assert {(0, 384, 384), (1, 384, 384), (1, 2, 384)} <= seen


def test_mixed_batch_equals_the_host_transform(hip, mixed):
    from countr_amd.pretrain_aug import PretrainAug
    recipes, want = mixed
    aug = PretrainAug("cuda")
    got = aug.batch(recipes).cpu()
    assert aug.launches == 5                                                 # tables + four passes, whatever the sizes
    assert got.shape == want.shape and torch.equal(got, want), _differing(got, want)


def test_groups_and_workspace_reuse(hip, mixed, small):
    """18 samples go in a group of 16 and a group of 2 that share the workspaces; then the mixed batch, the small one and the mixed one
    again from the same object: nothing stale is left behind by a batch of other sizes."""
    from countr_amd.pretrain_aug import PretrainAug
    aug = PretrainAug("cuda")
    recipes, want = small
    got = aug.batch(recipes).cpu()
    assert aug.launches == 10
    assert torch.equal(got, want), _differing(got, want)
    first = aug.batch(mixed[0])
    again_small = aug.batch(recipes)
    second = aug.batch(mixed[0])
    assert first.data_ptr() != second.data_ptr()                             # a new tensor per call: PretrainStep.load keeps the reference
    assert torch.equal(first, second) and torch.equal(first.cpu(), mixed[1]) and torch.equal(again_small.cpu(), want)


def test_unaligned_frames(hip):
    """Frames one byte off a 16-byte boundary: the 16-byte staging loads and the 4-byte loads of the vertical pass are not used for them.
    37 x 48 runs the vertical pass on the frame itself (its width is a multiple of 16), 384 x 512 runs the bicubic pass on the frame."""
    from countr_amd.data import fsc147 as D
    from countr_amd.pretrain_aug import PretrainAug
    aug = PretrainAug("cuda")
    entries, want, keep = [], [], []
    for k, (H, W) in enumerate([(37, 53), (37, 48), (384, 512), (400, 17)]):
        image = _image(H, W, salt=2000 + k)
        rec = D.recipe_pretrain(image, random.Random(k))
        want.append(D.transform_pretrain(image, random.Random(k)))
        arena = torch.zeros(rec["frame"].numel() + 32, dtype=torch.uint8, device="cuda")
        off = 1 if k != 3 else 0                                             # (one aligned frame in the same group)
        arena[off:off + rec["frame"].numel()].copy_(rec["frame"].reshape(-1))
        assert arena.data_ptr() % 16 == 0
        keep.append(arena)
        entries.append((arena.data_ptr() + off, H, W, rec["crop"], rec["flip"]))
    got = aug.run(entries).cpu()
    want = torch.stack(want)
    assert torch.equal(got, want), _differing(got, want)


def test_wide_crop_halves_the_horizontal_tile(hip):
    """A 16 x 8208 frame (both multiples of 16: stage 1 is skipped) with the crop 16 x 8100: the bicubic horizontal pass runs at scale
    21.09 with 87 taps, 256 output pixels would stage (ceil(21.09 * 255) + 87 + 1) * 3 + 48 = 16 449 bytes of a row and the 16 384-byte
    staging buffer takes 128 per work item instead.  Flip off and on."""
    from countr_amd.data import fsc147 as D
    from countr_amd.pretrain_aug import PretrainAug
    H, W, crop = 16, 8208, (0, 0, 16, 8100)
    image = _image(H, W, salt=5000)
    recipes, want = [], []
    for flip in (False, True):
        rec = D.recipe_pretrain(image, Scripted(H, W, crop, flip))
        assert rec["crop"] == crop and rec["flip"] == flip
        recipes.append(rec)
        want.append(D.transform_pretrain(image, Scripted(H, W, crop, flip)))
    got = PretrainAug("cuda").batch(recipes).cpu()
    want = torch.stack(want)
    assert torch.equal(got, want), _differing(got, want)


def test_batch_on_the_step_stream_feeds_the_step(hip):
    """batch() inside PretrainStep.on_stream(), then load + step: the loss of the step equals the one from the host-built tensor."""
    from countr_amd.data import fsc147 as D
    from countr_amd.pretrain_aug import PretrainAug
    from countr_amd.trainer import PretrainStep
    from functools import partial
    from countr_amd.models_mae_noct import MaskedAutoencoderViTNoCT
    from oracle import weights as W

    def build(name, seed):      # the smallest MAE configuration of the pretraining tests, fp32
        p, Dm, depth, Hh, Dd, ddepth, Hd = W.MAE_CONFIGS[name]
        m = MaskedAutoencoderViTNoCT(patch_size=p, embed_dim=Dm, depth=depth, num_heads=Hh, decoder_embed_dim=Dd, decoder_depth=ddepth,
                                     decoder_num_heads=Hd, mlp_ratio=4, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), precision="fp32")
        m.load_state_dict({k: torch.from_numpy(v) for k, v in W.make_state_dict_mae(name, seed=seed).items()}, strict=True)
        return m.to("cuda")
    images = [_image(37, 53, salt=3000 + k) for k in range(2)]
    recipes = [D.recipe_pretrain(im, random.Random(k)) for k, im in enumerate(images)]
    host = torch.stack([D.transform_pretrain(im, random.Random(k)) for k, im in enumerate(images)])
    _imgs, ids_shuffle, _r, _k = W.make_mae_inputs(batch=2, seed=7, mask_ratio=0.5)
    losses = []
    for device_path in (True, False):
        m = build("tiny_test", seed=5)
        step = PretrainStep(m, batch=2, mask_ratio=0.5, lr=1e-3, weight_decay=0.05, eps=1e-4, use_graph=True)
        aug = PretrainAug("cuda")
        with step.on_stream():
            imgs = aug.batch(recipes) if device_path else host
            step.load(imgs, torch.from_numpy(ids_shuffle).cuda())
            loss = step.step().clone()
        torch.cuda.synchronize()
        losses.append(loss.cpu())
    assert torch.isfinite(losses[0]).all() and torch.equal(losses[0], losses[1]), losses


def test_pretrain_cli_device_aug(tmp_path):
    root = tmp_path / "fsc"
    (root / "images_384_VarV2").mkdir(parents=True)
    names = []
    for k, (w, h) in enumerate([(640, 384), (512, 384), (700, 400), (53, 37)]):
        names.append("%d.png" % k)
        _image(h, w, salt=4000 + k).save(root / "images_384_VarV2" / names[-1])
    json.dump({n: {"points": [], "box_examples_coordinates": []} for n in names}, open(root / "annotation_FSC147_384.json", "w"))
    json.dump({"train": names, "val": [], "test": []}, open(root / "Train_Test_Val_FSC_147.json", "w"))
    r = subprocess.run([sys.executable, "FSC_pretrain.py", "--data_path", str(root), "--batch_size", "2", "--epochs", "1", "--warmup_epochs", "0",
                        "--num_workers", "2", "--output_dir", "", "--resume", "", "--log_every", "1", "--device_aug"],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 2 and all(np.isfinite(l["loss"]) and l["loss"] > 0 for l in lines)          # 4 images / batch 2
