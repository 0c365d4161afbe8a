"""GPU: the CARPK path -- countr_carpk_prep_u8 against F.interpolate on the CPU, countr_carpk_count against the host rule,
count_carpk against inference.density_map + the host rule, and the two CARPK CLIs."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import weights as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CROP_TOL = 1e-4     # absolute, values in [0, 1]: the crop_resize bar of tests/test_frames_gpu.py (three times the ulp of an fp32 source
                    # coordinate in [256, 512) times a neighbour difference <= 1; source coordinates here stay below 1280)
SUM_TOL = 1e-4      # relative: an fp32 sum of 256 terms carries at most 256 * 2^-24 ~ 1.5e-5, plus the fold
LOSS_TOL = 2e-3     # relative: the bar tests/test_trainer_gpu.py applies to the fp32 finetune loss against the oracle


def make_frame(H, Wd, seed):
    rs = np.random.RandomState(seed + H * 31 + Wd)
    f = rs.randint(0, 256, size=(H, Wd, 3)).astype(np.uint8)
    if seed % 2:
        yy, xx = np.mgrid[0:H, 0:Wd]
        f = np.stack([xx * 255.0 / (Wd - 1), yy * 255.0 / (H - 1), (xx + yy) * 255.0 / (Wd + H - 2)], 2).astype(np.uint8)
    return f


def raw_prep(hip, frames, rects, oh, ow, cols):
    """countr_carpk_prep_u8 through ctypes; the outputs are pre-filled so that an unwritten element shows."""
    n = len(frames)
    dev = [torch.from_numpy(f).cuda() for f in frames]
    img = torch.full((n, 3, oh, cols), -1.0, device="cuda")
    ex = torch.full((max(len(rects), 1), 3, 64, 64), -1.0, device="cuda")
    flat = [int(v) for r in rects for v in r]
    rc = hip.countr_carpk_prep_u8((C.c_void_p * n)(*[d.data_ptr() for d in dev]), (C.c_int * (2 * n))(*[v for f in frames for v in f.shape[:2]]),
                                  n, (C.c_int * max(len(flat), 1))(*flat), len(rects), oh, ow, cols, img.data_ptr(), ex.data_ptr(),
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, hip.countr_last_error()
    torch.cuda.synchronize()
    return img.cpu(), ex[:len(rects)].cpu(), dev


def host_prep(frame, oh, ow):
    s = (torch.from_numpy(frame) / 255).permute(2, 0, 1)[None]
    return s, F.interpolate(s, size=(oh, ow), mode="bilinear", align_corners=False)[0]


def check_rects(frames, rects, ex, dev):
    for k, (f, y1, x1, y2, x2) in enumerate(rects):
        s = (torch.from_numpy(frames[f]) / 255).permute(2, 0, 1)[None]
        want = F.interpolate(s[:, :, y1:y2 + 1, x1:x2 + 1], size=(64, 64), mode="bilinear", align_corners=False)[0]
        sd = (dev[f] / 255).permute(2, 0, 1)[None]
        on_gpu = F.interpolate(sd[:, :, y1:y2 + 1, x1:x2 + 1], size=(64, 64), mode="bilinear", align_corners=False)[0].cpu()
        err = (ex[k] - want).abs().max().item()
        print("rect %s: max abs err %.3e (equal to torch on the GPU: %s)" % ((f, y1, x1, y2, x2), err, torch.equal(ex[k], on_gpu)))
        assert err <= CROP_TOL, (rects[k], err)


def test_prep_matches_interpolate_on_cpu(hip):
    """The bar is F.interpolate on the CPU in fp32 within CROP_TOL; equality with torch's GPU result is printed, not asserted."""
    frame = make_frame(720, 1280, 0)
    # 1 x 1, 3 x 40, one touching the bottom-right corner, one reaching past it
    rects = [[0, 10, 20, 10, 20], [0, 5, 7, 7, 46], [0, 650, 1200, 719, 1279], [0, 700, 1250, 760, 1300]]
    img, ex, dev = raw_prep(hip, [frame], rects, 384, 683, 683)
    _s, want = host_prep(frame, 384, 683)
    err = (img[0] - want).abs().max().item()
    on_gpu = F.interpolate((dev[0] / 255).permute(2, 0, 1)[None], size=(384, 683), mode="bilinear", align_corners=False)[0].cpu()
    print("720 x 1280 -> 384 x 683: max abs err %.3e (equal to torch on the GPU: %s)" % (err, torch.equal(img[0], on_gpu)))
    assert err <= CROP_TOL
    check_rects([frame], rects, ex, dev)
    # the training form: only the left 384 columns are computed (16-byte stores), the same bits
    left, ex2, _d = raw_prep(hip, [frame], rects, 384, 683, 384)
    assert torch.equal(left, img[..., :384]) and torch.equal(ex2, ex)
    assert (left[0] - want[..., :384]).abs().max().item() <= CROP_TOL


def test_prep_odd_sizes_scalar_path(hip):
    frame = make_frame(45, 77, 1)
    rects = [[0, 3, 5, 3, 5], [0, 30, 60, 44, 76], [0, 40, 70, 50, 90]]
    img, ex, dev = raw_prep(hip, [frame], rects, 24, 43, 43)
    err = (img[0] - host_prep(frame, 24, 43)[1]).abs().max().item()
    print("45 x 77 -> 24 x 43: max abs err %.3e" % err)
    assert err <= CROP_TOL
    check_rects([frame], rects, ex, dev)


def test_prep_two_shapes_in_one_call(hip):
    from countr_amd.carpk import CarpkPrep
    frames = [make_frame(720, 1280, 2), make_frame(427, 640, 3)]
    rects = [[0, 100, 900, 160, 1010], [1, 400, 600, 426, 639]]
    prep = CarpkPrep("cuda")
    img, ex = prep.prepare(frames, rects)
    torch.cuda.synchronize()
    assert img.shape == (2, 3, 384, 683) and ex.shape == (2, 3, 64, 64)
    for k, f in enumerate(frames):
        err = (img[k].cpu() - host_prep(f, 384, 683)[1]).abs().max().item()
        print("frame %d %s: max abs err %.3e" % (k, f.shape, err))
        assert err <= CROP_TOL
    check_rects(frames, rects, ex.cpu(), [torch.from_numpy(f).cuda() for f in frames])
    # device frames take the same launch
    img2, ex2 = prep.prepare([torch.from_numpy(f).cuda() for f in frames], rects)
    assert torch.equal(img2, img) and torch.equal(ex2, ex)
    with pytest.raises(Exception):
        prep.prepare(frames[:1], [[0, 800, 100, 900, 200]])          # empty after clipping: an error, as interpolate of an empty crop is


def synthetic_maps(n, H, Wd, seed, boosts):
    """Maps whose cells sit near 0.43 with `boosts[i]` cells of image i lifted to ~1.7."""
    rs = np.random.RandomState(seed)
    m = rs.uniform(0, 0.2, size=(n, H, Wd)).astype(np.float32)
    for i in range(n):
        for _ in range(boosts[i]):
            cy, cx = rs.randint(0, H // 16), rs.randint(0, Wd // 16)
            m[i, cy * 16:cy * 16 + 16, cx * 16:cx * 16 + 16] = rs.uniform(0.3, 0.5, size=(16, 16))
    return m


def run_count(hip, maps, rects):
    from countr_amd.carpk import CarpkPrep
    prep = CarpkPrep("cuda")
    dev = torch.from_numpy(maps).cuda()
    a = prep.count(dev, rects).cpu().numpy()
    b = prep.count(dev, rects).cpu().numpy()
    assert a.tobytes() == b.tobytes()                                # fixed summation order: two runs, the same bits
    return a


@pytest.mark.parametrize("shape,boosts,rects", [
    # n_over 0 / several / several; e_cnt small, large, and (wholly outside + clipped by the map)
    ((3, 384, 683), [0, 7, 3], [[[10, 20, 30, 40], [200, 300, 20, 20]], [[0, 0, 383, 682], [100, 100, 150, 200]],
                                [[384, 0, 10, 10], [370, 670, 50, 50]]]),
    ((1, 32, 40), [1], [[[0, 0, 31, 39], [30, 38, 10, 10]]]),        # 8 columns dropped by the cells, not by the rectangles
    ((1, 16, 16), [0], [[[0, 0, 3, 3], [16, 16, 2, 2]]]),
])
def test_count_kernel_matches_the_host_rule(hip, shape, boosts, rects):
    from countr_amd.data import carpk as D
    maps = synthetic_maps(*shape, seed=shape[1], boosts=boosts)
    got = run_count(hip, maps, rects)
    n_overs, flags = [], []
    for i in range(shape[0]):
        pred, st = D.count_rule_host(maps[i], rects[i])
        assert np.abs(st["cells"] - 1.224).min() >= 1e-3 and abs(st["e_cnt"] - 0.5) >= 1e-3      # margins of the exact comparisons
        print("map %d: host pred %.6f total %.6f n_over %d e_cnt %.6f | device %s" % (i, pred, st["total"], st["n_over"], st["e_cnt"], got[i]))
        assert int(got[i, 2]) == st["n_over"]
        assert (got[i, 3] <= 0.5) == (st["e_cnt"] <= 0.5)
        for g, w in ((got[i, 0], pred), (got[i, 1], st["total"]), (got[i, 3], st["e_cnt"])):
            assert abs(g - w) <= SUM_TOL * abs(w), (i, g, w)
        n_overs.append(st["n_over"]); flags.append(st["e_cnt"] <= 0.5)
    if shape[0] == 3:
        assert n_overs[0] == 0 and min(n_overs[1:]) > 1 and True in flags and False in flags


def _model(precision):
    import models_mae_cross
    m = models_mae_cross.mae_vit_base_patch16(precision=precision)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.make_state_dict("mae_vit_base_patch16", seed=0).items()})
    return m.to("cuda").eval()


@pytest.fixture(scope="module", params=["fp32", "bf16"])
def model(request):
    return _model(request.param)


# Synthetic samples whose maps, under the pinned weights, keep every cell >= 1e-3 away from the threshold in both precisions (2 of the
# first 96 seeds do: a random-weight map puts ~1000 cells between 0.3 and 1.5).  Both take the e_cnt <= 0.5 branch; the other branch
# is covered by test_count_kernel_matches_the_host_rule and by the golden cases of tests/test_carpk_cpu.py.
E2E_SEEDS = (40, 79)


def test_count_carpk_end_to_end(model):
    from countr_amd import count_carpk, inference
    from countr_amd.carpk import carpk_prep
    from countr_amd.data import carpk as D
    items = [D.synthetic_item(s) for s in E2E_SEEDS]
    frames, boxes = [it["images"] for it in items], [it["boxes"] for it in items]
    res = count_carpk(model, frames, boxes)
    prep = carpk_prep("cuda")
    img, ex = prep.prepare(frames, [[k] + D.box_rect(boxes[k][j]) for k in range(2) for j in (0, 1)])
    ex = ex.view(2, 1, 2, 3, 64, 64)
    for k, (pred, dm, st) in enumerate(res):
        assert dm.shape == (384, 683)
        assert torch.equal(dm, inference.density_map(model, img[k:k + 1], ex[k], 2))
        hp, hs = D.count_rule_host(dm.cpu().numpy(), D.script_rects(boxes[k]))
        print("frame %d: pred %.6f (host %.6f) total %.6f (%.6f) n_over %d (%d) e_cnt %.6f (%.6f); margins %.3e %.3e"
              % (k, pred, hp, st["total"], hs["total"], st["n_over"], hs["n_over"], st["e_cnt"], hs["e_cnt"],
                 np.abs(hs["cells"] - 1.224).min(), abs(hs["e_cnt"] - 0.5)))
        assert np.abs(hs["cells"] - 1.224).min() >= 1e-3 and abs(hs["e_cnt"] - 0.5) >= 1e-3
        assert st["n_over"] == hs["n_over"] and (st["e_cnt"] <= 0.5) == (hs["e_cnt"] <= 0.5)
        for g, w in ((pred, hp), (st["total"], hs["total"]), (st["e_cnt"], hs["e_cnt"])):
            assert abs(g - w) <= SUM_TOL * abs(w), (k, g, w)


def test_count_carpk_reuses_its_buffers(model):
    from countr_amd import count_carpk
    from countr_amd.data import carpk as D
    items = [D.synthetic_item(s) for s in E2E_SEEDS]
    frames, boxes = [it["images"] for it in items], [it["boxes"] for it in items]
    res = count_carpk(model, frames, boxes)
    del res
    torch.cuda.synchronize()
    first = torch.cuda.memory_allocated()
    res = count_carpk(model, [f.copy() for f in frames], boxes)
    del res
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == first


def run(cmd):
    r = subprocess.run([sys.executable] + cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout


def cli_model(precision):
    import models_mae_cross
    torch.manual_seed(0)                                             # the CLIs' seeded random model (--resume '')
    return models_mae_cross.mae_vit_base_patch16(norm_pix_loss=False, precision=precision)


def test_test_cli_prints_the_counts(tmp_path):
    from countr_amd import count_carpk
    from countr_amd.data import carpk as D
    preds = {}
    for precision in ("fp32", "bf16"):
        out = run(["FSC_test_CARPK.py", "--synthetic", "4", "--resume", "", "--output_dir", str(tmp_path / precision), "--precision", precision])
        lines = [l for l in out.splitlines() if "pred_cnt:" in l]
        assert len(lines) == 4 and [l.split(":")[0] for l in lines] == ["%d/4" % k for k in range(4)]
        preds[precision] = [float(l.split("pred_cnt:")[1].split(",")[0]) for l in lines]
        assert all(np.isfinite(p) for p in preds[precision])
        assert len([l for l in out.splitlines() if l.startswith("Current MAE:") and "RMSE:" in l]) == 1
        assert (tmp_path / precision / "log.txt").exists() and (tmp_path / precision / "CAR_stat.png").exists()
    data = D.Synthetic(4, seed=0)
    m = cli_model("fp32").to("cuda").eval()
    direct = count_carpk(m, [data[k]["images"] for k in range(4)], [data[k]["boxes"] for k in range(4)])
    assert preds["fp32"] == [p for p, _dm, _st in direct]


def test_finetune_cli_first_loss_matches_the_oracle(tmp_path):
    from oracle import countr_ref as R
    from countr_amd.carpk import CarpkPrep
    from countr_amd.data import carpk as D
    out = run(["FSC_finetune_CARPK.py", "--synthetic", "3", "--epochs", "1", "--resume", "", "--output_dir", str(tmp_path), "--precision", "fp32"])
    lines = [l for l in out.splitlines() if "loss:" in l and "-shot" in l]
    assert len(lines) == 3 and all(np.isfinite(float(l.split("loss:")[1].split(",")[0])) for l in lines)
    assert (tmp_path / "checkpoint.pth").exists()                    # util/misc.save_model's default name, as upstream calls it
    loss = float(lines[0].split("loss:")[1].split(",")[0])
    idx = int(lines[0].split("exemplar")[1])
    item = D.Synthetic(3, seed=0)[0]
    imgs, boxes, gt = CarpkPrep("cuda").train_sample(item["images"], item["boxes"], idx)
    torch.cuda.synchronize()
    assert imgs.shape == (1, 3, 384, 384) and boxes.shape == (1, 1, 3, 64, 64) and gt.shape == (1, 384, 384)
    want_gt = D.train_target_host(item["boxes"])
    assert np.abs(gt[0].cpu().numpy() - want_gt).max() <= 1e-5 * want_gt.max()
    sd = {k: v.detach().numpy() for k, v in cli_model("fp32").state_dict().items()}
    with torch.no_grad():
        ref = R.masked_mse_loss(R.forward(sd, imgs.cpu().numpy(), boxes.cpu().numpy(), 1), gt.cpu(), torch.ones(384, 384)).item()
    print("first-step loss %.8f, oracle %.8f" % (loss, ref))
    assert abs(loss - ref) <= LOSS_TOL * abs(ref)
