"""CPU: the host statement of the evaluation report (countr_amd/report.py: compose_host, exemplar_strip_host), the 3 x 3 grid's point
sampling against F.interpolate, ReportWriter on CPU tensors and inference.count_image(..., return_crops=True)."""
import json

import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image

from countr_amd import inference, report


def f32(v):
    return np.float32(v)


def quant(x):
    """save_image's byte of one fp32 value: x * 255 + 0.5, clamped, truncated -- every step rounded to fp32."""
    return int(np.clip(f32(f32(f32(x) * f32(255)) + f32(0.5)), 0, 255))


def test_hand_worked_6x8_three_panels():
    h, w = 6, 8
    sam = torch.zeros(3, h, w)
    pred = torch.zeros(h, w)
    gt = torch.zeros(h, w)
    t = float(f32(0.01))                                        # -t is the fp32 value the script's `< -0.01` compares with
    pred[0, 0] = float(np.nextafter(f32(0.01), f32(1)))         # gt - pred just below -0.01: a false positive
    pred[0, 1] = t                                              # gt - pred == -0.01: not below, stays a true positive
    pred[0, 2], gt[0, 2] = 0.5, 0.6                             # channel 0 (against gt) kept, channel 1 (against 0) masked
    pred[0, 3], gt[0, 3] = 2.0, 3.0                             # beyond 1 on both sides
    k = f32(100) / f32(255)
    sam[:, 5, 0] = float(np.nextafter(k, f32(0)))               # k / 255 - eps and + eps: both byte k (round to nearest, not truncation)
    sam[:, 5, 1] = float(np.nextafter(k, f32(1)))
    sam[:, 5, 2] = float(f32(100.5) / f32(255))                 # the boundary between two bytes, whichever side fp32 puts it
    sam[0, 3, 0], sam[1, 3, 0], sam[2, 3, 0] = 0.25, 0.5, 1.0
    labels = np.zeros((h, w, 3), np.uint8)
    labels[2, 0] = (0, 255, 0)                                  # a 255-valued label channel
    labels[2, 1] = (1, 0, 0)                                    # the rasters are added as 0..255, not scaled: 1 saturates the clamp
    pos = [(1, 5, 4, 10)]                                       # crosses the right edge: the x = 10 side and the corners beyond 7 are cut
    out = report.compose_host(sam, pred, gt, pos, gt_cnt=4, pred_cnt=3.2, labels=labels)
    assert out.dtype == np.uint8 and out.shape == (h, 3 * w, 3)
    mix2, sam_box, tp = out[:, :w], out[:, w:2 * w], out[:, 2 * w:]
    # the outline
    outline = {(1, 5), (1, 6), (1, 7), (4, 5), (4, 6), (4, 7), (2, 5), (3, 5)}
    got = {(int(y), int(x)) for y, x in zip(*np.nonzero((sam_box == 255).all(-1)))}
    assert got == outline
    assert report.box_map(h, w, pos)[..., 0].sum() == 255 * len(outline) and report.box_map(h, w, pos, external=True).sum() == 0
    # labels: 255 and 1 both saturate their channel, the others keep the sample's byte
    assert sam_box[2, 0].tolist() == [0, 255, 0] and sam_box[2, 1].tolist() == [255, 0, 0]
    # the quantiser
    assert sam_box[5, 0].tolist() == [100] * 3 and sam_box[5, 1].tolist() == [100] * 3
    assert sam_box[5, 2].tolist() == [quant(f32(100.5) / f32(255))] * 3 and sam_box[5, 2, 0] in (100, 101)
    assert sam_box[3, 0].tolist() == [64, 128, 255]           # 0.25 * 255 + 0.5 = 64.25, 0.5 * 255 + 0.5 = 128.0
    # the threshold, on tp_img (sam = 0 there: the byte is the surviving prediction's)
    assert tp[0, 0].tolist() == [0, 0, 0]
    assert tp[0, 1].tolist() == [quant(t), quant(t), 0] == [3, 3, 0]
    # the channel swap: channel 1 of pred_img is masked (0 - 0.5 < -0.01), channel 0 is not (0.6 - 0.5), and [[1, 0, 2]] swaps them
    assert tp[0, 2].tolist() == [0, 128, 0]
    assert tp[0, 3].tolist() == [0, 255, 0]                     # 2.0 is not clamped before the quantiser; the quantiser's own clamp saturates
    assert tp[3, 0].tolist() == [quant(f32(0.25) * f32(0.6)), quant(f32(0.5) * f32(0.6)), quant(f32(1.0) * f32(0.6))] == [38, 77, 153]
    # mix2 = sam * 0.6 + |clamp01(pred_img) - clamp01(gt_img)|
    assert mix2[0, 2].tolist() == [quant(abs(f32(0.5) - f32(0.6))), 128, 0] == [26, 128, 0]
    assert mix2[0, 3].tolist() == [0, 255, 0]                   # both clamp to 1 in channel 0; channel 1 is clamp01(2) - 0
    assert mix2[0, 0].tolist() == [3, 3, 0] and mix2[0, 1].tolist() == [3, 3, 0]


def test_hand_worked_6x8_two_panels():
    h, w = 6, 8
    sam = torch.full((3, h, w), 0.5)
    pred = torch.zeros(h, w)
    pred[1, 1], pred[1, 2] = 0.2, -1.0
    text = np.zeros((h, w, 3), np.uint8)
    text[4, 6] = (255, 255, 255)
    out = report.compose_host(sam, pred, torch.zeros(h, w), [(0, 0, 2, 2)], gt_cnt=0, pred_cnt=1.5, text=text)
    assert out.shape == (h, 2 * w, 3)
    sam_box, den = out[:, :w], out[:, w:]
    assert sam_box[0, 0].tolist() == [255] * 3 and sam_box[1, 1].tolist() == [128] * 3 and sam_box[2, 1].tolist() == [255] * 3
    base = quant(f32(0.5) * f32(0.6))
    assert den[0, 0].tolist() == [base] * 3 == [77] * 3
    assert den[1, 1].tolist() == [quant(f32(0.5) * f32(0.6) + f32(0.2)), quant(f32(0.5) * f32(0.6) + f32(0.2)), base] == [128, 128, 77]
    assert den[1, 2].tolist() == [0, 0, base]
    assert den[4, 6].tolist() == [255] * 3
    # no exemplar outline with external exemplars
    ext = report.compose_host(sam, pred, torch.zeros(h, w), [(0, 0, 2, 2)], gt_cnt=0, pred_cnt=1.5, external=True, text=text)
    assert (ext[:, :w] == 128).all()


def test_grid_point_sampling_equals_interpolate():
    h, w = 6, 9
    g = torch.Generator().manual_seed(3)
    maps = [torch.randn(h, w, generator=g) for _ in range(9)]
    grid = torch.cat([torch.cat(maps[i:i + 3], -1) for i in (0, 3, 6)], 0)
    want = F.interpolate(grid[None, None], (h, w), mode="bilinear", align_corners=False)[0, 0]
    pts = torch.empty(h, w)
    for y in range(h):
        for x in range(w):
            Y, X = 3 * y + 1, 3 * x + 1
            pts[y, x] = maps[3 * (Y // h) + X // w][Y % h, X % w]
    assert torch.equal(pts, want)
    assert torch.equal(report.grid_sample_points(maps, h, w), want) and torch.equal(report.make_grid_host(maps, h, w), want)
    # and through compose_host: a list of nine maps draws the same picture as their resized grid
    sam = torch.rand(3, h, w, generator=g)
    gt = torch.rand(h, w, generator=g)
    a = report.compose_host(sam, maps, gt, [], 3, 2.0)
    b = report.compose_host(sam, want, gt, [], 3, 2.0)
    assert np.array_equal(a, b)


def test_exemplar_strip_host():
    g = torch.Generator().manual_seed(5)
    for S, shape in ((1, (64, 64, 3)), (3, (68, 200, 3)), (9, (134, 530, 3))):
        ex = torch.rand(S, 3, 64, 64, generator=g) * 1.2 - 0.1
        out = report.exemplar_strip_host(ex)
        assert out.dtype == np.uint8 and out.shape == shape == report.strip_shape(S) + (3,)
        assert np.array_equal(out, report.exemplar_strip_host(ex.unsqueeze(0)))       # the CLI's [1, S, 3, 64, 64]
        covered = np.zeros(shape[:2], bool)
        for k in range(S):
            y0, x0 = (0, 0) if S == 1 else (2 + 66 * (k // 8), 2 + 66 * (k % 8))
            assert np.array_equal(out[y0:y0 + 64, x0:x0 + 64], report.quantize_host(ex[k].clone())), (S, k)
            covered[y0:y0 + 64, x0:x0 + 64] = True
        assert (out[~covered] == 0).all()                       # padding and the empty cells of the last row
    assert report.quantize_host(torch.tensor([[[0.0, 1.0, -0.3, 1.7, 100 / 255]]] * 3))[0, :, 0].tolist() == [0, 255, 0, 255, 100]


def _fake_items(h=150):
    g = torch.Generator().manual_seed(11)
    items, results = [], []
    for name, w, gt_cnt, S in (("a/7.jpg", 176, 12, 3), ("b_9.png", 200, 0, 0)):
        sam = torch.rand(1, 3, h, w, generator=g)
        gt = torch.rand(h, w, generator=g) * (gt_cnt > 0)
        dm = torch.rand(h, w, generator=g) * 1.4 - 0.2
        boxes = torch.rand(1, S, 3, 64, 64, generator=g) if S else torch.zeros(0).unsqueeze(0)
        pos = [(10 * j, 10 * j, 10 * j + 40, 10 * j + 40) for j in range(S)]
        items.append(report.ReportItem(name, sam, boxes, pos, gt_cnt, gt))
        results.append((dm.sum().item() / 60 + 0.5, dm))
    return items, results


def test_report_writer_on_cpu(tmp_path):
    items, results = _fake_items()
    out = tmp_path / "Image"
    wr = report.ReportWriter(out, workers=2)
    paths = wr.add_group(items, results)
    stats = wr.close(timing={"Mean infer time": 0.25})
    names = sorted(p.name for p in out.iterdir())
    want = sorted(["full_7__%d.png" % round(results[0][0]), "full_b_9__%d.png" % round(results[1][0]), "boxes_7.png", "results.csv", "log.txt"])
    try:
        import matplotlib  # noqa: F401
        want = sorted(want + ["test_stat.png"])
    except ImportError:
        pass
    assert names == want and sorted(p.split("/")[-1] for p in paths) == sorted(n for n in want if n.startswith("full_"))
    for it, (pred, dm), path in zip(items, results, paths):
        png = np.asarray(Image.open(path))
        assert png.shape == (150, (3 if it.gt_cnt else 2) * it.sample.shape[-1], 3)
        assert np.array_equal(png, report.compose_host(it.sample, dm, it.gt_map, it.pos, it.gt_cnt, pred))
    assert np.array_equal(np.asarray(Image.open(out / "boxes_7.png")), report.exemplar_strip_host(items[0].boxes))
    # the labels were drawn: the middle panel differs from the same picture without them
    plain = report.compose_host(items[0].sample, results[0][1], items[0].gt_map, items[0].pos, 12, results[0][0], labels=np.zeros((150, 176, 3), np.uint8))
    assert not np.array_equal(plain, np.asarray(Image.open(paths[0])))
    assert (out / "results.csv").read_text() == "time,name,prediction\n1,a/7.jpg,%d\n2,b_9.png,%d\n" % (round(results[0][0]), round(results[1][0]))
    lines = (out / "log.txt").read_text().splitlines()
    assert len(lines) == 1
    log = json.loads(lines[0])
    errs = [abs(results[0][0] - 12), abs(results[1][0] - 0)]
    assert set(log) == {"MAE", "RMSE", "NAE", "Mean infer time"} and log == stats
    assert abs(log["MAE"] - sum(errs) / 2) < 1e-12 and abs(log["RMSE"] - (sum(e * e for e in errs) / 2) ** 0.5) < 1e-12
    assert abs(log["NAE"] - errs[0] / 12 / 2) < 1e-12 and log["Mean infer time"] == 0.25
    # a second run appends to log.txt; ranks > 0 (summary=False) write pictures only
    wr = report.ReportWriter(out, workers=1, summary=False)
    wr.add_group(items[:1], results[:1])
    wr.close()
    assert len((out / "log.txt").read_text().splitlines()) == 1
    other = tmp_path / "rank1"
    wr = report.ReportWriter(other, workers=100, summary=False)
    assert wr.pool._max_workers == 8
    wr.add_group(items[1:], results[1:])
    wr.close()
    assert sorted(p.name for p in other.iterdir()) == ["full_b_9__%d.png" % round(results[1][0])]


class _Stub(torch.nn.Module):
    """A model whose density is the constant 0.5 wherever it looks."""

    def forward(self, imgs, boxes, shot_num):
        return torch.full((imgs.shape[0], imgs.shape[2], 384), 0.5)


def test_count_image_return_crops():
    m = _Stub()
    sam = torch.rand(1, 3, 384, 384, generator=torch.Generator().manual_seed(2))
    boxes = torch.zeros(1, 3, 3, 64, 64)
    small, large = [(5, 5, 9, 9)], [(5, 5, 60, 60)]
    plain = inference.count_image(m, sam, boxes, 3, large, normalization=False)
    assert len(plain) == 2 and plain[1].shape == (384, 384) and abs(plain[0] - 0.5 * 384 * 384 / 60) < 1e-2
    pred, dm, crops = inference.count_image(m, sam, boxes, 3, large, normalization=False, return_crops=True)
    assert crops is None and pred == plain[0] and torch.equal(dm, plain[1])
    plain9 = inference.count_image(m, sam, boxes, 3, small, normalization=False)
    assert len(plain9) == 2
    pred, dm, crops = inference.count_image(m, sam, boxes, 3, small, normalization=False, return_crops=True)
    assert pred == plain9[0] and torch.equal(dm, plain9[1])
    assert len(crops) == 9 and all(c.shape == (384, 384) for c in crops) and crops[-1] is dm
    assert abs(pred - 9 * 0.5 * 384 * 384 / 60) < 1e-1
    both = inference.count_images(m, [(sam, boxes, large), (sam, boxes, small)], normalization=False, return_crops=True)
    assert both[0][2] is None and len(both[1][2]) == 9 and both[0][0] == plain[0] and both[1][0] == plain9[0]
    assert all(len(r) == 2 for r in inference.count_images(m, [(sam, boxes, large), (sam, boxes, small)], normalization=False))
