"""GPU: csrc/report.hip against the host statement of countr_amd/report.py, byte for byte -- countr_report_panels and
countr_report_quantize through the C ABI, ReportWriter's staging reuse, and FSC_test_cross.py --report on synthetic images."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from countr_amd import _lib, report

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 48


def _maps(rs, h, w):
    """gt and pred with values on both sides of 0 and 1, and differences on both sides of the -0.01 threshold (and exactly on it)."""
    gt = rs.uniform(-0.3, 1.3, size=(h, w)).astype(np.float32)
    t = np.float32(0.01)
    near = np.array([t, np.nextafter(t, np.float32(1)), np.nextafter(t, np.float32(0)), 0.0101, 0.0099], np.float32)
    delta = np.where(rs.uniform(size=(h, w)) < 0.5, rs.uniform(-1.2, 1.2, size=(h, w)), near[rs.randint(0, len(near), size=(h, w))]).astype(np.float32)
    pred = (gt + delta).astype(np.float32)
    zero = rs.uniform(size=(h, w)) < 0.2                     # gt = 0: pred itself sits at the threshold of both channels
    gt[zero] = 0
    pred[zero] = delta[zero]
    return torch.from_numpy(gt), torch.from_numpy(pred)


def _patch(rs, ph, pw):
    p = rs.randint(0, 256, size=(ph, pw, 3)).astype(np.uint8)
    p[rs.uniform(size=(ph, pw)) < 0.5] = 0
    p[0, 0] = (1, 0, 255)
    return p


def _canvas(h, w, patch, px, py):
    """The full raster compose_host adds: the patch pasted at (px, py), cut at the image's edges."""
    c = np.zeros((h, w, 3), np.uint8)
    ph, pw = patch.shape[:2]
    y0, x0, y1, x1 = max(py, 0), max(px, 0), min(py + ph, h), min(px + pw, w)
    c[y0:y1, x0:x1] = patch[y0 - py:y1 - py, x0 - px:x1 - px]
    return c


@pytest.fixture(scope="module")
def group():
    """The four images of the C-ABI test, on the host, with the panels compose_host makes of them (computed once)."""
    rs = np.random.RandomState(7)
    imgs = []
    for w, layout, grid, pos, patch in (
            (176, 3, False, [(5, 10, 30, 60), (40, 150, 60, 200), (10, 100, 20, 100)], (_patch(rs, 20, 60), -7, -3)),   # clipped, degenerate
            (176, 2, False, [(2, 3, 20, 30)], (_patch(rs, 12, 40), 150, 30)),                                            # text over the right edge
            (208, 3, True, [(0, 0, 47, 207)], None),                                                                    # nine maps
            (208, 3, False, [], (_patch(rs, 9, 33), 60, 39))):                                                          # external: no rectangle
        sam = torch.from_numpy(rs.uniform(0, 1, size=(3, H, w)).astype(np.float32))
        gt, pred = _maps(rs, H, w)
        maps = [pred] if not grid else [_maps(rs, H, w)[1] for _ in range(9)]
        canvas = _canvas(H, w, *patch) if patch else np.zeros((H, w, 3), np.uint8)
        gt_cnt = 5 if layout == 3 else 0
        want = report.compose_host(sam, maps if grid else pred, gt, pos, gt_cnt, 1.0, external=not pos, labels=canvas, text=canvas)
        assert want.shape == (H, layout * w, 3)
        imgs.append(dict(w=w, layout=layout, grid=grid, pos=pos, patch=patch, sam=sam, gt=gt, maps=maps, want=want))
    return imgs


def _run_panels(hip, imgs, sentinel):
    """countr_report_panels through ctypes: blob = rectangles, then the patches; panels at offsets with gaps between them."""
    nrects = sum(len(g["pos"]) for g in imgs)
    blob = np.zeros(16 * nrects + sum(-(-g["patch"][0].size // 16) * 16 for g in imgs if g["patch"]) + 16, np.uint8)
    rects = blob[:16 * nrects].view(np.int32).reshape(nrects, 4)
    descs = (_lib.ReportImage * len(imgs))()
    keep, off, r0, out_off, spans = [], 16 * nrects, 0, 32, []
    for d, g in zip(descs, imgs):
        dev = [g["sam"].cuda(), g["gt"].cuda()] + [m.cuda() for m in g["maps"]]
        keep.append(dev)
        d.sam, d.gt = dev[0].data_ptr(), dev[1].data_ptr()
        for k in range(9):
            d.maps[k] = dev[2 + k].data_ptr() if k < len(g["maps"]) else None
        d.w, d.layout, d.grid, d.out_off = g["w"], g["layout"], int(g["grid"]), out_off
        d.rect_off, d.rect_cnt = r0, len(g["pos"])
        for r in g["pos"]:
            rects[r0] = r
            r0 += 1
        if g["patch"]:
            p, px, py = g["patch"]
            blob[off:off + p.size] = p.reshape(-1)
            pt = _lib.ReportPatch(off, px, py, p.shape[1], p.shape[0])
            if g["layout"] == 3:
                d.labels = pt
            else:
                d.text = pt
            off += -(-p.size // 16) * 16
        size = H * g["layout"] * g["w"] * 3
        spans.append((out_off, size))
        out_off += size + 64
    out = torch.full((out_off + 100,), sentinel, dtype=torch.uint8, device="cuda")
    blob_dev = torch.from_numpy(blob).cuda()
    rc = hip.countr_report_panels(descs, len(imgs), H, blob_dev.data_ptr(), blob.size, 0, nrects, out.data_ptr(), out.numel(),
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, hip.countr_last_error()
    torch.cuda.synchronize()
    return out.cpu(), spans


def test_panels_equal_compose_host(hip, group):
    for sentinel in (0xA5, 0x5A):        # equal to the host's bytes under two different fills = every byte of a panel was written
        out, spans = _run_panels(hip, group, sentinel)
        inside = torch.zeros(out.numel(), dtype=torch.bool)
        for g, (o, size) in zip(group, spans):
            got = out[o:o + size].view(H, g["layout"] * g["w"], 3)
            want = torch.from_numpy(g["want"])
            diff = (got != want).nonzero()
            assert torch.equal(got, want), ("w %d layout %d grid %s: %d bytes differ, first at %s" %
                                            (g["w"], g["layout"], g["grid"], len(diff), diff[:1].tolist()))
            inside[o:o + size] = True
        assert (out[~inside] == sentinel).all()          # the gaps between the panels, the head and the tail keep the fill


def test_panels_refuse_bad_arguments(hip, group):
    """Every offset is checked on the host before anything is launched."""
    g = group[0]
    dev = [g["sam"].cuda(), g["gt"].cuda(), g["maps"][0].cuda()]
    out = torch.zeros(H * 3 * g["w"] * 3, dtype=torch.uint8, device="cuda")
    blob = torch.zeros(64, dtype=torch.uint8, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(**kw):
        d = (_lib.ReportImage * 1)()
        d[0].sam, d[0].gt, d[0].maps[0] = dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr()
        d[0].w, d[0].layout = g["w"], 3
        for k, v in kw.items():
            setattr(d[0], k, v)
        return hip.countr_report_panels(d, 1, H, blob.data_ptr(), 64, 0, 1, out.data_ptr(), out.numel(), st)

    assert call() == 0
    assert call(out_off=16) != 0                                 # the panel would end behind the buffer
    assert call(rect_cnt=2) != 0                                 # more rectangles than the blob holds
    assert call(labels=_lib.ReportPatch(32, 0, 0, 8, 8)) != 0    # a raster that ends behind the blob
    assert call(layout=4) != 0 and call(grid=1) != 0             # nine maps are needed for the grid
    torch.cuda.synchronize()
    assert (out.cpu() != 0).any()


def test_exemplar_strips_equal_host(hip):
    g = torch.Generator().manual_seed(4)
    sets = [torch.rand(S, 3, 64, 64, generator=g) * 1.4 - 0.2 for S in (3, 9, 1)]
    want = [report.exemplar_strip_host(e) for e in sets]
    shape = (C.c_int * 2)()
    for e, wnt in zip(sets, want):
        assert hip.countr_report_strip_shape(e.shape[0], 64, 64, shape) == 0 and tuple(shape) == wnt.shape[:2]
    dev = [e.cuda() for e in sets]
    strips = (_lib.ReportStrip * 3)()
    off, spans = 16, []
    for s, e, wnt in zip(strips, dev, want):
        s.ex, s.out_off, s.S = e.data_ptr(), off, e.shape[0]
        spans.append((off, wnt.size))
        off += wnt.size + 48
    out = torch.full((off,), 0xA5, dtype=torch.uint8, device="cuda")
    rc = hip.countr_report_quantize(strips, 3, 64, 64, out.data_ptr(), out.numel(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, hip.countr_last_error()
    torch.cuda.synchronize()
    out = out.cpu()
    inside = torch.zeros(out.numel(), dtype=torch.bool)
    for (o, size), wnt in zip(spans, want):
        assert torch.equal(out[o:o + size].view(wnt.shape), torch.from_numpy(wnt))
        inside[o:o + size] = True
    assert (out[~inside] == 0xA5).all()


def _writer_items(seed, h, specs):
    rs = np.random.RandomState(seed)
    items, results = [], []
    for k, (w, gt_cnt, S, grid, gt_on_device) in enumerate(specs):
        sam = torch.from_numpy(rs.uniform(0, 1, size=(1, 3, h, w)).astype(np.float32)).cuda()
        gt, pred = _maps(rs, h, w)
        gt = gt * (gt_cnt > 0)
        crops = [_maps(rs, h, w)[1].cuda() for _ in range(9)] if grid else None
        boxes = torch.from_numpy(rs.uniform(0, 1, size=(1, S, 3, 64, 64)).astype(np.float32)).cuda() if S else torch.zeros(0).unsqueeze(0).cuda()
        pos = [(12 * j, 15 * j, 12 * j + 40, 15 * j + 70) for j in range(S)]
        items.append(report.ReportItem("img%d_%d.jpg" % (seed, k), sam, boxes, pos, gt_cnt, gt.cuda() if gt_on_device else gt))
        results.append((float(pred.sum()) / 60 + 0.25 * k, crops[-1] if grid else pred.cuda(), crops))
    return items, results


def test_writer_reuses_its_staging(tmp_path, hip):
    """Two groups of different widths through one ReportWriter (the second and third reuse the first's buffers; 202 is no multiple of 4:
    the one-pixel path): every PNG decodes to compose_host's bytes of the same inputs, the labels being PIL's own here."""
    h = 160
    wr = report.ReportWriter(tmp_path, workers=3)
    groups = [_writer_items(1, h, [(176, 7, 3, False, False), (208, 0, 2, False, True)]),
              _writer_items(2, h, [(240, 3, 1, True, False), (176, 9, 0, False, True), (202, 4, 3, False, False)]),
              _writer_items(3, h, [(208, 2, 9, False, False)])]
    paths = [wr.add_group(items, results) for items, results in groups]
    assert len({id(s.out_host) for s in wr._stages}) == 2
    bufs = [(s.out_host.data_ptr(), s.blob_host.data_ptr()) for s in wr._stages]
    wr.add_group(*groups[0])                      # the same pictures again: nothing grows
    assert bufs == [(s.out_host.data_ptr(), s.blob_host.data_ptr()) for s in wr._stages]
    wr.close()
    for (items, results), ps in zip(groups, paths):
        for it, (pred, dm, crops), path in zip(items, results, ps):
            want = report.compose_host(it.sample.cpu(), [c.cpu() for c in crops] if crops else dm.cpu(), it.gt_map.cpu(), it.pos, it.gt_cnt, pred)
            got = np.asarray(Image.open(path))
            assert got.shape == want.shape and np.array_equal(got, want), (it.name, int((got != want).sum()))
            bp = tmp_path / ("boxes_%s.png" % it.name.split(".")[0])
            if it.boxes.nelement():
                assert np.array_equal(np.asarray(Image.open(bp)), report.exemplar_strip_host(it.boxes.cpu()))
            else:
                assert not bp.exists()
    assert (tmp_path / "results.csv").read_text().splitlines()[0] == "time,name,prediction"
    assert len((tmp_path / "results.csv").read_text().splitlines()) == 1 + 2 + 3 + 1 + 2


def _cli(args):
    r = subprocess.run([sys.executable, "FSC_test_cross.py", "--resume", "", "--synthetic", "3"] + args, cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    per_image = [l for l in r.stdout.splitlines() if "pred_cnt" in l]
    metrics = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    return per_image, metrics


def test_cli_report(tmp_path):
    """FSC_test_cross.py --synthetic 3: with --report the pictures and the summary files appear and the run counts what it counts without
    the flag; without the flag --output_dir stays empty."""
    out, empty = tmp_path / "with", tmp_path / "without"
    empty.mkdir()
    lines, metrics = _cli(["--report", "--output_dir", str(out)])
    lines0, metrics0 = _cli(["--output_dir", str(empty)])
    assert list(empty.iterdir()) == []
    # the metrics line: every key but the wall-clock one, which no two runs share
    assert set(metrics) == set(metrics0) and all(metrics[k] == metrics0[k] for k in metrics if k != "mean_infer_time_s")
    assert lines == lines0 and len(lines) == 3
    names = sorted(p.name for p in out.iterdir())
    assert len([n for n in names if n.startswith("full_synthetic_")]) == 3 and len([n for n in names if n.startswith("boxes_synthetic_")]) == 3
    assert "results.csv" in names and "log.txt" in names
    rows = (out / "results.csv").read_text().splitlines()
    assert rows[0] == "time,name,prediction" and [r.split(",")[:2] for r in rows[1:]] == [[str(k + 1), "synthetic_%d" % k] for k in range(3)]
    for k, row in enumerate(rows[1:]):
        pred = float(lines[k].split("pred_cnt:")[1].split(",")[0])
        assert abs(int(row.split(",")[2]) - pred) <= 0.5 + 1e-3 and (out / ("full_synthetic_%d__%s.png" % (k, row.split(",")[2]))).exists()
    log = [json.loads(l) for l in (out / "log.txt").read_text().splitlines()]
    assert len(log) == 1 and all(abs(log[0][k] - metrics[k]) < 1e-9 for k in ("MAE", "RMSE", "NAE")) and "Mean infer time" in log[0]
    full = Image.open(out / [n for n in names if n.startswith("full_synthetic_0__")][0])
    assert full.size[1] == 384 and full.size[0] % 3 == 0 and Image.open(out / "boxes_synthetic_0.png").size == (200, 68)


def test_cli_report_zero_shot(tmp_path):
    out = tmp_path / "zs"
    lines, _m = _cli(["--report", "--output_dir", str(out), "--box_bound", "0"])
    names = sorted(p.name for p in out.iterdir())
    assert len(lines) == 3 and len([n for n in names if n.startswith("full_")]) == 3 and not [n for n in names if n.startswith("boxes_")]
