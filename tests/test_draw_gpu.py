"""GPU: Painter.paint (csrc_draw/draw.hip) against draw_host byte for byte -- the rule is integers only, so there is no tolerance -- over
the shapes at which the kernels take another path and the marks that meet the frame's edges; the 4:2:0 kernel it shares with the
overlay; then annotate_clip on the tiny model against count_clip + overlay_host + clip_marks + draw_host, and the demo's --track with
--out_yuv."""
import functools
import json
import os
import re
import subprocess
import sys
from functools import partial

import numpy as np
import pytest
import torch

from oracle import weights as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAR = 1 << 20
SHAPES = [(5, 7), (37, 53), (64, 80)]          # tiny; odd, unaligned, element-wise 4:2:0; the 16-byte path


def mark_sets(H, Wd):
    from countr_amd.draw import Marks
    rs = np.random.RandomState(H * 131 + Wd)
    col = lambda: rs.randint(0, 256, 3)
    heavy = Marks()
    for _ in range(10):
        heavy.segment(rs.randint(-6, Wd + 6, 2), rs.randint(-6, Wd + 6, 2), rs.randint(0, 9), col())
        heavy.disc(rs.randint(-6, Wd + 6, 2), rs.randint(0, 17), col())
        heavy.text(rs.randint(-12, Wd), rs.randint(-8, H), bytes(rs.randint(20, 140, rs.randint(1, 7)).astype(np.uint8)), rs.randint(1, 4), col(),
                   col() if rs.rand() < 0.5 else None)
    return {
        "none": Marks(),
        "segments": Marks().segments(rs.randint(0, Wd, (6, 2)), rs.randint(0, Wd, (6, 2)), 1, rs.randint(0, 256, (6, 3))),
        "discs": Marks().discs(rs.randint(0, Wd, (6, 2)), 3, rs.randint(0, 256, (6, 3))),
        "texts": Marks().text(1, 1, "Id 42", 1, col(), col()).text(0, H // 2, "7/9", 2, col()),
        "heavy": heavy,
        "corner": Marks().segment((-3, -2), (4, 3), 8, col()).disc((Wd - 1, H - 1), 16, col()).disc((0, H - 1), 16, col()),
        "cut_text": Marks().text(Wd - 20, H - 30, "Wg", 8, col(), col()).text(Wd - 3, 0, "|", 8, col()),
        "zero_length": Marks().segment((2, 2), (2, 2), 0, col()).segment((Wd - 2, H - 2), (Wd - 2, H - 2), 3, col()).segment((-1, -1), (-1, -1), 1, col()),
        "diagonal": Marks().segment((-FAR, -FAR), (FAR, FAR), 2, col()).segment((FAR, -FAR + H), (-FAR, FAR), 0, col())
                           .segment((-FAR, H // 2), (FAR, H // 2 + 1), 1, col()).segment((Wd // 2, FAR), (Wd // 2, -FAR), 0, col()),
        "outside": Marks().segment((-40, -9), (-9, 200), 8, col()).disc((Wd + 16, H + 16), 16, col()).text(Wd, 0, "out", 8, col(), col())
                          .text(-FAR, -FAR, "out", 8, col(), col()).segment((FAR, FAR), (FAR, -FAR), 8, col()).text(0, -64, "above", 8, col(), col()),
    }


@functools.lru_cache(maxsize=None)
def case(H, Wd, name):
    """(the frame, its marks, draw_host's RGB): computed once, shared, left unchanged."""
    from countr_amd.draw import draw_host
    frame = np.random.RandomState(H + Wd).randint(0, 256, (H, Wd, 3)).astype(np.uint8)
    marks = mark_sets(H, Wd)[name]
    want = draw_host(frame, marks)
    frame.setflags(write=False)
    want.setflags(write=False)
    return frame, marks, want


@pytest.fixture(scope="module")
def painter():
    from countr_amd.draw import Painter
    return Painter("cuda")


def owners_clean(p):
    return all(int(t.count_nonzero()) == 0 for t in p.owners())


@pytest.mark.parametrize("H,Wd", SHAPES)
def test_paint_equals_draw_host_on_every_mark_set(painter, H, Wd):
    names = list(mark_sets(H, Wd))
    cases = [case(H, Wd, n) for n in names]
    dev = [torch.from_numpy(f.copy()).cuda() for f, _m, _w in cases]
    got = painter.paint(dev, [m for _f, m, _w in cases])
    assert all(g is d for g, d in zip(got, dev))                    # in place
    for name, g, (f, _m, want) in zip(names, got, cases):
        assert np.array_equal(g.cpu().numpy(), want), name
        changed = (want != f).any()
        assert changed == (name not in ("none", "outside")), name
    assert owners_clean(painter)
    # the 4:2:0 buffer comes from the painted frame
    from countr_amd.overlay import rgb_to_yuv_host
    dev = [torch.from_numpy(f.copy()).cuda() for f, _m, _w in cases]
    for g, (_f, _m, want) in zip(painter.paint(dev, [m for _f, m, _w in cases], out="nv12"), cases):
        assert np.array_equal(g.cpu().numpy(), rgb_to_yuv_host(want, "nv12", "bt709", "limited"))
    assert owners_clean(painter)


@pytest.mark.parametrize("out", ["nv12", "nv21", "i420"])
def test_every_format_matrix_and_range(painter, out):
    from countr_amd.draw import draw_host
    from countr_amd.overlay import frame_bytes
    frame, marks, want = case(37, 53, "heavy")
    for mx in ("bt601", "bt709"):
        for rg in ("limited", "full"):
            dev = torch.from_numpy(frame.copy()).cuda()
            got, = painter.paint([dev], [marks], out=out, matrix=mx, range=rg)
            assert got.shape == (frame_bytes(out, 53, 37),) and np.array_equal(got.cpu().numpy(), draw_host(frame, marks, out, mx, rg)), (mx, rg)
            assert np.array_equal(dev.cpu().numpy(), want)


def test_sixteen_frames_in_one_call_seventeen_chunked_and_two_runs(painter):
    names = list(mark_sets(37, 53))
    cases = [case(37, 53, names[k % len(names)]) for k in range(17)]
    runs = []
    for n in (16, 17, 17):
        dev = [torch.from_numpy(f.copy()).cuda() for f, _m, _w in cases[:n]]
        got = painter.paint(dev, [m for _f, m, _w in cases[:n]], out="i420", matrix="bt601", range="full")
        runs.append((torch.stack(dev).cpu().numpy(), torch.stack(got).cpu().numpy()))
        assert np.array_equal(runs[-1][0], np.stack([w for _f, _m, w in cases[:n]]))
        assert owners_clean(painter)
    assert np.array_equal(runs[1][0], runs[2][0]) and np.array_equal(runs[1][1], runs[2][1])      # two runs, the same bytes
    assert np.array_equal(runs[0][1], runs[1][1][:16])


def test_second_calls_leave_frame_and_buffers_as_they_were():
    from countr_amd.draw import Painter
    p = Painter("cuda")
    frame, marks, want = case(64, 80, "heavy")
    dev = torch.from_numpy(frame.copy()).cuda()
    p.paint([dev], [marks], out="nv12")
    held = p.buffers()
    assert len(held) == 4 and owners_clean(p)                       # the pack and its pinned twin, one owner plane, one 4:2:0 buffer
    p.paint([dev], [None])                                          # no marks: nothing is launched for them, the frame stays
    assert np.array_equal(dev.cpu().numpy(), want)
    dev.copy_(torch.from_numpy(frame.copy()))
    again, = p.paint([dev], [marks], out="nv12")
    assert p.buffers() == held and np.array_equal(dev.cpu().numpy(), want) and owners_clean(p)
    with pytest.raises(ValueError, match="contiguous uint8"):
        p.paint([dev[:, ::2]], [None])
    with pytest.raises(ValueError, match="one Marks"):
        p.paint([dev], [])


@pytest.mark.parametrize("H,Wd", SHAPES)
def test_unmarked_four_two_zero_is_the_overlay_s(painter, H, Wd):
    """The conversion kernel moved to a header both libraries include: an unmarked frame converts as Overlay.render converts it."""
    from countr_amd.overlay import Overlay
    frame = case(H, Wd, "none")[0]
    ov = Overlay("cuda")
    for out, mx, rg in (("nv12", "bt709", "limited"), ("nv21", "bt601", "full"), ("i420", "bt709", "full")):
        dev = torch.from_numpy(frame.copy()).cuda()
        a, = ov.render([dev], [None], out=out, matrix=mx, range=rg)
        b, = painter.paint([dev], [None], out=out, matrix=mx, range=rg)
        assert torch.equal(a, b), (out, mx, rg)


# ---- annotate_clip on the tiny configuration
@pytest.fixture(scope="module")
def model():
    import torch.nn as nn
    from countr_amd.models_mae_cross import SupervisedMAE
    p, D, depth, H, Dd, ddepth, Hd = W.CONFIGS["tiny_test"]
    m = SupervisedMAE(patch_size=p, embed_dim=D, depth=depth, num_heads=H, decoder_embed_dim=Dd, decoder_depth=ddepth, decoder_num_heads=Hd,
                      mlp_ratio=4, norm_layer=partial(nn.LayerNorm, eps=1e-6), precision="fp32")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.make_state_dict("tiny_test", seed=3).items()}, strict=True)
    return m.to("cuda").eval()


def nv12_frames(n, H=60, Wd=90, seed=7):
    from countr_amd import YuvFrame
    rs = np.random.RandomState(seed)
    return [YuvFrame(rs.randint(0, 256, (H, Wd)).astype(np.uint8), rs.randint(0, 256, ((H + 1) // 2, 2 * ((Wd + 1) // 2))).astype(np.uint8),
                     format="nv12") for _ in range(n)]


@pytest.mark.parametrize("group,camera", [(2, None), (4, None), (2, "translation")])
def test_annotate_clip_equals_count_clip_and_the_host_composition(model, group, camera):
    from countr_amd import annotate_clip, count_clip, overlay_host, yuv_host
    from countr_amd.draw import Trails, clip_marks, draw_host
    frames = nv12_frames(5)
    lines, names = [(45.0, -1.0, 45.0, 61.0)], ["gate"]
    kw = dict(max_dist=25.0, max_missed=1, min_hits=2, lines=lines, group=group, radius=3, rel_threshold=0.05, camera=camera)
    ref, clip = count_clip(model, frames, summaries=True, **kw)
    assert sum(len(r[2]) for r in ref) > 0 and clip.started > 0
    for out in ("rgb", "nv12"):
        trails, k, groups = Trails(3), 0, 0
        for got, so_far in annotate_clip(model, frames, line_names=names, out=out, trail=3, gain=2000.0, **kw):
            groups += 1
            assert len(got) == min(group, len(frames) - k)
            for g in got:
                r = ref[k]
                assert len(g) == (8 if camera else 7)
                assert g[0] == r[0] and torch.equal(g[1], r[1]) and all(np.array_equal(a, b) for a, b in zip(g[2:6], r[2:6]))
                where = r[7] if camera else None
                if camera:
                    assert np.array_equal(g[7], where)
                scene = r[2].astype(np.float64) + (where if camera else 0.0)
                marks = clip_marks(r[2], r[4], r[5], r[6], names, lines, r[0], where, size=(90, 60), trails=trails.update(scene, r[4]))
                base = overlay_host(yuv_host(frames[k]), r[1].float().cpu().numpy(), gain=2000.0)
                want = draw_host(base, marks, out, frames[k].matrix, frames[k].range)
                assert np.array_equal(g[6].cpu().numpy(), want), (out, k)
                assert len(marks.arrays()[1]) == len(r[2]) and (out != "rgb" or (want != base).any())
                k += 1
            assert so_far[:3] == tuple(int(v) for v in (ref[k - 1][6][1], ref[k - 1][6][2], ref[k - 1][6][6]))
        assert k == len(frames) and groups == -(-len(frames) // group) and np.array_equal(so_far.line_counts, clip.line_counts)
    assert list(annotate_clip(model, [], max_dist=3.0)) == []


# ---- the demo in a fresh child process
def test_demo_zero_track_writes_the_annotated_clip(tmp_path):
    from countr_amd.overlay import frame_bytes
    Wd, H, n = 80, 96, 3
    raw = np.random.RandomState(5).randint(0, 256, n * Wd * H * 3 // 2).astype(np.uint8)
    clip = tmp_path / "clip.yuv"
    clip.write_bytes(raw.tobytes())
    lines = tmp_path / "lines.json"
    lines.write_text(json.dumps({"gate": [[40, -1], [40, 97]], "mid": [[-1, 48], [81, 48]]}))
    base = [sys.executable, "demo_zero.py", "--yuv", "nv12:80x96", "--model_path", "", "--input_path", str(clip), "--track", "--track_dist", "30",
            "--lines_json", str(lines), "--track_hits", "2", "--group_images", "2", "--no_viz"]
    rows = []
    for extra in ([], ["--out_yuv", str(tmp_path / "out.yuv")]):
        r = subprocess.run(base + ["--output_path", str(tmp_path / ("out%d" % len(extra)))] + extra, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        rows.append(re.findall(r"^clip#(\d+): Count: (\S+) - Time: \S+ - (tracks: \d+ - crossed: \{.*\})$", r.stdout, re.M)
                    + [ln for ln in r.stdout.splitlines() if ln.startswith('{"clip"')])
    assert len(rows[0]) == n + 1 and rows[0] == rows[1]
    assert (tmp_path / "out.yuv").stat().st_size == n * frame_bytes("nv12", Wd, H)
    written = np.fromfile(tmp_path / "out.yuv", np.uint8)
    assert not np.array_equal(written, raw)
