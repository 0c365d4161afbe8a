"""GPU: csrc_flow/flow.hip against countr_amd.flow_host -- luma and motion byte for byte, the flux within the a-priori bound of an fp32
sum -- FlowCounter's chunking, history and refusals, count_flow end to end on the tiny model, and demo_zero.py --flow.

The bound.  The device and flow_host decide membership and form every term identically (fp64, the same operations; a term is rounded to
fp32 once on both sides), so they sum the SAME fp32 terms v: the device in fp32 in a fixed order, flow_host in float64.  An fp32 sum of n
terms in any order differs from the exact sum by at most (n - 1) u sum|v| / (1 - (n - 1) u) with u = 2^-24, which n u sum|v| covers for
every n here; the float64 sum's own error is far below that; one ulp of the result covers the final rounding of the comparison.  The
total of a map is bounded the same way over all its pixels.  count_flow's flux = scale * flux with scale = count / (total / 60) carries
both bounds exactly as tests/test_regions_gpu.py carries them for region_counts.  Derived, not measured."""
import ctypes as C
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
U = 2.0 ** -24
P1080 = (1080 / 384, 0.5 * 1080 / 384 - 0.5, 1080 / 384, 0.5 * 1080 / 384 - 0.5)      # a 384-high map of a 1080-high frame


def noise(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w)).astype(np.uint8)


def smooth(h, w, seed):
    rs = np.random.RandomState(seed)
    a = rs.uniform(0, 1, (h // 4 + 3, w // 4 + 3))
    a = np.kron(a, np.ones((4, 4)))
    k = np.ones(7) / 7
    for ax in (0, 1):
        a = np.apply_along_axis(lambda v: np.convolve(v, k, "same"), ax, a)
    a = a[4:4 + h, 4:4 + w]
    return np.floor(255 * (a - a.min()) / (a.max() - a.min())).astype(np.uint8)


def rgb_images(h, w, n, seed):
    """Prepared images of random bytes: three different planes, so the luma weights matter."""
    rs = np.random.RandomState(seed)
    return [(rs.randint(0, 256, (1, 3, h, w)).astype(np.uint8).astype(np.float32) / np.float32(255)) for _ in range(n)]


def translated(h, w, n, seed, step):
    """n lumas cut from one smooth texture, the cut moving by `step` = (dx, dy) per frame."""
    dx, dy = step
    big = smooth(h + abs(dy) * n, w + abs(dx) * n, seed)
    y0, x0 = (abs(dy) * n if dy < 0 else 0), (abs(dx) * n if dx < 0 else 0)
    return [np.ascontiguousarray(big[y0 + dy * t:y0 + dy * t + h, x0 + dx * t:x0 + dx * t + w]) for t in range(n)]


def run_both(images, maps, lines, placement=None, size=None, **kw):
    """One FlowCounter.run against flow_host on the same images: luma of the last frame and every motion field equal; every flux and total
    within the bound.  -> (the counter's results, the counter, the worst error / bound)."""
    from countr_amd import flow as F
    h, w = images[0].shape[-2:]
    size = size or (w, h)                                                          # W = w, H = h: the placement is the identity
    fc = F.FlowCounter("cuda", lines=lines, band=kw.pop("band", 8.0), **kw)
    dev_maps = [None if m is None else torch.from_numpy(m).cuda() for m in maps]
    got = fc.run([torch.from_numpy(im).cuda() for im in images], dev_maps, [size] * len(images), motion=True)
    lumas = [F.luma_host(im) for im in images]
    assert np.array_equal(fc.luma().cpu().numpy(), lumas[-1])
    if len(images) > fc.interval:
        assert np.array_equal(fc.luma(fc.interval).cpu().numpy(), lumas[-1 - fc.interval])
    assert fc.shape == (size[0], size[1], h, w)
    want, counts = F.flow_host(lumas, maps, lines=lines, placement=fc.placement, search=fc.search, interval=fc.interval, min_gain=fc.min_gain,
                               band=fc.band)
    worst = 0.0
    acc = np.zeros((len(fc.lines), 2))
    for t, ((flux, mv, total), (wflux, wmv, wtotal)) in enumerate(zip(got, want)):
        assert (mv is None) == (wmv is None) == (t < fc.interval), t
        if mv is not None:
            assert mv.dtype == np.int16 and np.array_equal(mv, wmv), (t, np.argwhere(mv != wmv)[:5])
        assert (flux is None) == (wflux is None), t
        if flux is None:
            continue
        assert flux.dtype == np.float32 and flux.shape == wflux.shape
        _f, _t, n, ab, tabs = F.flux_host(maps[t], wmv, fc.placement, lines, fc.band, fc.interval, members=True)
        bound = n * U * ab + np.spacing(np.abs(wflux).astype(np.float32))
        err = np.abs(flux.astype(np.float64) - wflux)
        assert (err <= bound).all(), (t, err, bound)
        assert ((n > 0) | (flux == 0)).all()                                       # no term: exactly zero
        assert abs(total - wtotal) <= maps[t].size * U * tabs + np.spacing(np.float32(abs(wtotal)))
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        acc += flux.astype(np.float64)
    done = fc.counts()
    assert done.frames == len(images) == counts.frames and done.counted == counts.counted
    assert np.array_equal(done.line_counts, acc)                                   # scale 1: the float64 sum of the frames' fp32 results
    return got, fc, worst


LINES = [(20.3, -3.0, 20.3, 500.0), (8.0, -3.0, 8.0, 500.0), (-5.0, 10.0, 300.0, 90.0), (100.0, 50.0, 100.0, 50.0), (150.0, 380.0, 2.0, 5.0)]


@pytest.mark.parametrize("h,w,search,interval,kind", [
    (384, 16, 4, 1, "rgb"),              # two cells a row: every window clamps
    (384, 16, 16, 1, "noise"),           # ... and the search area is three times the image's width
    (384, 176, 1, 1, "rgb"),             # nine candidates: most lanes of the minimum hold none
    (384, 176, 4, 3, "moving"),          # the forward's map of a 176-wide image, the history three frames deep
    (64, 176, 16, 1, "fast"),            # 1089 candidates: 18 rounds of a wave
    (32, 48, 4, 1, "flat"),
    (40, 72, 4, 2, "moving"),            # cells a row not a multiple of the four waves of a block
])
def test_luma_and_motion_equal_the_host_rule(h, w, search, interval, kind):
    from countr_amd import flow as F
    n = interval + 2
    if kind == "rgb":
        images = rgb_images(h, w, n, h + w)
    elif kind == "noise":
        images = [F.image_of_luma(noise(h, w, 3 + t)) for t in range(n)]
    elif kind == "flat":
        images = [F.image_of_luma(np.full((h, w), v, np.uint8)) for v in (90, 90, 97)]
    else:
        step = (11, -9) if kind == "fast" else (1, 1)
        images = [F.image_of_luma(l) for l in translated(h, w, n, 5, step)]
    maps = [np.random.RandomState(t).uniform(-0.5, 1.0, (h, w)).astype(np.float32) for t in range(n)]
    got, fc, worst = run_both(images, maps, LINES, search=search, interval=interval, min_gain=0 if kind in ("rgb", "noise") else 256)
    print("%s %dx%d search %d interval %d: worst flux error / bound %.3f" % (kind, h, w, search, interval, worst))
    mv = got[-1][1]
    if kind == "flat":
        assert not mv.any()
    elif kind in ("moving", "fast"):
        # cut moving by +step: the content moves by -step, the backward offset is +step
        inner = mv[2:-2, 2:-2].astype(np.int64)
        want = 16 * np.array(step) * interval
        assert (np.abs(inner - want) <= 8).all() and np.abs(got[-1][0]).sum() > 0


def test_blob_scene_flux_equals_the_host_rule_and_two_runs_give_the_same_bytes():
    from countr_amd import flow as F
    lumas, maps, lines, truth = F.blob_scene(h=96, w=192, objects=5, frames=20, speed=(1.0, 3.0), seed=0)
    images = [F.image_of_luma(l) for l in lumas]                                   # 20 frames: a chunk of 16 and one of 4
    got, fc, worst = run_both(images, maps, lines, search=4, interval=1)
    print("blob scene: worst flux error / bound %.3f, counts %s" % (worst, np.round(fc.counts().line_counts, 4).tolist()))
    assert fc.counts().line_counts.sum() > 0.5                                     # objects are inside the bands during these frames
    again, fc2, _w = run_both(images, maps, lines, search=4, interval=1)
    for (f1, m1, t1), (f2, m2, t2) in zip(got, again):
        assert (f1 is None and f2 is None) or (f1.tobytes() == f2.tobytes() and t1 == t2)
        assert (m1 is None and m2 is None) or m1.tobytes() == m2.tobytes()
    assert np.array_equal(fc.counts().line_counts, fc2.counts().line_counts)


@pytest.mark.parametrize("n", [16, 17])
def test_sixteen_frames_in_one_call_and_seventeen_chunked(n):
    from countr_amd import flow as F
    images = [F.image_of_luma(l) for l in translated(48, 64, n, 2, (1, 2))]
    maps = [np.random.RandomState(t).uniform(0, 1.0, (48, 64)).astype(np.float32) for t in range(n)]
    maps[5] = None                                                                 # a frame without a frame map: no flux, its luma stays in the history
    got, fc, _worst = run_both(images, maps, LINES[:3], search=4, interval=2)
    assert [g[0] is None for g in got] == [t < 2 or t == 5 for t in range(n)] and got[5][1] is not None
    # the same frames one at a time: the history crosses the calls
    one = F.FlowCounter("cuda", lines=LINES[:3], search=4, interval=2, band=8.0)
    for t in range(n):
        (flux, mv, total), = one.run([torch.from_numpy(images[t]).cuda()], [None if maps[t] is None else torch.from_numpy(maps[t]).cuda()],
                                     [(64, 48)], motion=True)
        assert (mv is None and got[t][1] is None) or np.array_equal(mv, got[t][1])
        assert (flux is None and got[t][0] is None) or (flux.tobytes() == got[t][0].tobytes() and total == got[t][2])
    assert np.array_equal(one.counts().line_counts, fc.counts().line_counts) and one.counts()[1:] == fc.counts()[1:]


def test_flux_kernel_on_arbitrary_motion_fields_through_the_c_abi():
    """countr_flow_flux alone: sixteen maps with random motion fields (every offset the motion kernel can produce), sixteen lines -- long,
    short, tilted, reversed, zero-length, outside the frame -- a 1080p placement, interval 3."""
    from countr_amd import _lib, flow as F
    L = _lib.flow_lib()
    h, w, n, interval, band = 384, 176, 16, 3, 22.5
    rs = np.random.RandomState(4)
    lines = np.concatenate([rs.uniform(-100, 1200, (12, 4)), [[250.0, -10.0, 250.0, 1090.0], [250.0, 1090.0, 250.0, -10.0], [5.0, 5.0, 5.0, 5.0],
                                                               [-500.0, -500.0, -400.0, -900.0]]]).astype(np.float32)
    maps = [rs.uniform(-0.5, 1.0, (h, w)).astype(np.float32) for _ in range(n)]
    V = [rs.randint(-16 * 16 - 8, 16 * 16 + 9, (h // 8, w // 8, 2)).astype(np.int16) for _ in range(n)]
    V[3][:] = 0                                                                    # a frame at rest counts nothing
    dm = [torch.from_numpy(m).cuda() for m in maps]
    dv = [torch.from_numpy(v).cuda() for v in V]
    ws = torch.empty(L.countr_flow_workspace(n, h), dtype=torch.uint8, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lines64 = F._lines(lines)
    outs = []
    for _rep in range(2):
        out = torch.full((n, F.OUT_FLOATS), float("nan"), device="cuda")
        recs = (_lib.FlowMap * n)()
        for k in range(n):
            recs[k].map, recs[k].motion, recs[k].out = dm[k].data_ptr(), dv[k].data_ptr(), out[k].data_ptr()
            recs[k].sx, recs[k].tx, recs[k].sy, recs[k].ty = P1080
        _lib.flow_check(L.countr_flow_flux(recs, n, h, w, lines64.ctypes.data_as(C.c_void_p), len(lines), band, interval, ws.data_ptr(), st))
        outs.append(out.cpu().numpy())
    assert outs[0].tobytes() == outs[1].tobytes()
    worst, terms = 0.0, 0
    for k in range(n):
        wflux, wtotal, cnt, ab, tabs = F.flux_host(maps[k], V[k], P1080, lines, band, interval, members=True)
        flux, total = outs[0][k, :32].reshape(16, 2), outs[0][k, 32]
        bound = cnt * U * ab + np.spacing(np.abs(wflux).astype(np.float32))
        err = np.abs(flux.astype(np.float64) - wflux)
        assert (err <= bound).all(), (k, err, bound)
        assert ((cnt > 0) | (flux == 0)).all() and not flux[14].any()              # the zero-length line
        assert abs(total - wtotal) <= h * w * U * tabs + np.spacing(np.float32(abs(wtotal)))
        worst, terms = max(worst, float((err / np.maximum(bound, 1e-300)).max())), terms + int(cnt.sum())
    assert not outs[0][3, :32].any() and terms > 50000
    print("flux through the C ABI: %d terms, worst error / bound %.3f" % (terms, worst))


def test_refusals():
    from countr_amd import _lib, flow as F
    fc = F.FlowCounter("cuda", lines=[(5.0, 0.0, 5.0, 30.0)])
    im = lambda h, w: torch.zeros(1, 3, h, w, device="cuda")
    fc.run([im(32, 48)], [torch.zeros(32, 48, device="cuda")], [(96, 64)])
    assert fc.band == 8.0 * 64 / 384 and fc.shape == (96, 64, 32, 48)
    with pytest.raises(ValueError, match="one frame shape"):
        fc.run([im(32, 56)], [None], [(96, 64)])
    with pytest.raises(ValueError, match="one frame shape"):
        fc.run([im(32, 48)], [None], [(96, 60)])
    with pytest.raises(ValueError, match="one map"):
        fc.run([im(32, 48)], [], [(96, 64)])
    with pytest.raises(ValueError, match="a map is a"):
        fc.run([im(32, 48)], [torch.zeros(32, 40, device="cuda")], [(96, 64)])
    with pytest.raises(ValueError, match="contiguous fp32"):
        fc.run([im(32, 48).half()], [None], [(96, 64)])
    assert fc.counts().frames == 1                                                 # a refused run leaves the counter as it was
    with pytest.raises(ValueError, match="multiples of 8"):
        F.FlowCounter("cuda", lines=[]).run([im(36, 48)], [None], [(48, 36)])
    with pytest.raises(_lib.CountrError, match="needs a GPU device"):
        F.FlowCounter("cpu", lines=[])
    for bad in (dict(search=0), dict(search=17), dict(interval=9), dict(min_gain=-1), dict(band=-1.0)):
        with pytest.raises(ValueError):
            F.FlowCounter("cuda", lines=[], **bad)
    # a refused library call raises with the library's text
    L = _lib.flow_lib()
    ptr = (C.c_void_p * 1)(im(8, 8).data_ptr())
    with pytest.raises(_lib.CountrError, match="1..16 frames a call, got 0"):
        _lib.flow_check(L.countr_flow_luma(ptr, ptr, 0, 8, 8, None), "countr_flow_luma")
    with pytest.raises(_lib.CountrError, match="search is 1..16, got 17"):
        _lib.flow_check(L.countr_flow_motion(ptr, ptr, ptr, 1, 8, 8, 17, 0, None), "countr_flow_motion")


# ---- count_flow on the tiny configuration, fp32
@pytest.fixture(scope="module")
def model():
    import torch.nn as nn
    from countr_amd.models_mae_cross import SupervisedMAE
    p, D, depth, H, Dd, ddepth, Hd = W.CONFIGS["tiny_test"]
    m = SupervisedMAE(patch_size=p, embed_dim=D, depth=depth, num_heads=H, decoder_embed_dim=Dd, decoder_depth=ddepth, decoder_num_heads=Hd,
                      mlp_ratio=4, norm_layer=partial(nn.LayerNorm, eps=1e-6), precision="fp32")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.make_state_dict("tiny_test", seed=3).items()}, strict=True)
    return m.to("cuda").eval()


FLOW_LINES = [(72.0, -1.0, 72.0, 97.0), (-1.0, 48.0, 145.0, 48.0), (10.0, 90.0, 130.0, 5.0)]
FLOW = dict(search=8, interval=2, min_gain=256)


def rgb_clip(n, H=96, Wd=144, seed=1):
    """Frames cut from one smooth texture, the cut moving by 1 px of the frame (4 px of the map) per frame."""
    planes = [translated(H, Wd, n, seed + c, (1, 0)) for c in range(3)]
    return [np.ascontiguousarray(np.stack([planes[c][t] for c in range(3)], -1)) for t in range(n)]


def nv12_clip(n, H=96, Wd=144, seed=2):
    from countr_amd import YuvFrame
    ys = translated(H, Wd, n, seed, (1, 0))
    rs = np.random.RandomState(seed)
    return [YuvFrame(y, rs.randint(100, 156, (H // 2, Wd)).astype(np.uint8), format="nv12") for y in ys]


def check_flow(model, frames, boxes, group):
    """count_flow over the clip in groups of `group`: count and map are count_frames' over the same groups bit for bit; motion equals
    flow_host's on the prepared images; every flux is within the bound of flow_host on the call's own maps, carried through scale."""
    from countr_amd import FlowCounts, count_flow, count_frames, flow as F, frames as FR
    got, clip = count_flow(model, frames, boxes, lines=FLOW_LINES, group=group, motion=True, **FLOW)
    assert len(got) == len(frames) and isinstance(clip, FlowCounts) and clip.frames == len(frames)
    ref, images, split = [], [], []
    for g0 in range(0, len(frames), group):
        bx = boxes[g0:g0 + group] if boxes is not None else None
        ref += count_frames(model, frames[g0:g0 + group], bx)
        items = FR.prepare_items("cuda", frames[g0:g0 + group], bx)
        images += [im.cpu().numpy() for im, _ex, _r in items]
        split += [cr is not None for _c, _dm, cr in FR.count_items_crops(model, items)]
    H, Wd = int(frames[0].shape[0]), int(frames[0].shape[1])
    h, w = images[0].shape[-2:]
    assert (h, w) == (384, 576)
    pl = FR.map_placement(Wd, H, w)
    lumas = [F.luma_host(im) for im in images]
    maps = [None if s else a[1].float().cpu().numpy() for a, s in zip(got, split)]
    want, _counts = F.flow_host(lumas, maps, lines=FLOW_LINES, placement=pl, band=F.default_band(H), **FLOW)
    acc, slack, worst = np.zeros((3, 2)), np.zeros((3, 2)), 0.0
    for t, (a, b, (_wf, wmv, _wt)) in enumerate(zip(got, ref, want)):
        assert len(a) == 4 and a[0] == b[0] and torch.equal(a[1], b[1])            # count_frames' bit for bit
        assert a[3].dtype == np.int16 and a[3].shape == (48, 72, 2)
        assert np.array_equal(a[3], wmv if wmv is not None else np.zeros((48, 72, 2), np.int16)), t
        if t < FLOW["interval"] or split[t]:
            assert a[2] is None
            continue
        wflux, wtotal, n, ab, tabs = F.flux_host(maps[t], wmv, pl, FLOW_LINES, F.default_band(H), FLOW["interval"], members=True)
        scale = a[0] / (wtotal / 60) if wtotal > 0 else 1.0
        wantf = scale * wflux
        rel_t = h * w * U * tabs / abs(wtotal) if wtotal else 0.0
        bound = abs(scale) * (n * U * ab + np.spacing(np.abs(wflux).astype(np.float32))) + np.abs(wantf) * 2 * rel_t + np.spacing(np.abs(wantf).astype(np.float32))
        err = np.abs(a[2].astype(np.float64) - wantf)
        assert a[2].dtype == np.float32 and a[2].shape == (3, 2) and (err <= bound).all(), (t, err, bound)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        acc += a[2].astype(np.float64)
        slack += np.spacing(np.abs(a[2]))
    counted = sum(1 for t in range(len(frames)) if t >= FLOW["interval"] and not split[t])
    assert clip.counted == counted and clip.line_counts.shape == (3, 2)
    # line_counts is the float64 sum of scale * flux before each frame's rounding to fp32
    assert (np.abs(clip.line_counts - acc) <= slack).all()
    print("group %d: %d frames counted, worst flux error / bound %.3f, line counts %s" % (group, counted, worst, np.round(clip.line_counts, 5).tolist()))
    return got, clip, split


def test_count_flow_on_host_rgb_frames(model):
    from countr_amd import FlowCounter, count_flow
    frames = rgb_clip(7)
    big = [(5, 5, 40, 40), (60, 10, 100, 50), (30, 50, 70, 90)]
    tiny = [(10, 10, 11, 11), (40, 20, 41, 21), (70, 40, 71, 41)]                  # under 10 px in the resized image: the 3 x 3 split
    boxes = [big, big, big, tiny, big, big, big]
    a, clip_a, split = check_flow(model, frames, boxes, 3)
    b, clip_b, _s = check_flow(model, frames, boxes, 8)
    assert split == [False, False, False, True, False, False, False]
    assert a[3][2] is None and a[3][3].any() and a[4][2] is not None              # the split frame: no flux, but motion, and its luma serves frame 5
    for x, y in zip(a, b):
        assert np.array_equal(x[3], y[3])                                          # the history crosses the group boundaries
    moving = np.stack([x[3] for x in a[2:]])[:, 2:-2, 2:-2].astype(np.int64)
    assert (np.abs(moving - (16 * 8, 0)) <= 8).all()                               # 1 px of the frame a frame = 4 map px, two frames back
    assert np.abs(clip_a.line_counts).sum() > 0
    zero, _c, _s = check_flow(model, frames, None, 8)
    assert all(r[2] is not None for r in zero[2:])
    # counter=: the live-stream case -- two calls continue one counter and equal one call
    fc = FlowCounter("cuda", lines=FLOW_LINES, **FLOW)
    p, _c = count_flow(model, frames[:3], boxes[:3], lines=None, group=3, counter=fc, motion=True)
    q, clip2 = count_flow(model, frames[3:], boxes[3:], lines=None, group=3, counter=fc, motion=True)
    for x, y in zip(p + q, a):
        assert np.array_equal(x[3], y[3]) and ((x[2] is None and y[2] is None) or x[2].tobytes() == y[2].tobytes())
    assert np.array_equal(clip2.line_counts, clip_a.line_counts) and clip2[1:] == clip_a[1:]
    with pytest.raises(ValueError, match="the lines are its own"):
        count_flow(model, frames[:1], lines=[], counter=fc)
    empty, none = count_flow(model, [], lines=FLOW_LINES)
    assert empty == [] and none.frames == 0 and none.counted == 0 and none.line_counts.shape == (3, 2) and not none.line_counts.any()
    plain, _c = count_flow(model, frames[:3], boxes[:3], lines=FLOW_LINES, **FLOW)
    assert all(len(r) == 3 for r in plain)


def test_count_flow_on_yuv_frames(model):
    frames = nv12_clip(5)
    a, _ca, _s = check_flow(model, frames, None, 3)
    b, _cb, _s = check_flow(model, frames, None, 8)
    for x, y in zip(a, b):
        assert np.array_equal(x[3], y[3])
    assert any(x[3].any() for x in a)


def test_count_flow_with_shared_exemplars_equals_count_items_on_the_shared_crop_items(model):
    """count_flow's (k, boxes): count_clip's form of it (tests/test_tracks_gpu.py), which runs the same walk over the clip."""
    from countr_amd import count_flow, frames as FR
    clip = nv12_clip(3, seed=9)
    bx = [(10, 10, 11, 11), (40, 20, 41, 21), (70, 40, 71, 41)]            # under 10 px: with rectangles these would take the 3 x 3 split
    got, _c = count_flow(model, clip, (1, bx), lines=FLOW_LINES, group=2, **FLOW)
    crops = FR.cut_exemplars("cuda", clip[1], bx)
    items = FR.shared_exemplar_items("cuda", clip, crops)
    ref = FR.count_items(model, items[:2]) + FR.count_items(model, items[2:])
    assert len(got) == 3
    for a, (c, dm) in zip(got, ref):
        assert a[0] == c and torch.equal(a[1], dm)
    with pytest.raises(ValueError, match=r"count_flow: \(k, boxes\) names a frame of the call"):
        count_flow(model, clip, (3, bx), lines=FLOW_LINES, **FLOW)


# ---- the demo in a fresh child process
def test_demo_zero_flow_on_a_raw_clip(tmp_path):
    Wd, H = 80, 96
    ys = translated(H, Wd, 4, 3, (1, 0))
    raw = b"".join(y.tobytes() + np.full(Wd * H // 2, 128, np.uint8).tobytes() for y in ys)
    clip = tmp_path / "clip.yuv"
    clip.write_bytes(raw)
    lines = tmp_path / "lines.json"
    lines.write_text(json.dumps({"gate": [[40, -1], [40, 97]], "mid": [[-1, 48], [81, 48]]}))
    out = tmp_path / "out"
    cmd = [sys.executable, "demo_zero.py", "--yuv", "nv12:80x96", "--model_path", "", "--output_path", str(out), "--input_path", str(clip),
           "--no_viz", "--group_images", "3", "--flow", "--lines_json", str(lines), "--flow_search", "6"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    rows = re.findall(r"^clip#(\d+): Count: (\S+) - Time: \S+ - flux: (.*)$", r.stdout, re.M)
    assert [int(k) for k, _c, _x in rows] == [0, 1, 2, 3], r.stdout
    shares = [json.loads(x) for _k, _c, x in rows]
    assert shares[0] is None and all(list(s) == ["gate", "mid"] for s in shares[1:])
    doc = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{"clip"')][-1])
    assert doc == json.load(open(out / "flow_clip.json")) and list(doc["clip"]) == ["flux"] and list(doc["clip"]["flux"]) == ["gate", "mid"]
    for name in ("gate", "mid"):
        for d in (0, 1):
            parts = [s[name][d] for s in shares[1:]]
            assert abs(doc["clip"]["flux"][name][d] - sum(parts)) <= 3 * float(np.spacing(np.float32(max(np.abs(parts)))))
    # --flow needs --yuv and --lines_json, and excludes --track
    r = subprocess.run(cmd[:-5] + ["--flow"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--flow is for --yuv, needs --lines_json" in r.stderr
    r = subprocess.run(cmd + ["--track", "--track_dist", "5"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--flow excludes --track" in r.stderr
