"""GPU: countr_class_fold (csrc_classes/classes.hip) through the C ABI against classes_host -- labels and areas exactly, won and total
within the a-priori bound of an fp32 sum -- ClassFolder's chunking and refusals, the engine's class-dependent tail
(forward_loaded_tail, forward_loaded_from) bit for bit against full forwards, and count_classes end to end on the tiny model.

The bound is tests/test_regions_gpu.py's: an fp32 sum of n terms in ANY order differs from the exact sum by at most
(n - 1) u sum|v| / (1 - (n - 1) u) with u = 2^-24, which n 2^-24 sum|v| covers for every n here; classes_host sums the same float32
products in float64, whose own error is far below that; one ulp of the result covers the final rounding of the comparison.  Derived,
not measured."""
import ctypes as C
import json
import os
import subprocess
import sys
from functools import partial

import numpy as np
import pytest
import torch

from oracle import weights as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZES = [(5, 7), (24, 40), (33, 130)]      # smaller than a strip of 16 rows; one and a half strips, under a wave wide; three strips
U = 2.0 ** -24
FLOOR = 0.125


def make_set(h, w, nc, seed):
    """nc maps from uniform(-0.5, 1.0) with scales that are powers of two, planted exact ties of v (between the first and the last
    class, and among all classes) and a region at or below FLOOR: one pixel's maximum equals it."""
    rs = np.random.RandomState(seed)
    maps = rs.uniform(-0.5, 1.0, (nc, h, w)).astype(np.float32)
    scale = np.asarray([(0.5, 1.0, 2.0)[c % 3] for c in range(nc)], np.float32)
    r = h // 2
    for c in range(nc):
        maps[c, r, : w // 2] = np.float32(0.75) / scale[c]                   # every class ties at 0.75: class 0 owns these pixels
    maps[nc - 1, 0, :3] = np.float32(4.0) / scale[nc - 1]                    # the first and the last class tie above the others
    maps[0, 0, :3] = np.float32(4.0) / scale[0]
    lo = rs.uniform(-0.5, FLOOR, (nc, w - w // 2)).astype(np.float32)
    for c in range(nc):
        maps[c, r, w // 2:] = lo[c] / scale[c]                               # v <= FLOOR (a power of two scales exactly)
    maps[0, r, w - 1] = np.float32(FLOOR) / scale[0]                         # the maximum EQUALS the floor: nobody
    return [m for m in maps], scale


def on_device(maps, offset=0):
    """Contiguous device copies; offset = 1 puts each map one float behind a 16-byte boundary (the kernel's one-pixel path)."""
    out = []
    for m in maps:
        buf = torch.empty(m.size + offset, dtype=torch.float32, device="cuda")
        buf[offset:].copy_(torch.from_numpy(m).reshape(-1))
        out.append(buf[offset:].view(m.shape))
    return out


@pytest.fixture(scope="module")
def folder():
    from countr_amd.classes import ClassFolder
    return ClassFolder("cuda")


def check(folder, sets, floor=FLOOR, offset=0):
    """One ClassFolder.fold against classes_host: labels and areas equal, won and total within the bound.  -> the GPU's results."""
    from countr_amd.classes import classes_host
    got = folder.fold([(on_device(maps, offset), scale) for maps, scale in sets], floor)
    assert len(got) == len(sets)
    for s, ((labels, won, total, area), (maps, scale)) in enumerate(zip(got, sets)):
        wl, ww, wt, wa, wabs, tabs = classes_host(maps, scale, floor, members=True)
        assert labels.dtype == torch.uint8 and labels.is_cuda and tuple(labels.shape) == maps[0].shape
        assert won.dtype == total.dtype == np.float32 and area.dtype == np.int32 and won.shape == total.shape == area.shape == (len(maps),)
        assert np.array_equal(labels.cpu().numpy(), wl), (s, np.argwhere(labels.cpu().numpy() != wl)[:5])
        assert np.array_equal(area, wa), (s, area, wa)
        assert area.sum() + int((wl == 255).sum()) == wl.size
        n = wl.size
        bw = wa * U * wabs + np.spacing(np.abs(ww).astype(np.float32))
        bt = n * U * tabs + np.spacing(np.abs(wt).astype(np.float32))
        ew, et = np.abs(won.astype(np.float64) - ww), np.abs(total.astype(np.float64) - wt)
        print("set %d: %d classes, worst won error / bound %.3f, total %.3f" % (s, len(maps), (ew / np.maximum(bw, 1e-300)).max(), (et / bt).max()))
        assert (ew <= bw).all() and (et <= bt).all(), (s, ew, bw, et, bt)
    return got


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("nc", [1, 2, 16])
@pytest.mark.parametrize("h,w", SIZES)
def test_fold_equals_the_host_rule(folder, h, w, nc, offset):
    maps, scale = make_set(h, w, nc, 1000 * nc + h * w)
    (labels, _won, _total, area), = check(folder, [(maps, scale)], offset=offset)
    lab = labels.cpu().numpy()
    r = h // 2
    assert (lab[r, : w // 2] == 0).all() and (lab[r, w // 2:] == 255).all() and (lab[0, :3] == 0).all()      # the planted ties and floor
    if nc == 1:                                       # one class, floor below the minimum: it wins everything
        (_l, won, total, area), = check(folder, [(maps, scale)], floor=-10.0, offset=offset)
        assert area.tolist() == [h * w] and won.tobytes() == total.tobytes()


def test_one_sixteen_and_seventeen_sets(folder):
    sets = [make_set(*SIZES[k % 3], (1, 2, 16)[(k // 3) % 3], 50 + k) for k in range(17)]
    a = check(folder, sets[:1])
    b = check(folder, sets[:16])
    c = check(folder, sets)                            # seventeen: two pairs of launches
    for x, y in ((a[0], c[0]), (b[15], c[15])):        # a set's results do not depend on its neighbours
        assert torch.equal(x[0], y[0]) and all(x[k].tobytes() == y[k].tobytes() for k in (1, 2, 3))


def test_second_run_and_side_stream_give_the_same_bytes(folder):
    sets = [(on_device(maps), scale) for maps, scale in (make_set(33, 130, 16, 7), make_set(24, 40, 2, 8), make_set(5, 7, 1, 9))]
    a = folder.fold(sets, FLOOR)
    b = folder.fold(sets, FLOOR)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = folder.fold(sets, FLOOR)
    torch.cuda.synchronize()
    for x, y, z in zip(a, b, c):
        assert torch.equal(x[0], y[0]) and torch.equal(x[0], z[0])
        for k in (1, 2, 3):
            assert x[k].tobytes() == y[k].tobytes() == z[k].tobytes()


def test_malformed_input_is_refused_with_a_text(folder):
    from countr_amd import _lib
    from countr_amd._lib import CountrError
    m = on_device([np.ones((5, 7), np.float32)])[0]
    for maps, scale, text in (([], [], "1..16 classes"),
                              ([m] * 17, [1.0] * 17, "1..16 classes"),
                              ([m, None], [1.0, 1.0], "null"),
                              ([m, m[:4]], [1.0, 1.0], "one shape"),
                              ([m, m.double()], [1.0, 1.0], "fp32")):
        with pytest.raises(CountrError, match=text):
            folder.fold([(maps, scale)])
    # the library's own refusals, through the C ABI (nothing is launched: every pointer below is refused or never read)
    K = _lib.classes_lib()
    out = torch.zeros(3 * 17 * 16, dtype=torch.int32, device="cuda")
    dev = torch.zeros(17 * C.sizeof(_lib.ClassSet), dtype=torch.uint8, device="cuda")
    lab = torch.zeros(35, dtype=torch.uint8, device="cuda")

    def call(sets, n):
        p = out.data_ptr()
        return K.countr_class_fold(sets, n, dev.data_ptr(), 0.0, p, p + 4 * 17 * 16, p + 8 * 17 * 16, dev.data_ptr(), None)

    def fresh():
        sets = (_lib.ClassSet * 17)()
        for d in sets:
            d.nc, d.h, d.w, d.labels, d.map[0], d.scale[0] = 1, 5, 7, lab.data_ptr(), m.data_ptr(), 1.0
        return sets

    for change, n, text in ((lambda s: None, 17, "1..16 sets"),
                            (lambda s: None, 0, "1..16 sets"),
                            (lambda s: setattr(s[0], "nc", 0), 1, "1..16 classes"),
                            (lambda s: setattr(s[1], "nc", 17), 2, "1..16 classes"),
                            (lambda s: setattr(s[0], "nc", 2), 1, "map 1: null"),
                            (lambda s: setattr(s[0], "w", (1 << 28) // 5 + 1), 1, "2\\^28 pixels"),
                            (lambda s: setattr(s[0], "labels", None), 1, "no label map")):
        sets = fresh()
        change(sets)
        with pytest.raises(CountrError, match=text):
            _lib.classes_check(call(sets, n), "countr_class_fold")
    (labels, won, total, area), = folder.fold([([m], [2.0])])      # and the folder works after the refusals
    assert area.tolist() == [35] and won.tolist() == [70.0] and total.tolist() == [70.0] and (labels == 0).all()


# ---- the engine's class-dependent tail, on the tiny configuration
def tiny_model(precision):
    import torch.nn as nn
    from countr_amd.models_mae_cross import SupervisedMAE
    p, D, depth, H, Dd, ddepth, Hd = W.CONFIGS["tiny_test"]
    m = SupervisedMAE(patch_size=p, embed_dim=D, depth=depth, num_heads=H, decoder_embed_dim=Dd, decoder_depth=ddepth, decoder_num_heads=Hd,
                      mlp_ratio=4, norm_layer=partial(nn.LayerNorm, eps=1e-6), precision=precision)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.make_state_dict("tiny_test", seed=3).items()}, strict=True)
    return m.to("cuda").eval()


@pytest.fixture(scope="module", params=["fp32", "bf16", "fp16"])
def model(request):
    return tiny_model(request.param)


def test_engine_tail_and_prefix_are_bit_identical_to_full_forwards(model):
    imgs, boxes_a, _gt, _mask = W.make_inputs(batch=2, shots=3, seed=5)
    _i, boxes_b, _g, _m = W.make_inputs(batch=2, shots=3, seed=6)
    imgs, boxes_a, boxes_b = (torch.from_numpy(v).cuda() for v in (imgs, boxes_a, boxes_b))
    eng = model._engine()
    with torch.no_grad():
        for S in (3, 1):                               # both plans exist before the first forward
            eng.plan(2, S, False)
        want_b3 = eng.forward(imgs, boxes_b, 3).clone()
        want_b1 = eng.forward(imgs, boxes_b, 1).clone()
        out_a = eng.forward(imgs, boxes_a, 3).clone()
        assert not torch.equal(out_a, want_b3)         # the exemplars matter
        p3, p1 = eng.plan(2, 3, False), eng.plan(2, 1, False)
        eng._load_boxes(p3, boxes_b, 3)
        got = eng.forward_loaded_tail(2, 3)
        assert got.data_ptr() == p3.buf["out"].data_ptr() and torch.equal(got, want_b3)
        eng._load_boxes(p3, boxes_a, 3)                # and back again: the prefix is still in place
        assert torch.equal(eng.forward_loaded_tail(2, 3), out_a)
        # another shot count: the latent comes from plan (2, 3); the plan's own is poisoned first, so the copy is what feeds the decoder
        p1.buf["latent"].zero_()
        p1.buf["out"].zero_()
        eng._load_boxes(p1, boxes_b, 1)
        assert torch.equal(eng.forward_loaded_from(2, 1, 3), want_b1)
        eng._load_boxes(p1, boxes_a, 1)
        got = eng.forward_loaded_tail(2, 1).clone()
        assert torch.equal(got, eng.forward(imgs, boxes_a, 1))
        # zero-shot: nothing is class-dependent, the output is reused
        want_0 = eng.forward(imgs, boxes_a, 0).clone()
        assert torch.equal(eng.forward_loaded_tail(2, 0), want_0)
        assert torch.equal(eng.forward_loaded_from(2, 0, 3), want_0)
        torch.cuda.synchronize()


# ---- end to end
FRAMES = [np.random.RandomState(11).randint(0, 256, (60, 90, 3)).astype(np.uint8), np.random.RandomState(12).randint(0, 256, (48, 120, 3)).astype(np.uint8)]
LARGE_A = [[(5, 5, 30, 30), (40, 10, 70, 40), (55, 25, 85, 55)], [(5, 5, 30, 30), (50, 10, 80, 40), (90, 8, 115, 36)]]
LARGE_B = [[(10, 20, 45, 50), (30, 2, 60, 28), (62, 8, 88, 30)], [(20, 10, 60, 44), (2, 2, 40, 20), (70, 15, 110, 45)]]
ONE = [[(20, 15, 60, 50)], [(30, 5, 90, 40)]]
# frame 0: exemplars under 10 px in the resized image -> the 3 x 3 path; frame 1: large exemplars
SMALL = [[(10, 10, 11, 11), (40, 20, 41, 21), (70, 40, 71, 41)], [(5, 5, 30, 30), (50, 10, 80, 40), (90, 8, 115, 36)]]
CLASSES = {"a": LARGE_A, "b": LARGE_B, "one": ONE, "any": None, "small": SMALL}


def test_count_classes_end_to_end(model, monkeypatch):
    from countr_amd import ClassCounts, count_classes, count_frames
    from countr_amd.classes import classes_host
    eng = model._engine()
    ref = {name: count_frames(model, FRAMES, boxes) for name, boxes in CLASSES.items()}      # (also the first use of the weights: check_ln_fold)
    launches = []
    inner = eng.run

    def recording(ops, stream=None):
        launches.append(sum(1 for fn, _args, _keep in ops if fn is eng.L.countr_im2patch))
        return inner(ops, stream)

    monkeypatch.setattr(eng, "run", recording)
    for name, boxes in CLASSES.items():
        count_frames(model, FRAMES, boxes)
    assert sum(launches) == 6                          # a forward each, and two for the class with a split frame
    del launches[:]
    res = count_classes(model, FRAMES, CLASSES, floor=0.0)
    # one encoder forward per distinct window list: both frames plain, frame 0's nine crops, frame 1 alone
    assert sum(launches) == 3
    monkeypatch.undo()
    assert len(res) == 2 and all(isinstance(r, ClassCounts) and r.names == tuple(CLASSES) for r in res)
    for f, r in enumerate(res):
        for c, name in enumerate(CLASSES):
            cnt, dm = ref[name][f]
            assert r.counts[c] == cnt and torch.equal(r.maps[c], dm), (f, name, r.counts[c], cnt)      # count_frames' bit for bit
    assert res[0].labels is None and res[0].won is None and res[0].total is None and res[0].area is None      # "small" is split on frame 0
    r = res[1]
    nc, (h, w) = len(CLASSES), r.maps[0].shape
    assert r.labels.dtype == torch.uint8 and r.labels.is_cuda and tuple(r.labels.shape) == (384, 960) == (h, w)
    assert r.won.dtype == r.total.dtype == np.float32 and r.area.dtype == np.int32 and r.won.shape == r.total.shape == r.area.shape == (nc,)
    maps = [m.cpu().numpy() for m in r.maps]
    sums = [float(m.sum().item()) for m in r.maps]
    scale = np.asarray([r.counts[c] / sums[c] if sums[c] != 0 else 1.0 / 60 for c in range(nc)], np.float32)
    wl, ww, wt, wa, wabs, tabs = classes_host(maps, scale, 0.0, members=True)
    assert np.array_equal(r.labels.cpu().numpy(), wl) and np.array_equal(r.area, wa)
    assert r.area.sum() + int((wl == 255).sum()) == h * w
    n = h * w
    bw = wa * U * wabs + np.spacing(np.abs(ww).astype(np.float32))
    bt = n * U * tabs + np.spacing(np.abs(wt).astype(np.float32))
    ew, et = np.abs(r.won.astype(np.float64) - ww), np.abs(r.total.astype(np.float64) - wt)
    ec = np.abs(r.total.astype(np.float64) - np.asarray(r.counts, np.float64))
    print("counts %s\nwon %s\ntotal %s\narea %s\nwon err / bound %s\ntotal err / bound %s\n|total - count| / bound %s"
          % (r.counts, r.won, r.total, r.area, ew / np.maximum(bw, 1e-300), et / bt, ec / bt))
    assert (ew <= bw).all() and (et <= bt).all()
    assert (ec <= bt).all()                            # scale[c] = counts[c] / sum(maps[c]): the totals are the counts
    # fold=False: the same counts and maps, no fold, and any number of classes
    many = {"c%d" % k: (LARGE_A, LARGE_B, None)[k % 3] for k in range(17)}
    with pytest.raises(ValueError, match="at most 16 classes"):
        count_classes(model, FRAMES, many)
    plain = count_classes(model, FRAMES, many, fold=False)
    for f, r in enumerate(plain):
        assert r.labels is None and len(r.counts) == 17
        for k in range(17):
            cnt, dm = ref[("a", "b", "any")[k % 3]][f]
            assert r.counts[k] == cnt and torch.equal(r.maps[k], dm)


def test_demo_classes_json(tmp_path):
    """demo.py --classes_json as a user would run it (a subprocess, the randomly initialised model): the lines, the JSON and the tinted
    picture; its counts are count_classes' on the same model built here."""
    from PIL import Image
    rs = np.random.RandomState(81)
    frame = rs.randint(0, 256, size=(120, 200, 3)).astype(np.uint8)
    Image.fromarray(frame).save(tmp_path / "lot.png")
    named = {"cars": [[20, 20, 60, 50], [100, 30, 150, 70], [60, 70, 110, 110]], "people": [[10, 60, 40, 110], [150, 10, 190, 60], [80, 5, 120, 40]]}
    (tmp_path / "classes.json").write_text(json.dumps(named))
    base = [sys.executable, "demo.py", "--input_path", str(tmp_path / "lot.png"), "--model_path", "", "--precision", "fp32"]
    r = subprocess.run(base + ["--output_path", str(tmp_path / "out"), "--classes_json", str(tmp_path / "classes.json")], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    out = r.stdout.splitlines()
    js = json.loads((tmp_path / "out" / "classes_lot.json").read_text())
    assert set(js) == {"classes"} and list(js["classes"]) == list(named)
    assert all(set(v) == {"count", "won", "area"} and np.isfinite(v["count"]) for v in js["classes"].values())
    assert [l.split()[1].rstrip(":") for l in out if l.startswith("  class ")] == list(named)
    assert Image.open(tmp_path / "out" / "viz_lot.jpg").size == (640, 384)
    assert not any(l.startswith("Count:") for l in out)
    import models_mae_cross
    from countr_amd import count_classes
    torch.manual_seed(0)
    model = models_mae_cross.__dict__["mae_vit_base_patch16"](norm_pix_loss="store_true", precision="fp32").to("cuda").eval()
    res, = count_classes(model, [frame], {n: [[tuple(b) for b in bx]] for n, bx in named.items()})
    for c, n in enumerate(named):
        assert js["classes"][n]["count"] == float(res.counts[c])
        assert js["classes"][n]["won"] == float(res.won[c]) and js["classes"][n]["area"] == int(res.area[c])
    assert sum(v["area"] for v in js["classes"].values()) + int((res.labels == 255).sum().item()) == 384 * 640
