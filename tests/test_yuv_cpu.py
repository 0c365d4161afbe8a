"""CPU: countr_amd.yuv_host, the numpy statement of the rule of include/countr_hip_yuv.h, against the float matrices the integer
coefficients round, against Pillow, against a hand-computed literal of the LINEAR chroma reconstruction, and the layouts of YuvFrame.

The bar is "within 1", from the number formats: a coefficient is round(256 x the exact one), off by at most 0.5 / 256, and a channel
is a sum of at most three products with |Y - yoff| <= 255 and |U - 128|, |V - 128| <= 128, so the integer rule's value before its
rounding is off by less than (0.5 * 255 + 0.5 * 128 + 0.5 * 128) / 256 < 1 (10-bit samples scale both sides alike).  Two numbers
less than 1 apart, both rounded half up and clamped, differ by at most 1.  Pillow's YCbCr -> RGB (BT.601 full range in fixed point
of its own) is held to the same bar."""
import numpy as np
import pytest

from countr_amd import YuvFrame, yuv_host
from countr_amd import yuv as Y

KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
PAIRS = [("bt601", "full"), ("bt709", "full"), ("bt601", "limited"), ("bt709", "limited")]


def float_rgb(y, u, v, matrix, range_, bits=8):
    """The exact matrix in float64 on `bits`-bit samples, scaled to 8 bits, rounded half up and clamped."""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    s = float(1 << (bits - 8))
    y, u, v = (np.asarray(a, np.float64) / s for a in (y, u, v))
    if range_ == "limited":
        yy, d, e = (y - 16.0) * 255.0 / 219.0, (u - 128.0) * 255.0 / 224.0, (v - 128.0) * 255.0 / 224.0
    else:
        yy, d, e = y, u - 128.0, v - 128.0
    r = yy + 2.0 * (1.0 - kr) * e
    b = yy + 2.0 * (1.0 - kb) * d
    g = yy - (2.0 * kb * (1.0 - kb) / kg) * d - (2.0 * kr * (1.0 - kr) / kg) * e
    return np.clip(np.floor(np.stack([r, g, b], -1) + 0.5), 0, 255).astype(np.int16)


@pytest.fixture(scope="module")
def all_triples():
    """A 4096 x 4096 i420 frame that holds every 8-bit (Y, U, V) triple once under NEAREST: chroma sample (j, i) is U = j & 255,
    V = i & 255, and its 64 copies x 4 luma pixels carry the 256 values of Y.  -> (y, u, v planes, full-size U, V)."""
    j, i = np.arange(2048)[:, None], np.arange(2048)[None, :]
    u = np.ascontiguousarray(np.broadcast_to(j & 255, (2048, 2048)).astype(np.uint8))
    v = np.ascontiguousarray(np.broadcast_to(i & 255, (2048, 2048)).astype(np.uint8))
    yy, xx = np.arange(4096)[:, None], np.arange(4096)[None, :]
    y = ((((yy >> 1) >> 8) * 8 + ((xx >> 1) >> 8)) * 4 + (yy & 1) * 2 + (xx & 1)).astype(np.uint8)
    codes = (y.astype(np.int64) << 16) | (np.repeat(np.repeat(u, 2, 0), 2, 1).astype(np.int64) << 8) | np.repeat(np.repeat(v, 2, 0), 2, 1)
    assert np.unique(codes).size == 1 << 24
    return y, u, v, np.repeat(np.repeat(u, 2, 0), 2, 1), np.repeat(np.repeat(v, 2, 0), 2, 1)


@pytest.mark.parametrize("matrix,range_", PAIRS)
def test_every_8_bit_triple_is_within_1_of_the_float_matrix(all_triples, matrix, range_):
    y, u, v, uf, vf = all_triples
    got = yuv_host(YuvFrame(y, u, v, format="i420", matrix=matrix, range=range_))
    assert got.dtype == np.uint8 and got.shape == (4096, 4096, 3)
    worst = 0
    for r0 in range(0, 4096, 512):                                # (in slabs: the float64 planes of the whole frame are 400 MB)
        want = float_rgb(y[r0:r0 + 512], uf[r0:r0 + 512], vf[r0:r0 + 512], matrix, range_)
        worst = max(worst, int(np.abs(got[r0:r0 + 512].astype(np.int16) - want).max()))
    print("%s %s: largest distance from the float matrix %d" % (matrix, range_, worst))
    assert worst <= 1


def test_bt601_full_is_within_1_of_pillow(all_triples):
    from PIL import Image
    y, u, v, uf, vf = all_triples
    got = yuv_host(YuvFrame(y, u, v, format="i420", matrix="bt601", range="full"))
    worst = 0
    for r0 in range(0, 4096, 512):
        ycc = np.stack([y[r0:r0 + 512], uf[r0:r0 + 512], vf[r0:r0 + 512]], -1)
        want = np.asarray(Image.frombytes("YCbCr", (4096, 512), np.ascontiguousarray(ycc).tobytes()).convert("RGB"), dtype=np.int16)
        worst = max(worst, int(np.abs(got[r0:r0 + 512].astype(np.int16) - want).max()))
    print("bt601 full: largest distance from Pillow %d" % worst)
    assert worst <= 1


@pytest.mark.parametrize("matrix,range_", PAIRS)
def test_seeded_10_bit_samples_are_within_1_of_the_float_matrix(matrix, range_):
    rs = np.random.RandomState(1010)
    y, c = rs.randint(0, 1024, (1024, 1024)), rs.randint(0, 1024, (512, 1024))
    low = rs.randint(0, 64, (1024, 1024))                         # the six low bits of a word are not part of the sample
    f = YuvFrame(((y << 6) | low).astype(np.uint16), (c << 6).astype(np.uint16), format="p010", matrix=matrix, range=range_)
    got = yuv_host(f)
    assert np.array_equal(got, yuv_host(YuvFrame((y << 6).astype(np.uint16), (c << 6).astype(np.uint16), format="p010", matrix=matrix, range=range_)))
    up = lambda p: np.repeat(np.repeat(p, 2, 0), 2, 1)
    want = float_rgb(y, up(c[:, 0::2]), up(c[:, 1::2]), matrix, range_, bits=10)
    worst = int(np.abs(got.astype(np.int16) - want).max())
    print("%s %s, 10 bits: largest distance from the float matrix %d" % (matrix, range_, worst))
    assert worst <= 1


def test_grey_and_primary_literals():
    one = lambda y, u, v, **kw: yuv_host(YuvFrame(np.array([[y]], np.uint8), np.array([[u, v]], np.uint8), **kw))[0, 0].tolist()
    assert one(100, 128, 128, matrix="bt601", range="full") == [100, 100, 100]
    assert one(16, 128, 128) == [0, 0, 0] and one(235, 128, 128) == [255, 255, 255] and one(126, 128, 128) == [128, 128, 128]
    assert one(0, 128, 128) == [0, 0, 0] and one(255, 128, 128) == [255, 255, 255]          # clamped below and above
    # C = 298 * (81 - 16) = 19370: (C + 409 * 112 + 128) >> 8 = 255; (C - 100 * -38 - 208 * 112 + 128) >> 8 = 0; (C + 516 * -38 + 128) >> 8 = -1
    assert one(81, 90, 240, matrix="bt601", range="limited") == [255, 0, 0]
    p = lambda y, u, v: yuv_host(YuvFrame(np.array([[y << 6]], np.uint16), np.array([[u << 6, v << 6]], np.uint16), format="p010"))[0, 0].tolist()
    assert p(64, 512, 512) == [0, 0, 0] and p(940, 512, 512) == [255, 255, 255] and p(502, 512, 512) == [127, 127, 127]


U22 = np.array([[10, 50], [90, 250]], np.uint8)
V22 = np.array([[1, 2], [4, 9]], np.uint8)
# LINEAR by hand.  Rows: s = 3 c[j] + c[jn] with (j, jn) = (0, 0), (0, 1), (1, 0), (1, 1); columns: (s0 + 2) >> 2, (s0 + s1 + 4) >> 3,
# (s1 + 2) >> 2, (s1 + s1 + 4) >> 3.  For U the s rows are [40, 200], [120, 400], [280, 800], [360, 1000]; for V [4, 8], [7, 15], [13, 29],
# [16, 36]
U44 = [[10, 30, 50, 50], [30, 65, 100, 100], [70, 135, 200, 200], [90, 170, 250, 250]]
V44 = [[1, 2, 2, 2], [2, 3, 4, 4], [3, 5, 7, 7], [4, 7, 9, 9]]


def test_linear_chroma_on_a_4_x_4_literal():
    assert Y.upsample_host(U22.astype(np.int32), 4, 4, "linear").tolist() == U44
    assert Y.upsample_host(V22.astype(np.int32), 4, 4, "linear").tolist() == V44
    assert Y.upsample_host(U22.astype(np.int32), 4, 4, "nearest").tolist() == [[10, 10, 50, 50]] * 2 + [[90, 90, 250, 250]] * 2
    # an odd size keeps the leading part: the last chroma row and column then serve one luma row and column
    assert Y.upsample_host(U22.astype(np.int32), 3, 3, "linear").tolist() == [r[:3] for r in U44[:3]]
    luma = np.arange(16, dtype=np.uint8).reshape(4, 4) * 13 + 20
    for matrix, range_ in PAIRS:
        got = yuv_host(YuvFrame(luma, U22, V22, format="i420", matrix=matrix, range=range_, chroma="linear"))
        assert np.array_equal(got, Y.convert_host(luma, np.array(U44), np.array(V44), matrix, range_))
        # full-resolution chroma planes under NEAREST reach the same pixels through an 8 x 8 frame's even rows and columns
        big = yuv_host(YuvFrame(np.repeat(np.repeat(luma, 2, 0), 2, 1), np.array(U44, np.uint8), np.array(V44, np.uint8), format="i420",
                                matrix=matrix, range=range_))
        assert np.array_equal(big[::2, ::2], got)
    nv = np.stack([U22, V22], -1).reshape(2, 4)
    assert np.array_equal(yuv_host(YuvFrame(luma, nv, chroma="linear")), Y.convert_host(luma, np.array(U44), np.array(V44), "bt709", "limited"))
    p10 = yuv_host(YuvFrame(luma.astype(np.uint16) << 8, nv.astype(np.uint16) << 6, format="p010", chroma="linear"))
    assert np.array_equal(p10, Y.convert_host(luma.astype(np.int32) << 2, np.array(U44), np.array(V44), "bt709", "limited", bits=10))


@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (6, 8), (33, 130)])
def test_constant_chroma_gives_the_same_image_under_linear_and_nearest(H, W):
    rs = np.random.RandomState(H * 100 + W)
    hc, wc = (H + 1) // 2, (W + 1) // 2
    y = rs.randint(0, 256, (H, W)).astype(np.uint8)
    c = np.tile(np.array([77, 201], np.uint8), (hc, wc))
    a = yuv_host(YuvFrame(y, c, chroma="nearest"))
    assert a.shape == (H, W, 3) and a.flags["C_CONTIGUOUS"] and np.array_equal(a, yuv_host(YuvFrame(y, c, chroma="linear")))
    y16, c16 = rs.randint(0, 1024, (H, W)).astype(np.uint16) << 6, np.tile(np.array([300 << 6, 801 << 6], np.uint16), (hc, wc))
    assert np.array_equal(yuv_host(YuvFrame(y16, c16, format="p010", chroma="nearest")), yuv_host(YuvFrame(y16, c16, format="p010", chroma="linear")))


@pytest.mark.parametrize("chroma", ["nearest", "linear"])
@pytest.mark.parametrize("H,W", [(3, 5), (6, 8), (33, 130)])
def test_formats_of_the_same_samples_agree(H, W, chroma):
    rs = np.random.RandomState(H + W)
    hc, wc = (H + 1) // 2, (W + 1) // 2
    y, u, v = rs.randint(0, 256, (H, W)).astype(np.uint8), rs.randint(0, 256, (hc, wc)).astype(np.uint8), rs.randint(0, 256, (hc, wc)).astype(np.uint8)
    kw = dict(matrix="bt601", range="limited", chroma=chroma)
    want = yuv_host(YuvFrame(y, u, v, format="i420", **kw))
    uv, vu = np.stack([u, v], -1).reshape(hc, 2 * wc), np.stack([v, u], -1).reshape(hc, 2 * wc)
    assert np.array_equal(yuv_host(YuvFrame(y, uv, format="nv12", **kw)), want)
    assert np.array_equal(yuv_host(YuvFrame(y, vu, format="nv21", **kw)), want)
    assert not np.array_equal(yuv_host(YuvFrame(y, uv, format="nv21", **kw)), want)
    # a pitch is a row stride: planes cut out of wider buffers give the same image
    wide_y, wide_c = np.full((H, W + 9), 255, np.uint8), np.full((hc, 2 * wc + 6), 255, np.uint8)
    wide_y[:, :W], wide_c[:, :2 * wc] = y, uv
    assert np.array_equal(yuv_host(YuvFrame(wide_y[:, :W], wide_c[:, :2 * wc], format="nv12", **kw)), want)
    # CPU tensors are planes too
    import torch
    assert np.array_equal(yuv_host(YuvFrame(torch.from_numpy(wide_y)[:, :W], torch.from_numpy(wide_c)[:, :2 * wc], format="nv12", **kw)), want)


@pytest.mark.parametrize("W,H", [(5, 3), (7, 5), (8, 6), (1, 1)])
def test_from_buffer_views_for_odd_sizes(W, H):
    hc, wc = (H + 1) // 2, (W + 1) // 2
    n = W * H + 2 * wc * hc
    raw = (np.arange(n) * 7 % 251).astype(np.uint8)
    f = YuvFrame.from_buffer(raw.tobytes(), W, H)
    assert f.shape == (H, W, 3) and f.format == "nv12" and f.matrix == "bt709" and f.range == "limited" and f.chroma == "nearest"
    assert np.array_equal(f.y, raw[:W * H].reshape(H, W)) and np.array_equal(f.c0, raw[W * H:].reshape(hc, 2 * wc)) and f.c1 is None
    g = YuvFrame.from_buffer(raw, W, H, format="i420", chroma="linear")
    assert np.array_equal(g.c0, raw[W * H:W * H + wc * hc].reshape(hc, wc)) and np.array_equal(g.c1, raw[W * H + wc * hc:].reshape(hc, wc))
    assert np.shares_memory(g.y, raw) and g.chroma == "linear"
    words = (np.arange(n) * 977 % 65536).astype("<u2")
    p = YuvFrame.from_buffer(words.tobytes(), W, H, format="p010")
    assert p.y.dtype == np.uint16 and np.array_equal(p.y, words[:W * H].reshape(H, W)) and np.array_equal(p.c0, words[W * H:].reshape(hc, 2 * wc))
    import torch
    t = YuvFrame.from_buffer(torch.from_numpy(raw.copy()), W, H, format="nv21")
    assert np.array_equal(yuv_host(t), yuv_host(YuvFrame.from_buffer(raw, W, H, format="nv21")))
    with pytest.raises(ValueError, match="has %d bytes, the buffer %d" % (n, n + 1)):
        YuvFrame.from_buffer(bytes(n + 1), W, H)
    with pytest.raises(ValueError, match="has %d bytes" % (2 * n)):
        YuvFrame.from_buffer(bytes(n), W, H, format="p010")


def test_shape_and_dtype_refusals():
    y, c = np.zeros((4, 6), np.uint8), np.zeros((2, 6), np.uint8)
    YuvFrame(y, c)
    with pytest.raises(ValueError, match="format is one of"):
        YuvFrame(y, c, format="yuy2")
    with pytest.raises(ValueError, match="matrix is one of"):
        YuvFrame(y, c, matrix="bt2020")
    with pytest.raises(ValueError, match="range is one of"):
        YuvFrame(y, c, range="tv")
    with pytest.raises(ValueError, match="chroma is one of"):
        YuvFrame(y, c, chroma="cubic")
    with pytest.raises(ValueError, match="c1"):
        YuvFrame(y, c, c)
    with pytest.raises(ValueError, match="c1"):
        YuvFrame(y, np.zeros((2, 3), np.uint8), format="i420")
    with pytest.raises(ValueError, match="2-D plane"):
        YuvFrame(np.zeros((4, 6, 1), np.uint8), c)
    with pytest.raises(ValueError, match="nv12 planes are uint8, y is uint16"):
        YuvFrame(y.astype(np.uint16), c)
    with pytest.raises(ValueError, match="p010 planes are uint16, c0 is uint8"):
        YuvFrame(y.astype(np.uint16), c, format="p010")
    with pytest.raises(ValueError, match=r"c0 of shape \(2, 6\), got \(2, 3\)"):
        YuvFrame(y, np.zeros((2, 3), np.uint8))
    with pytest.raises(ValueError, match=r"c0 of shape \(3, 6\)"):
        YuvFrame(np.zeros((5, 5), np.uint8), c)                  # odd sizes round the chroma planes up
    with pytest.raises(ValueError, match=r"c1 of shape \(2, 3\)"):
        YuvFrame(y, np.zeros((2, 3), np.uint8), np.zeros((2, 4), np.uint8), format="i420")
    with pytest.raises(ValueError, match="last stride"):
        YuvFrame(np.zeros((4, 12), np.uint8)[:, ::2], c)
    with pytest.raises(ValueError, match="1..16384"):
        YuvFrame(np.zeros((1, 16385), np.uint8), np.zeros((1, 16386), np.uint8))
