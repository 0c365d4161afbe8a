"""The embedding, references and assertions of tests/gpoison.py on the CPU, before any kernel meets them: an fp32 torch emulation of each
operation that reads the embedded storage passes the assertions the kernels' outputs are given, and deliberately wrong variants of it (a
lost K-tail mask, ragged M read and stored as a full tile, the ldc pad written, conv taps taken from the flat neighbours, one split-K
slab too many, a pixel reduction one k-tile past P) fail them.  No kernel runs here and no wrong variant is ever applied to one."""
import pytest
import torch

import gpoison as GP
from kedges import GUARD

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
DT_IDS = ["fp32", "bf16", "fp16"]
TOL = {torch.float32: 1e-4, torch.bfloat16: 2e-2, torch.float16: 2.5e-3}      # the max-norm bars of kedges.DT, per storage type


def fails(fn, *args, **kw):
    try:
        fn(*args, **kw)
    except AssertionError:
        return True
    return False


# ---------------------------------------------------------------------------------------------------------------- the embedding itself
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_embedding_poisons_pads_and_bands_and_keeps_alignment(dtype):
    body = GP.vals((5, 24), 1, dtype)
    e = GP.embed(body, ld=32, front=3, back=GP.ragged_band(32))
    assert e.lo % 8 == 0 and e.lo >= 8 and e.back == 256 * 32 and (e.ptr - e.flat.data_ptr()) % 16 == 0
    assert torch.equal(e.t, body) and e.flat.numel() == e.lo + 5 * 32 + e.back
    whole = GP.read_at(e, 5, 32)
    assert bool(torch.isnan(whole[:, 24:]).all()) and bool(torch.isnan(e.flat[:e.lo]).all()) and bool(torch.isnan(e.flat[e.lo + 5 * 32:]).all())
    assert e.intact() and e.unchanged()
    e.t.fill_(1.0)                                          # the body may change (an output) ...
    assert e.intact() and not e.unchanged()
    for at in (e.lo - 1, e.lo + 24, e.lo + 31, e.lo + 4 * 32 + 24, e.lo + 5 * 32, e.flat.numel() - 1):      # ... nothing else: bands, every pad
        h = GP.embed(body, ld=32, front=3, back=16)
        if at < h.flat.numel():
            h.flat[at] = 0.0
            assert not h.intact(), at
    o = GP.Embedded(3, 8, 16, dtype)                       # an output: a plain NaN stored onto its payload NaN shows, in the band and in a pad
    assert bool(torch.isnan(o.flat.float()).all()) and o.intact()
    for at in (o.lo - 1, o.lo + 8, o.lo + 3 * 16):
        o = GP.Embedded(3, 8, 16, dtype)
        o.flat[at] = float("nan")
        assert not o.intact(), at
    assert GP.band(1) == 8 and GP.band(9) == 16 and GP.conv_band(7, 64) == (2 * 7 + 2 + 256) * 64 and GUARD % 8 == 0


def test_packed_buffer_keeps_unused_slices_poisoned():
    q = GP.packed(6, 3, 16, (0, 1), 7, torch.bfloat16)
    for i, fin in ((0, True), (1, True), (2, False)):
        v, p = q.cols_slice(i, 16)
        assert bool(torch.isfinite(v.float()).all()) == fin and bool(torch.isnan(v.float()).all()) == (not fin)
        assert p == q.ptr + i * 16 * 2
    g = GP.packed(6, 3, 16, (1,), 7, torch.float16)        # dy as the middle third of a packed gradient
    assert bool(torch.isnan(g.cols_slice(0, 16)[0].float()).all()) and bool(torch.isfinite(g.cols_slice(1, 16)[0].float()).all())


def test_splitk_ranges_follow_the_kernel():
    assert GP.splitk_ranges(200, 3) == [(0, 128), (128, 200), (200, 200)]          # a range that ends inside a k-tile, an empty slab
    assert GP.splitk_ranges(128, 5) == [(0, 64), (64, 128), (128, 128), (128, 128), (128, 128)]
    assert GP.splitk_ranges(256, 1) == [(0, 256)]


# ---------------------------------------------------------------------------------------------------------------- matmul
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("M,N,K", [(8, 8, 8), (136, 72, 40), (40, 128, 128)])
def test_matmul_emulation_inside_and_wrong_variants_outside(dtype, M, N, K):
    chunk = 4 if dtype == torch.float32 else 8
    A = GP.embed(GP.vals((M, K), 1, dtype), ld=K + chunk, back=GP.ragged_band(K + chunk))
    B = GP.embed(GP.vals((N, K), 2, dtype), ld=K + chunk)
    ref = GP.matmul_ref(A, B)

    def run(**kw):
        out = GP.Embedded(M, N, N + 8, dtype, back=GP.ragged_band(N + 8))
        GP.emu_matmul(A, B, out, **kw)
        GP.assert_close(out.t, ref, TOL[dtype])
        GP.assert_surroundings([out], [A, B])
    run()
    assert fails(run, k_read="ld"), "lost K-tail mask"
    assert fails(run, rows_read=GP.TILE_ROWS, store_rows=GP.TILE_ROWS), "ragged M stored past the end"
    assert fails(run, store_cols=N + 8), "ldc pad written"


# ---------------------------------------------------------------------------------------------------------------- 3 x 3 convolution
@pytest.mark.parametrize("Bn,H,W,Cin,Cout", [(1, 5, 7, 64, 64), (2, 3, 4, 64, 8), (1, 1, 6, 64, 8)])
def test_conv_emulation_inside_and_flat_neighbour_taps_outside(Bn, H, W, Cin, Cout):
    dtype = torch.bfloat16
    P = Bn * H * W
    x = GP.embed(GP.vals((P, Cin), 3, dtype), front=GP.conv_band(W, Cin), back=GP.conv_band(W, Cin))
    w = GP.embed(GP.vals((Cout, 9 * Cin), 4, dtype, 0.1), ld=9 * Cin + 8)
    ref = GP.conv_ref(x, w, None, Bn, H, W)

    def run(**kw):
        out = GP.Embedded(P, Cout, Cout + 8, dtype)
        GP.emu_conv3x3(x, w, out, Bn, H, W, **kw)
        GP.assert_close(out.t, ref, TOL[dtype])
        GP.assert_surroundings([out], [x, w])
    run()
    assert fails(run, flat_rows=True), "first / last image row taken from the flat neighbours"


# ---------------------------------------------------------------------------------------------------------------- split-K reduction, wgrad
@pytest.mark.parametrize("sk,count", [(1, 40), (3, 1000), (5, 8 * 9 * 64)])
def test_splitk_reduction_emulation_inside_and_one_slab_too_many_outside(sk, count):
    parts = GP.slabs(GP.vals((sk, count), 5))
    assert bool(torch.isnan(GP.read_at(parts, sk + 1, count)[sk]).all())
    ref = parts.t.double().sum(0)

    def run(**kw):
        out = GP.Embedded(1, count)
        GP.emu_splitk_reduce(parts, out, sk, **kw)
        GP.assert_close(out.t[0], ref, 1e-5)
        GP.assert_surroundings([out], [parts])
    run()
    assert fails(run, extra_slabs=1), "one slab too many"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_wgrad_emulation_inside_and_one_ktile_past_the_pixels_outside(dtype):
    P, N, K = 64, 128, 128
    g = GP.packed(P, 3, N, (1,), 6, dtype, back=64 * 3 * N + GUARD)       # dy = the middle third of a packed gradient
    dyv, _ = g.cols_slice(1, N)
    x = GP.embed(GP.vals((P, K), 9, dtype), ld=K + 8, back=64 * (K + 8) + GUARD)
    ref = dyv.double().t() @ x.t.double()

    class Slice:                                            # the slice as an operand of its own: same storage, same pitch
        flat, ld, lo, cols = g.flat, g.ld, g.lo + N, N
    dy = Slice()

    def run(**kw):
        part = GP.Embedded(N, K)
        GP.emu_wgrad(dy, x, part, P, **kw)
        GP.assert_close(part.t, ref, 2e-5, 1e-9)
        GP.assert_surroundings([part], [g, x])
    run()
    assert fails(run, extra_pixels=64), "pixel reduction one k-tile past P"
