"""The MFMA GEMM family (gemm_kernel.hpp, linear.hip, gemm256.hip, conv_wgrad.hip, the reductions of gemm.hip) with NaN next to every
operand and guard bands around every output (tests/gpoison.py): pad columns, the bands in front of and behind each matrix, the unused
slices of packed buffers and the slab behind the last split-K slab are NaN, so a load mask that lets a neighbour through makes the result
NaN instead of "a little off", and a store outside an output changes a band.  Every case asserts: finite and within the bar of the test of
the same kernel in tests/test_gemm_gpu.py against fp64 of the bodies alone; every output band and pad bit-intact; every input bit-unchanged.

Shapes are the smallest that reach each form; the comment at each says which condition of the qualification code it sits on.  Where the
library can say which kernel runs it is asserted (countr_gemm_gn_rows, countr_gemm_rowsum_slabs, countr_gemm_group_tiles, the refusal of
the LayerNorm fields by the generic kernel).  What no query can tell is said at the case: the linear forms of linear.hip and gemm256.hip
(under COUNTR_G256=2 a decline falls to linear.hip silently), the head / tail split of the 256 x 256 convolution and the linear weight
gradients with 128 columns are pinned by the environment switches and the qualification arithmetic quoted in the comments alone."""
import ctypes as C

import pytest
import torch

import gpoison as GP
import halfprec as HP
from countr_amd import _lib
from kedges import GUARD

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLS = pytest.mark.parametrize("fl", HP.FLAVOURS, ids=HP.FLAVOUR_IDS)
# (torch dtype, dtype code of the C ABI, flavour): the generic kernel's fp32 parity mode runs on the bf16 build
MODES = pytest.mark.parametrize("dt,code,fl", [(torch.float32, 0, None), (torch.bfloat16, 1, HP.BF16), (torch.float16, 1, HP.FP16)],
                                ids=["fp32", "bf16", "fp16"])
PAIRS = pytest.mark.parametrize("ma,mb", [(0, 0), (0, 1), (1, 1), (1, 0)], ids=["row_row", "row_col", "col_col", "col_row"])


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _args(**kw):
    a = _lib.GemmArgs()
    a.alpha = 1.0; a.nbatch = 1; a.nb1 = 1; a.splitk = 1
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _lib_of(hip, fl):
    return HP.library(fl, default=hip) if fl is not None else hip


def _env(monkeypatch, **kw):
    for k, v in kw.items():
        monkeypatch.setenv("COUNTR_" + k, str(v))


def _emb(body, ld=None, **kw):
    return GP.embed(body, ld, device=DEV, **kw)


def _out(rows, cols, ld=None, dtype=torch.float32, **kw):
    return GP.Embedded(rows, cols, ld, dtype, DEV, **kw)


def _vec(n, seed):
    """An fp32 vector (bias, column sums) with poison on both sides."""
    return _emb(GP.vals((1, n), seed))


def _operand(body, mode, chunk):
    """Logical [rows, K] as the kernel takes it: ROW as it is, COL transposed; pitch = row + one chunk; a full tile of rows behind it."""
    st = (body if mode == 0 else body.t()).contiguous()
    ld = st.shape[1] + chunk
    return _emb(st, ld, back=GP.ragged_band(ld))


def _logical(e, mode):
    return e.t if mode == 0 else e.t.t()


def _sync():
    torch.cuda.synchronize()


# ================================================================================================================ generic kernel
# (8, 8, 8): one chunk.  (136, 72, 40): everything ragged, one partial k-tile, per-lane addressing.  (200, 136, 200): 4 tiles x 1 <= 256
# workgroups and >= 3 k-tiles: the wave-specialised variant, with a partial fourth k-tile.  (128, 128, 192): full k-tiles: uniform-base
# addressing.  (2176, 2048, 72): 17 x 16 = 272 > 256 workgroups: the plain two-stage variant.
GENERIC_SHAPES = [(8, 8, 8), (136, 72, 40), (200, 136, 200), (128, 128, 192), (2176, 2048, 72)]


def _generic(hip, monkeypatch, fl):
    _env(monkeypatch, LEAN=0, G256=0)             # linear.hip and conv_wgrad.hip decline under COUNTR_LEAN=0, gemm256.hip under COUNTR_G256=0
    return _lib_of(hip, fl)


@pytest.mark.parametrize("M,N,K", GENERIC_SHAPES)
@PAIRS
@MODES
def test_generic_kernel_with_poisoned_pads_and_bands(hip, monkeypatch, dt, code, fl, ma, mb, M, N, K):
    L = _generic(hip, monkeypatch, fl)
    chunk = 8 if code else 4
    A, B = _operand(GP.vals((M, K), 1, dt), ma, chunk), _operand(GP.vals((N, K), 2, dt), mb, chunk)
    out = _out(M, N, N + 4, back=GP.ragged_band(N + 4))
    a = _args(A=A.ptr, B=B.ptr, C=out.ptr, lda=A.ld, ldb=B.ld, ldc=out.ld, M=M, N=N, K=K)
    _lib.check(L.countr_gemm(C.byref(a), code, ma, mb, _stream()), "gemm")
    _sync()
    ref = _logical(A, ma).double() @ _logical(B, mb).double().t()
    GP.assert_close(out.t, ref, 1e-4, 1e-5)                          # test_gemm_modes
    GP.assert_surroundings([out], [A, B])


# K = 200, sk = 3: 4 (bf16) / 7 (fp32) k-tiles cut into whole k-tiles per slab: one range ends at K inside a k-tile, in bf16 the last slab is
# empty.  K = 128, sk = 5: more slabs than the 2 bf16 k-tiles: three empty slabs, which must be exact zeros.
@pytest.mark.parametrize("K,sk", [(200, 3), (128, 5)])
@PAIRS
@MODES
def test_generic_splitk_slabs_with_poisoned_operands(hip, monkeypatch, dt, code, fl, ma, mb, K, sk):
    L = _generic(hip, monkeypatch, fl)
    M, N, chunk = 136, 72, 8 if code else 4
    A, B = _operand(GP.vals((M, K), 3, dt), ma, chunk), _operand(GP.vals((N, K), 4, dt), mb, chunk)
    part = _out(sk, M * N, back=M * N)                                # slab `sk` is a band
    rowsum = code == 1 and (ma, mb) == (1, 1)                         # the fused bias gradient, in the wgrad arrangement its own test uses
    rs = _out(sk, M)
    a = _args(A=A.ptr, B=B.ptr, partial=part.ptr, lda=A.ld, ldb=B.ld, ldc=N, M=M, N=N, K=K, splitk=sk)
    if rowsum:
        a.rowsum_partial = rs.ptr
    _lib.check(L.countr_gemm(C.byref(a), code, ma, mb, _stream()), "gemm split-K")
    _sync()
    la, lb = _logical(A, ma).double(), _logical(B, mb).double()
    ref = la @ lb.t()
    assert bool(torch.isfinite(part.t).all())
    for z, (k0, k1) in enumerate(GP.splitk_ranges(K, sk, 64 if code else 32)):
        got = part.t[z].view(M, N)
        if k1 <= k0:
            assert bool((got == 0).all()), ("empty slab not zero", z)
        else:
            assert (got.double() - la[:, k0:k1] @ lb[:, k0:k1].t()).abs().max().item() <= 2e-4 * ref.abs().max().item(), z
    GP.assert_close(part.t.double().sum(0).view(M, N), ref, 2e-4)     # test_gemm_batched_and_splitk
    if rowsum:
        GP.assert_close(rs.t.double().sum(0), la.sum(1), 1e-4, 1e-4)  # test_wgrad_with_fused_bias_gradient
    else:
        assert rs.unchanged()
    GP.assert_surroundings([part, rs], [A, B])


@MODES
def test_generic_batched_q_kT_out_of_a_packed_qkv_with_poisoned_v(hip, monkeypatch, dt, code, fl):
    """q k^T per (image, head) read straight out of [B N, 3 H dh]: the v third, the bands and the score pads are NaN.  72 tokens: ragged
    M and N; dh = 64: one k-tile."""
    L = _generic(hip, monkeypatch, fl)
    Bsz, Ntok, H, dh = 2, 72, 3, 64
    qkv = GP.packed(Bsz * Ntok, 3, H * dh, (0, 1), 7, dt, DEV, back=GP.ragged_band(3 * H * dh))
    ldc = Ntok + 4
    sc = _out(Bsz * H * Ntok, Ntok, ldc, back=GP.ragged_band(ldc))
    (q, qp), (k, kp) = qkv.cols_slice(0, H * dh), qkv.cols_slice(1, H * dh)
    a = _args(A=qp, B=kp, C=sc.ptr, lda=qkv.ld, ldb=qkv.ld, ldc=ldc, M=Ntok, N=Ntok, K=dh, nbatch=Bsz * H, nb1=H,
              sA0=Ntok * qkv.ld, sB0=Ntok * qkv.ld, sA1=dh, sB1=dh, sC0=H * Ntok * ldc, sC1=Ntok * ldc, alpha=dh ** -0.5)
    _lib.check(L.countr_gemm(C.byref(a), code, 0, 0, _stream()), "gemm batched")
    _sync()
    qh = q.double().reshape(Bsz, Ntok, H, dh).permute(0, 2, 1, 3)
    kh = k.double().reshape(Bsz, Ntok, H, dh).permute(0, 2, 1, 3)
    ref = (qh @ kh.transpose(-1, -2)) * dh ** -0.5
    GP.assert_close(sc.t.reshape(Bsz, H, Ntok, Ntok), ref, 1e-4, 1e-5)   # test_gemm_batched_and_splitk
    GP.assert_surroundings([sc], [qkv])


# the small geometries of test_conv3x3_implicit_gemm: widths below the 64-pixel k-step, a single row, maps smaller than one k-step
@pytest.mark.parametrize("Bn,H,W,Cin,Cout", [(1, 5, 7, 64, 64), (1, 1, 40, 128, 136), (16, 2, 6, 64, 72), (8, 4, 4, 64, 64)])
@MODES
def test_generic_convolution_modes_on_an_embedded_map(hip, monkeypatch, dt, code, fl, Bn, H, W, Cin, Cout):
    """(IM2ROW, ROW) forward and (COL, IM2COL) split-K weight gradient: the taps above the first and below the last image row lie in NaN
    bands of (2 W + 2 + 256) pixels, the weights have a NaN ldb pad, dy has a NaN lda pad."""
    L = _generic(hip, monkeypatch, fl)
    P, chunk = Bn * H * W, 8 if code else 4
    cb = GP.conv_band(W, Cin)
    x = _emb(GP.vals((P, Cin), 10, dt), front=cb, back=cb)
    w = _emb(GP.vals((Cout, 9 * Cin), 11, dt, 0.1), 9 * Cin + chunk)
    bias = _vec(Cout, 12)
    out = _out(P, Cout, Cout + 4, back=GP.ragged_band(Cout + 4))
    a = _args(A=x.ptr, B=w.ptr, C=out.ptr, bias=bias.ptr, ldb=w.ld, ldc=out.ld, M=P, N=Cout, K=9 * Cin, H=H, W=W, Cin=Cin)
    _lib.check(L.countr_gemm(C.byref(a), code, 2, 0, _stream()), "conv fwd")
    _sync()
    GP.assert_close(out.t, GP.conv_ref(x, w, bias.t[0], Bn, H, W), 2e-4)          # test_conv3x3_implicit_gemm
    GP.assert_surroundings([out], [x, w, bias])
    dy = _emb(GP.vals((P, Cout), 13, dt), Cout + chunk, front=GP.band(64 * (Cout + chunk)), back=GP.ragged_band(Cout + chunk))
    sk = 3
    part = _out(sk, Cout * 9 * Cin, back=Cout * 9 * Cin)
    a = _args(A=dy.ptr, B=x.ptr, partial=part.ptr, lda=dy.ld, ldc=9 * Cin, M=Cout, N=9 * Cin, K=P, H=H, W=W, Cin=Cin, splitk=sk)
    _lib.check(L.countr_gemm(C.byref(a), code, 1, 3, _stream()), "conv wgrad")
    _sync()
    gw, _ = GP.conv_wgrad_ref(dy, x, Bn, H, W)
    GP.assert_close(part.t.double().sum(0).view(Cout, 9 * Cin), gw, 2e-4)
    GP.assert_surroundings([part], [dy, x])


# ================================================================================================================ lean linear (linear.hip)
# COUNTR_G256=0 keeps gemm256.hip out.  tiles = ceil(M / 128) (N / 128):
#   <= 256 tiles: the 128 x 128 wave-specialised form -- M = 40 / 128 / 200 (ragged, full, ragged second tile), K = 128 (the minimum: the
#       3-stage prologue alone) and 192 (one k-tile more);
#   M = 128 * 129 + 40, N = 256: 260 tiles, g256 = 65 * 2 <= 256: not the 192-row form -> 256 x 128;
#   M = 33000, N = 256, K = 128: g256 = 129 * 2 = 258 > 256, g192 = 172: span192 = 3 <= span256 = 4 -> 192 x 256 (the residual epilogue has
#       no such form and stays on 256 x 128).
LEAN_LINEAR_SHAPES = [(M, 128, K) for M in (40, 128, 200) for K in (128, 192)] + [(128 * 129 + 40, 256, 128), (33000, 256, 128)]


@pytest.mark.parametrize("epi", ["bf16", "gelu", "gelu_pre", "res", "gbwd"])
@pytest.mark.parametrize("M,N,K", LEAN_LINEAR_SHAPES)
@FLS
def test_lean_linear_forms_and_epilogues_with_poisoned_surroundings(hip, monkeypatch, fl, M, N, K, epi):
    _env(monkeypatch, LEAN=1, G256=0)
    _linear_case(_lib_of(hip, fl), fl, M, N, K, epi)


def _linear_case(L, fl, M, N, K, epi):
    """One nn.Linear launch: A and W at pitch K + 8, C (and C2, the residual) at pitch N + 8 / N + 4, a full tile of NaN rows behind every
    ragged operand.  Bars: test_lean_linear_matches_fp64_and_generic / test_g256_linear_matches_fp64_and_lean (the same figures),
    test_gelu_backward_epilogue_on_the_lean_kernel for GELU'."""
    A = _emb(GP.vals((M, K), 21, fl.dtype), K + 8, back=GP.ragged_band(K + 8))
    W = _emb(GP.vals((N, K), 22, fl.dtype, 0.25), K + 8, back=GP.ragged_band(K + 8))
    bias = None if epi == "gbwd" else _vec(N, 23)
    obf = epi != "res"
    ldc = N + 8
    out = _out(M, N, ldc, fl.dtype if obf else torch.float32, back=GP.ragged_band(ldc))
    a = _args(A=A.ptr, B=W.ptr, C=out.ptr, lda=A.ld, ldb=W.ld, ldc=ldc, M=M, N=N, K=K, out_bf16=int(obf))
    z = GP.matmul_ref(A, W)
    ins, outs = [A, W], [out]
    if bias is not None:
        a.bias = bias.ptr
        z = z + bias.t[0].double()
        ins.append(bias)
    ref = z
    if epi.startswith("gelu"):
        a.act = _lib.ACT_GELU
        ref = torch.nn.functional.gelu(z)
    if epi == "gelu_pre":
        pre = _out(M, N, ldc, fl.dtype, back=GP.ragged_band(ldc))
        a.C2 = pre.ptr
        outs.append(pre)
    if epi == "res":
        rmod = 8
        res = _emb(GP.vals((rmod, N), 24), N + 4)
        a.resid, a.ldres, a.res_mod = res.ptr, res.ld, rmod
        ref = z + res.t.double()[torch.arange(M, device=DEV) % rmod]
        ins.append(res)
    if epi == "gbwd":                                                  # C2 is an INPUT here: the saved pre-activation, in C's layout
        pre = _emb(GP.vals((M, N), 25, fl.dtype, 3.0), ldc, back=GP.ragged_band(ldc))
        a.C2, a.act = pre.ptr, _lib.ACT_GELU_BWD
        xg = pre.t.double().clone().requires_grad_(True)
        torch.nn.functional.gelu(xg).backward(z)
        ref = xg.grad
        ins.append(pre)
    _lib.check(L.countr_gemm(C.byref(a), 1, 0, 0, _stream()), "linear")
    _sync()
    if epi == "gbwd":
        GP.assert_close(out.t, ref, HP.bar(fl, 2e-2))
    else:
        GP.assert_close(out.t, ref, HP.bar(fl, 4e-3) if obf else 2e-5, 3e-5)
    if epi == "gelu_pre":
        GP.assert_close(pre.t, z, HP.bar(fl, 4e-3))
    GP.assert_surroundings(outs, ins, epi)


def _ln_producer(L, fl, M, N, K):
    """fp32 out = A W^T + b + residual, with the 16-bit copy (pitch ldc) and the {sum, sum of squares} of every 64-column block."""
    A = _emb(GP.vals((M, K), 61, fl.dtype), K + 8, back=GP.ragged_band(K + 8))
    W = _emb(GP.vals((N, K), 62, fl.dtype, 0.25), K + 8, back=GP.ragged_band(K + 8))
    bias, res = _vec(N, 63), _emb(GP.vals((M, N), 64, scale=2.0), N + 4, back=GP.ragged_band(N + 4))
    ldc = N + 8
    out = _out(M, N, ldc, back=GP.ragged_band(ldc))
    xcopy = _out(M, N, ldc, fl.dtype, back=GP.ragged_band(ldc))
    stats = _out(M, (N // 64) * 2, back=GP.ragged_band((N // 64) * 2))
    a = _args(A=A.ptr, B=W.ptr, C=out.ptr, bias=bias.ptr, resid=res.ptr, lda=A.ld, ldb=W.ld, ldc=ldc, ldres=res.ld, M=M, N=N, K=K,
              ln_xcopy=xcopy.ptr, ln_stats_out=stats.ptr)
    return a, (A, W, bias, res), (out, xcopy, stats)


def _check_ln_producer(fl, ins, outs, M, N, tol, joint=False):
    """joint: both statistics held to 1e-5 of the largest of them together (test_g256_linear_residual_and_layernorm_producer); otherwise
    1e-4 on the sums and 1e-5 on the sums of squares (test_lean_linear_layernorm_folding)."""
    (A, W, bias, res), (out, xcopy, stats) = ins, outs
    GP.assert_close(out.t, GP.matmul_ref(A, W) + bias.t[0].double() + res.t.double(), tol)
    assert torch.equal(xcopy.t, out.t.to(fl.dtype))                   # the copy is the rounded fp32 output
    blocks = out.t.double().reshape(M, N // 64, 64)
    st = stats.t.view(M, N // 64, 2)
    if joint:
        GP.assert_close(st, torch.stack([blocks.sum(-1), (blocks ** 2).sum(-1)], dim=-1), 1e-5)
    else:
        GP.assert_close(st[..., 0], blocks.sum(-1), 1e-4)
        GP.assert_close(st[..., 1], (blocks ** 2).sum(-1), 1e-5)
    GP.assert_surroundings(outs, ins)


def _ln_consumer(L, fl, M, N, K):
    """16-bit out = GELU(rstd (x W^T - mean colsum) + b) from per-64-column row partials: the construction and the bar of
    test_g256_linear_layernorm_consumer, which holds both kernels to it."""
    x = GP.vals((M, K), 131, scale=2.0) + GP.vals((M, 1), 132)
    xs = x.double()
    xb = _emb(x.to(fl.dtype), K + 8, back=GP.ragged_band(K + 8))
    W = _emb(GP.vals((N, K), 133, fl.dtype, 0.25), K + 8, back=GP.ragged_band(K + 8))
    bias = _vec(N, 134)
    st = torch.stack([xs.view(M, K // 64, 64).sum(-1), (xs * xs).view(M, K // 64, 64).sum(-1)], dim=-1).float().reshape(M, -1)
    stats = _emb(st, back=GP.ragged_band(st.shape[1]))
    colsum = _emb(W.t.double().sum(1).float().reshape(1, N))
    ldc = N + 8
    out = _out(M, N, ldc, fl.dtype, back=GP.ragged_band(ldc))
    a = _args(A=xb.ptr, B=W.ptr, C=out.ptr, bias=bias.ptr, lda=xb.ld, ldb=W.ld, ldc=ldc, M=M, N=N, K=K, act=_lib.ACT_GELU, out_bf16=1,
              ln_stats=stats.ptr, ln_colsum=colsum.ptr, ln_nblk=K // 64, ln_eps=1e-6)
    mean = xs.mean(1, keepdim=True).to(DEV)
    rstd = (1.0 / torch.sqrt(xs.var(1, unbiased=False, keepdim=True) + 1e-6)).to(DEV)
    ref = torch.nn.functional.gelu(rstd * (GP.matmul_ref(xb, W) - mean * colsum.t.double()) + bias.t[0].double())
    return a, (xb, W, bias, stats, colsum), (out,), ref


@pytest.mark.parametrize("M,N", [(40, 128), (200, 128), (128 * 129 + 40, 256), (33000, 256)])
@FLS
def test_lean_linear_layernorm_fields_guarded_and_refused_by_the_generic_kernel(hip, monkeypatch, fl, M, N):
    """The LayerNorm producer and consumer epilogues (K = 128: a consumer needs K % 128 == 0), every field embedded or guarded, on the
    128 x 128 form, on the 256 x 128 form and -- the consumer at M = 33000; the producer is a residual epilogue and stays on 256 x 128 -- on
    the 192 x 256 form (LEAN_LINEAR_SHAPES).  That a lean kernel ran is what the fields themselves prove: the generic kernel refuses them,
    loudly, and leaves every buffer as it was."""
    L = _lib_of(hip, fl)
    K = 128
    _env(monkeypatch, LEAN=1, G256=0)
    a, ins, outs = _ln_producer(L, fl, M, N, K)
    _lib.check(L.countr_gemm(C.byref(a), 1, 0, 0, _stream()), "producer")
    _sync()
    _check_ln_producer(fl, ins, outs, M, N, 2e-5)
    c, cins, couts, ref = _ln_consumer(L, fl, M, N, K)
    _lib.check(L.countr_gemm(C.byref(c), 1, 0, 0, _stream()), "consumer")
    _sync()
    GP.assert_close(couts[0].t, ref, HP.bar(fl, 6e-3), 3e-5)
    GP.assert_surroundings(couts, cins)
    _env(monkeypatch, LEAN=0)
    for b, bins, bouts in (_ln_producer(L, fl, M, N, K), _ln_consumer(L, fl, M, N, K)[:3]):
        assert L.countr_gemm(C.byref(b), 1, 0, 0, _stream()) != 0 and b"LayerNorm" in L.countr_last_error()
        _sync()
        assert GP.all_unchanged(*bins, *bouts)


def test_the_poison_is_live_on_the_device(hip, monkeypatch):
    """A positive control: the same launch with K told as the pitch, so that the NaN pad IS part of every row, on the generic kernel and
    on linear.hip.  The product over those columns is NaN by the arithmetic alone; every address stays inside the operands' own rows.
    What a kernel with a lost K-tail mask would do to the cases above, shown on the device without a wrong kernel."""
    dt = torch.bfloat16
    for lean, (M, N, K, pad) in ((0, (136, 72, 40, 8)), (1, (40, 128, 128, 64))):
        _env(monkeypatch, LEAN=lean, G256=0)
        A = _emb(GP.vals((M, K), 1, dt), K + pad, back=GP.ragged_band(K + pad))
        B = _emb(GP.vals((N, K), 2, dt), K + pad, back=GP.ragged_band(K + pad))
        for told_k in (K, K + pad):
            out = _out(M, N, N + 8, dt, back=GP.ragged_band(N + 8))
            a = _args(A=A.ptr, B=B.ptr, C=out.ptr, lda=A.ld, ldb=B.ld, ldc=out.ld, M=M, N=N, K=told_k, out_bf16=1)
            _lib.check(hip.countr_gemm(C.byref(a), 1, 0, 0, _stream()), "gemm")
            _sync()
            assert bool(torch.isfinite(out.t.float()).all()) == (told_k == K), (lean, told_k)
            assert out.intact() and A.unchanged() and B.unchanged()


# ================================================================================================================ gemm256.hip (COUNTR_G256=2)
# N = 256, K = 256: one column tile, the shortest legal K (4 k-tiles: prologue and drain overlap); M = 40 (most staged rows masked), 256 (a
# full tile), 300 (a ragged second tile).  COUNTR_G256=2 takes the kernel wherever it qualifies: N % 256 == 0, K % 128 == 0, K >= 256.
# No query tells this kernel from linear.hip, to which a decline would fall silently: the switch and these conditions are the pin.
@pytest.mark.parametrize("epi", ["bf16", "gelu_pre", "res", "producer", "consumer"])
@pytest.mark.parametrize("M", [40, 256, 300])
@FLS
def test_g256_linear_with_poisoned_surroundings(hip, monkeypatch, fl, M, epi):
    L = _lib_of(hip, fl)
    _env(monkeypatch, LEAN=1, G256=2)
    N = K = 256
    if epi == "producer":
        a, ins, outs = _ln_producer(L, fl, M, N, K)
        _lib.check(L.countr_gemm(C.byref(a), 1, 0, 0, _stream()), "producer")
        _sync()
        _check_ln_producer(fl, ins, outs, M, N, 4e-3, joint=True)     # test_g256_linear_residual_and_layernorm_producer
    elif epi == "consumer":
        c, cins, couts, ref = _ln_consumer(L, fl, M, N, K)
        _lib.check(L.countr_gemm(C.byref(c), 1, 0, 0, _stream()), "consumer")
        _sync()
        GP.assert_close(couts[0].t, ref, HP.bar(fl, 6e-3), 3e-5)
        GP.assert_surroundings(couts, cins)
    else:
        _linear_case(L, fl, M, N, K, epi)


def _conv_case(L, fl, Bn, H, W, Cin, Cout, use_bias):
    """(IM2ROW, ROW) forward on a lean convolution kernel: map between two NaN bands of (2 W + 2 + 256) pixels, weights with a NaN ldb
    pad, output at pitch Cout + 8, gn_rows guarded; launched without and with gn_rows on the same operands, against one fp64 reference.
    countr_gemm_gn_rows says that a kernel with the GroupNorm epilogue -- gemm256.hip or
    linear.hip, never the generic one -- takes the launch.  Bars: test_lean_conv3x3_matches_fp64_and_generic,
    test_conv3x3_groupnorm_row_partials."""
    P = Bn * H * W
    cb = GP.conv_band(W, Cin)
    x = _emb(GP.vals((P, Cin), 51, fl.dtype), front=cb, back=cb)
    w = _emb(GP.vals((Cout, 9 * Cin), 52, fl.dtype, 0.1), 9 * Cin + 8)
    bias = _vec(Cout, 53) if use_bias else None
    ldc = Cout + 8
    ref = GP.conv_ref(x, w, bias.t[0] if use_bias else None, Bn, H, W)
    for use_gn in (False, True):
        out = _out(P, Cout, ldc, fl.dtype, back=GP.ragged_band(ldc))
        rows = _out(P, (Cout // 32) * 2, back=GP.ragged_band((Cout // 32) * 2))
        a = _args(A=x.ptr, B=w.ptr, C=out.ptr, ldb=w.ld, ldc=ldc, M=P, N=Cout, K=9 * Cin, H=H, W=W, Cin=Cin, out_bf16=1)
        if use_bias:
            a.bias = bias.ptr
        a.gn_rows = rows.ptr
        assert L.countr_gemm_gn_rows(C.byref(a), 1, 2, 0) == 1, "the launch would not run on a lean convolution kernel"
        if not use_gn:
            a.gn_rows = None
        _lib.check(L.countr_gemm(C.byref(a), 1, 2, 0, _stream()), "conv")
        _sync()
        GP.assert_close(out.t, ref, HP.bar(fl, 4e-3), what=use_gn)
        if use_gn:
            v = out.t.double().reshape(P, Cout // 32, 32)
            r = rows.t.view(P, Cout // 32, 2)
            GP.assert_close(r[..., 0], v.sum(-1), 2e-6, 1e-6)
            GP.assert_close(r[..., 1], (v * v).sum(-1), 2e-6, 1e-6)
        else:
            assert rows.unchanged()
        GP.assert_surroundings([out, rows], [x, w] + ([bias] if use_bias else []), use_gn)


# (1, 20, 12, 128, 256): a map smaller than one 256-row tile; (3, 10, 10, 256, 256): 300 rows, tiles across image boundaries, a ragged second
# tile.  (23, 64, 64, 128, 256): 368 tiles = one full round of 256 + rem = 112 in [96, 128] -> countr_big_conv runs the head here and the last
# 28672 rows as a tail launch of linear.hip's 128 x 256 form.  It is the smallest such shape: the rule needs >= 256 + 96 tiles of 256 rows
# x 256 columns whatever the width (a wider N only trades rows for column tiles), and Cin = 128 is the smallest this kernel takes.  The split
# rests on that arithmetic alone (368 tiles, full = 256, rem = 112): countr_gemm_gn_rows is 1 with or without the tail launch, and no query
# tells gemm256.hip from linear.hip here.
@pytest.mark.parametrize("Bn,H,W,Cin,Cout", [(1, 20, 12, 128, 256), (3, 10, 10, 256, 256), (23, 64, 64, 128, 256)])
@FLS
def test_g256_convolution_on_an_embedded_map(hip, monkeypatch, fl, Bn, H, W, Cin, Cout):
    _env(monkeypatch, LEAN=1, LEAN_CONV=1, G256=2)
    _conv_case(_lib_of(hip, fl), fl, Bn, H, W, Cin, Cout, True)


# COUNTR_G256=0: linear.hip alone, which takes maps of more than 256 tiles of 128 x 128.  (2, 96, 96, 128, 256): 144 x 2 = 288 tiles,
# N % 256 == 0 -> the 128 x 256 form.  (1, 182, 182, 64, 128): 259 x 1 tiles, N % 256 != 0 -> the 256 x 128 form, a ragged last tile.
@pytest.mark.parametrize("use_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("Bn,H,W,Cin,Cout", [(2, 96, 96, 128, 256), (1, 182, 182, 64, 128)])
@FLS
def test_lean_convolution_on_an_embedded_map(hip, monkeypatch, fl, Bn, H, W, Cin, Cout, use_bias):
    _env(monkeypatch, LEAN=1, LEAN_CONV=1, G256=0)
    _conv_case(_lib_of(hip, fl), fl, Bn, H, W, Cin, Cout, use_bias)


# ================================================================================================================ lean wgrad (conv_wgrad.hip)
# The small shapes test_lean_conv_wgrad_matches_fp64_and_generic names, each with a slab count: one slab; several; more slabs than
# k-tiles (P = 384 pixels: six 64-pixel or four 96-pixel k-tiles, eight slabs).  Form 3 applies where W % 64 == 0 or W % 96 == 0 and falls
# back to 2, form 2 applies where Cin % 256 == 0 and falls back to 1: a requested form that would fall back repeats another case and is
# left out, but for one (form 3 asked of the 16-pixel rows, which runs form 1).  countr_gemm_rowsum_slabs tells the lean kernel from the
# generic one (splitk slabs) and form 3 from forms 1 and 2; countr_gemm_tiles tells forms 1 and 2 apart.
CWG_SHAPES = [(2, 8, 16, 128, 128, 1), (3, 5, 64, 256, 128, 4), (1, 4, 96, 128, 128, 3), (2, 2, 96, 256, 128, 8), (2, 3, 192, 128, 128, 1)]


def _cwg_took(form, W, Cin):
    return 3 if (form == 3 and (W % 64 == 0 or W % 96 == 0)) else 2 if (form >= 2 and Cin % 256 == 0) else 1


CWG_CASES = [(f,) + s for s in CWG_SHAPES for f in (1, 2, 3) if _cwg_took(f, s[2], s[3]) == f] + [(3,) + CWG_SHAPES[0]]


@pytest.mark.parametrize("with_bias", [True, False], ids=["rowsum", "norowsum"])
@pytest.mark.parametrize("form,Bn,H,W,Cin,Cout,sk", CWG_CASES)
@FLS
def test_lean_conv_wgrad_on_embedded_maps(hip, monkeypatch, fl, form, Bn, H, W, Cin, Cout, sk, with_bias):
    L = _lib_of(hip, fl)
    _env(monkeypatch, LEAN=1, LEAN_WGRAD=1, LEAN_WGRAD_FORM=form)
    P, N = Bn * H * W, 9 * Cin
    cb = GP.conv_band(W, Cin)
    x = _emb(GP.vals((P, Cin), 72, fl.dtype), front=cb, back=cb)
    dy = _emb(GP.vals((P, Cout), 71, fl.dtype), front=GP.conv_band(W, Cout), back=GP.conv_band(W, Cout))
    a = _args(A=dy.ptr, B=x.ptr, lda=Cout, ldc=N, M=Cout, N=N, K=P, H=H, W=W, Cin=Cin, splitk=sk)
    slabs = L.countr_gemm_rowsum_slabs(C.byref(a), 1, 1, 3)
    took = _cwg_took(form, W, Cin)
    assert slabs == sk * (3 * (Cin // 128) if took == 3 else N // 128), "not on the lean kernel (the generic one writes splitk slabs)"
    tiles = (Cout // 128) * (3 * (Cin // 128) if took == 3 else N // (128 * took))
    assert L.countr_gemm_tiles(C.byref(a), 1, 1, 3) == tiles, "not the form the case is about"
    part = _out(sk, Cout * N, back=Cout * N)
    rs = _out(slabs, Cout, back=GP.ragged_band(Cout))
    a.partial = part.ptr
    if with_bias:
        a.rowsum_partial, a.rowsum_slabs = rs.ptr, slabs
    _lib.check(L.countr_gemm(C.byref(a), 1, 1, 3, _stream()), "wgrad")
    _sync()
    gw, gb = GP.conv_wgrad_ref(dy, x, Bn, H, W)
    GP.assert_close(part.t.double().sum(0).view(Cout, N), gw, 2e-5, 1e-9)        # test_lean_conv_wgrad_matches_fp64_and_generic
    assert bool(torch.isfinite(part.t).all())
    if with_bias:
        GP.assert_close(rs.t.double().sum(0), gb, 2e-5, 1e-9)
    else:
        assert rs.unchanged()
    GP.assert_surroundings([part, rs], [dy, x])


def _lwgrad_problem(L, fl, R, N, K, sk, seed, with_bias=True):
    """dW [N, K] = dy^T x: dy is the middle third of a packed gradient [R, 3 N] whose other thirds are NaN, x has a row 8 wider than K; a
    k-tile of NaN rows (and more) behind both."""
    g = GP.packed(R, 3, N, (1,), seed, fl.dtype, DEV, back=GP.ragged_band(3 * N))
    dyv, dyp = g.cols_slice(1, N)
    x = _emb(GP.vals((R, K), seed + 5, fl.dtype), K + 8, back=GP.ragged_band(K + 8))
    a = _args(A=dyp, B=x.ptr, lda=g.ld, ldb=x.ld, ldc=K, M=N, N=K, K=R, splitk=sk)
    slabs = L.countr_gemm_rowsum_slabs(C.byref(a), 1, 1, 1)
    # the lean kernel writes splitk x K / 128 slabs, the generic one splitk: the query tells them apart where K > 128 only
    assert slabs == sk * (K // 128), "not on the lean kernel (the generic one writes splitk slabs)"
    part = _out(sk, N * K, back=N * K)
    rs = _out(slabs, N, back=GP.ragged_band(N))
    a.partial = part.ptr
    if with_bias:
        a.rowsum_partial, a.rowsum_slabs = rs.ptr, slabs
    return a, (g, x), (part, rs), dyv


def _check_lwgrad(ins, outs, dyv, N, K, with_bias=True):
    (g, x), (part, rs) = ins, outs
    GP.assert_close(part.t.double().sum(0).view(N, K), dyv.double().t() @ x.t.double(), 2e-5, 1e-9)   # test_lean_linear_wgrad_matches_fp64_and_generic
    if with_bias:
        GP.assert_close(rs.t.double().sum(0), dyv.double().sum(0), 2e-5, 1e-9)
    else:
        assert rs.unchanged()
    GP.assert_surroundings(outs, ins)


# (64, 128, 128): one k-tile, one tile; (192, 256, 128): three k-tiles in two slabs (the second ends early) and in five (two empty slabs).
# At K = 128 the lean kernel and the generic one write the same number of row-sum slabs, so countr_gemm_rowsum_slabs cannot tell them
# apart: those shapes are pinned by COUNTR_LEAN / COUNTR_LEAN_LWGRAD and cwg_form's conditions alone (M, N % 128 == 0, rows % 64 == 0, ldc == N,
# pitches % 8 == 0, 16-byte aligned pointers).  (192, 256, 256) is the same launch two column tiles wide, where the query does tell: 2 sk
# slabs on the lean kernel, sk on the generic one.
@pytest.mark.parametrize("with_bias", [True, False], ids=["rowsum", "norowsum"])
@pytest.mark.parametrize("R,N,K,sk", [(64, 128, 128, 1), (192, 256, 128, 2), (192, 256, 128, 5), (192, 256, 256, 2)])
@FLS
def test_lean_linear_wgrad_out_of_a_poisoned_packed_gradient(hip, monkeypatch, fl, R, N, K, sk, with_bias):
    L = _lib_of(hip, fl)
    _env(monkeypatch, LEAN=1, LEAN_LWGRAD=1)
    monkeypatch.delenv("COUNTR_LEAN_WGRAD_FORM", raising=False)
    a, ins, outs, dyv = _lwgrad_problem(L, fl, R, N, K, sk, 81, with_bias)
    _lib.check(L.countr_gemm(C.byref(a), 1, 1, 1, _stream()), "linear wgrad")
    _sync()
    _check_lwgrad(ins, outs, dyv, N, K, with_bias)


@pytest.mark.parametrize("shapes", [[(128, 128), (256, 128)], [(128, 256), (256, 256), (128, 256)]], ids=["two_128", "three_256"])
@FLS
def test_grouped_linear_wgrads_out_of_poisoned_packed_gradients(hip, monkeypatch, fl, shapes):
    """countr_gemm_group: two problems on 128-column tiles, three on 256-column tiles (every K % 256 == 0); countr_gemm_group_tiles > 0
    says that they run as ONE launch of the grouped form (0 = one by one), and is all that pins two_128; in three_256 the row-sum slab
    count tells the lean kernel from the generic one as well."""
    L = _lib_of(hip, fl)
    _env(monkeypatch, LEAN=1, LEAN_LWGRAD=1)
    monkeypatch.delenv("COUNTR_LEAN_WGRAD_FORM", raising=False)
    R, sk, n = 192, 2, len(shapes)
    arr = (_lib.GemmArgs * n)()
    probs = []
    for i, (N, K) in enumerate(shapes):
        a, ins, outs, dyv = _lwgrad_problem(L, fl, R, N, K, sk, 91 + 10 * i)
        C.memmove(C.byref(arr[i]), C.byref(a), C.sizeof(a))
        probs.append((ins, outs, dyv, N, K))
    wide = all(K % 256 == 0 for _, K in shapes)
    assert L.countr_gemm_group_tiles(arr, n, 1, 1, 1) == sum((N // 128) * (K // (256 if wide else 128)) for N, K in shapes)
    _lib.check(L.countr_gemm_group(arr, n, 1, 1, 1, _stream()), "group")
    _sync()
    for p in probs:
        _check_lwgrad(*p)


# ================================================================================================================ reductions (gemm.hip)
# counts that are no multiple of a 256-thread block: 37 x 36 / 4 = 333 four-column threads; 40 x 72 = 2880 elements; 1001 (scalar path: no
# multiple of 4 either), 1000 (16-byte path), 70 columns of 16 (wide path)
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("obf", [0, 1], ids=["f32out", "halfout"])
@FLS
def test_splitk_finish_with_a_poisoned_next_slab(hip, fl, obf, with_bias):
    L = _lib_of(hip, fl)
    sk, M, N = 3, 37, 36
    parts = GP.slabs(GP.vals((sk, M * N), 31), DEV)
    bias = _vec(N, 33) if with_bias else None
    out = _out(M, N, dtype=fl.dtype if obf else torch.float32)
    _lib.check(L.countr_splitk_finish(parts.ptr, out.ptr, bias.ptr if with_bias else None, sk, M, N, obf, _stream()), "finish")
    _sync()
    ref = parts.t.double().sum(0).view(M, N) + (bias.t[0].double() if with_bias else 0.0)
    GP.assert_close(out.t, ref, HP.bar(fl, 8e-3) if obf else 2e-5)               # test_splitk_finish_matches_unsplit_conv
    GP.assert_surroundings([out], [parts] + ([bias] if with_bias else []))


@pytest.mark.parametrize("with_rowsum", [False, True], ids=["plain", "rowsums"])
@pytest.mark.parametrize("acc", [0, 1], ids=["store", "accumulate"])
@pytest.mark.parametrize("taps", [0, 9], ids=["flat", "taps"])
def test_splitk_reduce_with_a_poisoned_next_slab(hip, taps, acc, with_rowsum):
    sk, M, N = 3, 40, 72                                              # N = 9 taps x 8 channels
    parts = GP.slabs(GP.vals((sk, M * N), 35), DEV)
    rsp = GP.slabs(GP.vals((sk, M), 36), DEV)
    out0, rso0 = GP.vals((1, M * N), 37), GP.vals((1, M), 38)
    out = _emb(out0) if acc else _out(1, M * N)
    rso = _emb(rso0) if acc else _out(1, M)
    _lib.check(hip.countr_splitk_reduce(parts.ptr, out.ptr, sk, M, N, taps, acc, rsp.ptr if with_rowsum else None,
                                        rso.ptr if with_rowsum else None, _stream()), "reduce")
    _sync()
    ref = parts.t.double().sum(0).view(M, N)
    if taps:                                                          # [co][tap][ci] -> [co][ci][tap]
        ref = ref.view(M, taps, N // taps).transpose(1, 2).reshape(M, N)
    if acc:
        ref = ref + out0.double().view(M, N).to(DEV)
    GP.assert_close(out.t.view(M, N), ref, 2e-4)                      # test_gemm_batched_and_splitk
    if with_rowsum:
        GP.assert_close(rso.t[0], rsp.t.double().sum(0) + (rso0[0].double().to(DEV) if acc else 0.0), 1e-4, 1e-4)
    else:
        assert rso.unchanged()
    GP.assert_surroundings([out, rso], [parts, rsp])


def test_reduce_table_paths_with_poisoned_next_slabs(hip):
    """countr_reduce_table: the scalar path (with and without the tap permutation, accumulate on and off), the 16-byte path (bit 34: count,
    stride and pointers multiples of 4 floats) and the wide path (bit 33: many strided slabs, as the LayerNorm dgamma / dbeta partials)."""
    entries, blk, checks, ins, outs = [], 0, [], [], []
    for (sk, M, N, taps, acc, vec4) in ((3, 1, 1001, 0, 0, 0), (7, 8, 9 * 8, 9, 1, 0), (5, 1, 1000, 0, 0, 1), (6, 5, 9 * 8, 9, 1, 1), (4, 1, 1000, 0, 1, 1)):
        parts = GP.slabs(GP.vals((sk, M * N), 40 + sk), DEV)
        out0 = GP.vals((1, M * N), 50 + sk)
        out = _emb(out0) if acc else _out(1, M * N)
        ref = parts.t.double().sum(0).view(M, N)
        if taps:
            ref = ref.view(M, taps, N // taps).transpose(1, 2).reshape(M, N)
        ref = ref.reshape(-1) + (out0[0].double().to(DEV) if acc else 0.0)
        entries.append([parts.ptr, out.ptr, sk | (acc << 32) | (vec4 << 34), M * N, M * N, N, taps, blk])
        blk += -(-(M * N) // (1024 if vec4 else 256))
        ins.append(parts); outs.append(out); checks.append((out, ref))
    for (nb, D, acc) in ((40, 70, 0), (33, 70, 1)):                   # workspace rows {dgamma[D], dbeta[D]}: the halves are each other's neighbours
        ws = _emb(GP.vals((nb, 2 * D), 60 + nb), back=2 * D)
        for half in (0, 1):
            out0 = GP.vals((1, D), 70 + nb + half)
            out = _emb(out0) if acc else _out(1, D)
            ref = ws.t[:, half * D:(half + 1) * D].double().sum(0) + (out0[0].double().to(DEV) if acc else 0.0)
            entries.append([ws.ptr + 4 * half * D, out.ptr, nb | (acc << 32) | (1 << 33), 2 * D, D, 0, 0, blk])
            blk += -(-D // 16)
            ins.append(ws); outs.append(out); checks.append((out, ref))
    firsts = [e[7] for e in entries] + [blk]
    owner = torch.cat([torch.full((firsts[i + 1] - firsts[i],), i, dtype=torch.int32) for i in range(len(entries))])
    if owner.numel() & 1:
        owner = torch.cat([owner, owner.new_zeros(1)])
    tab = torch.cat([torch.tensor(entries, dtype=torch.int64).reshape(-1), owner.view(torch.int64)]).to(DEV)
    _lib.check(hip.countr_reduce_table(tab.data_ptr(), len(entries), blk, _stream()), "reduce_table")
    _sync()
    for i, (out, ref) in enumerate(checks):
        GP.assert_close(out.t[0], ref, 0.0, 1e-5 * max(ref.abs().max().item(), 1.0), i)     # test_reduce_table_matches_individual_reductions
    GP.assert_surroundings(outs, ins)
    assert GUARD % 4 == 0                                             # (the 16-byte path's pointers: bands keep them aligned)
