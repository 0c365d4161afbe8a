"""Shape edges of the small HIP kernels through the C ABI, each against an fp64 reference of the same operation on the same (already
rounded) inputs: softmax rows (ragged 64-column groups, n = 1, the n = 1024 limit, a row pitch), cross attention from the packed k | v
buffer, column sums (ragged column tile, accumulate 0 / 1), the grid-stride trip of the GELU backward, the scalar paths of the masked MSE
and the patch gather, AdamW ranges with gaps, the per-pixel first exemplar conv -- and the refusals of their launchers.

The inputs, references and assertions live in tests/kedges.py; tests/test_kernel_edges_cpu.py shows on the CPU that an fp32 emulation passes
each assertion and wrong variants do not.  Every output is allocated between guard bands that must come back bit-identical.  The cases
that only widen an existing test (cross attention S = 2, 4..7; LayerNorm D = 4 .. 2048 and small row counts) are in
tests/test_kernels_gpu.py."""
import ctypes as C

import pytest
import torch

import attnref as AR
import halfprec as HP
import kedges as KE
from countr_amd import _lib
from oracle import countr_ref as R
from test_kernels_gpu import DT, F32_TOL, P, relerr, st

pytestmark = pytest.mark.gpu

assert DT == KE.DT
MODES = pytest.mark.parametrize("tdt,code,tol", DT)


def G(shape, dtype=torch.float32, **kw):
    return KE.Guarded(shape, dtype, "cuda", **kw)


def refused(hip, rc, name):
    """A refusal: non-zero return code and an error text that names the function."""
    return rc != 0 and name.encode() in hip.countr_last_error()


# ---------------------------------------------------------------------------------------------------------------- softmax
@pytest.mark.parametrize("family", KE.SOFTMAX_FAMILIES)
@pytest.mark.parametrize("rows,n", KE.SOFTMAX_SHAPES)
@MODES
def test_softmax_fwd_bwd_shapes(hip, tdt, code, tol, rows, n, family):
    hip = HP.library(tdt, hip)
    s = KE.softmax_scores(family, rows, n)
    sd = s.cuda()
    p = G((rows, n), tdt)
    _lib.check(hip.countr_softmax_fwd(P(sd), P(p.t), rows, n, code, st()))
    KE.assert_softmax(p.t, s, n, tdt, tol)
    dp = KE.softmax_dp(rows, n)
    dpd = dp.cuda()
    ds = G((rows, n), tdt)
    _lib.check(hip.countr_softmax_bwd(P(p.t), P(dpd), P(ds.t), rows, n, KE.SOFTMAX_BWD_SCALE, code, st()))
    KE.assert_softmax_bwd(ds.t, p.t, dp, KE.SOFTMAX_BWD_SCALE, tdt, tol)
    assert KE.all_intact(p, ds)


@pytest.mark.parametrize("family", KE.SOFTMAX_FAMILIES)
@pytest.mark.parametrize("n,ld", KE.SOFTMAX_LD)
@MODES
def test_softmax_fwd_row_pitch_writes_exact_zeros_behind_n(hip, tdt, code, tol, n, ld, family):
    """countr_softmax_fwd_ld: columns n .. ld - 1 of the scores hold 1e30 and are never read into the statistics; the same columns of P are
    exact zeros (the unfused PV product multiplies them with rows of the next image)."""
    hip = HP.library(tdt, hip)
    rows = KE.SOFTMAX_LD_ROWS
    s = KE.softmax_scores(family, rows, n, ld)
    sd = G((rows, ld), fill=KE.SOFTMAX_PAD, body=s)           # (the scores are read with a pitch: finite values around them)
    p = G((rows, ld), tdt)
    _lib.check(hip.countr_softmax_fwd_ld(P(sd.t), P(p.t), rows, n, ld, code, st()))
    KE.assert_softmax(p.t, s, n, tdt, tol)
    assert p.intact() and sd.unchanged()


@MODES
def test_softmax_refusals_leave_the_output_untouched(hip, tdt, code, tol):
    hip = HP.library(tdt, hip)
    rows = 4
    sd = torch.zeros((rows, 1032), device="cuda")
    pin = torch.zeros((rows, 1025), device="cuda", dtype=tdt)
    p, ds = G((rows, 1032), tdt), G((rows, 1025), tdt)
    assert refused(hip, hip.countr_softmax_fwd(P(sd), P(p.t), rows, 1025, code, st()), "countr_softmax_fwd: need")          # n = 1025
    assert refused(hip, hip.countr_softmax_bwd(P(pin), P(sd), P(ds.t), rows, 1025, 0.25, code, st()), "countr_softmax_bwd")   # n = 1025
    assert refused(hip, hip.countr_softmax_fwd_ld(P(sd), P(p.t), rows, 64, 63, code, st()), "countr_softmax_fwd: need")       # ld < n
    assert refused(hip, hip.countr_softmax_fwd_ld(P(sd), P(p.t), rows, 1000, 1032, code, st()), "countr_softmax_fwd: need")   # ld = 1032
    torch.cuda.synchronize()
    assert p.unchanged() and ds.unchanged()


# ---------------------------------------------------------------------------------------------------------------- cross attention
def _xattn(hip, tdt, code, q, do, k, v, ldkv, B, N, S):
    """Forward and backward from k / v views at row pitch ldkv; returns the outputs and their guards."""
    D, Hh, scale = KE.XATTN_D, KE.XATTN_HEADS, 32 ** -0.5
    h16 = KE.half_of(tdt)
    g = {"out": G((B, N, D), tdt), "dq": G((B, N, D), tdt), "dk": G((B, S, D)), "dv": G((B, S, D)),
         "dkb": G((B, S, D), h16), "dvb": G((B, S, D), h16), "ws": G(hip.countr_xattn_bwd_workspace_floats(B, N, S, D))}
    _lib.check(hip.countr_xattn_fwd(P(q), P(k), P(v), P(g["out"].t), B, N, S, D, Hh, ldkv, scale, code, st()))
    _lib.check(hip.countr_xattn_bwd(P(q), P(k), P(v), P(do), P(g["dq"].t), P(g["dk"].t), P(g["dv"].t), P(g["ws"].t), B, N, S, D, Hh, ldkv,
                                    scale, code, P(g["dkb"].t), P(g["dvb"].t), st()))
    torch.cuda.synchronize()
    assert KE.all_intact(*g.values())
    return {n: x.t for n, x in g.items()}


@pytest.mark.parametrize("S", KE.XATTN_PACKED_S)
@MODES
def test_cross_attention_from_the_packed_kv_buffer(hip, tdt, code, tol, S):
    """The engine's default layout: k | v are the column halves of one [B * S, 1024] buffer, ldkv = 1024.  Bit-identical to the same case
    from separate contiguous k and v (ldkv = 512), and within the bars of _cross_attention_fwd_bwd against fp64."""
    hip = HP.library(tdt, hip)
    B, N, D, Hh, scale = KE.XATTN_B, KE.XATTN_PACKED_N, KE.XATTN_D, KE.XATTN_HEADS, 32 ** -0.5
    q, k, v, do = KE.xattn_inputs(N, S, tdt)
    qd, dod = q.cuda(), do.cuda()
    kv = G((B * S, 2 * D), tdt, fill=1.0, body=KE.pack_kv(k, v))           # (read with a pitch: finite values around it)
    packed = _xattn(hip, tdt, code, qd, dod, kv.t[:, :D], kv.t[:, D:], 2 * D, B, N, S)
    assert kv.unchanged()
    apart = _xattn(hip, tdt, code, qd, dod, k.cuda(), v.cuda(), D, B, N, S)
    for n in ("out", "dq", "dk", "dv", "dkb", "dvb"):
        assert torch.equal(KE.bits(packed[n]), KE.bits(apart[n])), n
    h16 = KE.half_of(tdt)
    assert torch.equal(packed["dkb"], packed["dk"].to(h16)) and torch.equal(packed["dvb"], packed["dv"].to(h16))
    vals, comp = AR.cross_attention(q, k, v, do, Hh, scale)
    ref = KE.xattn_reference(q, k, v, do)
    assert relerr(packed["out"], ref["out"]) < tol and relerr(packed["dq"], ref["dq"]) < tol
    assert relerr(packed["dk"], ref["dk"]) < 1e-3 and relerr(packed["dv"], ref["dv"]) < 1e-3
    fl = HP.BY_DTYPE[tdt] if code else None
    for name in ("out", "dq"):
        AR.assert_attn_rows(packed[name].reshape(B, N, Hh, 32), vals[name], comp[name][0], fl, AR.K_ONE_ROUNDING, F32_TOL, comp[name][1], name)
    for name in ("dk", "dv"):
        AR.assert_attn_rows(packed[name].reshape(B, S, Hh, 32), vals[name], comp[name][0], None, 0, F32_TOL, None, name)


# ---------------------------------------------------------------------------------------------------------------- LayerNorm
@MODES
def test_layernorm_fwd_refusals_leave_the_output_untouched(hip, tdt, code, tol):
    hip = HP.library(tdt, hip)
    rows = 3
    x = torch.zeros((rows, 2052), device="cuda")
    y, mean, rstd = G((rows, 2052), tdt), G(rows), G(rows)
    for r, D in ((rows, 2052), (rows, 6), (0, 512)):
        assert refused(hip, hip.countr_layernorm_fwd(P(x), P(x), P(x), P(y.t), P(mean.t), P(rstd.t), r, D, 1e-6, code, st()), "countr_layernorm_fwd"), (r, D)
    torch.cuda.synchronize()
    assert y.unchanged() and mean.unchanged() and rstd.unchanged()


# ---------------------------------------------------------------------------------------------------------------- column sums
@pytest.mark.parametrize("M,N", KE.COLSUM_SHAPES)
@MODES
def test_colsum_shapes_both_accumulate_modes(hip, tdt, code, tol, M, N):
    """N = 24: two column tiles of two 8-column vectors, half of the second empty; 520, 2056: a ragged last tile of 32; M below the row
    lanes of a block (parts clipped to 1); accumulate = 0 overwrites a sentinel."""
    hip = HP.library(tdt, hip)
    x = KE.colsum_input(M, N, tdt)
    xd = x.cuda()
    ws = G(hip.countr_colsum_nparts() * N)
    for acc, start in ((0, KE.COLSUM_SENTINEL), (1, 1.0)):
        before = torch.full((N,), start)
        out = G(N, body=before)
        _lib.check(hip.countr_colsum(P(xd), P(out.t), P(ws.t), M, N, code, acc, st()))
        KE.assert_colsum(out.t, x, acc, before)
        assert out.intact() and ws.intact(), acc


@MODES
def test_colsum_refuses_a_width_that_is_no_multiple_of_8(hip, tdt, code, tol):
    hip = HP.library(tdt, hip)
    xd = torch.zeros((4, 16), device="cuda", dtype=tdt)
    out, ws = G(16), G(hip.countr_colsum_nparts() * 16)
    assert refused(hip, hip.countr_colsum(P(xd), P(out.t), P(ws.t), 4, 12, code, 0, st()), "countr_colsum")
    torch.cuda.synchronize()
    assert out.unchanged() and ws.unchanged()


# ---------------------------------------------------------------------------------------------------------------- GELU backward
@pytest.mark.parametrize("n", KE.GELU_N)
@MODES
def test_gelu_bwd_small_sizes(hip, tdt, code, tol, n):
    hip = HP.library(tdt, hip)
    pre, dh = KE.gelu_inputs(n, tdt)
    pred, dhd = pre.cuda(), dh.cuda()
    out = G(n, tdt)
    _lib.check(hip.countr_gelu_bwd(P(dhd), P(pred), P(out.t), n, code, st()))
    KE.assert_gelu_bwd(out.t.cpu(), pre, dh, tol)
    assert out.intact()


def test_gelu_bwd_grid_stride_trip_past_the_block_cap(hip):
    """fp32, n just past 8192 blocks x 256 threads x 8: the first 257 threads take a second trip.  All elements are compared; the fp64
    reference is evaluated on the device."""
    tdt, code, tol = DT[0]
    n = KE.GELU_PAST_CAP
    pre, dh = KE.gelu_inputs(n, tdt)
    pred, dhd = pre.cuda(), dh.cuda()
    out = G(n, tdt)
    _lib.check(hip.countr_gelu_bwd(P(dhd), P(pred), P(out.t), n, code, st()))
    KE.assert_gelu_bwd(out.t, pred, dhd, tol)
    assert bool(torch.isfinite(out.t).all()) and out.intact()


@MODES
def test_gelu_bwd_refuses_a_size_that_is_no_multiple_of_8(hip, tdt, code, tol):
    hip = HP.library(tdt, hip)
    x = torch.zeros(16, device="cuda", dtype=tdt)
    out = G(16, tdt)
    assert refused(hip, hip.countr_gelu_bwd(P(x), P(x), P(out.t), 12, code, st()), "countr_gelu_bwd")
    torch.cuda.synchronize()
    assert out.unchanged()


# ---------------------------------------------------------------------------------------------------------------- masked MSE
def _masked_mse(L, pred, gt, mask, gs, off, with_dpred=True):
    """One call with `pred` `off` floats off a 16-byte boundary (off != 0: the scalar path whatever HW is); returns sums, dpred."""
    B, HW = pred.shape
    pd = G((B, HW), fill=0.5, body=pred, lead=off)
    assert pd.t.data_ptr() % 16 == 4 * off
    gd, md = gt.cuda(), mask.cuda()
    dp, sums, ws = G((B, HW)), G(1 + 2 * B), G(L.countr_masked_mse_workspace_floats(B))
    _lib.check(L.countr_masked_mse(P(pd.t), P(gd), P(md), P(dp.t) if with_dpred else None, P(sums.t), P(ws.t), B, HW, gs, st()))
    torch.cuda.synchronize()
    assert KE.all_intact(dp, sums, ws) and pd.unchanged()
    assert with_dpred or dp.unchanged()
    return sums.t, dp.t


@pytest.mark.parametrize("gs", KE.MSE_SCALES)
@pytest.mark.parametrize("B,HW,off", KE.MSE_CASES)
@pytest.mark.parametrize("fl", HP.FLAVOURS, ids=HP.FLAVOUR_IDS)
def test_masked_mse_shapes_scalar_path_and_grad_scale(hip, fl, B, HW, off, gs):
    """HW = 4: one float4, 63 of the 64 blocks of an image contribute zeros; 7, 1023: HW % 4 != 0, the scalar path; 64 * 256 * 4 + 4: one
    thread takes a second trip; (3, 4096) with pred one float off a 16-byte boundary: the scalar path at HW % 4 == 0, compared with the
    vector path on the same data.  The kernel is fp32 in both libraries."""
    L = HP.library(fl, hip)
    pred, gt, mask = KE.mse_inputs(B, HW)
    ref = KE.mse_reference(pred, gt, mask, gs)
    sums, dp = _masked_mse(L, pred, gt, mask, gs, off)
    KE.assert_masked_mse(sums, dp, ref)
    sums0, _ = _masked_mse(L, pred, gt, mask, gs, off, with_dpred=False)         # dpred = NULL: the same sums
    assert torch.equal(sums0, sums)
    if off:
        sums_v, dp_v = _masked_mse(L, pred, gt, mask, gs, 0)                     # the vector path on the same data
        KE.assert_masked_mse(sums_v, dp_v, ref)
        assert relerr(sums, sums_v) < 1e-5 and relerr(dp, dp_v) < 1e-5


# ---------------------------------------------------------------------------------------------------------------- AdamW
def _adam_arrays(ranges, wds, groups):
    n = len(ranges)
    return ((C.c_int64 * n)(*[a for a, _ in ranges]), (C.c_int64 * n)(*[b for _, b in ranges]), (C.c_float * n)(*wds),
            (C.c_int * n)(*groups) if groups is not None else None)


@pytest.mark.parametrize("fl", HP.FLAVOURS, ids=HP.FLAVOUR_IDS)
def test_adamw_ranges_with_gaps_unaligned_starts_and_a_one_element_range(hip, fl):
    """Three steps of the device-hyper form (counter group g joins at step g + 1, so the three groups' bias corrections differ), one of the
    scalar form.  Inside the ranges: torch.optim.AdamW in fp64; outside: p, m, v and the 16-bit shadow keep their bits; the gradient
    norm is that of the ranges stepped."""
    L = HP.library(fl, hip)
    n = KE.ADAM_N
    inside = KE.adam_inside()
    p0 = KE.rnd((n,), 31)
    grads = [KE.rnd((n,), 41 + i) for i in range(3)]
    steps_of_range = [set(range(KE.ADAM_GROUP_START[g] - 1, 3)) for g in KE.ADAM_GROUPS]
    refs = KE.adam_reference(p0, grads, steps_of_range)
    m0, v0 = torch.full((n,), 0.25), torch.full((n,), 0.5)          # outside the ranges: values that must survive; inside: zero
    m0[inside] = 0.0; v0[inside] = 0.0
    sh0 = torch.full((n,), 3.0).to(fl.dtype)
    p, m, v, sh = G(n, body=p0), G(n, body=m0), G(n, body=v0), G(n, fl.dtype, body=sh0)
    gn = G(L.countr_adamw_gnorm_floats(), body=torch.zeros(L.countr_adamw_gnorm_floats()))
    bc = lambda t: (1 - KE.ADAM_B1 ** max(t, 1), 1 - KE.ADAM_B2 ** max(t, 1))
    for i, g in enumerate(grads):
        step = i + 1
        live = [r for r, gr in enumerate(KE.ADAM_GROUPS) if KE.ADAM_GROUP_START[gr] <= step]
        starts, ends, wds, groups = _adam_arrays([KE.ADAM_RANGES[r] for r in live], [KE.ADAM_WDS[r] for r in live], [KE.ADAM_GROUPS[r] for r in live])
        t = [step - s + 1 for s in KE.ADAM_GROUP_START]
        hyper = torch.tensor([KE.ADAM_LR, *bc(t[0]), 1.0, *bc(t[1]), *bc(t[2])], device="cuda")
        gd = g.cuda()
        _lib.check(L.countr_adamw_step(P(p.t), P(gd), P(m.t), P(v.t), P(sh.t), len(live), starts, ends, wds, groups, None, 0.0, KE.ADAM_B1,
                                       KE.ADAM_B2, KE.ADAM_EPS, 0, 0.0, P(hyper), P(gn.t), st()))
        KE.assert_adam(p.t, refs[i], p0)
        want = sum(g[a:b].double().pow(2).sum() for a, b in (KE.ADAM_RANGES[r] for r in live)).sqrt().item()
        assert abs(gn.t[0].item() - want) < 1e-5 * want, step
    mc, vc, sc = m.t.cpu(), v.t.cpu(), sh.t.cpu()
    assert torch.equal(KE.bits(mc[~inside]), KE.bits(m0[~inside])) and torch.equal(KE.bits(vc[~inside]), KE.bits(v0[~inside]))
    assert torch.equal(KE.bits(sc[~inside]), KE.bits(sh0[~inside]))
    assert torch.equal(sc[inside], p.t.cpu()[inside].to(fl.dtype))              # the shadow IS the rounding of the stored parameter
    assert bool((mc[inside] != 0).all()) and bool((vc[inside] > 0).all())
    assert KE.all_intact(p, m, v, sh, gn)
    # scalar form: every range at `step` = 1, no groups, no shadow, no norm
    p2, m2, v2 = G(n, body=p0), G(n, body=m0), G(n, body=v0)
    starts, ends, wds, _ = _adam_arrays(KE.ADAM_RANGES, KE.ADAM_WDS, None)
    g0 = grads[0].cuda()
    _lib.check(L.countr_adamw_step(P(p2.t), P(g0), P(m2.t), P(v2.t), None, len(KE.ADAM_RANGES), starts, ends, wds, None, None,
                                   KE.ADAM_LR, KE.ADAM_B1, KE.ADAM_B2, KE.ADAM_EPS, 1, 1.0, None, None, st()))
    KE.assert_adam(p2.t, KE.adam_reference(p0, grads[:1], [{0}] * len(KE.ADAM_RANGES))[0], p0)
    assert torch.equal(KE.bits(m2.t.cpu()[~inside]), KE.bits(m0[~inside])) and torch.equal(KE.bits(v2.t.cpu()[~inside]), KE.bits(v0[~inside]))
    assert KE.all_intact(p2, m2, v2)


def test_adamw_takes_16_ranges_and_refuses_17(hip):
    n = 400
    p0, g = KE.rnd((n,), 31), KE.rnd((n,), 41)
    gd = g.cuda()
    for nr in (16, 17):
        ranges = [(10 * i + 1, 10 * i + 2) for i in range(nr)]
        starts, ends, wds, _ = _adam_arrays(ranges, [0.05] * nr, None)
        p, m, v = G(n, body=p0), G(n, body=torch.zeros(n)), G(n, body=torch.zeros(n))
        rc = hip.countr_adamw_step(P(p.t), P(gd), P(m.t), P(v.t), None, nr, starts, ends, wds, None, None, KE.ADAM_LR, KE.ADAM_B1,
                                   KE.ADAM_B2, KE.ADAM_EPS, 1, 1.0, None, None, st())
        torch.cuda.synchronize()
        if nr == 17:
            assert refused(hip, rc, "countr_adamw_step") and p.unchanged() and m.unchanged() and v.unchanged()
            continue
        _lib.check(rc)
        idx = torch.tensor([a for a, _ in ranges])
        stepped = torch.zeros(n, dtype=torch.bool)
        stepped[idx] = True
        want, _, _ = R.adamw_step(p0.double()[idx], g.double()[idx], torch.zeros(16, dtype=torch.float64), torch.zeros(16, dtype=torch.float64),
                                  1, KE.ADAM_LR, KE.ADAM_B1, KE.ADAM_B2, KE.ADAM_EPS, wd=0.05)
        pc = p.t.cpu()
        assert relerr(pc[idx], want) < 1e-5
        assert torch.equal(KE.bits(pc[~stepped]), KE.bits(p0[~stepped])) and bool((m.t.cpu()[~stepped] == 0).all())
        assert KE.all_intact(p, m, v)


# ---------------------------------------------------------------------------------------------------------------- patch gather, first conv
@pytest.mark.parametrize("B,H,W,patch", KE.IM2PATCH_CASES)
@MODES
def test_im2patch_scalar_kernel_and_cropped_sizes(hip, tdt, code, tol, B, H, W, patch):
    """patch 14 (K = 588, fp32 output as the engine stores it), a non-square grid, W % 4 != 0, H and W with a remainder: the scalar kernel;
    (1, 16, 24, 8): the vec8 kernel on a non-square grid."""
    hip = HP.library(tdt, hip)
    if patch == 14:
        tdt, code = torch.float32, 0
    img = KE.im2patch_image(B, H, W)
    ref = KE.im2patch_ref(img, patch)
    imgd = G((B, 3, H, W), fill=0.5, body=img)                # (read with a pitch: finite values around it)
    out = G(ref.shape, tdt)
    _lib.check(hip.countr_im2patch(P(imgd.t), P(out.t), B, H, W, patch, code, st()))
    KE.assert_im2patch(out.t, ref, tdt)
    assert out.intact() and imgd.unchanged()


@pytest.mark.parametrize("S,H,W", KE.C3_SHAPES)
@MODES
def test_first_exemplar_conv_default_dispatch_at_odd_widths(hip, tdt, code, tol, S, H, W):
    """W % 4 != 0: the default dispatch takes the per-pixel kernel; forward against fp64 conv2d, weight and bias gradients against its
    backward (fewer pixels than blocks: empty blocks contribute zeros)."""
    hip = HP.library(tdt, hip)
    x, w, bias, dy = KE.c3_inputs(S, H, W, tdt)
    ref = KE.c3_reference(x, w, bias, dy)
    xd = G((S, 3, H, W), fill=0.5, body=x)
    wd, bd, dyd = w.cuda(), bias.cuda(), dy.cuda()
    y = G((S, H, W, 64), tdt)
    _lib.check(hip.countr_conv3x3_c3_fwd(P(xd.t), P(wd), P(bd), P(y.t), S, H, W, code, st()))
    dw, db, ws = G((64, 3, 3, 3)), G(64), G(hip.countr_conv3x3_c3_wgrad_nblocks() * 64 * 28)
    _lib.check(hip.countr_conv3x3_c3_wgrad(P(xd.t), P(dyd), P(dw.t), P(db.t), P(ws.t), S, H, W, code, 0, st()))
    KE.assert_c3(y.t, dw.t, db.t, ref, tdt, tol)
    assert KE.all_intact(y, dw, db, ws) and xd.unchanged()
