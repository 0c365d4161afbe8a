"""The references, bars and guard bands of tests/kedges.py on the CPU, before any kernel meets them: for every input family of
tests/test_kernel_edges_gpu.py (and of the cases it adds to tests/test_kernels_gpu.py) an fp32 torch emulation of the operation -- rounded
to the 16-bit type where the kernel stores 16 bits -- passes the very assertion the kernel's output is given, and deliberately wrong
variants of the emulation (a lost last column, a pad column left non-zero, key S - 1 left out, pitch D where 2 D is right, ...) fail it.
No kernel runs here and no wrong variant is ever applied to one."""
import pytest
import torch

import attnref as AR
import halfprec as HP
import kedges as KE

DT_IDS = ["fp32", "bf16", "fp16"]
MODES = pytest.mark.parametrize("tdt,code,tol", KE.DT, ids=DT_IDS)


def fails(fn, *args):
    try:
        fn(*args)
    except AssertionError:
        return True
    return False


# ---------------------------------------------------------------------------------------------------------------- guard bands
def test_guard_bands_see_a_store_on_either_side_and_nothing_else():
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        g = KE.Guarded((3, 5), dtype, lead=1)
        assert g.t.shape == (3, 5) and g.buf.numel() == 15 + 2 * KE.GUARD + 1 and g.intact() and g.unchanged()
        assert g.t.data_ptr() - g.buf.data_ptr() == (KE.GUARD + 1) * g.buf.element_size()
        g.t.fill_(1.0)
        assert g.intact() and not g.unchanged()
        for at in (g.lo - 1, g.lo + g.n):                  # the element just before and just behind the tensor
            h = KE.Guarded((3, 5), dtype, lead=1)
            h.buf[at] = 0.0
            assert not h.intact()
    g = KE.Guarded(4, fill=7.0)                            # NaN against NaN is "identical": the comparison is of bits
    g.buf[0] = float("nan")
    assert not g.intact()


# ---------------------------------------------------------------------------------------------------------------- softmax
@pytest.mark.parametrize("family", KE.SOFTMAX_FAMILIES)
@MODES
def test_softmax_emulation_inside_and_wrong_variants_outside(family, tdt, code, tol):
    cases = [(rows, n, n) for rows, n in KE.SOFTMAX_SHAPES] + [(KE.SOFTMAX_LD_ROWS, n, ld) for n, ld in KE.SOFTMAX_LD]
    for rows, n, ld in cases:
        s = KE.softmax_scores(family, rows, n, ld)
        assert torch.isfinite(s).all() and (ld == n or bool((s[:, n:] == KE.SOFTMAX_PAD).all()))
        p = KE.softmax_emulate(s, n, tdt)
        KE.assert_softmax(p, s, n, tdt, tol)
        if n > 1:                                           # the last column left out of the statistics (and stored as zero)
            q = KE.softmax_emulate(s, n - 1, tdt)
            assert fails(KE.assert_softmax, q, s, n, tdt, tol), (rows, n, ld, "last column dropped")
        if ld > n:                                          # a pad column left non-zero; a pad score read into the statistics
            q = p.clone()
            q[rows - 1, ld - 1] = 2.0 ** -20
            assert fails(KE.assert_softmax, q, s, n, tdt, tol), (rows, n, ld, "pad column not zero")
            q = KE.softmax_emulate(s, n + 1, tdt)
            assert fails(KE.assert_softmax, q, s, n, tdt, tol), (rows, n, ld, "pad score read")
        if n == 1:                                          # "exactly 1" is exact: one bf16 ulp below fails
            q = p.clone()
            q[0, 0] = 1.0 - 2.0 ** -8
            assert fails(KE.assert_softmax, q, s, n, tdt, tol)


@pytest.mark.parametrize("family", KE.SOFTMAX_FAMILIES)
@MODES
def test_softmax_backward_emulation_inside_and_wrong_variants_outside(family, tdt, code, tol):
    for rows, n in KE.SOFTMAX_SHAPES:
        p = KE.softmax_emulate(KE.softmax_scores(family, rows, n), n, tdt)
        dp = KE.softmax_dp(rows, n)
        ds = KE.softmax_bwd_emulate(p, dp, KE.SOFTMAX_BWD_SCALE, tdt)
        KE.assert_softmax_bwd(ds, p, dp, KE.SOFTMAX_BWD_SCALE, tdt, tol)
        if n > 1 and family != "spike":                     # the row's dot product without its last column
            pf = p.float()
            dot = (pf[:, :-1] * dp[:, :-1]).sum(-1, keepdim=True)
            q = (pf * (dp - dot) * KE.SOFTMAX_BWD_SCALE).to(tdt)
            assert fails(KE.assert_softmax_bwd, q, p, dp, KE.SOFTMAX_BWD_SCALE, tdt, tol), (rows, n)


# ---------------------------------------------------------------------------------------------------------------- cross attention
def xattn_excess(got, vals, comp, fl):
    worst = []
    for n in ("out", "dq"):
        worst.append(AR.attn_excess(got[n], vals[n], comp[n][0], fl, AR.K_ONE_ROUNDING, AR.F32_TOL, comp[n][1]))
    for n in ("dk", "dv"):
        worst.append(AR.attn_excess(got[n], vals[n], comp[n][0], None, 0, AR.F32_TOL))
    return max(worst)


@pytest.mark.parametrize("N,S", KE.XATTN_CASES)
@pytest.mark.parametrize("fl", HP.FLAVOURS, ids=HP.FLAVOUR_IDS)
def test_cross_attention_cases_emulation_inside_and_wrong_variants_outside(fl, N, S):
    B, D, Hh, scale = KE.XATTN_B, KE.XATTN_D, KE.XATTN_HEADS, 32 ** -0.5
    q, k, v, do = KE.xattn_inputs(N, S, fl.dtype)
    vals, comp = AR.cross_attention(q, k, v, do, Hh, scale)
    assert xattn_excess(AR.emulate_cross(vals, fl), vals, comp, fl) <= 0
    if S > 1:                                               # key S - 1 left out: the softmax runs over S - 1 keys, its dk and dv stay zero
        short, _ = AR.cross_attention(q, k[:, :S - 1], v[:, :S - 1], do, Hh, scale)
        wrong = {n: short[n] for n in ("out", "dq")}
        for n in ("dk", "dv"):
            wrong[n] = torch.cat([short[n], torch.zeros_like(vals[n][:, :1])], 1)
        assert xattn_excess(AR.emulate_cross(wrong, fl), vals, comp, fl) > 0
    # the packed buffer read at pitch D where 2 D is right: rows of v taken for rows of k and the reverse
    kv = KE.pack_kv(k, v)
    k2, v2 = KE.kv_read_at_pitch(kv, B, S, D, 2 * D)
    assert torch.equal(k2, k) and torch.equal(v2, v)
    k1, v1 = KE.kv_read_at_pitch(torch.cat([kv.reshape(-1), torch.zeros(B * S * D, dtype=kv.dtype)]).reshape(-1, 2 * D), B, S, D, D)
    wrong, _ = AR.cross_attention(q, k1, v1, do, Hh, scale)
    assert xattn_excess(AR.emulate_cross(wrong, fl), vals, comp, fl) > 0


# ---------------------------------------------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("rows,D", [(1157, D) for D in KE.LN_D] + [(rows, D) for rows in KE.LN_ROWS for D in KE.LN_ROWS_D])
@MODES
def test_layernorm_emulation_inside_and_a_lost_last_column_outside(rows, D, tdt, code, tol):
    x, g, b, dy = KE.ln_inputs(rows, D, tdt)
    ref = KE.ln_reference(x, g, b, dy)
    KE.assert_layernorm(*KE.ln_emulate(x, g, b, dy, tdt), ref, tdt, tol)
    assert fails(KE.assert_layernorm, *KE.ln_emulate(x, g, b, dy, tdt, cols=D - 1), ref, tdt, tol)
    if D > 256:                                             # the ragged last 256-column group lost
        assert fails(KE.assert_layernorm, *KE.ln_emulate(x, g, b, dy, tdt, cols=(D - 1) // 256 * 256), ref, tdt, tol)


# ---------------------------------------------------------------------------------------------------------------- column sums
@pytest.mark.parametrize("M,N", KE.COLSUM_SHAPES)
@MODES
def test_colsum_emulation_inside_and_wrong_variants_outside(M, N, tdt, code, tol):
    x = KE.colsum_input(M, N, tdt)
    ones, sent = torch.ones(N), torch.full((N,), KE.COLSUM_SENTINEL)
    s = x.float().sum(0)
    KE.assert_colsum(s + 1, x, 1, ones)
    KE.assert_colsum(s, x, 0, sent)
    assert fails(KE.assert_colsum, s + sent, x, 0, sent)            # added to the sentinel instead of overwriting it
    assert fails(KE.assert_colsum, s, x, 1, ones)                   # overwritten where it must accumulate
    lost = s.clone()
    lost[N - 8:] = 0.0                                              # the last 8-column vector (the ragged tile's) never summed
    assert fails(KE.assert_colsum, lost, x, 0, sent)
    if M > 1:
        assert fails(KE.assert_colsum, x[:M - 1].float().sum(0), x, 0, sent)       # last row lost


# ---------------------------------------------------------------------------------------------------------------- GELU backward
@pytest.mark.parametrize("n", KE.GELU_N + [8 * 8192 + 8 * 257])    # (a stand-in for the size past the block cap: the same inputs and reference)
@MODES
def test_gelu_backward_emulation_inside_and_a_stale_tail_outside(n, tdt, code, tol):
    pre, dh = KE.gelu_inputs(n, tdt)
    x = pre.float().requires_grad_(True)
    torch.nn.functional.gelu(x).backward(dh.float())
    out = x.grad.to(tdt)
    KE.assert_gelu_bwd(out, pre, dh, tol)
    ref = KE.gelu_bwd_ref(pre, dh)
    i = int(ref[n - 8:].abs().argmax()) + n - 8                     # the last vector never written (zero), judged at its largest element
    if ref[i].abs() > tol * ref.abs().max():
        wrong = out.clone()
        wrong[n - 8:] = 0
        assert fails(KE.assert_gelu_bwd, wrong, pre, dh, tol)
    wrong = (dh.float() * torch.sigmoid(1.702 * pre.float())).to(tdt)           # another function altogether: x sigmoid(1.702 x) without its second term
    assert fails(KE.assert_gelu_bwd, wrong, pre, dh, tol)


# ---------------------------------------------------------------------------------------------------------------- masked MSE
@pytest.mark.parametrize("B,HW,off", KE.MSE_CASES)
@pytest.mark.parametrize("gs", KE.MSE_SCALES)
def test_masked_mse_emulation_inside_and_wrong_variants_outside(B, HW, off, gs):
    pred, gt, mask = KE.mse_inputs(B, HW)
    assert mask.sum() > 0
    ref = KE.mse_reference(pred, gt, mask, gs)
    sums, dp = KE.mse_emulate(pred, gt, mask, gs)
    KE.assert_masked_mse(sums, dp, ref)
    KE.assert_masked_mse(sums, None, ref)                           # (dpred = NULL: the sums alone)
    if gs != 1.0:
        assert fails(KE.assert_masked_mse, sums, dp / gs, ref)      # grad_scale ignored
    last = torch.zeros(HW)
    last[HW - 1] = 1.0                                              # the last pixel left out of every sum and of dpred
    s2, d2 = KE.mse_emulate(pred * (1 - last), gt * (1 - last), mask, gs)
    assert fails(KE.assert_masked_mse, s2, None, ref)
    if mask[HW - 1] > 0:
        assert fails(KE.assert_masked_mse, sums, d2, ref)
    assert fails(KE.assert_masked_mse, sums * torch.cat([torch.full((1,), 1.0 + 1e-4), torch.ones(2 * B)]), dp, ref)


# ---------------------------------------------------------------------------------------------------------------- AdamW
def test_adamw_emulation_inside_and_wrong_variants_outside():
    p0 = KE.rnd((KE.ADAM_N,), 31)
    grads = [KE.rnd((KE.ADAM_N,), 41 + i) for i in range(3)]
    steps_of_range = [set(range(KE.ADAM_GROUP_START[g] - 1, 3)) for g in KE.ADAM_GROUPS]
    refs = KE.adam_reference(p0, grads, steps_of_range)
    p, m, v = p0.clone(), torch.zeros(KE.ADAM_N), torch.zeros(KE.ADAM_N)
    for i, g in enumerate(grads):
        t = [max(0, i + 2 - KE.ADAM_GROUP_START[gr]) for gr in KE.ADAM_GROUPS]
        p, m, v = KE.adam_emulate_step(p, g, m, v, t)
        KE.assert_adam(p, refs[i], p0)
    inside = KE.adam_inside()
    assert int(inside.sum()) == sum(b - a for a, b in KE.ADAM_RANGES) and not bool(inside[1001:1500].any())
    wrong = p.clone()
    wrong[1200] = wrong[1200] * (1 - KE.ADAM_LR * 0.05)             # weight decay applied inside a gap
    assert fails(KE.assert_adam, wrong, refs[2], p0)
    # every range on the counter of group 0 (bias corrections of step 3 for a range at its first step)
    q, m, v = p0.clone(), torch.zeros(KE.ADAM_N), torch.zeros(KE.ADAM_N)
    for i, g in enumerate(grads):
        t = [max(0, i + 2 - KE.ADAM_GROUP_START[gr]) for gr in KE.ADAM_GROUPS]
        q, m, v = KE.adam_emulate_step(q, g, m, v, [i + 1 if x else 0 for x in t])
    assert fails(KE.assert_adam, q, refs[2], p0)
    a, b = KE.ADAM_RANGES[2]
    wrong = p.clone()
    wrong[b - 1] = p0[b - 1]                                        # the last element of a range whose length is no multiple of 4 not stepped
    assert fails(KE.assert_adam, wrong, refs[2], p0)


# ---------------------------------------------------------------------------------------------------------------- patch gather, first conv
@pytest.mark.parametrize("B,H,W,p", KE.IM2PATCH_CASES)
@MODES
def test_im2patch_reference_and_wrong_variants(B, H, W, p, tdt, code, tol):
    img = KE.im2patch_image(B, H, W)
    ref = KE.im2patch_ref(img, p)
    gh, gw = H // p, W // p
    assert ref.shape == (B * gh * gw, 3 * p * p)
    t, c, py, px = B * gh * gw - 1, 2, p - 1, p - 2                 # one element by hand: last token, last channel, last row
    assert ref[t, (c * p + py) * p + px] == img[B - 1, c, (gh - 1) * p + py, (gw - 1) * p + px]
    KE.assert_im2patch(ref.to(tdt), ref, tdt)
    if W % p:                                                       # the cropped width used as the row pitch of the image
        wrong = KE.im2patch_ref(img.reshape(-1)[:B * 3 * H * gw * p].reshape(B, 3, H, gw * p), p)
        assert fails(KE.assert_im2patch, wrong.to(tdt), ref, tdt)
    wrong = ref.clone()
    wrong[-1, -1] = wrong[-1, -2]                                   # the last element from its neighbour
    assert fails(KE.assert_im2patch, wrong.to(tdt), ref, tdt)


@pytest.mark.parametrize("S,H,W", KE.C3_SHAPES)
@MODES
def test_first_conv_emulation_inside_and_wrong_variants_outside(S, H, W, tdt, code, tol):
    x, w, bias, dy = KE.c3_inputs(S, H, W, tdt)
    ref = KE.c3_reference(x, w, bias, dy)
    wr, br = w.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    y = torch.nn.functional.conv2d(x, wr, br, padding=1)
    y.backward(dy.float().permute(0, 3, 1, 2))
    y = y.detach().permute(0, 2, 3, 1).to(tdt)
    KE.assert_c3(y, wr.grad, br.grad, ref, tdt, tol)
    wrong = y.clone()
    wrong[S - 1, H - 1, W - 1] = 0                                  # the last pixel never written
    assert fails(KE.assert_c3, wrong, wr.grad, br.grad, ref, tdt, tol)
    dyl = dy.float().clone()
    dyl[S - 1, H - 1, W - 1] = 0                                    # the last pixel left out of the weight and bias gradients
    w2, b2 = w.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    torch.nn.functional.conv2d(x, w2, b2, padding=1).backward(dyl.permute(0, 3, 1, 2))
    assert fails(KE.assert_c3, y, w2.grad, b2.grad, ref, tdt, tol)
