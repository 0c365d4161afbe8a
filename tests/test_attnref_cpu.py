"""The row-wise attention bound (tests/attnref.py) on the CPU: at every shape the GPU tests run, a fp64 emulation of the kernels' 16-bit
rounding points stays inside the bound with the committed K, and every mutant of the REFERENCE -- the mistakes a hand-scheduled attention
kernel makes in one row, one tile or one lane -- falls outside it.  No kernel runs here and no mutant is ever applied to one."""
import math

import pytest
import torch

import attnref as AR
import halfprec as HP

FA_OUT = {HP.BF16: 1.5e-2, HP.FP16: 2e-3}        # the max-norm bars of tests/test_kernels_gpu.py
FA_GRAD = {HP.BF16: 2.5e-2, HP.FP16: 4e-3}


def relerr(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def dS_of(ref, P=None, delta=None):
    P = ref.P if P is None else P
    if delta is None:
        delta = (ref.do * ref.out).sum(-1, keepdim=True)
    return P * (ref.do @ ref.v.transpose(-1, -2) - delta)


def spiked_key(name, N):
    """(batch, head, key) of the spiked key of a backward case."""
    return (0, 0, N - 1) if name.startswith("grid") else (0, 0, N // 3)


# ---- forward mutants: ref -> mutated out [B, H, N, dh], or None where the mutant does not exist at this shape
def fwd_last_key_left_out(ref, name):
    return ref.P[..., :-1] @ ref.v[..., :-1, :]                      # lse (the normalisation) kept


def fwd_last_row_from_its_neighbour(ref, name):
    if ref.out.shape[-2] < 2:
        return None
    out = ref.out.clone()
    out[..., -1, :] = ref.out[..., -2, :]
    return out


def fwd_two_columns_swapped(ref, name):
    """The two lanes of one packed pair (columns 2c, 2c + 1) of the middle row of batch 0, head 0: the pair of that row whose values
    differ most (a swap of two equal values is no error)."""
    out = ref.out.clone()
    i = out.shape[-2] // 2
    row = ref.out[0, 0, i]
    c = 2 * int((row[0::2] - row[1::2]).abs().argmax())
    out[0, 0, i, c], out[0, 0, i, c + 1] = row[c + 1], row[c]
    return out


def fwd_unrescaled_before_the_jump(ref, name):
    """One row of batch 0 whose maximum lies behind key tile 0: what was accumulated before the maximum's tile keeps its old reference
    max, i.e. enters exp(jump) too large.  The row with the largest jump."""
    sc = ref.sc[0]
    H, N, _ = sc.shape
    if N <= 64:
        return None
    start = (sc.argmax(-1) // 64) * 64                               # first key of the maximum's tile, per (head, row)
    before = torch.arange(N)[None, None, :] < start[..., None]
    m_old = sc.masked_fill(~before, -math.inf).amax(-1)
    jump = sc.amax(-1) - m_old                                       # +inf where the maximum lies in tile 0 (nothing before it)
    jump = torch.where(torch.isfinite(jump), jump, torch.full_like(jump, -1.0))
    h, i = divmod(int(jump.argmax()), N)
    if jump[h, i] <= 0:
        return None
    j0 = int(start[h, i])
    out = ref.out.clone()
    early = ref.P[0, h, i, :j0] @ ref.v[0, h, :j0]
    log_l = ref.lse[0, h, i] - sc[h, i].max()                        # l of the finished row, relative to its final maximum
    stale = torch.exp(sc[h, i, :j0] - m_old[h, i] - log_l) @ ref.v[0, h, :j0]
    out[0, h, i] = ref.out[0, h, i] - early + stale
    return out


FWD_MUTANTS = [fwd_last_key_left_out, fwd_last_row_from_its_neighbour, fwd_two_columns_swapped, fwd_unrescaled_before_the_jump]


# ---- backward mutants: ref -> {name: mutated gradient} of the outputs the mutant touches, or None
def bwd_lse_of_the_last_row_off(ref, name, units=0.25):
    P = ref.P.clone()
    P[..., -1, :] *= 2.0 ** -units
    return dict(zip(("dq", "dk", "dv"), AR.backward(ref.q, ref.k, ref.v, ref.do, P, ref.out, ref.scale)))


def bwd_last_key_tile_dropped_from_dq(ref, name):
    N = ref.q.shape[-2]
    if N < 2:
        return None                                                  # dq of a one-token sequence is zero
    j0 = 64 * ((N + 63) // 64 - 1)
    return {"dq": ref.scale * dS_of(ref)[..., :j0] @ ref.k[..., :j0, :]}


def bwd_last_query_tile_dropped_from_dk_dv(ref, name):
    N = ref.q.shape[-2]
    i0 = 64 * ((N + 63) // 64 - 1)
    dS = dS_of(ref)[..., :i0, :]
    return {"dk": ref.scale * dS.transpose(-1, -2) @ ref.q[..., :i0, :], "dv": ref.P[..., :i0, :].transpose(-1, -2) @ ref.do[..., :i0, :]}


def bwd_delta_from_half_the_channels(ref, name):
    h = ref.q.shape[-1] // 2
    delta = (ref.do[..., :h] * ref.out[..., :h]).sum(-1, keepdim=True)
    return dict(zip(("dq", "dk", "dv"), AR.backward(ref.q, ref.k, ref.v, ref.do, ref.P, ref.out, ref.scale, delta)))


def bwd_dv_of_ordinary_keys_scaled(ref, name):
    b, h, j = spiked_key(name, ref.q.shape[-2])
    dv = ref.grads["dv"] * 0.75
    dv[b, h, j] = ref.grads["dv"][b, h, j]
    return {"dv": dv}


BWD_MUTANTS = [bwd_lse_of_the_last_row_off, bwd_last_key_tile_dropped_from_dq, bwd_last_query_tile_dropped_from_dk_dv,
               bwd_delta_from_half_the_channels, bwd_dv_of_ordinary_keys_scaled]


def excess(ref, fl, n, got):
    want = ref.out if n == "out" else ref.grads[n]
    c, T = ref.comp[n]
    return AR.attn_excess(got, want, c, fl, AR.k_of(n, fl), AR.F32_TOL, T)


def case_params():
    for fl, fid in zip(HP.FLAVOURS, HP.FLAVOUR_IDS):
        for name, make in AR.CASES(fl):
            yield pytest.param(fl, name, make, id="%s-%s" % (fid, name.replace(" ", "")))


@pytest.mark.parametrize("fl,name,make", list(case_params()))
def test_emulation_inside_and_every_mutant_outside_the_bound(fl, name, make):
    ref = AR.reference_of(make())
    wrong = []
    for n, e in AR.emulate(ref, fl).items():
        want = ref.out if n == "out" else ref.grads[n]
        x = AR.ratio(e, want, ref.comp[n][0], fl)
        if x > AR.MEASURED[n][AR.flavour_name(fl)] * (1 + 1e-3):     # the committed figures are the maximum over these very cases
            wrong.append(("emulation ratio above the committed MEASURED", n, x))
        ex = excess(ref, fl, n, e)
        if not ex <= 0.0:
            wrong.append(("emulation outside the bound", n, ex))
    for mutant in FWD_MUTANTS:
        out = mutant(ref, name)
        if out is not None and not excess(ref, fl, "out", out) > 0.0:
            wrong.append(("mutant inside the bound", mutant.__name__, excess(ref, fl, "out", out)))
    if ref.do is not None:
        for mutant in BWD_MUTANTS:
            grads = mutant(ref, name)
            if grads is not None:
                worst = max(excess(ref, fl, n, g) for n, g in grads.items())
                if not worst > 0.0:
                    wrong.append(("mutant inside the bound", mutant.__name__, worst))
    assert not wrong, wrong


@pytest.mark.parametrize("fl", HP.FLAVOURS, ids=HP.FLAVOUR_IDS)
def test_grid_lift_condition_holds_on_the_reference(fl):
    """Every shape of the grid with N > 64 has, in head 2 of batch 0, more than 8 rows whose maximum lies over 64 log2 units above key
    tile 0 (the bf16 fast path overflows and the strip runs again) and more than 8 rows within one unit, beside ordinary heads.  The GPU
    test asserts the same on its own reference."""
    for (B, N, H, dh) in AR.GRID_SHAPES:
        if N > 64:
            far, near = AR.lift_rows(AR.reference_of(AR.inputs_grid(fl, B, N, H, dh)))
            assert far > 8 and near > 8, (B, N, H, dh, far, near)


@pytest.mark.parametrize("mutant", [bwd_lse_of_the_last_row_off, bwd_dv_of_ordinary_keys_scaled])
def test_the_max_norm_bars_pass_these_mutants(mutant):
    """Why the row-wise measure exists: at (1, 576, 12, 64), with the backward test's own inputs, a last row whose P is 16 % off and
    a dv that is 25 % short in every ordinary row both stay under the max-norm bars of test_flash_attention_bwd."""
    fl, name = HP.BF16, "bwd(1, 576, 12, 64)"
    ref = AR.reference_of(AR.inputs_bwd_spiked(fl, 1, 576, 12, 64))
    grads = mutant(ref, name)
    for n, g in grads.items():
        assert relerr(g, ref.grads[n]) < FA_GRAD[fl], n
    assert max(excess(ref, fl, n, g) for n, g in grads.items()) > 0.0


def test_k_is_twice_the_measured_ratio_rounded_up():
    for n, per in AR.MEASURED.items():
        for f, x in per.items():
            assert x > 0 and AR.K[n][f] == math.ceil(2 * x)


def test_attn_excess_is_relative_to_the_rows_own_companion():
    ref = torch.zeros(2, 4, dtype=torch.float64)
    comp = torch.tensor([[100.0] * 4, [1.0] * 4], dtype=torch.float64)
    out = ref.clone()
    out[1, 2] = 1e-3                                                   # 1e-3 of ITS row's companion: outside a 2e-4 floor ...
    assert AR.attn_excess(out, ref, comp, None, 0, 2e-4) > 0
    out = ref.clone()
    out[0, 2] = 1e-3                                                   # ... and inside it in the row whose companion is 100
    assert AR.attn_excess(out, ref, comp, None, 0, 2e-4) <= 0
    assert AR.attn_excess(ref, ref, comp, HP.BF16, 2, 2e-4) <= 0
    out = ref.clone()
    out[0, 0] = 100 * 3 * HP.BF16.u                                     # K u companion: 3 units against K = 2, then K = 4
    assert AR.attn_excess(out, ref, comp, HP.BF16, 2, 0.0) > 0 and AR.attn_excess(out, ref, comp, HP.BF16, 4, 0.0) <= 0
    T = torch.full_like(ref, 1000.0)                                   # the fp16 subnormal term, absent for bf16
    out = ref.clone()
    out[1, 1] = 500 * HP.FP16.tiny
    assert AR.attn_excess(out, ref, torch.zeros_like(ref), HP.FP16, 2, 0.0, T) <= 0
    assert AR.attn_excess(out, ref, torch.zeros_like(ref), HP.BF16, 2, 0.0, T) > 0


def test_attn_excess_on_non_finite_values():
    ref = torch.ones(2, 4, dtype=torch.float64)
    for bad in (float("nan"), float("inf")):
        out = ref.clone()
        out[1, 3] = bad
        assert AR.attn_excess(out, ref, ref, HP.FP16, 4, 2e-4) == float("inf")
    with pytest.raises(AssertionError):
        AR.assert_attn_rows(out, ref, ref, HP.FP16, 4, 2e-4)


@pytest.mark.parametrize("N,S", [(576, 3), (1, 1), (65, 9)])
@pytest.mark.parametrize("fl", HP.FLAVOURS, ids=HP.FLAVOUR_IDS)
def test_cross_attention_emulation_and_a_wrong_row(fl, N, S):
    B, D, Hh = 2, 512, 16
    q, do = AR.rnd((B, N, D), 15).to(fl.dtype), AR.rnd((B, N, D), 18).to(fl.dtype)
    k, v = AR.rnd((B, S, D), 16).to(fl.dtype), AR.rnd((B, S, D), 17).to(fl.dtype)
    vals, comp = AR.cross_attention(q, k, v, do, Hh, 32 ** -0.5)
    emu = AR.emulate_cross({n: t for n, t in vals.items()}, fl)
    for n in ("out", "dq"):
        assert AR.attn_excess(emu[n], vals[n], comp[n][0], fl, AR.K_ONE_ROUNDING, AR.F32_TOL, comp[n][1]) <= 0, n
    out = vals["out"].clone()
    c = comp["out"][0][B - 1, N - 1, Hh - 1]
    out[B - 1, N - 1, Hh - 1] += 3 * fl.u * c + 2 * AR.F32_TOL * c.amax()  # the last row's last head: 3 u companion + two floors off
    assert AR.attn_excess(out, vals["out"], comp["out"][0], fl, AR.K_ONE_ROUNDING, AR.F32_TOL, comp["out"][1]) > 0
    dv = vals["dv"].clone()
    dv[0, S - 1, 0] *= 1.0 + 2e-3                                       # an fp32 sum: the floor of its own row alone
    assert AR.attn_excess(dv, vals["dv"], comp["dv"][0], None, 0, AR.F32_TOL) > 0
