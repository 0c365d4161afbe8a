"""The fused self-attention kernels at the key-tile counts and row counts where their pipelines change shape, against the fp64 reference
and the row-wise companion bound of tests/attnref.py (whose constants come from a CPU emulation of the kernels' rounding points, never
from a kernel: tests/test_attnref_cpu.py).

The forward loops over T = ceil(N / 64) key tiles with a prologue, a skewed steady state and a drain that differ for T = 1, 2, 3, 4 and
from 5 on (the dh = 64 LDS-DMA ring has four slots); a ragged last tile is masked in the prologue (T = 1) or in the step before the
last; a workgroup holds 128 query rows in four waves of 32.  The grid: N = 1, 17, 33, 63 (T = 1 ragged, one wave with 1 / 17 / 32 live
rows or two, the others idle), 64, 65 (a one-key tail tile), 127, 128, 129 (a second row block of one row), 192, 193, 257 (T = 5, three
row blocks); B H = 3 walks the workgroups in plain order, B H = 8 in the XCD-swizzled one.  The backward has the same tile loop in both
of its passes."""
import ctypes as C

import pytest
import torch

import attnref as AR
import halfprec as HP
from countr_amd import _lib

pytestmark = pytest.mark.gpu


def st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t):
    return C.c_void_p(t.data_ptr())


def guarded(rows, width, dtype):
    """A NaN-filled [rows + 1, width] buffer: the kernel is given `rows` rows, the last one is the guard that must stay NaN."""
    return torch.full((rows + 1, width), float("nan"), device="cuda", dtype=dtype)


def run_forward(hip, fl, inp):
    B, N, _, H, dh = inp.qkv.shape
    qd = inp.qkv.cuda()
    out = guarded(B * N, H * dh, fl.dtype)
    lse = guarded(B * H * N, 1, torch.float32)
    _lib.check(hip.countr_attn_fwd(P(qd), P(out), P(lse), B, N, H, dh, inp.scale, st()))
    torch.cuda.synchronize()
    assert torch.isnan(out[-1]).all() and torch.isnan(lse[-1]).all(), "a row >= N was stored"
    return qd, out, lse


def check_forward(fl, ref, out, lse, what):
    B, H, N, dh = ref.q.shape
    o = out[:-1].reshape(B, N, H * dh)
    assert torch.isfinite(o.float()).all(), what
    ex = AR.lse_excess(lse[:-1].reshape(B, H, N), ref.lse)
    assert ex <= 0.0, (what, "lse off by", ex)
    AR.assert_self_attention_rows(ref, fl, out=o, what=what)


@pytest.mark.parametrize("B,N,H,dh", AR.GRID_SHAPES)
@pytest.mark.parametrize("fl", HP.FLAVOURS, ids=HP.FLAVOUR_IDS)
def test_self_attention_fwd_bwd_small_shape_grid(hip, fl, B, N, H, dh):
    hip = HP.library(fl, hip)
    inp = AR.inputs_grid(fl, B, N, H, dh)
    ref = AR.reference_of(inp)
    if N > 64:      # head 2: rows far above the first key tile (bf16: the fast path overflows, the strip runs again) and rows that are not
        far, near = AR.lift_rows(ref)
        assert far > 8 and near > 8, (far, near)
    qd, out, lse = run_forward(hip, fl, inp)
    check_forward(fl, ref, out, lse, "forward")
    dod = inp.do.cuda()
    delta = torch.empty((B, H, N), device="cuda")
    dqkv = guarded(B * N, 3 * H * dh, fl.dtype)
    _lib.check(hip.countr_attn_bwd(P(qd), P(out), P(dod), P(lse), P(delta), P(dqkv), B, N, H, dh, inp.scale, st()))
    torch.cuda.synchronize()
    assert torch.isnan(dqkv[-1]).all(), "a row >= N was stored"
    g = dqkv[:-1].reshape(B, N, 3, H, dh)
    assert torch.isfinite(g.float()).all()
    AR.assert_self_attention_rows(ref, fl, dqkv=g, what="backward")


@pytest.mark.parametrize("fl", HP.FLAVOURS, ids=HP.FLAVOUR_IDS)
def test_self_attention_bwd_at_the_huge_models_token_count(hip, fl):
    """N = 729 = 11 x 64 + 25: six row blocks, the last with 89 rows, a ragged twelfth tile."""
    hip = HP.library(fl, hip)
    B, N, H, dh = AR.BWD_HUGE
    inp = AR.inputs_bwd_spiked(fl, B, N, H, dh)
    ref = AR.reference_of(inp)
    qd, out, lse = run_forward(hip, fl, inp)
    check_forward(fl, ref, out, lse, "forward")
    dod = inp.do.cuda()
    delta = torch.empty((B, H, N), device="cuda")
    dqkv = guarded(B * N, 3 * H * dh, fl.dtype)
    _lib.check(hip.countr_attn_bwd(P(qd), P(out), P(dod), P(lse), P(delta), P(dqkv), B, N, H, dh, inp.scale, st()))
    torch.cuda.synchronize()
    assert torch.isnan(dqkv[-1]).all(), "a row >= N was stored"
    g = dqkv[:-1].reshape(B, N, 3, H, dh)
    assert torch.isfinite(g.float()).all()
    AR.assert_self_attention_rows(ref, fl, dqkv=g, what="backward")


@pytest.mark.parametrize("B,N,H", AR.PRE_SMALL)
@pytest.mark.parametrize("fl", HP.FLAVOURS, ids=HP.FLAVOUR_IDS)
def test_self_attention_fwd_prescaled_q_two_and_three_key_tiles(hip, fl, B, N, H):
    hip = HP.library(fl, hip)
    inp = AR.inputs_fwd_prescaled(fl, B, N, H)
    _, out, lse = run_forward(hip, fl, inp)
    check_forward(fl, AR.reference_of(inp), out, lse, "pre-scaled q")


@pytest.mark.parametrize("fl", HP.FLAVOURS, ids=HP.FLAVOUR_IDS)
def test_self_attention_fwd_prescaled_q_refuses_a_ragged_sequence(hip, fl):
    """scale <= 0 is built for N % 64 == 0 only; N = 65 returns an error before anything is launched and stores nothing."""
    hip = HP.library(fl, hip)
    B, N, H, dh = 1, 65, 3, 64
    qd = AR.rnd((B, N, 3, H, dh), 52).to(fl.dtype).cuda()
    out = guarded(B * N, H * dh, fl.dtype)
    lse = guarded(B * H * N, 1, torch.float32)
    assert hip.countr_attn_fwd(P(qd), P(out), P(lse), B, N, H, dh, 0.0, st()) != 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(lse).all()
