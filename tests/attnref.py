"""fp64 reference, row-wise error bound and rounding emulation for the fused attention kernels (flash_attn_fwd.hip, flash_attn.hip) and the
cross attention of attention.hip.  Pure torch, any device; nothing here touches a kernel.

Why another bound.  halfprec.elementwise_excess is for outputs that are ONE rounding of an fp32 result.  Attention rounds P and dS to the
16-bit type before they enter an MFMA, and the stored O before it feeds delta, so an output element carries the roundings of a whole row
of products: its error is proportional not to |ref| but to the COMPANION, the same sum with absolute values inside (P the exact softmax,
s the scale):

    out : P @ |V|                       dv : P^T @ |dO|
    cS  = P o (|dO| @ |V|^T + rowsum(|dO| o |O|))            (budget of dS = P o (dO V^T - delta))
    dq  : s cS @ |K|                    dk : s cS^T @ |Q|

and the bound of one element is

    |out - ref| <= K u companion + tiny T + floor rowmax(companion)

u and tiny from halfprec.Flavour; T the sum of |second operand| over the contracted index (|V|, |dO|, s|K|, s|Q| summed over keys or
queries): a P or dS below the fp16 subnormal spacing is stored with an absolute error of tiny (0 for bf16); floor is the project's fp32
bar (2e-4), relative to the companion maximum of the element's OWN row (the dh channels of one token and head), not the tensor's.  The
max-norm relerr of the kernel tests is set by the spiked key's row (19 to 106 times an ordinary row); this bound is not.

Rounding points the emulation assumes (everything else of the kernels is fp32 and is modelled as exact):
  forward, flash_attn_fwd.hip
    :307-308  l is summed from the UNROUNDED p (exp_unit)
    :309      P = pack2bf(exp2(s c - m_ref)), the operand of the PV MFMA.  m_ref is the first tile's row max (bf16 fast path) or the
              running max within 8 log2 units (exact loop, fp16 always); the emulation uses the true row max: the same relative rounding,
              and the LARGEST subnormal loss an fp16 P can have.  One difference follows: the emulation's P of a row's largest score is
              exactly 1 and rounds without error, the kernels' is 2^(max - m_ref) and does not, so on a row that one key dominates the
              kernels may use up to twice the emulation's figure.  The doubling in K covers it: to first order |err| <= (P rounding
              + output rounding) companion = 4u companion for bf16 (a bf16 rounding is up to 2u relative), 2u for fp16.
    :560      out = pack2bf(o / l)
    :564      lse is fp32, never rounded to 16 bits
  backward, flash_attn.hip
    :100-106  delta (dQ pass) = dO . O from the STORED 16-bit O;  :160-171 the same in the dK / dV pass
    :226-229  P = exp2(s c - lse2) and dS = P (dP - delta) in fp32, dS from the UNROUNDED P
    :237-240  dS = pack2bf(...), the operand of the dQ and dK MFMAs
    :242-245  P = pack2bf(...), the operand of the dV MFMA (dK / dV pass only)
    :290      dq = pack2bf(scale acc), dk = pack2bf(scale acc), dv = pack2bf(acc)
  cross attention, attention.hip: fp32 throughout; out (:119, :238) and dq (:188, :345) are stored through st8<T>, ONE rounding; dk and dv
    are fp32 sums (:365).

The constants K.  `python tests/attnref.py` runs the emulation on every shape the GPU tests use (CASES below, both flavours) and prints, per
output and flavour, the largest |emu - ref| / (u companion).  K is twice that, rounded up to an integer: one ulp (2u) per rounding, the
project's convention (halfprec.py), which also covers what the emulation does not model -- fp32 accumulation order, l summed from rounded
or unrounded P.  The kernels are never the yardstick: MEASURED and K below come from that command alone."""
import collections
import math

import torch

import halfprec as HP

LN2 = 0.6931471805599453
LOG2E = 1.4426950408889634
F32_TOL = 2e-4

# largest |emu - ref| / (u companion) over CASES, as printed by `python tests/attnref.py`
MEASURED = {
    "out": {"bf16": 1.977, "fp16": 1.878},      # K = 4, 4
    "dq": {"bf16": 1.163, "fp16": 0.553},       # K = 3, 2
    "dk": {"bf16": 0.601, "fp16": 0.279},       # K = 2, 1
    "dv": {"bf16": 2.438, "fp16": 1.099},       # K = 5, 3
}
K = {name: {fl: int(math.ceil(2 * v)) for fl, v in per.items()} for name, per in MEASURED.items()}
K_ONE_ROUNDING = 2          # cross attention out / dq: one rounding of an fp32 result, |err| <= u |ref| <= u companion, doubled


def flavour_name(fl):
    return "bf16" if fl is HP.BF16 else "fp16"


def k_of(name, fl):
    return K[name][flavour_name(fl)]


# ---------------------------------------------------------------------------------------------------------------- layouts
def heads(qkv):
    """q, k, v of a packed [B, N, 3, H, dh] tensor as fp64 [B, H, N, dh] (on the CPU)."""
    x = qkv.detach().double().cpu()
    return tuple(x[:, :, i].permute(0, 2, 1, 3) for i in range(3))


def to_heads(x, H):
    """[B, N, H*dh] (or [B, N, H, dh]) -> fp64 [B, H, N, dh]"""
    x = x.detach().double().cpu()
    B, N = x.shape[:2]
    return x.reshape(B, N, H, -1).permute(0, 2, 1, 3)


def to_rows(x):
    """[B, H, N, dh] -> [B, N, H, dh], the layout of the kernels' outputs: a ROW is the last axis."""
    return x.permute(0, 2, 1, 3).contiguous()


# ---------------------------------------------------------------------------------------------------------------- fp64 reference
def forward(q, k, v, scale):
    """scores, P, out, lse (natural log) of softmax(q k^T scale) v; everything [B, H, N, *] fp64."""
    sc = (q @ k.transpose(-1, -2)) * scale
    lse = torch.logsumexp(sc, -1)
    P = torch.exp(sc - lse[..., None])
    return sc, P, P @ v, lse


def backward(q, k, v, do, P, out, scale, delta=None):
    """dq, dk, dv of the same from P and out (delta = rowsum(dO o out) unless given)."""
    dP = do @ v.transpose(-1, -2)
    if delta is None:
        delta = (do * out).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    return scale * dS @ k, scale * dS.transpose(-1, -2) @ q, P.transpose(-1, -2) @ do


def companions(q, k, v, do, P, out, scale):
    """(companion, T) per output name; do may be None (forward only)."""
    N = q.shape[-2]
    c = {"out": (P @ v.abs(), v.abs().sum(-2, keepdim=True).expand(-1, -1, N, -1))}
    if do is not None:
        M = k.shape[-2]
        cS = P * (do.abs() @ v.abs().transpose(-1, -2) + (do.abs() * out.abs()).sum(-1, keepdim=True))
        c["dv"] = (P.transpose(-1, -2) @ do.abs(), do.abs().sum(-2, keepdim=True).expand(-1, -1, M, -1))
        c["dq"] = (scale * cS @ k.abs(), scale * k.abs().sum(-2, keepdim=True).expand(-1, -1, N, -1))
        c["dk"] = (scale * cS.transpose(-1, -2) @ q.abs(), scale * q.abs().sum(-2, keepdim=True).expand(-1, -1, M, -1))
    return c


Ref = collections.namedtuple("Ref", "q k v do scale sc P out lse grads comp")


def self_attention(qkv, do=None, scale=None, prescaled=False):
    """The whole reference of one case.  qkv packed [B, N, 3, H, dh]; do [B, N, H*dh] or None; prescaled: q already carries
    dh^-0.5 log2(e), the kernel works in the exp2 domain (scale = ln 2 on the stored q).  Fields are [B, H, N, *]; grads and comp are
    dicts by output name."""
    q, k, v = heads(qkv)
    if prescaled:
        scale = LN2
    elif scale is None:
        scale = q.shape[-1] ** -0.5
    sc, P, out, lse = forward(q, k, v, scale)
    grads = {}
    if do is not None:
        do = to_heads(do, q.shape[1])
        grads = dict(zip(("dq", "dk", "dv"), backward(q, k, v, do, P, out, scale)))
    return Ref(q, k, v, do, scale, sc, P, out, lse, grads, companions(q, k, v, do, P, out, scale))


def cross_attention(q, k, v, do, heads_, scale):
    """Cross attention of countr_xattn_fwd / countr_xattn_bwd: q, do [B, N, D], k, v [B, S, D].  Returns (values, companions) with
    out, dq as [B, N, H, dh] and dk, dv as [B, S, H, dh]; companions as (companion, T) pairs like `companions`."""
    qh, kh, vh, doh = (to_heads(t, heads_) for t in (q, k, v, do))
    _, P, out, _ = forward(qh, kh, vh, scale)
    dq, dk, dv = backward(qh, kh, vh, doh, P, out, scale)
    comp = companions(qh, kh, vh, doh, P, out, scale)
    vals = {"out": out, "dq": dq, "dk": dk, "dv": dv}
    return {n: to_rows(t) for n, t in vals.items()}, {n: (to_rows(c), to_rows(t)) for n, (c, t) in comp.items()}


# ---------------------------------------------------------------------------------------------------------------- the bound
def attn_excess(out, ref, companion, flavour, K, floor, T=None):
    """max over ALL elements of |out - ref| - (K u companion + tiny T + floor rowmax(companion)) in fp64; <= 0: the bound holds everywhere.
    The three tensors have one shape, rows along the last axis.  flavour None: an fp32 output (u = tiny = 0, the floor alone).  A
    non-finite element of `out` where `ref` is finite (or the reverse) gives +inf."""
    o = out.detach().double().cpu()
    r = ref.detach().double().cpu()
    c = companion.detach().double().cpu()
    assert o.shape == r.shape == c.shape, (o.shape, r.shape, c.shape)
    if o.numel() == 0:
        return 0.0
    if not bool((torch.isfinite(o) == torch.isfinite(r)).all()) or not bool(torch.isfinite(r).all()):
        return float("inf")
    u, tiny = (flavour.u, flavour.tiny) if flavour is not None else (0.0, 0.0)
    bound = K * u * c + floor * c.amax(-1, keepdim=True)
    if T is not None and tiny:
        bound = bound + tiny * T.detach().double().cpu()
    return ((o - r).abs() - bound).max().item()


def assert_attn_rows(out, ref, companion, flavour, K, floor, T=None, what=""):
    ex = attn_excess(out, ref, companion, flavour, K, floor, T)
    assert ex <= 0.0, (what, "row-wise bound exceeded by", ex)


def assert_self_attention_rows(ref, fl, out=None, dqkv=None, what=""):
    """The kernels' outputs (out [B, N, H*dh], dqkv [B, N, 3, H, dh]; either may be None) against a Ref, each with its own K."""
    H = ref.q.shape[1]
    got = {}
    if out is not None:
        got["out"] = to_heads(out, H)
    if dqkv is not None:
        got.update({n: to_heads(dqkv[:, :, i], H) for i, n in enumerate(("dq", "dk", "dv"))})
    for n, g in got.items():
        want = ref.out if n == "out" else ref.grads[n]
        c, T = ref.comp[n]
        assert_attn_rows(g, want, c, fl, k_of(n, fl), F32_TOL, T, (what, n))


def lse_excess(lse, ref):
    """max of |lse - ref| - 1e-4 max(1, |ref|): the per-element form of the suite's lse bar."""
    a = lse.detach().double().cpu()
    r = ref.double()
    if not bool(torch.isfinite(a).all()):
        return float("inf")
    return ((a - r).abs() - 1e-4 * r.abs().clamp_min(1.0)).max().item()


# ---------------------------------------------------------------------------------------------------------------- emulation
def r16(x, fl):
    """Round an fp64 tensor to the flavour's 16-bit type (through fp32, as the kernels' pack2bf does) and back."""
    return x.float().to(fl.dtype).double()


def emulate(ref, fl):
    """The kernels' arithmetic in fp64 with their 16-bit roundings (module docstring): {"out", "dq", "dk", "dv"} as [B, H, N, dh]."""
    q, k, v, do, s = ref.q, ref.k, ref.v, ref.do, ref.scale
    m = ref.sc.amax(-1, keepdim=True)
    p = torch.exp(ref.sc - m)
    l = p.sum(-1, keepdim=True)                                 # from the unrounded p
    res = {"out": r16((r16(p, fl) @ v) / l, fl)}
    if do is not None:
        P = torch.exp(ref.sc - ref.lse[..., None])              # fp32 in the kernel, from the fp32 lse
        delta = (do * res["out"]).sum(-1, keepdim=True)         # the stored O
        dS16 = r16(P * (do @ v.transpose(-1, -2) - delta), fl)
        res["dq"] = r16(s * (dS16 @ k), fl)
        res["dk"] = r16(s * (dS16.transpose(-1, -2) @ q), fl)
        res["dv"] = r16(r16(P, fl).transpose(-1, -2) @ do, fl)
    return res


def emulate_cross(vals, fl):
    """Cross attention: out and dq rounded once, dk and dv untouched."""
    return {n: (r16(t, fl) if n in ("out", "dq") else t) for n, t in vals.items()}


def ratio(emu, ref, companion, fl):
    """max |emu - ref| / (u companion), the figure K is derived from (0 / 0 counts as 0)."""
    d = (emu - ref).abs()
    return torch.where(d == 0, torch.zeros_like(d), d / (fl.u * companion)).max().item()


# ---------------------------------------------------------------------------------------------------------------- inputs
def rnd(shape, seed, scale=1.0, dtype=torch.float32):
    """The suite's seeded normal sample (tests/test_kernels_gpu.py)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def signs(dh, seed):
    return (torch.randint(0, 2, (dh,), generator=torch.Generator().manual_seed(seed)) * 2 - 1).float()


Inputs = collections.namedtuple("Inputs", "qkv do scale prescaled")      # scale: what the kernel is given (0.0 = pre-scaled q)


def inputs_fwd_spiked(fl, B, N, H, dh):
    qkv = rnd((B, N, 3, H, dh), 50, 1.0).to(fl.dtype)
    qkv[0, N // 2, 1, 0] = 6.0  # one key with large logits against every query -> running max jumps mid-sequence
    return Inputs(qkv, None, dh ** -0.5, False)


def inputs_fwd_prescaled(fl, B, N, H):
    dh = 64
    qkv = rnd((B, N, 3, H, dh), 52, 1.0)
    qkv[0, N // 2, 1, 0] = 6.0
    qkv[0, N - 3, 1, H - 1] = -5.0
    qkv[:, :, 0] *= dh ** -0.5 * LOG2E
    return Inputs(qkv.to(fl.dtype), None, 0.0, True)


def inputs_fwd_far_above(fl, N, H, dh, pre, spike):
    B = 2
    qkv = rnd((B, N, 3, H, dh), 57, 1.0)
    sign = signs(dh, 58)
    for j in (70, N // 2 + 5, N - 2):                       # all behind key tile 0
        qkv[0, j, 1, 1] = spike * sign
    qkv[1, N - 1, 1, H - 1] = spike * sign                  # ... and the very last key of another (batch, head)
    if pre:
        qkv[:, :, 0] *= dh ** -0.5 * LOG2E
    return Inputs(qkv.to(fl.dtype), None, 0.0 if pre else dh ** -0.5, pre)


def inputs_fwd_ragged_spike(fl, N, H, dh):
    qkv = rnd((2, N, 3, H, dh), 59, 1.0)
    sign = signs(dh, 60)
    qkv[0, N - 1, 1, 1] = 40.0 * sign
    qkv[0, 10, 1, 1] = -6.0 * sign
    return Inputs(qkv.to(fl.dtype), None, dh ** -0.5, False)


def inputs_bwd_spiked(fl, B, N, H, dh):
    qkv = (rnd((B, N, 3, H, dh), 60, 1.0)).to(fl.dtype)
    qkv[0, N // 3, 1, 0] = 5.0
    return Inputs(qkv, rnd((B, N, H * dh), 61, 1.0).to(fl.dtype), dh ** -0.5, False)


GRID_LIFT = 60.0      # the lifted key of head 2 scores up to 60 |z| natural units (86 log2 units) above or below the others


def grid_lift_key(N):
    return 64 + (N - 64) // 2 if N > 64 else None


def inputs_grid(fl, B, N, H, dh):
    """The small-shape grid: a spiked key at N - 1 (head 0) and one at key 0 (head 1) of batch 0; for N > 64 one key behind tile 0
    (head 2) that lies far above the first tile's maximum for the query rows on one side of a sign pattern and far below it for the
    others."""
    qkv = rnd((B, N, 3, H, dh), 70, 1.0)
    qkv[0, N - 1, 1, 0] = 6.0
    qkv[0, 0, 1, 1] = 6.0
    if N > 64:
        qkv[0, grid_lift_key(N), 1, 2] = GRID_LIFT * signs(dh, 72)
    return Inputs(qkv.to(fl.dtype), rnd((B, N, H * dh), 71, 1.0).to(fl.dtype), dh ** -0.5, False)


def lift_rows(ref):
    """(rows of batch 0, head 2 whose maximum lies more than 64 log2 units above the first key tile's, rows where it lies less than 1
    above): the reference-side condition of the far-above tests."""
    sc = ref.sc[0, 2]
    top = (sc.max(-1).values - sc[:, :64].max(-1).values) * (1.0 if ref.scale == LN2 else LOG2E)
    return int((top > 64).sum()), int((top < 1).sum())


FWD_SHAPES = [(2, 576, 12, 64), (2, 576, 16, 32), (1, 200, 3, 64), (1, 64, 2, 32), (2, 729, 16, 32)]
PRE_SHAPES = [(2, 576, 12), (1, 64, 3), (1, 1088, 2)]
FAR_SHAPES = [(576, 12, 64, False, 40.0), (576, 12, 64, True, 40.0), (576, 12, 64, True, 250.0), (576, 16, 32, False, 60.0),
              (200, 3, 64, False, 60.0), (288, 12, 64, False, 250.0)]
RAGGED_SPIKE_SHAPES = [(200, 3, 64), (729, 16, 32)]                      # fp16 library only
BWD_SHAPES = [(2, 576, 16, 32), (1, 576, 12, 64), (1, 200, 3, 32), (2, 64, 2, 64)]
GRID_N = [1, 17, 33, 63, 64, 65, 127, 128, 129, 192, 193, 257]
GRID_BH = [(1, 3), (2, 4)]
GRID_SHAPES = [(B, N, H, dh) for dh in (32, 64) for (B, H) in GRID_BH for N in GRID_N]
BWD_HUGE = (1, 729, 16, 32)
PRE_SMALL = [(1, 128, 3), (2, 192, 4)]


def CASES(fl):
    """(name, Inputs) of every attention case the GPU tests run on this flavour, lazily."""
    for s in FWD_SHAPES:
        yield "fwd%s" % (s,), (lambda s=s: inputs_fwd_spiked(fl, *s))
    for s in PRE_SHAPES + PRE_SMALL:
        yield "pre%s" % (s,), (lambda s=s: inputs_fwd_prescaled(fl, *s))
    for s in FAR_SHAPES:
        yield "far%s" % (s,), (lambda s=s: inputs_fwd_far_above(fl, *s))
    if fl is HP.FP16:
        for s in RAGGED_SPIKE_SHAPES:
            yield "ragged%s" % (s,), (lambda s=s: inputs_fwd_ragged_spike(fl, *s))
    for s in BWD_SHAPES + [BWD_HUGE]:
        yield "bwd%s" % (s,), (lambda s=s: inputs_bwd_spiked(fl, *s))
    for s in GRID_SHAPES:
        yield "grid%s" % (s,), (lambda s=s: inputs_grid(fl, *s))


def reference_of(inp):
    return self_attention(inp.qkv, inp.do, None if inp.prescaled else inp.scale, inp.prescaled)


def measure():
    worst = {n: {} for n in ("out", "dq", "dk", "dv")}
    for fl in HP.FLAVOURS:
        for name, make in CASES(fl):
            ref = reference_of(make())
            emu = emulate(ref, fl)
            for n, e in emu.items():
                want = ref.out if n == "out" else ref.grads[n]
                x = ratio(e, want, ref.comp[n][0], fl)
                if x > worst[n].get(flavour_name(fl), (0.0, ""))[0]:
                    worst[n][flavour_name(fl)] = (x, name)
    for n, per in worst.items():
        for f, (x, name) in per.items():
            print("%-3s %s  measured %.3f  (%s)  -> K = %d" % (n, f, x, name, int(math.ceil(2 * x))))


if __name__ == "__main__":
    measure()
