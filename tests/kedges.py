"""Shape-edge cases of the small kernels (softmax, LayerNorm, column sums, GELU backward, masked MSE, AdamW, patch gather, first exemplar
conv): the seeded inputs, the fp64 references, the assertions and the guard bands.  Pure torch; nothing here touches a kernel.

tests/test_kernel_edges_gpu.py and the widened cases of tests/test_kernels_gpu.py hand the kernels' outputs to the assertions below;
tests/test_kernel_edges_cpu.py hands them an fp32 torch emulation of the same operation (rounded to the 16-bit type where the kernel stores
16 bits), which must pass, and deliberately wrong variants of it, which must not -- the pattern of tests/attnref.py and
tests/test_attnref_cpu.py.  No bar is new: DT's max-norm bar per mode, 1e-4 / 1e-5 for fp32 reductions as the existing test of the same
kernel has it, halfprec.assert_elementwise with the fp32 bar as floor for 16-bit outputs that are one rounding of an fp32 result."""
import math

import torch

import halfprec as HP

# (torch dtype, dtype code of the C ABI, max-norm bar): the three modes of tests/test_kernels_gpu.py
DT = [(torch.float32, 0, 2e-4), (torch.bfloat16, 1, 2e-2), (torch.float16, 1, 2.5e-3)]
F32_TOL = DT[0][2]
GUARD = 256                 # sentinel elements before and after every output (1 KiB of fp32: pointers keep their 16-byte alignment)


def rnd(shape, seed, scale=1.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def relerr(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def flavour(tdt):
    return HP.BY_DTYPE.get(tdt)


def half_of(tdt):
    """The 16-bit type of the library a mode runs on (fp32 mode runs on the bf16 build)."""
    return tdt if tdt in HP.BY_DTYPE else torch.bfloat16


# ---------------------------------------------------------------------------------------------------------------- guard bands
def bits(t):
    return t.view({1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


class Guarded:
    """A tensor `t` of `shape` inside one allocation with GUARD sentinel elements before and after it (and `lead` more in front: an
    offset of `lead` elements from the allocator's alignment).  The sentinel (NaN unless `fill` says otherwise) also fills `t`, or `body`
    does.  intact(): the bands are bit-identical to what they were; unchanged(): so is the tensor itself (a refused call)."""

    def __init__(self, shape, dtype=torch.float32, device="cpu", fill=float("nan"), body=None, lead=0):
        shape = tuple(shape) if isinstance(shape, (tuple, list, torch.Size)) else (shape,)
        n = math.prod(shape)
        self.lo = GUARD + lead
        self.buf = torch.full((self.lo + n + GUARD,), fill, dtype=dtype, device=device)
        self.t = self.buf[self.lo:self.lo + n].view(shape)
        if body is not None:
            self.t.copy_(body)
        self.n = n
        self.was = bits(self.buf).clone()

    def intact(self):
        now = bits(self.buf)
        return torch.equal(now[:self.lo], self.was[:self.lo]) and torch.equal(now[self.lo + self.n:], self.was[self.lo + self.n:])

    def unchanged(self):
        return torch.equal(bits(self.buf), self.was)


def all_intact(*gs):
    return all(g.intact() for g in gs)


# ---------------------------------------------------------------------------------------------------------------- softmax
SOFTMAX_SHAPES = [(1, 1), (3, 63), (5, 64), (7, 65), (6, 729), (4, 1024), (9, 1023)]      # (rows, n)
SOFTMAX_LD = [(729, 736), (1, 8), (63, 64), (1017, 1024)]                                   # (n, ld), at SOFTMAX_LD_ROWS rows
SOFTMAX_LD_ROWS = 5
SOFTMAX_FAMILIES = ["normal", "offset", "spike"]
SOFTMAX_PAD = 1e30          # what the score pad columns n .. ld - 1 hold: finite, and fatal to the statistics if ever read
SOFTMAX_BWD_SCALE = 0.25


def softmax_scores(family, rows, n, ld=None):
    """fp32 scores [rows, ld], pad columns = SOFTMAX_PAD.  normal: N(0, 3^2), the existing test's; offset: the same at +1e4 (exp of the raw
    score overflows, the row maximum must be subtracted first); spike: one score per row 80 above the largest of the others (every other
    P is below 2^-115: fp16 flushes it, the sum is the spike alone)."""
    ld = n if ld is None else ld
    s = torch.full((rows, ld), SOFTMAX_PAD)
    body = rnd((rows, n), 13, 3.0)
    if n > 1:
        body[rows - 1, n - 1] = body[rows - 1, :n - 1].max() + 1.0     # the last row's LAST column is its heaviest: a lost ragged tail shows under a max-norm bar
    if family == "offset":
        body = body + 1e4
    elif family == "spike":
        for r in range(rows):
            j = softmax_spike_column(r, rows, n)
            rest = torch.cat([body[r, :j], body[r, j + 1:]])
            body[r, j] = (rest.max().item() if n > 1 else 0.0) + 80.0
    else:
        assert family == "normal", family
    s[:, :n] = body
    return s


def softmax_spike_column(r, rows, n):
    return n - 1 if r == rows - 1 else (7 * r + 3) % n


def softmax_dp(rows, n):
    """The backward's dP: the existing test's N(0, 1), with a large last element (see softmax_scores)."""
    dp = rnd((rows, n), 14)
    dp[rows - 1, n - 1] = 2.0
    return dp


def softmax_ref(s, n):
    return torch.softmax(s[:, :n].double(), -1)


def assert_softmax(p, s, n, tdt, tol):
    """p [rows, ld] of any device against the fp64 softmax of the first n columns of the fp32 scores s [rows, ld]."""
    p = p.detach().cpu()
    pr = softmax_ref(s, n)
    assert relerr(p[:, :n], pr) < tol, relerr(p[:, :n], pr)
    if flavour(tdt):
        HP.assert_elementwise(p[:, :n], pr, flavour(tdt), F32_TOL, "softmax")
    assert torch.equal(p[:, n:], torch.zeros_like(p[:, n:])), "pad columns of P are not exact zeros"
    if n == 1:
        assert torch.equal(p[:, :1], torch.ones_like(p[:, :1])), "softmax of one score is not exactly 1"


def softmax_emulate(s, n, tdt):
    """fp32 torch softmax of columns < n, zeros behind, rounded to the mode's type."""
    p = torch.zeros(s.shape)
    p[:, :n] = torch.softmax(s[:, :n], -1)
    return p.to(tdt)


def softmax_bwd_ref(p, dp, scale):
    pp, dd = p.detach().double().cpu(), dp.double()
    return pp * (dd - (pp * dd).sum(-1, keepdim=True)) * scale


def assert_softmax_bwd(ds, p, dp, scale, tdt, tol):
    """ds against the fp64 backward evaluated from the kernel's own (rounded) P, as test_softmax_fwd_bwd does."""
    ref = softmax_bwd_ref(p, dp, scale)
    assert relerr(ds, ref) < tol, relerr(ds, ref)
    if flavour(tdt):
        HP.assert_elementwise(ds.detach().cpu(), ref, flavour(tdt), F32_TOL, "softmax bwd")
    if p.shape[-1] == 1:
        assert torch.equal(ds.detach().cpu().float(), torch.zeros(p.shape)), "dS of a one-score row is not exactly 0"


def softmax_bwd_emulate(p, dp, scale, tdt):
    pf = p.detach().cpu().float()
    return (pf * (dp - (pf * dp).sum(-1, keepdim=True)) * scale).to(tdt)


# ---------------------------------------------------------------------------------------------------------------- cross attention
XATTN_S = [2, 4, 5, 7]                                  # added to test_cross_attention_fwd_bwd (N = 576)
XATTN_SHORT = [(65, 2), (1, 5), (17, 7)]                # added to the short-sequence test
XATTN_PACKED_S = [1, 2, 3, 5, 8, 9, 14]                 # k | v as the column halves of one [B * S, 1024] buffer
XATTN_PACKED_N = 37                                     # three backward blocks per image, the last of five rows
XATTN_B, XATTN_D, XATTN_HEADS = 2, 512, 16
XATTN_CASES = [(576, S) for S in XATTN_S] + XATTN_SHORT + [(XATTN_PACKED_N, S) for S in XATTN_PACKED_S]


def xattn_inputs(N, S, tdt):
    """q, k, v, do of _cross_attention_fwd_bwd (tests/test_kernels_gpu.py), rounded to the mode's type."""
    B, D = XATTN_B, XATTN_D
    return (rnd((B, N, D), 15).to(tdt), rnd((B, S, D), 16).to(tdt), rnd((B, S, D), 17).to(tdt), rnd((B, N, D), 18).to(tdt))


def xattn_reference(q, k, v, do):
    """fp64 out, dq, dk, dv by autograd, as _cross_attention_fwd_bwd computes them (its max-norm bars are stated against these: at S = 1
    autograd's dq is an exact zero, the hand-written backward of tests/attnref.py leaves 1e-17)."""
    B, N, D = q.shape
    S, Hh, scale = k.shape[1], XATTN_HEADS, 32 ** -0.5
    qr, kr, vr = (t.double().requires_grad_(True) for t in (q, k, v))
    qh, kh, vh = (t.reshape(B, -1, Hh, 32).transpose(1, 2) for t in (qr, kr, vr))
    a = torch.softmax(qh @ kh.transpose(-1, -2) * scale, -1)
    out = (a @ vh).transpose(1, 2).reshape(B, N, D)
    out.backward(do.double())
    return {"out": out.detach(), "dq": qr.grad, "dk": kr.grad, "dv": vr.grad}


def pack_kv(k, v):
    """[B * S, 2 D]: row = (k row | v row), the engine's default layout (ldkv = 2 D)."""
    B, S, D = k.shape
    return torch.cat([k.reshape(B * S, D), v.reshape(B * S, D)], 1).contiguous()


def kv_read_at_pitch(kv, B, S, D, ld):
    """What a kernel reads as k and v from the packed buffer (k at element 0, v at element D) when it walks rows at pitch ld."""
    flat = kv.reshape(-1)
    rows = torch.arange(B * S)[:, None] * ld + torch.arange(D)[None, :]
    return flat[rows].reshape(B, S, D), flat[rows + D].reshape(B, S, D)


# ---------------------------------------------------------------------------------------------------------------- LayerNorm
LN_D = [4, 252, 384, 640, 1280, 2048]                   # added to test_layernorm_fwd_bwd at rows = 1157
LN_ROWS = [1, 3, 9, 2049]                               # x LN_ROWS_D: below one grid pass of the backward (256 blocks x 8 waves), and one row past it
LN_ROWS_D = [512, 1280]


def ln_inputs(rows, D, tdt):
    """x, gamma, beta (fp32), dy (the mode's type) of test_layernorm_fwd_bwd."""
    return rnd((rows, D), 1, 2.0) + 0.3, 1 + 0.1 * rnd((D,), 2), 0.1 * rnd((D,), 3), rnd((rows, D), 4).to(tdt)


def ln_reference(x, g, b, dy):
    """fp64: y, dx, dgamma, dbeta of nn.LayerNorm(eps = 1e-6)."""
    xr, gr, br = (t.double().requires_grad_(True) for t in (x, g, b))
    mu = xr.mean(-1, keepdim=True)
    var = ((xr - mu) ** 2).mean(-1, keepdim=True)
    y = (xr - mu) / torch.sqrt(var + 1e-6) * gr + br
    y.backward(dy.double())
    return y.detach(), xr.grad, gr.grad, br.grad


def assert_layernorm(y, dx, dg, db, ref, tdt, tol):
    yr, dxr, dgr, dbr = ref
    assert relerr(y, yr) < tol, relerr(y, yr)
    if flavour(tdt):
        HP.assert_elementwise(y, yr, flavour(tdt), F32_TOL, "layernorm y")
    assert relerr(dx, dxr) < 1e-4, relerr(dx, dxr)
    assert relerr(dg, dgr) < 1e-4, relerr(dg, dgr)
    assert relerr(db, dbr) < 1e-4, relerr(db, dbr)


def ln_emulate(x, g, b, dy, tdt, cols=None):
    """fp32 torch; cols < D: the statistics and the column sums of the backward see only the first `cols` columns (a lost ragged group)."""
    D = x.shape[-1]
    cols = D if cols is None else cols
    xr, gr, br = (t.clone().requires_grad_(True) for t in (x, g, b))
    mu = xr[:, :cols].mean(-1, keepdim=True)
    var = ((xr[:, :cols] - mu) ** 2).mean(-1, keepdim=True)
    y = (xr - mu) / torch.sqrt(var + 1e-6) * gr + br
    y.backward(dy.float())
    return y.detach().to(tdt), xr.grad, gr.grad, br.grad


# ---------------------------------------------------------------------------------------------------------------- column sums
COLSUM_SHAPES = [(1, 8), (3, 24), (130, 24), (1, 2048), (257, 520), (1152, 2056)]          # (M, N)
COLSUM_SENTINEL = 777.0     # what `out` holds before an accumulate = 0 call: must be overwritten, not added to


def colsum_input(M, N, tdt):
    return rnd((M, N), 27).to(tdt)


def assert_colsum(out, x, accumulate, before):
    """out against the fp64 column sums of the rounded x, plus what out held before where the call accumulates."""
    ref = x.double().sum(0) + (before.double() if accumulate else 0.0)
    assert relerr(out, ref) < 1e-4, relerr(out, ref)


# ---------------------------------------------------------------------------------------------------------------- GELU backward
GELU_N = [8, 8 * 257]
GELU_PAST_CAP = 8192 * 256 * 8 + 8 * 257                # one grid pass of the capped grid (8192 blocks x 256 threads x 8) and 257 vectors more


def gelu_inputs(n, tdt):
    return rnd((n,), 26, 1.5).to(tdt), rnd((n,), 27).to(tdt)


def gelu_bwd_ref(pre, dh):
    """dh * d/dx [x Phi(x)] in fp64 (nn.GELU, erf form), on the device of its arguments."""
    x, d = pre.double(), dh.double()
    return d * (0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi))


def assert_gelu_bwd(out, pre, dh, tol):
    ref = gelu_bwd_ref(pre, dh)
    err = ((out.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()       # relerr, where the tensors live
    assert err < tol, err


# ---------------------------------------------------------------------------------------------------------------- masked MSE
MSE_CASES = [(1, 4, 0), (1, 7, 0), (5, 1023, 0), (2, 64 * 256 * 4 + 4, 0), (3, 4096, 1)]     # (B, HW, floats `pred` is off a 16-byte boundary)
MSE_SCALES = [1.0, 128.0]


def mse_inputs(B, HW):
    g = torch.Generator().manual_seed(30)
    pred, gt = torch.rand((B, HW), generator=g), torch.rand((B, HW), generator=g)
    return pred, gt, (torch.rand(HW, generator=g) < 0.8).float()


def mse_reference(pred, gt, mask, grad_scale):
    """fp64: loss = sum((pred - gt)^2 mask / HW) / B, grad_scale * dloss/dpred, counts of pred and gt (sum / 60)."""
    B, HW = pred.shape
    pr = pred.double().requires_grad_(True)
    loss = (((pr - gt.double()) ** 2) * mask.double() / HW).sum() / B
    loss.backward()
    return loss.detach(), pr.grad * grad_scale, pred.double().sum(1) / 60.0, gt.double().sum(1) / 60.0


def assert_masked_mse(sums, dpred, ref):
    loss, dref, cp, cg = ref
    B = cp.numel()
    sums = sums.detach().double().cpu()
    assert abs(sums[0].item() - loss.item()) <= 1e-5 * loss.item(), (sums[0].item(), loss.item())
    assert relerr(sums[1:1 + B], cp) < 1e-5 and relerr(sums[1 + B:], cg) < 1e-5
    if dpred is not None:
        assert relerr(dpred, dref) < 1e-5, relerr(dpred, dref)


def mse_emulate(pred, gt, mask, grad_scale):
    B, HW = pred.shape
    d = pred - gt
    sums = torch.cat([((d * d * mask).sum() / (HW * B)).reshape(1), pred.sum(1) / 60.0, gt.sum(1) / 60.0])
    return sums, 2.0 * d * mask / (HW * B) * grad_scale


# ---------------------------------------------------------------------------------------------------------------- AdamW
ADAM_N = 5000
ADAM_RANGES = [(3, 4), (4, 1001), (1500, 1503), (2049, 4099)]       # a one-element range, starts off a multiple of 4, gaps between ranges
ADAM_WDS = [0.05, 0.0, 0.1, 0.02]
ADAM_GROUPS = [0, 1, 2, 1]                                          # the step counter each range follows
ADAM_GROUP_START = [1, 2, 3]                                        # the step at which a group's counter starts: group g has taken max(0, step - start + 1) steps
ADAM_LR, ADAM_B1, ADAM_B2, ADAM_EPS = 1e-3, 0.9, 0.95, 1e-8


def adam_inside():
    m = torch.zeros(ADAM_N, dtype=torch.bool)
    for a, b in ADAM_RANGES:
        m[a:b] = True
    return m


def adam_reference(p0, grads, steps_of_range):
    """torch.optim.AdamW in fp64, one parameter per range; grads: one [ADAM_N] gradient per step; steps_of_range[r]: the steps (indices
    into grads) range r takes part in.  Returns the parameters after every step, as full vectors (outside the ranges: p0)."""
    params = [torch.nn.Parameter(p0[a:b].double().clone()) for a, b in ADAM_RANGES]
    opt = torch.optim.AdamW([{"params": [q], "weight_decay": wd} for q, wd in zip(params, ADAM_WDS)], lr=ADAM_LR,
                            betas=(ADAM_B1, ADAM_B2), eps=ADAM_EPS)
    out = []
    for i, g in enumerate(grads):
        for r, ((a, b), q) in enumerate(zip(ADAM_RANGES, params)):
            q.grad = g[a:b].double().clone() if i in steps_of_range[r] else None
        opt.step()
        full = p0.double().clone()
        for (a, b), q in zip(ADAM_RANGES, params):
            full[a:b] = q.detach()
        out.append(full)
    return out


def adam_emulate_step(p, g, m, v, t_of_range):
    """One fp32 step over the ranges (t_of_range[r]: steps range r has taken, this one included; 0 = not stepped); returns new p, m, v."""
    p, m, v = p.clone(), m.clone(), v.clone()
    for (a, b), wd, t in zip(ADAM_RANGES, ADAM_WDS, t_of_range):
        if t < 1:
            continue
        m[a:b] = ADAM_B1 * m[a:b] + (1 - ADAM_B1) * g[a:b]
        v[a:b] = ADAM_B2 * v[a:b] + (1 - ADAM_B2) * g[a:b] * g[a:b]
        p[a:b] = p[a:b] * (1 - ADAM_LR * wd) - ADAM_LR * (m[a:b] / (1 - ADAM_B1 ** t)) / ((v[a:b] / (1 - ADAM_B2 ** t)).sqrt() + ADAM_EPS)
    return p, m, v


def assert_adam(p, ref, before):
    """Inside the ranges the fp64 AdamW within 1e-5 (max-norm, the bar of _masked_mse_and_adamw); outside bit-identical to `before`."""
    inside = adam_inside()
    p = p.detach().cpu()
    assert relerr(p[inside], ref[inside]) < 1e-5, relerr(p[inside], ref[inside])
    assert torch.equal(bits(p[~inside]), bits(before[~inside])), "an element outside the ranges changed"


# ---------------------------------------------------------------------------------------------------------------- patch gather, first conv
IM2PATCH_CASES = [(2, 28, 42, 14), (1, 16, 24, 8), (1, 19, 30, 8), (1, 24, 18, 6)]          # (B, H, W, patch)
C3_SHAPES = [(2, 5, 7), (1, 1, 1), (3, 9, 6)]                                               # (S, H, W): W % 4 != 0, the per-pixel kernel


def im2patch_image(B, H, W):
    return torch.rand((B, 3, H, W), generator=torch.Generator().manual_seed(19))


def im2patch_ref(img, p):
    B, _, H, W = img.shape
    gh, gw = H // p, W // p
    return img[:, :, :gh * p, :gw * p].reshape(B, 3, gh, p, gw, p).permute(0, 2, 4, 1, 3, 5).reshape(B * gh * gw, 3 * p * p)


def assert_im2patch(out, ref, tdt):
    """A gather computes nothing: exact in fp32, the rounding of the pixel in 16 bits."""
    if flavour(tdt):
        HP.assert_elementwise(out, ref, flavour(tdt), 0.0, "im2patch")
        assert torch.equal(out.detach().cpu(), ref.to(tdt))
    else:
        assert torch.equal(out.detach().cpu(), ref)


def c3_inputs(S, H, W, tdt):
    x = torch.rand((S, 3, H, W), generator=torch.Generator().manual_seed(61))
    return x, rnd((64, 3, 3, 3), 62, 0.2), rnd((64,), 63, 0.1), rnd((S, H, W, 64), 72).to(tdt)


def c3_reference(x, w, bias, dy):
    """fp64 conv2d (padding 1), NHWC, and the gradients of w and bias under dy."""
    wr, br = w.double().requires_grad_(True), bias.double().requires_grad_(True)
    y = torch.nn.functional.conv2d(x.double(), wr, br, padding=1)
    y.backward(dy.double().permute(0, 3, 1, 2))
    return y.detach().permute(0, 2, 3, 1), wr.grad, br.grad


def assert_c3(y, dw, db, ref, tdt, tol):
    yr, dwr, dbr = ref
    assert relerr(y, yr) < tol, relerr(y, yr)
    if flavour(tdt):
        HP.assert_elementwise(y, yr, flavour(tdt), F32_TOL, "c3 conv")
    assert relerr(dw, dwr) < 1e-4 and relerr(db, dbr) < 1e-4, (relerr(dw, dwr), relerr(db, dbr))
