"""fp64 references of the launches of the exemplar CNN (conv, InstanceNorm, ReLU, pool) and of the density head (conv, GroupNorm, ReLU,
bilinear x2), and the bars a launch is held to when it is compared with fp64 arithmetic on ITS OWN inputs -- the rounded buffers the
engine left in place -- so that every stage is one rounding of an fp32 computation (tests/halfprec.py's element-wise bound).

Maps are NHWC [N, H, W, C], as the engine keeps them; convolution weights are OHWI [Co, 3, 3, Ci] (the engine's forward shadow) unless
stated.  Every helper runs where its inputs live (CPU or GPU) and returns fp64.  Nothing here is measured on the code under test:
F32_TOL is the fp32 bar of tests/test_kernels_gpu.py, STAT_TOL the bar of test_groupnorm_statistics_from_row_partials.
tests/test_stagecheck_cpu.py checks every helper against torch autograd."""
import os

import torch
import torch.nn.functional as F

import halfprec as HP

F32_TOL = 2e-4
STAT_TOL = 3e-6
GATE_MARGIN = 2.0 ** -16      # a ReLU gate decided from an fp32 y is taken as undecidable within this of zero (relative to |gamma xhat| + |beta|)
GATE_SHARE = 1e-4             # ... and a stage may leave out at most this share of a map for it


# ---------------------------------------------------------------- 3x3 convolution, pad 1, as nine shifted matrix products
def _pad(x):
    return F.pad(x.double(), (0, 0, 1, 1, 1, 1))


def conv3x3(x, w, bias=None):
    """y[n, h, w, co] = sum x[n, h + ky - 1, w + kx - 1, ci] w[co, ky, kx, ci] (+ bias)."""
    N, H, W, Ci = x.shape
    w, xp = w.double(), _pad(x)
    out = torch.zeros((N * H * W, w.shape[0]), dtype=torch.float64, device=x.device)
    for ky in range(3):
        for kx in range(3):
            out += xp[:, ky:ky + H, kx:kx + W].reshape(-1, Ci) @ w[:, ky, kx].t()
    if bias is not None:
        out += bias.double()
    return out.view(N, H, W, -1)


def conv3x3_dgrad(dy, w):
    """dx[n, h, w, ci] = sum dy[n, h - ky + 1, w - kx + 1, co] w[co, ky, kx, ci]."""
    N, H, W, Co = dy.shape
    w, dp = w.double(), _pad(dy)
    out = torch.zeros((N * H * W, w.shape[3]), dtype=torch.float64, device=dy.device)
    for ky in range(3):
        for kx in range(3):
            out += dp[:, 2 - ky:2 - ky + H, 2 - kx:2 - kx + W].reshape(-1, Co) @ w[:, ky, kx]
    return out.view(N, H, W, -1)


def conv3x3_wgrad(dy, x):
    """dw[co, ci, ky, kx] = sum dy[n, h, w, co] x[n, h + ky - 1, w + kx - 1, ci]: torch's OIHW, the layout of the parameter gradient."""
    N, H, W, Ci = x.shape
    d, xp = dy.double().reshape(N * H * W, -1), _pad(x)
    out = torch.zeros((d.shape[1], Ci, 3, 3), dtype=torch.float64, device=x.device)
    for ky in range(3):
        for kx in range(3):
            out[:, :, ky, kx] = d.t() @ xp[:, ky:ky + H, kx:kx + W].reshape(-1, Ci)
    return out


def bias_grad(dy):
    return dy.double().reshape(-1, dy.shape[-1]).sum(0)


def ohwi(w_oihw):
    return w_oihw.permute(0, 2, 3, 1).contiguous()


def ohwi_of_dgrad_form(wd, Co, Ci):
    """The engine's dgrad shadow Wd[ci][2 - ky][2 - kx][co] (a forward convolution with it IS the input gradient) back as OHWI."""
    return wd.view(Ci, 3, 3, Co).flip(1, 2).permute(3, 1, 2, 0).contiguous()


# ---------------------------------------------------------------- the two pools
def _windows(x):
    """[N, H, W, C] -> [N, H/2, W/2, C, 4], a window's pixels in torch's scan order (0,0), (0,1), (1,0), (1,1)."""
    N, H, W, C = x.shape
    assert H % 2 == 0 and W % 2 == 0
    return x.reshape(N, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(N, H // 2, W // 2, C, 4)


def maxpool2(x):
    """MaxPool2d(2) in x's own dtype (exact)."""
    return _windows(x).amax(-1)


def maxpool2_bwd(x, dy):
    """dy routed to the FIRST maximum of every window of x, as torch does."""
    N, H, W, C = x.shape
    w = _windows(x)
    best, arg = w[..., 0], torch.zeros(w.shape[:-1], dtype=torch.long, device=x.device)
    for q in (1, 2, 3):
        up = w[..., q] > best
        best, arg = torch.where(up, w[..., q], best), torch.where(up, torch.full_like(arg, q), arg)
    g = (arg.unsqueeze(-1) == torch.arange(4, device=x.device)).double() * dy.double().unsqueeze(-1)
    return g.view(N, H // 2, W // 2, C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(N, H, W, C)


def avgpool(x):
    """AdaptiveAvgPool2d(1): [N, H, W, C] -> [N, C]."""
    return x.double().mean((1, 2))


def avgpool_bwd(dy, H, W):
    return (dy.double() / (H * W))[:, None, None, :].expand(dy.shape[0], H, W, dy.shape[1])


# ---------------------------------------------------------------- InstanceNorm2d(affine=False) + ReLU + pool
def instnorm_stats(x, eps=1e-5):
    """[N, H, W, C] -> [N, C, 2] = (mean, rstd), biased variance."""
    x = x.double()
    return torch.stack([x.mean((1, 2)), (x.var((1, 2), unbiased=False) + eps).rsqrt()], -1)


def instnorm_xhat(x, stats):
    return (x.double() - stats[:, None, None, :, 0].double()) * stats[:, None, None, :, 1].double()


def instnorm_relu_pool_bwd(xhat, rstd, dyp, avg):
    """Backward of pool(relu(xhat)), xhat = (x - mean) rstd, w.r.t. x FROM A STORED xhat [N, H, W, C] and rstd [N, C]: the gate and the
    max-pool routing read the stored values (exact), dx = rstd (g - mean(g) - xhat mean(g xhat))."""
    N, H, W, C = xhat.shape
    xh = xhat.double()
    g = avgpool_bwd(dyp, H, W) if avg else maxpool2_bwd(xhat, dyp)
    g = g * (xh > 0)
    m1, m2 = g.mean((1, 2), keepdim=True), (g * xh).mean((1, 2), keepdim=True)
    return rstd.double()[:, None, None, :] * (g - m1 - xh * m2)


# ---------------------------------------------------------------- GroupNorm(G, C) + ReLU (+ the fused 1x1 head)
def groupnorm_stats(x, G=8, eps=1e-5):
    """[B, ..., C] -> [B, G, 2] = (mean, rstd) over a group's channels and all pixels."""
    B, C = x.shape[0], x.shape[-1]
    v = x.double().reshape(B, -1, G, C // G)
    return torch.stack([v.mean((1, 3)), (v.var((1, 3), unbiased=False) + eps).rsqrt()], -1)


def _per_channel(stats, x):
    B, C, G = x.shape[0], x.shape[-1], stats.shape[1]
    shape = [B] + [1] * (x.dim() - 2) + [C]
    return (stats[..., 0].double().repeat_interleave(C // G, 1).view(shape), stats[..., 1].double().repeat_interleave(C // G, 1).view(shape))


def groupnorm_relu(x, stats, gamma, beta):
    mean, rstd = _per_channel(stats, x)
    return torch.relu((x.double() - mean) * rstd * gamma.double() + beta.double())


def head1x1(y, w1, b1):
    """Conv2d(C, 1, 1): [B, ..., C] -> [B, ...]."""
    return (y.double() * w1.double().reshape(-1)).sum(-1) + b1.double().reshape(())


def groupnorm_relu_bwd(x, stats, gamma, beta, dy=None, d1=None, w1=None):
    """Backward of y = relu(gamma xhat + beta) w.r.t. x, from x [B, ..., C] and its (mean, rstd) [B, G, 2]; the gradient of y is dy, or
    d1[..., None] * w1 for the fused 1x1 head.  Returns
      dx    = rstd (g gamma - m1 - xhat m2), g = dy 1[y > 0], m1 / m2 the group means of g gamma and g gamma xhat;
      sums  [B, 3, C] = per image {sum g, sum g xhat, sum d1 y} (dbeta, dgamma, dw1 before the sum over images; the last plane is
            zero without d1);
      near  the elements whose pre-activation lies within GATE_MARGIN (|gamma xhat| + |beta|) of zero."""
    B, C, G = x.shape[0], x.shape[-1], stats.shape[1]
    mean, rstd = _per_channel(stats, x)
    ga, be = gamma.double(), beta.double()
    xh = (x.double() - mean) * rstd
    y = xh * ga + be
    near = y.abs() <= GATE_MARGIN * ((ga * xh).abs() + be.abs())
    if dy is None:
        dy = d1.double().unsqueeze(-1) * w1.double().reshape(-1)
    g = dy.double() * (y > 0)
    red = tuple(range(1, x.dim() - 1))
    third = (d1.double().unsqueeze(-1) * torch.relu(y)).sum(red) if d1 is not None else torch.zeros((B, C), dtype=torch.float64, device=x.device)
    sums = torch.stack([g.sum(red), (g * xh).sum(red), third], 1)
    del y
    gg = g * ga
    n = float(x[0].numel() // G)
    shape = [B] + [1] * (x.dim() - 2) + [C]
    grp = lambda t: (t.sum(red).view(B, G, C // G).sum(-1) / n).repeat_interleave(C // G, 1).view(shape)
    m1, m2 = grp(gg), grp(gg * xh)
    return rstd * (gg - m1 - xh * m2), sums, near


# ---------------------------------------------------------------- bilinear x2, align_corners=False, and its adjoint
def _up_matrix(n, device):
    """[2n, n]: out[2i] = .25 in[i - 1] + .75 in[i], out[2i + 1] = .75 in[i] + .25 in[i + 1], indices clamped."""
    U = torch.zeros((2 * n, n), dtype=torch.float64, device=device)
    i = torch.arange(n, device=device)
    for rows, cols, wgt in ((2 * i, (i - 1).clamp(min=0), 0.25), (2 * i, i, 0.75), (2 * i + 1, i, 0.75), (2 * i + 1, (i + 1).clamp(max=n - 1), 0.25)):
        U.index_put_((rows, cols), torch.full((n,), wgt, dtype=torch.float64, device=device), accumulate=True)
    return U


def upsample2x(x):
    N, H, W, C = x.shape
    t = torch.einsum("ph,nhwc->npwc", _up_matrix(H, x.device), x.double())
    return torch.einsum("qw,npwc->npqc", _up_matrix(W, x.device), t)


def upsample2x_bwd(dy):
    N, H2, W2, C = dy.shape
    t = torch.einsum("ph,npqc->nhqc", _up_matrix(H2 // 2, dy.device), dy.double())
    return torch.einsum("qw,nhqc->nhwc", _up_matrix(W2 // 2, dy.device), t)


# ---------------------------------------------------------------- the bars
_LOG = os.environ.get("COUNTR_STAGE_AUDIT_LOG")     # a file that receives one line per check: how much of its bar the stage used


def _log(what, kind, value):
    if _LOG:
        with open(_LOG, "a") as f:
            f.write("%-78s %-22s %.3e\n" % (what, kind, value))


def assert_16bit(out, ref, flavour, what, keep=None):
    """A 16-bit output that is ONE rounding of an fp32 computation: HP's element-wise bound with the fp32 bar as floor.  keep (bool mask):
    the elements compared (only the GroupNorm backward's undecidable ReLU gates may be left out)."""
    assert out.dtype == flavour.dtype and out.numel() == ref.numel(), (what, out.dtype, out.shape, ref.shape)
    o, r = out.reshape(-1), ref.reshape(-1)
    if keep is not None:
        o, r = o[keep.reshape(-1)], r[keep.reshape(-1)]
    if _LOG:
        od, rd = o.double(), r.double()
        top = rd.abs().max()
        _log(what, "16-bit used/allowed", ((od - rd).abs() / (2 * flavour.u * rd.abs() + flavour.tiny + F32_TOL * top)).max().item())
    ex = HP.elementwise_excess(o, r, flavour, F32_TOL)
    assert ex <= 0.0, (what, "element-wise bound exceeded by", ex)


def _maxnorm(out, ref, tol, what, kind):
    assert out.dtype == torch.float32 and out.numel() == ref.numel(), (what, out.dtype, out.shape, ref.shape)
    o, r = out.double().reshape(-1), ref.double().reshape(-1)
    assert bool(torch.isfinite(o).all()), (what, "non-finite values")
    err, top = (o - r).abs().max().item(), r.abs().max().item()
    _log(what, kind, err / max(top, 1e-300))
    assert err <= tol * top, (what, "max |out - ref| / max |ref| =", err / max(top, 1e-300), "bar", tol)


def assert_f32(out, ref, what):
    """An fp32 output: max |out - ref| <= F32_TOL max |ref|."""
    _maxnorm(out, ref, F32_TOL, what, "fp32 err/max|ref|")


def assert_stats(out, ref, what):
    """(mean, rstd) statistics: 3e-6 max |ref|."""
    _maxnorm(out, ref, STAT_TOL, what, "stats err/max|ref|")


def gate_keep(near, what):
    """The comparison mask of a GroupNorm backward; asserts ON THE REFERENCE ALONE that it leaves out at most GATE_SHARE of the map."""
    share = near.double().mean().item()
    _log(what, "gate share left out", share)
    assert share <= GATE_SHARE, (what, "share of undecidable ReLU gates", share)
    return ~near
