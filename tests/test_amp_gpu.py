"""GPU: the dynamic loss scale of the fp16 mode and the loss / index kernels around it, at kernel level through the C ABI:
countr_adamw_step_amp (amp_check_kernel, adamw_kernel's skip, gnorm_finish_kernel / amp_update), countr_masked_mse(_amp) on its scalar
path, countr_patch_mse_amp and countr_mae_indices.  The fp32-only kernels run on both libraries, the 16-bit outputs on the fp16 one.
References: torch.optim.AdamW in fp64 on g / scale, torch.amp.GradScaler's update rule (written out, and a real CPU GradScaler driven
with the same found-inf sequence), fp64 autograd of the losses, torch.argsort."""
import ctypes as C

import pytest
import torch

import halfprec as HP
from countr_amd import _lib
from oracle import countr_ref as R
from oracle import mae_ref as M

pytestmark = pytest.mark.gpu
LIBS = pytest.mark.parametrize("fl", HP.FLAVOURS, ids=HP.FLAVOUR_IDS)


def st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


# ---------------------------------------------------------------- countr_adamw_step_amp
N_FLAT = 2100003                      # > 2048 x 256 x 4 = 2,097,152: one sweep of amp_check_kernel's grid over a single range does not reach the end
BOUNDS = [(0, 5), (5, 6), (7, 60000), (60000, N_FLAT)]        # index 6 belongs to no range; the last range has an odd length
WDS = (0.05, 0.0, 0.01, 0.05)
SWEEP = 2048 * 256                    # elements one unrolled band of the first sweep covers, counted from a range's start
INTERVAL = 3


class Scaler:
    """GradScaler.update() written out: found_inf -> scale / 2, tracker 0; else tracker + 1, and at `interval` scale x 2, tracker 0."""
    def __init__(self, scale):
        self.scale, self.good, self.skipped = scale, 0, 0
        p = torch.nn.Parameter(torch.zeros(1))
        self.p, self.opt = p, torch.optim.SGD([p], lr=0.0)
        self.real = torch.amp.GradScaler("cpu", init_scale=scale, growth_interval=INTERVAL)

    def update(self, found_inf):
        if found_inf:
            self.scale, self.good, self.skipped = self.scale * 0.5, 0, self.skipped + 1
        else:
            self.good += 1
            if self.good == INTERVAL:
                self.scale, self.good = self.scale * 2.0, 0
        self.p.grad = torch.full((1,), float("inf") if found_inf else 1.0)
        self.real.scale(torch.ones(1))
        self.real.step(self.opt)
        self.real.update()
        sd = self.real.state_dict()
        assert (sd["scale"], sd["_growth_tracker"]) == (self.scale, self.good)

    def amp(self):
        return [self.scale, float(self.good), 0.0, float(self.skipped), float(INTERVAL), 0.0, 0.0, 0.0]


@pytest.mark.parametrize("with_ws", [True, False], ids=["gnorm_ws", "no_ws"])
@pytest.mark.parametrize("layout", ["four_ranges", "one_range"])
@LIBS
def test_adamw_step_amp(hip, fl, layout, with_ws):
    """Flat buffers of 2,100,003 floats.  four_ranges: [0,5) [5,6) [7,60000) [60000,n), counter groups 0, 1, 2, 0 (device hyper);
    one_range: [0,n), where amp_check_kernel's grid of 2048 x 256 x 4 needs a second outer trip (behind 2,097,152).  A clean step
    matches torch's AdamW in fp64 on g / scale (p, m, v 1e-5, the 16-bit shadow = p rounded, the gradient norm 1e-5); ONE non-finite
    gradient element -- +inf, -inf and NaN in turn -- at the first and last index of ranges, in the one-element range, in each of the
    four unrolled bands of the first sweep, behind the first sweep and at n - 1 skips the step: p, m, v and the shadow bit-identical,
    gnorm_ws[0] = inf, amp = {scale / 2, 0, 0, skipped + 1, interval}; one in the gap between ranges or inside a zero_grad range does
    not; neither does a finite 3e38; the scale doubles exactly after `interval` clean steps."""
    L = HP.library(fl, hip)
    n = N_FLAT
    bounds = BOUNDS if layout == "four_ranges" else [(0, n)]
    wds_l = WDS if layout == "four_ranges" else (0.05,)
    nr = len(bounds)
    starts, ends = (C.c_int64 * nr)(*[b[0] for b in bounds]), (C.c_int64 * nr)(*[b[1] for b in bounds])
    wds = (C.c_float * nr)(*wds_l)
    groups = (C.c_int * nr)(*([0, 1, 2, 0][:nr]))
    gen = torch.Generator().manual_seed(71)
    p0 = torch.randn(n, generator=gen)
    p = p0.cuda().clone(); m = torch.zeros(n, device="cuda"); v = torch.zeros(n, device="cuda")
    shadow = torch.zeros(n, device="cuda", dtype=fl.dtype)
    gn = torch.full((L.countr_adamw_gnorm_floats(),), -1.0, device="cuda") if with_ws else None
    sc = Scaler(65536.0)
    amp = torch.tensor(sc.amp(), device="cuda")
    params = [torch.nn.Parameter(p0[a:b].double().clone()) for a, b in bounds]
    opt = torch.optim.AdamW([{"params": [q], "weight_decay": w} for q, w in zip(params, wds_l)], lr=1e-3, betas=(0.9, 0.95), eps=1e-8)
    t = [0]

    def launch(gdev, zero=None):
        bc = (1 - 0.9 ** max(t[0], 1), 1 - 0.95 ** max(t[0], 1))
        hyper = torch.tensor([1e-3, *bc, 1.0, *bc, *bc], device="cuda")       # every range steps every time: the three counters agree
        z = (C.c_int * nr)(*(zero or [0] * nr))
        _lib.check(L.countr_adamw_step_amp(P(p), P(gdev), P(m), P(v), P(shadow), nr, starts, ends, wds, groups, z, 0.0, 0.9, 0.95, 1e-8, 0, 0.0,
                                           P(hyper), P(gn), P(amp), st()), "adamw_step_amp")
        torch.cuda.synchronize()

    def clean_step(seed, poke=None, zero=None):
        """A step that must NOT skip: gradient g * scale (exact: the scale is a power of two), poke = (index, value) written on top."""
        g = torch.randn(n, generator=torch.Generator().manual_seed(seed))
        gdev = (g * sc.scale).cuda()
        if poke:
            gdev[poke[0]] = poke[1]
        t[0] += 1
        launch(gdev, zero)
        for i, (q, (a, b)) in enumerate(zip(params, bounds)):
            q.grad = torch.zeros_like(q) if zero and zero[i] else g[a:b].double().clone()
        opt.step()
        sc.update(False)
        want = torch.cat([q.detach() for q in params]) if nr == 1 else torch.cat([params[0].detach(), params[1].detach(), p0[6:7].double(), params[2].detach(), params[3].detach()])
        assert relerr(p, want) < 1e-5
        wm = [opt.state[q]["exp_avg"] for q in params]; wv = [opt.state[q]["exp_avg_sq"] for q in params]
        for (a, b), em, ev in zip(bounds, wm, wv):
            assert relerr(m[a:b], em) < 1e-5 and relerr(v[a:b], ev) < 1e-5
        live = torch.ones(n, dtype=torch.bool)
        if nr > 1:
            live[6] = False
            assert p[6].item() == p0[6].item() and m[6].item() == 0.0 and v[6].item() == 0.0 and shadow[6].item() == 0.0    # the gap is never touched
        assert torch.equal(shadow[live.cuda()], p.to(fl.dtype)[live.cuda()])
        if with_ws:
            for i, (a, b) in enumerate(bounds):
                if zero and zero[i]:
                    live[a:b] = False
            norm = g[live].double().pow(2).sum().sqrt().item()
            assert abs(gn[0].item() - norm) < 1e-5 * norm
        assert amp.tolist() == sc.amp()

    def skipped_step(seed, index, value):
        g = torch.randn(n, generator=torch.Generator().manual_seed(seed))
        gdev = (g * sc.scale).cuda()
        gdev[index] = value
        before = [x.clone() for x in (p, m, v, shadow)]
        if with_ws:
            gn.fill_(-1.0)
        launch(gdev)
        sc.update(True)
        for name, a, b in zip("p m v shadow".split(), before, (p, m, v, shadow)):
            assert torch.equal(a, b), (name, index, value)
        if with_ws:
            assert gn[0].item() == float("inf"), (index, value)
        assert amp.tolist() == sc.amp(), (index, value)

    clean_step(100)
    inf = float("inf")
    vals = [inf, -inf, float("nan")]
    if nr > 1:
        first = 60000          # the long range: bands are counted from its start
        where = [0, 4, 5, 59999, 60000, first + 100, first + SWEEP + 101, first + 2 * SWEEP + 102, first + 3 * SWEEP + 103, 2097152 + 5, n - 1]
    else:
        where = [0, 100, SWEEP + 101, 2 * SWEEP + 102, 3 * SWEEP + 103, 4 * SWEEP - 1, 4 * SWEEP, 2097152 + 5, n - 2, n - 1]      # 4 x SWEEP = 2,097,152: second trip
    for k, index in enumerate(where):
        skipped_step(200 + k, index, vals[k % 3])
    for k, value in enumerate(vals):                   # ... and every kind at the very end of the odd-length range
        skipped_step(300 + k, n - 1, value)
    assert sc.skipped == len(where) + 3 and sc.scale == 65536.0 * 0.5 ** sc.skipped
    if nr > 1:
        clean_step(101, poke=(6, inf))                 # in the gap: read by nobody
        clean_step(102, poke=(30000, float("nan")), zero=[0, 0, 1, 0])      # inside a zero_grad range: stepped with g = 0, not read
        assert amp[1].item() == 2.0
        scale_before = sc.scale
        clean_step(103)                                # the third clean step since the last skip: growth, exactly here
        assert amp[0].item() == 2 * scale_before and amp[1].item() == 0.0
    else:
        clean_step(101); clean_step(102)
        assert amp[0].item() == 65536.0 * 0.5 ** sc.skipped and amp[1].item() == 2.0
        clean_step(103)                                # the third clean step since the last skip
        assert amp[0].item() == 65536.0 * 0.5 ** sc.skipped * 2 and amp[1].item() == 0.0
    # a finite 3e38 is no overflow: the step is taken (tracker + 1, nothing skipped).  Its square overflows v and the norm, as in torch.
    g = torch.randn(n, generator=torch.Generator().manual_seed(104))
    gdev = (g * sc.scale).cuda()
    gdev[12345] = 3e38
    before_p, skipped = p.clone(), amp[3].item()
    t[0] += 1
    launch(gdev)
    sc.update(False)
    assert amp.tolist() == sc.amp() and amp[3].item() == skipped
    assert (p != before_p).float().mean().item() > 0.99


# ---------------------------------------------------------------- countr_masked_mse / countr_masked_mse_amp
@pytest.mark.parametrize("with_dpred", [True, False], ids=["dpred", "no_dpred"])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("HW,offset", [(1027, 0), (1024, 1)], ids=["hw1027", "hw1024_unaligned_pred"])
@LIBS
def test_masked_mse_scalar_path_and_loss_scale(hip, fl, HW, offset, B, with_dpred):
    """masked_mse_kernel's scalar path (HW % 4 != 0, or a pointer that is not 16-byte aligned: pred one float into its buffer) against
    fp64 at the bars of test_masked_mse_and_adamw (1e-5), and the loss scale: with amp[0] = 2^k, dpred is bit-equal to 2^k times the
    unscaled one (a power of two only moves the exponent) and the sums do not change."""
    L = HP.library(fl, hip)
    g = torch.Generator().manual_seed(30 + HW + B)
    pred = torch.rand((B, HW), generator=g); gt = torch.rand((B, HW), generator=g)
    mask = (torch.rand(HW, generator=g) < 0.8).float()
    buf = torch.zeros(B * HW + 4, device="cuda")
    buf[offset:offset + B * HW] = pred.reshape(-1).cuda()
    pd = buf[offset:offset + B * HW]
    assert pd.data_ptr() % 16 == 4 * offset
    gd, md = gt.cuda(), mask.cuda()
    ws = torch.empty(L.countr_masked_mse_workspace_floats(B), device="cuda")
    pr = pred.double().requires_grad_(True)
    loss = ((pr - gt.double()) ** 2 * mask.double()).sum() / HW / B                  # FSC_finetune_cross.py:290-303
    loss.backward()
    outs = {}
    for k in (None, 0, 16):
        dp = torch.full((B, HW), float("nan"), device="cuda") if with_dpred else None
        sums = torch.full((1 + 2 * B,), float("nan"), device="cuda")
        if k is None:
            _lib.check(L.countr_masked_mse(P(pd), P(gd), P(md), P(dp), P(sums), P(ws), B, HW, 1.0, st()))
        else:
            amp = torch.tensor([2.0 ** k, 0, 0, 0, 2000, 0, 0, 0], device="cuda")
            _lib.check(L.countr_masked_mse_amp(P(pd), P(gd), P(md), P(dp), P(sums), P(ws), B, HW, 1.0, P(amp), st()))
        torch.cuda.synchronize()
        assert abs(sums[0].item() - loss.item()) < 1e-5 * loss.item()
        assert relerr(sums[1:1 + B], R.counts(pred.double())) < 1e-5 and relerr(sums[1 + B:], R.counts(gt.double())) < 1e-5
        outs[k] = (dp, sums)
    if with_dpred:
        assert relerr(outs[None][0], pr.grad) < 1e-5
        assert torch.equal(outs[0][0], outs[None][0]) and torch.equal(outs[16][0], outs[None][0] * 65536.0)
    assert torch.equal(outs[0][1], outs[None][1]) and torch.equal(outs[16][1], outs[None][1])
    assert torch.equal(buf[:offset], torch.zeros(offset, device="cuda")) and buf[offset + B * HW:].abs().max().item() == 0.0


# ---------------------------------------------------------------- countr_patch_mse_amp
@pytest.mark.parametrize("norm_pix", [False, True], ids=["plain", "norm_pix"])
@pytest.mark.parametrize("H,W,patch", [(32, 48, 16), (28, 28, 14)])
def test_patch_mse_loss_scale_fp16(H, W, patch, norm_pix):
    _patch_mse_loss_scale_fp16(H, W, patch, norm_pix, False)


@pytest.mark.parametrize("norm_pix", [False, True], ids=["plain", "norm_pix"])
@pytest.mark.parametrize("H,W,patch", [(32, 48, 16), (28, 28, 14)])
def test_patch_mse_fp16_dpred_is_the_rounding_of_the_fp32_dpred(H, W, patch, norm_pix):
    """The fp16 dpred of a call is bit-equal to .to(float16) of the fp32 dpred of the same call, with and without the 2^16 scale: the
    gradient is ONE fp32 value, d * gs, and the 16-bit form its rounding.  (Product and conversion folded into one v_fma_mixlo_f16 --
    the exact product rounded once, what the compiler makes of stf(d * gs) in the fp16 build if left alone -- differs by one fp16 ulp
    wherever the fp32 value is an exact tie between two fp16 numbers: 1 to 5 of 4704 - 9216 elements here, e.g. fp32 0x1.3c2p-13 ->
    0x1.3c4p-13 instead of 0x1.3c0p-13, subnormals included: 0x1.fp-21 -> 0x1.ep-21 instead of 0x1p-20.  patch_mse_kernel keeps the
    product in a register of its own for that reason.)"""
    _patch_mse_loss_scale_fp16(H, W, patch, norm_pix, True)


def _patch_mse_loss_scale_fp16(H, W, patch, norm_pix, rounding_of_fp32):
    """fp16 library, B = 2.  fp32 dpred with scale 2^16 is bit-equal to 2^16 times the unscaled one; (the fp16 dpred against the rounded fp32 one: the test
    below); WITHOUT the scale a share of the fp16 elements is subnormal or zero -- the gradient is
    2 (pred - target) / (F rows) with F rows = 9216 (patch 16: 768 x 12) or 4704 (patch 14: 588 x 8), below 2^-14 wherever
    |pred - target| < 0.28 / 0.14 -- measured on the fp64 reference rounded by torch (not on the kernel) and required to the element:
    patch 16 plain 1688 of 9216, norm_pix 1334; patch 14 plain 441 of 4704, norm_pix 380 (the closest element is 1.5e-4 relative from
    the 2^-14 boundary, the fp32 error 1e-7); with 2^16 none is, and the fp16 dpred meets the element-wise bound against fp64."""
    L, fl, B = HP.library(HP.FP16), HP.FP16, 2
    g = torch.Generator().manual_seed(2)
    imgs = torch.rand(B, 3, H, W, generator=g)
    Ln, F = (H // patch) * (W // patch), 3 * patch * patch
    pred = torch.randn(B * Ln, F, generator=g)
    x = imgs.double().reshape(B, 3, H // patch, patch, W // patch, patch)
    target = torch.einsum("nchpwq->nhwpqc", x).reshape(B, Ln, F)                        # patchify: (py, px, c) feature order
    if norm_pix:
        target = (target - target.mean(-1, keepdim=True)) / (target.var(-1, keepdim=True) + 1e-6) ** 0.5
    pr = pred.double().requires_grad_(True)
    loss = ((pr.view(B, Ln, F) - target) ** 2).mean(-1).sum() / (B * Ln)
    loss.backward()
    ws = torch.empty(L.countr_patch_mse_workspace_floats(B, H, W, patch), device="cuda")
    pd, im = pred.cuda(), imgs.cuda()
    got = {}
    for k in (None, 16):
        for dt in (0, 1):
            dp = torch.full((B * Ln, F), float("nan"), device="cuda", dtype=fl.dtype if dt else torch.float32)
            out = torch.full((1,), float("nan"), device="cuda")
            if k is None:
                _lib.check(L.countr_patch_mse(P(pd), P(im), P(dp), P(out), P(ws), B, H, W, patch, int(norm_pix), 1.0, dt, st()))
            else:
                amp = torch.tensor([2.0 ** k, 0, 0, 0, 2000, 0, 0, 0], device="cuda")
                _lib.check(L.countr_patch_mse_amp(P(pd), P(im), P(dp), P(out), P(ws), B, H, W, patch, int(norm_pix), 1.0, dt, P(amp), st()))
            torch.cuda.synchronize()
            assert abs(out.item() - loss.item()) <= 2e-6 * loss.item()
            got[k, dt] = dp
    if rounding_of_fp32:
        for k in (None, 16):
            bad = (got[k, 1] != got[k, 0].to(fl.dtype)).nonzero()
            print("fp16 dpred != round(fp32 dpred): %d of %d elements (scale 2^%s)" % (bad.shape[0], got[k, 1].numel(), k or 0))
            for i, j in bad[:6].tolist():
                print("   fp32 %s  kernel fp16 %s  torch %s" % (float(got[k, 0][i, j]).hex(), float(got[k, 1][i, j]).hex(),
                                                              float(got[k, 0][i, j].to(fl.dtype)).hex()))
        for k in (None, 16):
            assert torch.equal(got[k, 1], got[k, 0].to(fl.dtype))
        return
    assert relerr(got[None, 0], pr.grad) <= 2e-6                                        # (the bar of tests/test_mae_gpu.py)
    assert torch.equal(got[16, 0], got[None, 0] * 65536.0)
    small = lambda t: int((t.abs() < 2.0 ** -14).sum().item())                       # subnormal or zero in fp16
    want = small(pr.grad.to(fl.dtype))
    assert want == {(16, False): 1688, (16, True): 1334, (14, False): 441, (14, True): 380}[patch, norm_pix]
    print("fp16 dpred without the loss scale: %d of %d elements subnormal or zero (fp64 reference, rounded)" % (want, pr.grad.numel()))
    assert small(got[None, 1]) == want and want > 0
    assert small(got[16, 1]) == small((pr.grad * 65536.0).to(fl.dtype)) < want
    HP.assert_elementwise(got[16, 1], pr.grad * 65536.0, fl, 2e-6, "patch_mse dpred x 2^16")


# ---------------------------------------------------------------- countr_mae_indices
@pytest.mark.parametrize("K", [49, 147, 196])
@LIBS
def test_mae_indices(hip, fl, K):
    """random_masking's index buffers (models_mae_noct.py:119-132) from the argsort of the noise: ids_restore = argsort(ids_shuffle),
    mask = gather(ones with the first K zeroed, ids_restore), kept = ids_shuffle[:, :K]; every buffer starts as a sentinel with guard
    elements behind it, and every element is written exactly where specified.  mask_src = NULL at K = N."""
    L = HP.library(fl, hip)
    B, N = 3, 196
    noise = torch.rand(B, N, generator=torch.Generator().manual_seed(9))
    ids_shuffle = torch.argsort(noise, dim=1)
    ids_restore = torch.argsort(ids_shuffle, dim=1)
    keep = ids_shuffle[:, :K]
    mask = torch.ones(B, N); mask[:, :K] = 0
    mask = torch.gather(mask, 1, ids_restore)
    S, G = -77, 8
    d_restore = torch.full((B * N + G,), S, dtype=torch.int64, device="cuda")
    d_kpos = torch.full((B * K + G,), S, dtype=torch.int32, device="cuda"); d_ksrc = torch.full_like(d_kpos, S)
    d_rsrc = torch.full((B * N + G,), S, dtype=torch.int32, device="cuda")
    d_msrc = torch.full((B * (N - K) + G,), S, dtype=torch.int32, device="cuda")
    d_mask = torch.full((B * N + G,), float(S), device="cuda")
    _lib.check(L.countr_mae_indices(P(ids_shuffle.cuda()), P(d_restore), P(d_kpos), P(d_ksrc), P(d_rsrc), P(d_msrc) if K < N else None, P(d_mask),
                                    B, N, K, st()), "mae_indices")
    torch.cuda.synchronize()
    off = (torch.arange(B) * N).unsqueeze(1)
    assert torch.equal(d_restore[:B * N].cpu(), ids_restore.reshape(-1))
    assert torch.equal(d_kpos[:B * K].cpu().long(), keep.reshape(-1))
    assert torch.equal(d_ksrc[:B * K].cpu().long(), (keep + off).reshape(-1))
    assert torch.equal(d_mask[:B * N].cpu(), mask.reshape(-1))
    want_r = torch.where(ids_restore < K, ids_restore + (torch.arange(B) * K).unsqueeze(1), torch.full_like(ids_restore, -1))
    assert torch.equal(d_rsrc[:B * N].cpu().long(), want_r.reshape(-1))
    assert torch.equal(d_msrc[:B * (N - K)].cpu().long(), (ids_shuffle[:, K:] + off).reshape(-1))
    for buf, used in ((d_restore, B * N), (d_kpos, B * K), (d_ksrc, B * K), (d_rsrc, B * N), (d_msrc, B * (N - K)), (d_mask, B * N)):
        assert (buf[used:] == S).all()
    if K < N:
        assert L.countr_mae_indices(P(ids_shuffle.cuda()), P(d_restore), P(d_kpos), P(d_ksrc), P(d_rsrc), None, P(d_mask), B, N, K, st()) != 0
