"""The fp64 stage references of tests/stagecheck.py against torch autograd in fp64 on small random maps, and the other way round: every
reference, held to the bar the stage audit uses, REJECTS a result that lost one border row of a gradient (the kind of error the
whole-model cosine bars of tests/test_model_gpu.py let through)."""
import pytest
import torch
import torch.nn.functional as F

import halfprec as HP
import stagecheck as SC

N, H, W, CI, CO = 2, 6, 10, 5, 7       # H != W, odd channel counts


def rnd(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def nchw(x):
    return x.permute(0, 3, 1, 2)


def nhwc(x):
    return x.permute(0, 2, 3, 1)


def close(a, b):
    return (a - b).abs().max().item() <= 1e-12 * max(b.abs().max().item(), 1.0)


def rejected(check, *args):
    with pytest.raises(AssertionError):
        check(*args)
    return True


def drop_row(t, dim=1, row=0):
    """t with one border row (index `row` of the map's height axis) zeroed."""
    t = t.clone()
    t.select(dim, row).zero_()
    return t


def as_f32_result(check_ref, good, bad, what):
    """`good` passes the fp32 bar against the reference, `bad` does not."""
    SC.assert_f32(good.float(), check_ref, what)
    assert rejected(SC.assert_f32, bad.float(), check_ref, what)


def test_convolution_forward_dgrad_wgrad_bias():
    x, w, b, dy = rnd((N, H, W, CI), 1).requires_grad_(True), rnd((CO, 3, 3, CI), 2), rnd((CO,), 3), rnd((N, H, W, CO), 4)
    w_oihw = w.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    br = b.clone().requires_grad_(True)
    y = nhwc(F.conv2d(nchw(x), w_oihw, br, padding=1))
    y.backward(dy)
    assert close(SC.conv3x3(x.detach(), w, b), y.detach())
    assert close(SC.conv3x3_dgrad(dy, w), x.grad)
    assert close(SC.conv3x3_wgrad(dy, x.detach()), w_oihw.grad)
    assert close(SC.bias_grad(dy), br.grad)
    assert torch.equal(SC.ohwi(w_oihw.detach()), w)
    # the engine's dgrad shadow: Wd[ci][2 - ky][2 - kx][co]; a forward convolution with it is the input gradient
    wd = w.permute(3, 1, 2, 0).flip(1, 2).contiguous()
    assert torch.equal(SC.ohwi_of_dgrad_form(wd.reshape(-1), CO, CI), w)
    assert close(SC.conv3x3(dy, wd), x.grad)
    # one border row lost: of the output map, of the input gradient, and of dy on its way into the weight / bias gradient
    as_f32_result(SC.conv3x3(x.detach(), w, b), y.detach(), drop_row(y.detach(), row=H - 1), "conv fwd")
    as_f32_result(SC.conv3x3_dgrad(dy, w), x.grad, drop_row(x.grad), "conv dgrad")
    for row in (0, H - 1):
        cut = drop_row(dy, row=row)
        as_f32_result(SC.conv3x3_wgrad(dy, x.detach()), w_oihw.grad, SC.conv3x3_wgrad(cut, x.detach()), "conv wgrad")
        as_f32_result(SC.bias_grad(dy), br.grad, SC.bias_grad(cut), "conv bias grad")


def test_pools_route_to_the_first_maximum_like_torch():
    # values on a coarse grid: most windows hold ties
    x = (rnd((N, H, W, CI), 5) * 2).round().div(2).requires_grad_(True)
    dy = rnd((N, H // 2, W // 2, CI), 6)
    y = nhwc(F.max_pool2d(nchw(x), 2))
    y.backward(dy)
    assert torch.equal(SC.maxpool2(x.detach()), y.detach())
    assert torch.equal(SC.maxpool2(x.detach().to(torch.bfloat16)), y.detach().to(torch.bfloat16))
    assert close(SC.maxpool2_bwd(x.detach(), dy), x.grad)
    x2 = rnd((N, H, W, CI), 7).requires_grad_(True)
    d2 = rnd((N, CI), 8)
    a = x2.mean((1, 2))
    a.backward(d2)
    assert close(SC.avgpool(x2.detach()), a.detach()) and close(SC.avgpool_bwd(d2, H, W), x2.grad)
    as_f32_result(SC.maxpool2_bwd(x.detach(), dy), x.grad, drop_row(x.grad), "max-pool bwd")
    as_f32_result(SC.avgpool_bwd(d2, H, W), x2.grad, drop_row(x2.grad, row=H - 1), "avg-pool bwd")


@pytest.mark.parametrize("avg", [0, 1])
def test_instancenorm_backward_from_a_stored_xhat(avg):
    x = (rnd((N, H, W, CI), 9) * 1.3 + 0.4).requires_grad_(True)
    dyp = rnd((N, CI) if avg else (N, H // 2, W // 2, CI), 10)
    mu = x.mean((1, 2), keepdim=True)
    rstd = (((x - mu) ** 2).mean((1, 2), keepdim=True) + 1e-5).rsqrt()
    xhat = (x - mu) * rstd
    a = torch.relu(xhat)
    y = a.mean((1, 2)) if avg else nhwc(F.max_pool2d(nchw(a), 2))
    y.backward(dyp)
    stats = SC.instnorm_stats(x.detach())
    assert close(stats[..., 0], mu.detach().reshape(N, CI)) and close(stats[..., 1], rstd.detach().reshape(N, CI))
    assert close(SC.instnorm_xhat(x.detach(), stats), xhat.detach())
    ref = SC.instnorm_relu_pool_bwd(xhat.detach(), stats[..., 1], dyp, avg)
    assert close(ref, x.grad)
    as_f32_result(ref, x.grad, drop_row(x.grad), "instnorm bwd")
    # the element-wise 16-bit bar sees the same loss
    for fl in HP.FLAVOURS:
        SC.assert_16bit(ref.to(fl.dtype), ref, fl, "instnorm bwd")
        assert rejected(SC.assert_16bit, drop_row(ref, row=H - 1).to(fl.dtype), ref, fl, "instnorm bwd")
    if not avg:      # a border row of the pooled gradient that never arrives
        cut = SC.instnorm_relu_pool_bwd(xhat.detach(), stats[..., 1], drop_row(dyp), avg)
        assert rejected(SC.assert_f32, cut.float(), ref, "instnorm bwd")


@pytest.mark.parametrize("fused_head", [False, True])
def test_groupnorm_relu_forward_backward_and_image_sums(fused_head):
    B, C, G = 2, 16, 4
    x = (rnd((B, H, W, C), 11) * 1.5 + 0.2).requires_grad_(True)
    ga, be = (1 + 0.1 * rnd((C,), 12)).requires_grad_(True), (0.1 * rnd((C,), 13)).requires_grad_(True)
    w1, b1 = (0.3 * rnd((C,), 14)).requires_grad_(True), rnd((1,), 15)
    y = nhwc(torch.relu(F.group_norm(nchw(x), G, ga, be, eps=1e-5)))
    stats = SC.groupnorm_stats(x.detach(), G)
    assert close(SC.groupnorm_relu(x.detach(), stats, ga.detach(), be.detach()), y.detach())
    if fused_head:
        d1 = rnd((B, H, W), 16)
        o = (y * w1).sum(-1) + b1
        assert close(SC.head1x1(y.detach(), w1.detach(), b1), o.detach())
        o.backward(d1)
        dx, sums, near = SC.groupnorm_relu_bwd(x.detach(), stats, ga.detach(), be.detach(), d1=d1, w1=w1.detach())
        assert close(sums[:, 2].sum(0), w1.grad)
    else:
        dy = rnd((B, H, W, C), 17)
        y.backward(dy)
        dx, sums, near = SC.groupnorm_relu_bwd(x.detach(), stats, ga.detach(), be.detach(), dy=dy)
        assert not bool(sums[:, 2].any())
    assert close(dx, x.grad) and close(sums[:, 0].sum(0), be.grad) and close(sums[:, 1].sum(0), ga.grad)
    assert not bool(near.any()) and bool(SC.gate_keep(near, "gn").all())
    as_f32_result(dx, x.grad, drop_row(x.grad), "groupnorm bwd")
    if not fused_head:     # dy with a border row zeroed: the per-image sums (dbeta, dgamma) and dx notice
        _dx, cut, _ = SC.groupnorm_relu_bwd(x.detach(), stats, ga.detach(), be.detach(), dy=drop_row(dy, row=H - 1))
        assert rejected(SC.assert_f32, cut[:, :2].float(), sums[:, :2], "groupnorm image sums")
        assert rejected(SC.assert_f32, _dx.float(), dx, "groupnorm bwd")


def test_groupnorm_gate_margin_marks_pre_activations_at_zero():
    B, C, G = 1, 8, 2
    x = rnd((B, 4, 4, C), 18)
    stats = SC.groupnorm_stats(x, G)
    ga = torch.ones(C, dtype=torch.float64)
    xh = (x - stats[..., 0].repeat_interleave(C // G, 1).view(B, 1, 1, C)) * stats[..., 1].repeat_interleave(C // G, 1).view(B, 1, 1, C)
    be = torch.zeros(C, dtype=torch.float64)
    be[3] = -xh[0, 2, 1, 3]                      # y = 0 (to rounding) at exactly one element
    _, _, near = SC.groupnorm_relu_bwd(x, stats, ga, be, dy=torch.ones_like(x))
    assert int(near.sum()) == 1 and bool(near[0, 2, 1, 3])
    with pytest.raises(AssertionError):
        SC.gate_keep(near, "gn")               # 1 of 128 elements is more than 1e-4 of the map


def test_bilinear_x2_and_its_adjoint():
    x = rnd((N, H, W, CI), 19).requires_grad_(True)
    dy = rnd((N, 2 * H, 2 * W, CI), 20)
    y = nhwc(F.interpolate(nchw(x), scale_factor=2, mode="bilinear", align_corners=False))
    y.backward(dy)
    assert close(SC.upsample2x(x.detach()), y.detach())
    assert close(SC.upsample2x_bwd(dy), x.grad)
    as_f32_result(SC.upsample2x(x.detach()), y.detach(), drop_row(y.detach(), row=2 * H - 1), "bilinear x2")
    as_f32_result(SC.upsample2x_bwd(dy), x.grad, drop_row(x.grad), "bilinear x2 bwd")
    as_f32_result(SC.upsample2x_bwd(dy), x.grad, SC.upsample2x_bwd(drop_row(dy)), "bilinear x2 bwd")


def test_bars():
    ref = rnd((3, 5, 4, 2), 21)
    SC.assert_f32((ref * (1 + 1e-5)).float(), ref, "f32")
    assert rejected(SC.assert_f32, (ref * (1 + 1e-3)).float(), ref, "f32")
    assert rejected(SC.assert_f32, ref, ref, "an fp64 'output' is a wiring error")
    SC.assert_stats((ref * (1 + 1e-6)).float(), ref, "stats")
    assert rejected(SC.assert_stats, (ref * (1 + 2e-5)).float(), ref, "stats")
    bad = ref.float().clone()
    bad[0, 0, 0, 0] = float("nan")
    assert rejected(SC.assert_f32, bad, ref, "nan")
    for fl in HP.FLAVOURS:
        assert rejected(SC.assert_16bit, ref.float(), ref, fl, "wrong dtype")
        keep = torch.ones(ref.shape, dtype=torch.bool)
        out = ref.to(fl.dtype)
        out[1, 1, 1, 1] += 1.0
        keep[1, 1, 1, 1] = False
        assert rejected(SC.assert_16bit, out, ref, fl, "one wrong element")
        SC.assert_16bit(out, ref, fl, "... left out", keep)
