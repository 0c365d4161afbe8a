"""CPU: the element-wise bound of tests/halfprec.py accepts a correctly rounded result at the edges of both 16-bit formats and
rejects a small-element error that the max-norm measure of the kernel tests accepts."""
import pytest
import torch

import halfprec as HP


def relerr(a, b):                       # the measure of tests/test_kernels_gpu.py
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def edge_values():
    g = torch.Generator().manual_seed(7)
    body = torch.randn(4096, generator=g, dtype=torch.float64) * torch.logspace(-9, 4, 4096, dtype=torch.float64)
    edges = torch.tensor([0.0, -0.0, 65504.0, -65504.0, 2.0 ** -24, -2.0 ** -24, 3 * 2.0 ** -24, 1023 * 2.0 ** -24, 2.0 ** -14,
                          2.0 ** -25 * (1 + 2.0 ** -10), 2.0 ** -25, 1e-9, -1e-9, 0.0], dtype=torch.float64)
    return torch.cat([edges, body.clamp(-65504.0, 65504.0)])


@pytest.mark.parametrize("fl", HP.FLAVOURS, ids=HP.FLAVOUR_IDS)
@pytest.mark.parametrize("floor", [0.0, 1e-6, 2e-4])
def test_rounded_reference_meets_the_bound(fl, floor):
    ref = edge_values()
    assert ref.abs().max().item() == 65504.0 and (ref == 0).sum() >= 3 and ((ref != 0) & (ref.abs() < 2.0 ** -14)).sum() > 100
    out = ref.to(fl.dtype)                                    # the reference alone, rounded by torch: at most u |ref| (+ tiny / 2) away
    assert torch.isfinite(out.float()).all()
    assert HP.elementwise_excess(out, ref, fl, floor) <= 0.0
    HP.assert_elementwise(out, ref, fl, floor)
    # ... from an fp32 value one fp32 ulp off the exact one as well (the margin the second u is for)
    near = torch.nextafter(ref.float(), torch.full_like(ref.float(), float("inf"))).clamp(max=65504.0)
    assert HP.elementwise_excess(near.to(fl.dtype), ref, fl, floor) <= 0.0


@pytest.mark.parametrize("fl,old_bar", [(HP.BF16, 2e-2), (HP.FP16, 2.5e-3)], ids=HP.FLAVOUR_IDS)
def test_small_element_error_fails_the_bound_but_not_the_max_norm(fl, old_bar):
    """One element of magnitude 1e-3 max|ref| off by 8 u relative (four ulps: a wrong neighbour's bits, not a rounding).  The max-norm
    measure sees 8e-3 u and accepts it at both bars.  The element-wise bound sees it wherever floor max|ref| is below the error, i.e.
    with the floor of an exact kernel (cast, gather: 1e-6) at this magnitude, and with the 2e-4 floor of the arithmetic kernels on an
    element of 0.1 max|ref|."""
    g = torch.Generator().manual_seed(8)
    ref = torch.randn(8192, generator=g, dtype=torch.float64)
    ref[0] = 8.0                                              # the maximum
    for magnitude, floor in ((1e-3, 1e-6), (1e-3, 0.0), (0.1, 2e-4)):
        ref[100] = magnitude * 8.0 * 1.2345
        good = ref.to(fl.dtype)
        bad = good.clone()
        bad[100] = (good[100].double() * (1 + 8 * fl.u)).to(fl.dtype)
        assert HP.elementwise_excess(good, ref, fl, floor) <= 0.0
        assert HP.elementwise_excess(bad, ref, fl, floor) > 0.0, (magnitude, floor)
        with pytest.raises(AssertionError):
            HP.assert_elementwise(bad, ref, fl, floor)
        assert relerr(bad, ref) < old_bar and relerr(bad, ref) < 1.01 * relerr(good, ref) + 8 * fl.u * magnitude * 1.3


def test_non_finite_elements():
    ref = torch.tensor([1.0, float("inf"), float("nan"), -float("inf")], dtype=torch.float64)
    assert HP.elementwise_excess(ref.to(torch.float16), ref, HP.FP16, 0.0) <= 0.0
    bad = ref.to(torch.float16); bad[0] = float("inf")
    assert HP.elementwise_excess(bad, ref, HP.FP16, 1.0) == float("inf")
    bad = ref.to(torch.float16); bad[1] = 65504.0
    assert HP.elementwise_excess(bad, ref, HP.FP16, 1.0) == float("inf")


def test_flavours():
    assert HP.bar(HP.FP16, 2e-2) == 2.5e-3 and HP.bar(torch.bfloat16, 2e-2) == 2e-2
    assert HP.library(torch.float32, default="session") == "session" and HP.library(HP.BF16, default="session") == "session"
    assert [f.u for f in HP.FLAVOURS] == [2.0 ** -9, 2.0 ** -11] and HP.FP16.tiny == torch.finfo(torch.float16).smallest_normal * 2.0 ** -10
