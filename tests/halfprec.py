"""The two 16-bit builds of the library as test parameters, and an element-wise error bound for 16-bit kernel outputs.

A flavour is (library variant, torch dtype, half-ulp u, smallest subnormal): libcountr_hip.so stores bfloat16 (u = 2^-9, its
subnormals lie below anything a test produces: tiny = 0), libcountr_hip_f16.so (-DCOUNTR_HALF_FP16=1) IEEE fp16 (u = 2^-11, subnormal
spacing 2^-24).  The dtype CODE of the C ABI is the same for both (COUNTR_BF16 = "the 16-bit type of this build").

elementwise_excess is for outputs that are ONE rounding of an fp32 computation on 16-bit-exact inputs:

    |out - ref| <= 2 u |ref| + tiny + floor * max|ref|        for every element

2 u |ref| is one ulp of the element -- twice the round-to-nearest bound, so an fp32 value that lands on the other side of a rounding
boundary of the exact one still passes; tiny is the same ulp where the format is subnormal; floor is the bar the test already states for
the same kernel in fp32 mode (the error of the fp32 computation itself, relative to the largest value).  Nothing is measured.  The
max-norm relerr of the kernel tests cannot see an error confined to small elements (a wrong lane of a packed pair, a flushed
subnormal); this bound can.  Outputs that carry MORE than one 16-bit rounding (fused attention: P, dS and the stored O are rounded before
they are summed) have their own row-wise bound in tests/attnref.py."""
import collections

import torch

Flavour = collections.namedtuple("Flavour", "variant dtype u tiny")
BF16 = Flavour("", torch.bfloat16, 2.0 ** -9, 0.0)
FP16 = Flavour("f16", torch.float16, 2.0 ** -11, 2.0 ** -24)
FLAVOURS = [BF16, FP16]
FLAVOUR_IDS = ["bf16", "fp16"]
BY_DTYPE = {BF16.dtype: BF16, FP16.dtype: FP16}

_ready = set()


def library(flavour_or_dtype, default=None):
    """The initialised library of a flavour (or of a torch dtype; torch.float32 and anything else that is no 16-bit flavour gets
    `default`, the session's bf16 library)."""
    fl = flavour_or_dtype if isinstance(flavour_or_dtype, Flavour) else BY_DTYPE.get(flavour_or_dtype)
    if fl is None or (fl.variant == "" and default is not None):
        return default
    from countr_amd import _lib
    L = _lib.lib(fl.variant)
    if fl.variant not in _ready:
        _lib.check(L.countr_init(0), "countr_init")
        _ready.add(fl.variant)
    return L


def bar(flavour_or_dtype, bf16_bar):
    """A max-norm bar stated for a bf16 output, for this flavour: fp16 has three more mantissa bits (2^-11 against 2^-8)."""
    fl = flavour_or_dtype if isinstance(flavour_or_dtype, Flavour) else BY_DTYPE[flavour_or_dtype]
    return bf16_bar / 8 if fl is FP16 else bf16_bar


def elementwise_excess(out, ref, flavour, floor):
    """max over ALL elements of |out - ref| - (2 u |ref| + tiny + floor max|ref|), in fp64: <= 0 means the bound holds everywhere.
    A non-finite element of `out` where `ref` is finite (or the reverse) gives +inf; equal infinities and NaN against NaN pass.
    Computed where `out` lives (the same fp64 operations: a 19 M-element head map stays on the GPU)."""
    o = out.detach().double().reshape(-1)
    r = ref.detach().double().reshape(-1).to(o.device)
    assert o.shape == r.shape, (out.shape, ref.shape)
    fin = torch.isfinite(r)
    same = (o == r) | (torch.isnan(o) & torch.isnan(r))
    if not bool((same | fin).all()) or not bool((same | torch.isfinite(o)).all()):
        return float("inf")
    top = r[fin].abs().max().item() if bool(fin.any()) else 0.0
    d = torch.where(same, torch.zeros_like(o), (o - r).abs() - (2 * flavour.u * r.abs() + flavour.tiny + floor * top))
    return d.max().item()


def assert_elementwise(out, ref, flavour, floor, what=""):
    ex = elementwise_excess(out, ref, flavour, floor)
    assert ex <= 0.0, (what, "element-wise bound exceeded by", ex)
