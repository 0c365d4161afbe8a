"""Operands and outputs of the GEMM family with poisoned surroundings: the embedding, the band sizes, the fp64 references, the
assertions and fp32 torch emulations that read the embedded STORAGE the way a kernel does.  Pure torch; nothing here touches a kernel.

Every load mask of gemm_kernel.hpp, linear.hip, gemm256.hip and conv_wgrad.hip (ragged M, the K tail, split-K ranges, padding taps,
leading dimensions larger than the row) is the only thing between the kernel and whatever lies next to the operand: the buffer
descriptors are open.  Here "whatever lies next to it" is NaN -- the pad columns cols .. ld - 1 of every row, a band in front of the
operand and a band behind it, the slices of a packed buffer the launch does not use, the slab behind the last split-K slab -- so a read
that escapes the matrix and reaches an output makes that output NaN, and a store that escapes the output changes a band's bits.

tests/test_gemm_poison_cpu.py hands the assertions below the emulations (which must pass) and deliberately wrong variants of them
(which must not); tests/test_gemm_poison_gpu.py hands them the kernels' outputs.  The pattern of tests/kedges.py, whose GUARD (the
default band) and bits() are reused.  No bar is set here: every case takes the bar of the test of the same kernel in tests/test_gemm_gpu.py."""
import torch

from kedges import GUARD, bits

NAN = float("nan")
# what OUTPUT allocations hold before a launch: a quiet NaN with a payload.  Arithmetic on the inputs' plain NaN gives the plain NaN, so
# a kernel that reads poison and stores it into a band -- NaN onto NaN -- still changes the band's bits.
OUT_NAN_BITS = {torch.float32: 0x7fc00abc, torch.bfloat16: 0x7fc5, torch.float16: 0x7e05}
TILE_ROWS = 256             # the tallest workgroup tile of the family (gemm256.hip; linear.hip's 256 x 128 form)


# ---------------------------------------------------------------------------------------------------------------- band sizes
def band(n):
    """A band length: at least n, a multiple of 8 elements (16 bytes of a 16-bit type: the operand pointer keeps the alignment the lean
    kernels ask for; misaligned they would decline and the generic kernel would run unnoticed)."""
    return -(-max(int(n), 8) // 8) * 8


def ragged_band(ld):
    """Behind an operand with fewer rows than the tile: one full tile of rows at its pitch (a kernel that ignores M reads poison, not
    the end of the allocation)."""
    return band(TILE_ROWS * ld)


def conv_band(W, Cin):
    """On both sides of an NHWC map: the span the convolution kernels' own descriptor checks speak of ((2 W + 2 + 256) pixels)."""
    return band((2 * W + 2 + TILE_ROWS) * Cin)


# ---------------------------------------------------------------------------------------------------------------- values
def vals(shape, seed, dtype=torch.float32, scale=1.0):
    """Uniform (-scale, scale) from a seeded CPU generator (the _mk of tests/test_gemm_gpu.py), rounded to dtype."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return ((torch.rand(shape, generator=g, dtype=torch.float32) * 2 - 1) * scale).to(dtype)


# ---------------------------------------------------------------------------------------------------------------- embedding
class Embedded:
    """A [rows, cols] matrix at pitch ld >= cols inside ONE allocation: front band | rows x ld | back band.  Both bands and the pad
    columns cols .. ld - 1 of every row hold `fill` (NaN); the body holds `body` (an input) or `fill` too (an output, which the launch
    must overwrite; its NaN carries a payload, see OUT_NAN_BITS).  t: the strided view of the body; ptr: its address; flat: the whole
    allocation; lo: the body's first element.
    intact(): everything but the body is bit-identical to what it was; unchanged(): so is the body (an input, a refused call)."""

    def __init__(self, rows, cols, ld=None, dtype=torch.float32, device="cpu", body=None, front=GUARD, back=GUARD, fill=NAN):
        ld = cols if ld is None else ld
        assert ld >= cols >= 1 and rows >= 1
        self.rows, self.cols, self.ld = rows, cols, ld
        self.lo, self.back = band(front), band(back)
        self.flat = torch.full((self.lo + rows * ld + self.back,), fill, dtype=dtype, device=device)
        self.t = self._body(self.flat)
        if body is not None:
            self.t.copy_(body.reshape(rows, cols))
        elif fill != fill and dtype in OUT_NAN_BITS:
            bits(self.flat).fill_(OUT_NAN_BITS[dtype])
        self.was = bits(self.flat).clone()
        self.was_outside = self._outside(self.was)

    def _body(self, flat):
        return flat.as_strided((self.rows, self.cols), (self.ld, 1), self.lo)

    def _outside(self, b):
        b = b.clone()
        self._body(b).zero_()
        return b

    @property
    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        return torch.equal(self._outside(bits(self.flat)), self.was_outside)

    def unchanged(self):
        return torch.equal(bits(self.flat), self.was)

    def cols_slice(self, i, width):
        """Slice i of a packed row (columns i * width .. (i + 1) * width - 1): the view and its address."""
        v = self.t[:, i * width:(i + 1) * width]
        return v, self.ptr + i * width * self.flat.element_size()


def embed(body, ld=None, device=None, front=GUARD, back=GUARD):
    """An input operand: the finite 2-D `body` embedded at pitch ld on `device`."""
    device = body.device if device is None else device
    return Embedded(body.shape[0], body.shape[1], ld, body.dtype, device, body=body, front=front, back=back)


def packed(R, n_slices, width, finite, seed, dtype, device="cpu", front=GUARD, back=GUARD):
    """[R, n_slices * width] (a packed qkv, a packed gradient): the slices named in `finite` hold values (seed + slice), every other
    slice is NaN.  Read with cols_slice()."""
    body = torch.full((R, n_slices * width), NAN, dtype=dtype)
    for i in finite:
        body[:, i * width:(i + 1) * width] = vals((R, width), seed + i, dtype)
    return embed(body, device=device, front=front, back=back)


def slabs(parts, device=None):
    """Split-K slabs [splitk, count] as the body of an allocation whose NEXT slab (slab `splitk`) is NaN: a back band of one slab."""
    return embed(parts, device=device, back=max(GUARD, parts.shape[1]))


def all_unchanged(*es):
    return all(e.unchanged() for e in es)


# ---------------------------------------------------------------------------------------------------------------- assertions
def assert_close(got, ref, tol, extra=0.0, what=""):
    """finite, and max |got - ref| <= tol max |ref| + extra (the max-norm form of every bar in tests/test_gemm_gpu.py)."""
    assert bool(torch.isfinite(got.float()).all()), (what, "not finite: a poisoned neighbour reached the output")
    ref = ref.to(got.device)
    err, top = (got.double() - ref.double()).abs().max().item(), ref.abs().max().item()
    assert err <= tol * top + extra, (what, err, top)


def assert_surroundings(outputs=(), inputs=(), what=""):
    for i, e in enumerate(outputs):
        assert e.intact(), (what, "store outside output", i)
    for i, e in enumerate(inputs):
        assert e.unchanged(), (what, "input changed", i)


# ---------------------------------------------------------------------------------------------------------------- references (fp64, bodies alone)
def matmul_ref(A, B):
    """A [M, K] B[N, K]^T from the bodies."""
    return A.t.double() @ B.t.double().t()


def conv_ref(x, w, bias, Bn, H, W):
    """x: Embedded [Bn H W, Cin] (NHWC), w: Embedded [Cout, 9 Cin] (OHWI) -> fp64 [Bn H W, Cout], zero padding 1."""
    Cin, Cout = x.cols, w.rows
    xi = x.t.double().reshape(Bn, H, W, Cin).permute(0, 3, 1, 2)
    wi = w.t.double().reshape(Cout, 3, 3, Cin).permute(0, 3, 1, 2)
    y = torch.nn.functional.conv2d(xi, wi, None if bias is None else bias.double().to(xi.device), padding=1)
    return y.permute(0, 2, 3, 1).reshape(Bn * H * W, Cout)


def conv_wgrad_ref(dy, x, Bn, H, W):
    """dy: Embedded [P, Cout], x: Embedded [P, Cin] -> fp64 (dW [Cout, 9 Cin] in OHWI order, db [Cout])."""
    Cin, Cout = x.cols, dy.cols
    xi = x.t.double().reshape(Bn, H, W, Cin).permute(0, 3, 1, 2)
    wz = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64, device=xi.device, requires_grad=True)
    y = torch.nn.functional.conv2d(xi, wz, None, padding=1)
    (gw,) = torch.autograd.grad(y, wz, dy.t.double().reshape(Bn, H, W, Cout).permute(0, 3, 1, 2))
    return gw.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin), dy.t.double().sum(0)


def splitk_ranges(K, sk, bk=64):
    """The k-range of every slab as gemm_kernel.hpp cuts it (whole k-tiles per slab; a range may end inside the last k-tile; slabs
    behind the last k-tile are empty)."""
    tiles = -(-K // bk)
    per = -(-tiles // sk)
    return [(min(K, z * per * bk), min(K, (z + 1) * per * bk)) for z in range(sk)]


# ---------------------------------------------------------------------------------------------------------------- emulations (fp32, on the storage)
def read_at(e, rows, cols, first_row=0):
    """What a kernel that walks e's storage at its pitch reads as a [rows, cols] matrix from row first_row on -- pads, bands and all."""
    return e.flat.as_strided((rows, cols), (e.ld, 1), e.lo + first_row * e.ld)


def emu_matmul(A, B, out, k_read=None, rows_read=None, store_rows=None, store_cols=None):
    """out = A B^T in fp32.  The defaults are the operation; the wrong variants: k_read = "ld" reduces over the whole pitch (a lost K-tail
    mask), rows_read / store_rows > M reads and stores a full tile of rows (ragged M written past the end), store_cols > N writes the ldc
    pad."""
    M, N, K = A.rows, B.rows, A.cols
    ka, kb = (A.ld, B.ld) if k_read == "ld" else (K, K)
    rows_read = M if rows_read is None else rows_read
    a = read_at(A, rows_read, ka).float()
    b = read_at(B, N, kb).float()
    k = min(ka, kb)
    c = a[:, :k] @ b[:, :k].t()
    store_rows = M if store_rows is None else store_rows
    store_cols = N if store_cols is None else store_cols
    full = torch.zeros((store_rows, store_cols))
    full[:min(store_rows, rows_read), :N] = c[:store_rows]
    read_at(out, store_rows, store_cols).copy_(full.to(out.flat.dtype))


def emu_conv3x3(x, w, out, Bn, H, W, flat_rows=False):
    """3 x 3 convolution (padding 1) as the im2row gather over the flat [P, Cin] storage: tap (dy, dx) of pixel p is flat pixel
    p + dy W + dx.  flat_rows: only the x border is masked -- the taps above the first and below the last image row come from the flat
    neighbours (the band, the next image) where zero padding is right."""
    Cin, Cout, P = x.cols, w.rows, Bn * H * W
    p = torch.arange(P)
    px, py = p % W, (p // W) % H
    wt = w.t.float().reshape(Cout, 9, Cin)
    acc = torch.zeros((P, Cout))
    flat = x.flat.float()
    for tap in range(9):
        dy, dx = tap // 3 - 1, tap % 3 - 1
        ok = (px + dx >= 0) & (px + dx < W)
        if not flat_rows:
            ok &= (py + dy >= 0) & (py + dy < H)
        q = p + dy * W + dx
        rows = flat[(x.lo + q[:, None] * x.ld + torch.arange(Cin)[None, :]).clamp(0, flat.numel() - 1)]
        acc += torch.where(ok[:, None], rows, torch.zeros(())) @ wt[:, tap].t()
    out.t.copy_(acc.to(out.flat.dtype))


def emu_splitk_reduce(parts, out, splitk, extra_slabs=0):
    """out = sum of the first splitk (+ extra_slabs: one slab too many) slabs, walking the storage at the slab pitch."""
    out.t.copy_(read_at(parts, splitk + extra_slabs, parts.cols).sum(0).reshape(out.t.shape))


def emu_wgrad(dy, x, part, P, extra_pixels=0):
    """part = dy^T x over P (+ extra_pixels: a k-tile past P) pixel rows of both operands' storage."""
    d = read_at(dy, P + extra_pixels, dy.cols).float()
    v = read_at(x, P + extra_pixels, x.cols).float()
    part.t.copy_((d.t() @ v).reshape(part.t.shape))
