"""CPU: the refusals of the core library's host layer (csrc/elementwise.hip, norm.hip, attention.hip, mae.hip and the exports of gemm.hip)
that are reached before any HIP call: null pointers, a bad C, n % 8, D % 4, G != 8, 0 or too many entries in the table forms, a counter
group outside 0..2.  Each is called in both libraries; the return code and the EXACT text of countr_last_error() are literals."""
import ctypes as C

import pytest

from countr_amd import _lib

P = 0x10000          # a non-null, 64 KiB-aligned "device pointer": every case below is refused before anything reads it
F32, BF16 = _lib.F32, _lib.BF16


def _ptrs(*values):
    return (C.c_void_p * len(values))(*values)


def _ints(*values):
    return (C.c_int * len(values))(*values)


def _i64(*values):
    return (C.c_int64 * len(values))(*values)


def _f32(*values):
    return (C.c_float * len(values))(*values)


def _gemm(**fields):
    a = _lib.GemmArgs()
    for k, v in dict(dict(A=P, B=P, C=P, M=128, N=128, K=128, lda=128, ldb=128, ldc=128), **fields).items():
        setattr(a, k, v)
    return C.byref(a)


T_IM2PATCH = "countr_im2patch: bad args"
T_UP_F = "countr_upsample2x_fwd: C must be 1 or a multiple of 8"
T_UP_B = "countr_upsample2x_bwd: C must be 1 or a multiple of 8"
T_COPY_N = "countr_copy_multi: 1..8 copies"
T_COPY_E = "countr_copy_multi: null, empty or not 16-byte aligned"
T_PRO = "countr_step_prologue: null / unaligned argument (16-byte pointers, mask_n % 4 == 0)"
T_GELU = "countr_gelu_bwd: n must be a multiple of 8"
T_SHADOW_N = "countr_conv_shadows: 1..32 weights"
T_TR_N = "countr_transpose16: 1..96 matrices"
T_TR_E = "countr_transpose16: rows and cols multiples of 64, 16-byte aligned matrices"
T_ADAM = "countr_adamw_step: bad args (1..16 ranges, step >= 1)"
T_ADAM_G = "countr_adamw_step: counter group must be 0, 1 or 2"
T_COLSUM = "countr_colsum: N must be a multiple of 8"
T_LN_F = "countr_layernorm_fwd: bad args (need D % 4 == 0, D <= 2048)"
T_LN_B = "countr_layernorm_bwd: bad args"
T_GN_F = "countr_groupnorm_relu_fwd: bad args (C must be 256, G <= 16)"
T_GN_ROWS = "countr_groupnorm_relu_fwd_rows: row partials are those of 8 groups of 32 channels in a 16-bit map"
T_GN_B = "countr_groupnorm_relu_bwd: bad args"
T_IN_F = "countr_instnorm_relu_pool_fwd: bad args (C % 64, even H/W)"
T_IN_B = "countr_instnorm_relu_pool_bwd: bad args"
T_SM_F = "countr_softmax_fwd: need 0 < n <= ld <= 1024"
T_SM_B = "countr_softmax_bwd: bad args"
T_XA_F = "countr_xattn_fwd: need S >= 1, D == 512, head_dim == 32"
T_XA_B = "countr_xattn_bwd: bad args (S >= 1, D == 512, head_dim == 32)"
T_MAE = "countr_mae_indices: bad args"
T_GATHER = "countr_gather_rows: null pointer or cols not a multiple of 4"
T_PMSE = "countr_patch_mse: bad args (H, W multiples of patch; 3*patch^2 <= 1024)"
T_SK_F = "countr_splitk_finish: bad args (N % 4 == 0)"
T_SK_R = "countr_splitk_reduce: bad args"
T_GROUP = "countr_gemm_group: 1 to 10 launches"


def _adam(p=P, nranges=1, groups=None, step=1, hyper=None, amp=False):
    args = [p, P, P, P, None, nranges, _i64(0, 64), _i64(64, 128), _f32(0.0, 0.0), groups, None, 1e-3, 0.9, 0.95, 1e-8, step, 1.0,
            hyper, None]
    return tuple(args + ([None] if amp else []) + [None])


# (id, export, arguments, text); every one returns -1
CASES = [
    # ---- elementwise.hip
    ("im2patch-null", "countr_im2patch", (None, P, 1, 32, 32, 16, BF16, None), T_IM2PATCH),
    ("im2patch-null-out", "countr_im2patch", (P, None, 1, 32, 32, 16, F32, None), T_IM2PATCH),
    ("im2patch-patch0", "countr_im2patch", (P, P, 1, 32, 32, 0, BF16, None), T_IM2PATCH),
    ("c3fwd-null", "countr_conv3x3_c3_fwd", (P, P, None, P, 1, 8, 8, BF16, None), "countr_conv3x3_c3_fwd: null"),
    ("c3wgrad-null", "countr_conv3x3_c3_wgrad", (P, P, P, P, None, 1, 8, 8, BF16, 0, None), "countr_conv3x3_c3_wgrad: null"),
    ("c3wgrad-2^31", "countr_conv3x3_c3_wgrad", (P, P, P, P, P, 32768, 256, 256, F32, 0, None),
     "countr_conv3x3_c3_wgrad: more than 2^31 pixels"),
    ("up2fwd-null", "countr_upsample2x_fwd", (None, P, 1, 8, 8, 8, BF16, None), T_UP_F),
    ("up2fwd-C12", "countr_upsample2x_fwd", (P, P, 1, 8, 8, 12, F32, None), T_UP_F),
    ("up2bwd-null", "countr_upsample2x_bwd", (P, None, 1, 8, 8, 8, BF16, None), T_UP_B),
    ("up2bwd-C2", "countr_upsample2x_bwd", (P, P, 1, 8, 8, 2, BF16, None), T_UP_B),
    ("copy-0", "countr_copy_multi", (0, _ptrs(P), _ptrs(P), _i64(16), None), T_COPY_N),
    ("copy-9", "countr_copy_multi", (9, _ptrs(*[P] * 9), _ptrs(*[P] * 9), _i64(*[16] * 9), None), T_COPY_N),
    ("copy-null-table", "countr_copy_multi", (1, None, _ptrs(P), _i64(16), None), T_COPY_N),
    ("copy-null-dst", "countr_copy_multi", (2, _ptrs(P, P), _ptrs(P, None), _i64(16, 16), None), T_COPY_E),
    ("copy-empty", "countr_copy_multi", (1, _ptrs(P), _ptrs(P), _i64(0), None), T_COPY_E),
    ("copy-24-bytes", "countr_copy_multi", (1, _ptrs(P), _ptrs(P), _i64(24), None), T_COPY_E),
    ("copy-unaligned", "countr_copy_multi", (1, _ptrs(P + 8), _ptrs(P), _i64(16), None), T_COPY_E),
    ("prologue-null", "countr_step_prologue", (None, 4, P, P, None, 0, None), T_PRO),
    ("prologue-slots0", "countr_step_prologue", (P, 0, P, P, None, 0, None), T_PRO),
    ("prologue-unaligned", "countr_step_prologue", (P, 4, P + 8, P, None, 0, None), T_PRO),
    ("prologue-mask-n", "countr_step_prologue", (P, 4, P, P, P, 6, None), T_PRO),
    ("gelu-null", "countr_gelu_bwd", (P, None, P, 64, BF16, None), T_GELU),
    ("gelu-n12", "countr_gelu_bwd", (P, P, P, 12, F32, None), T_GELU),
    ("cast-null", "countr_cast_permute", (None, P, 64, 0, 8, 8, 1, BF16, None), "countr_cast_permute: null"),
    ("shadows-0", "countr_conv_shadows", (0, _ptrs(P), _ptrs(P), _ptrs(P), _ints(8), _ints(8), _ints(1), BF16, None), T_SHADOW_N),
    ("shadows-33", "countr_conv_shadows", (33, _ptrs(*[P] * 33), _ptrs(*[P] * 33), _ptrs(*[P] * 33), _ints(*[8] * 33), _ints(*[8] * 33),
                                           _ints(*[1] * 33), BF16, None), T_SHADOW_N),
    ("shadows-null-table", "countr_conv_shadows", (1, _ptrs(P), _ptrs(P), None, _ints(8), _ints(8), _ints(1), F32, None), T_SHADOW_N),
    ("shadows-null-src", "countr_conv_shadows", (2, _ptrs(P, None), _ptrs(P, P), _ptrs(P, P), _ints(8, 8), _ints(8, 8), _ints(1, 1), BF16, None),
     "countr_conv_shadows: null"),
    ("shadows-10-taps", "countr_conv_shadows", (1, _ptrs(P), _ptrs(P), _ptrs(P), _ints(8), _ints(8), _ints(10), BF16, None),
     "countr_conv_shadows: at most 9 taps"),
    ("transpose-0", "countr_transpose16", (0, _ptrs(P), _ptrs(P), _ints(64), _ints(64), None), T_TR_N),
    ("transpose-97", "countr_transpose16", (97, _ptrs(*[P] * 97), _ptrs(*[P] * 97), _ints(*[64] * 97), _ints(*[64] * 97), None), T_TR_N),
    ("transpose-rows-96", "countr_transpose16", (1, _ptrs(P), _ptrs(P), _ints(96), _ints(64), None), T_TR_E),
    ("transpose-cols-32", "countr_transpose16", (1, _ptrs(P), _ptrs(P), _ints(64), _ints(32), None), T_TR_E),
    ("transpose-null-entry", "countr_transpose16", (2, _ptrs(P, None), _ptrs(P, P), _ints(64, 64), _ints(64, 64), None), T_TR_E),
    ("transpose-unaligned", "countr_transpose16", (1, _ptrs(P), _ptrs(P + 8), _ints(64), _ints(64), None), T_TR_E),
    ("mse-null", "countr_masked_mse", (P, None, P, None, P, P, 1, 64, 1.0, None), "countr_masked_mse: null"),
    ("mse-amp-null", "countr_masked_mse_amp", (P, P, P, None, P, None, 1, 64, 1.0, None, None), "countr_masked_mse: null"),
    ("adamw-null", "countr_adamw_step", _adam(p=None), T_ADAM),
    ("adamw-0-ranges", "countr_adamw_step", _adam(nranges=0), T_ADAM),
    ("adamw-17-ranges", "countr_adamw_step", _adam(nranges=17), T_ADAM),
    ("adamw-step0", "countr_adamw_step", _adam(step=0), T_ADAM),
    ("adamw-group3", "countr_adamw_step", _adam(nranges=2, groups=_ints(0, 3)), T_ADAM_G),
    ("adamw-group-neg", "countr_adamw_step", _adam(groups=_ints(-1), step=0, hyper=P), T_ADAM_G),
    ("adamw-amp-17-ranges", "countr_adamw_step_amp", _adam(nranges=17, amp=True), T_ADAM),
    ("adamw-amp-group3", "countr_adamw_step_amp", _adam(nranges=2, groups=_ints(1, 3), amp=True), T_ADAM_G),
    ("colsum-null", "countr_colsum", (P, P, None, 8, 64, BF16, 0, None), T_COLSUM),
    ("colsum-N12", "countr_colsum", (P, P, P, 8, 12, F32, 0, None), T_COLSUM),
    # ---- norm.hip
    ("ln-fwd-null", "countr_layernorm_fwd", (P, None, P, P, P, P, 8, 64, 1e-6, 1, None), T_LN_F),
    ("ln-fwd-D6", "countr_layernorm_fwd", (P, P, P, P, P, P, 8, 6, 1e-6, 0, None), T_LN_F),
    ("ln-fwd-D2052", "countr_layernorm_fwd", (P, P, P, P, P, P, 8, 2052, 1e-6, 1, None), T_LN_F),
    ("ln-fwd-rows0", "countr_layernorm_fwd", (P, P, P, P, P, P, 0, 64, 1e-6, 1, None), T_LN_F),
    ("ln-bwd-null", "countr_layernorm_bwd", (P, P, P, P, P, P, P, P, None, 8, 64, 1, 0, 0, None, None), T_LN_B),
    ("ln-bwd-D6", "countr_layernorm_bwd", (P, P, P, P, P, P, P, P, P, 8, 6, 0, 0, 0, None, None), T_LN_B),
    ("ln-bwd-D2052", "countr_layernorm_bwd", (P, P, P, P, P, P, P, P, P, 8, 2052, 1, 0, 0, None, None), T_LN_B),
    ("colsum-partials-null", "countr_colsum_partials", (None, P, 4, 64, 0, None), "countr_colsum_partials: null"),
    ("gn-fwd-null", "countr_groupnorm_relu_fwd", (P, P, P, P, None, None, None, None, P, 1, 64, 256, 8, 1e-5, BF16, None), T_GN_F),
    ("gn-fwd-C128", "countr_groupnorm_relu_fwd", (P, P, P, P, None, None, None, P, P, 1, 64, 128, 8, 1e-5, BF16, None), T_GN_F),
    ("gn-fwd-G32", "countr_groupnorm_relu_fwd", (P, P, P, P, None, None, None, P, P, 1, 64, 256, 32, 1e-5, F32, None), T_GN_F),
    ("gn-fwd-G64", "countr_groupnorm_relu_fwd", (P, P, P, P, None, None, None, P, P, 1, 64, 256, 64, 1e-5, F32, None), T_GN_F),
    ("gn-fwd-no-output", "countr_groupnorm_relu_fwd", (P, P, P, None, None, None, None, P, P, 1, 64, 256, 8, 1e-5, BF16, None), T_GN_F),
    ("gn-rows-null", "countr_groupnorm_relu_fwd_rows", (P, None, P, P, P, None, None, None, P, P, 1, 64, 256, 8, 1e-5, BF16, None),
     "countr_groupnorm_relu_fwd_rows: null row partials"),
    ("gn-rows-C128", "countr_groupnorm_relu_fwd_rows", (P, P, P, P, P, None, None, None, P, P, 1, 64, 128, 8, 1e-5, BF16, None), T_GN_F),
    ("gn-rows-G16", "countr_groupnorm_relu_fwd_rows", (P, P, P, P, P, None, None, None, P, P, 1, 64, 256, 16, 1e-5, BF16, None), T_GN_ROWS),
    ("gn-rows-fp32", "countr_groupnorm_relu_fwd_rows", (P, P, P, P, P, None, None, None, P, P, 1, 64, 256, 8, 1e-5, F32, None), T_GN_ROWS),
    ("gn-rows-unaligned", "countr_groupnorm_relu_fwd_rows", (P, P + 4, P, P, P, None, None, None, P, P, 1, 64, 256, 8, 1e-5, BF16, None),
     T_GN_ROWS),
    ("gn-bwd-null", "countr_groupnorm_relu_bwd", (P, P, None, None, None, P, P, P, P, P, None, None, P, 1, 64, 256, 8, BF16, 0, None), T_GN_B),
    ("gn-bwd-C128", "countr_groupnorm_relu_bwd", (P, P, None, None, P, P, P, P, P, P, None, None, P, 1, 64, 128, 8, BF16, 0, None), T_GN_B),
    ("gn-bwd-no-gradient", "countr_groupnorm_relu_bwd", (P, None, P, None, P, P, P, P, P, P, None, None, P, 1, 64, 256, 8, F32, 0, None), T_GN_B),
    ("gn-bwd-G4", "countr_groupnorm_relu_bwd", (P, P, None, None, P, P, P, P, P, P, None, None, P, 1, 64, 256, 4, BF16, 0, None),
     "countr_groupnorm_relu_bwd: G must be 8"),
    ("gn-bwd-G16", "countr_groupnorm_relu_bwd", (P, P, None, None, P, P, P, P, P, P, None, None, P, 1, 64, 256, 16, F32, 0, None),
     "countr_groupnorm_relu_bwd: G must be 8"),
    ("in-fwd-null", "countr_instnorm_relu_pool_fwd", (P, None, P, 1, 8, 8, 64, 0, 1e-5, BF16, None, None, 0, None), T_IN_F),
    ("in-fwd-C32", "countr_instnorm_relu_pool_fwd", (P, P, P, 1, 8, 8, 32, 0, 1e-5, F32, None, None, 0, None), T_IN_F),
    ("in-fwd-odd-H", "countr_instnorm_relu_pool_fwd", (P, P, P, 1, 7, 8, 64, 0, 1e-5, BF16, None, None, 0, None), T_IN_F),
    ("in-fwd-odd-W", "countr_instnorm_relu_pool_fwd", (P, P, P, 1, 8, 9, 64, 1, 1e-5, BF16, None, None, 1, None), T_IN_F),
    ("in-fwd-xhat-in-place", "countr_instnorm_relu_pool_fwd", (P, P + 4096, P, 1, 8, 8, 64, 0, 1e-5, BF16, None, P, 1, None),
     "countr_instnorm_relu_pool_fwd: a bf16 x-hat cannot be stored in place of an fp32 map"),
    ("in-bwd-null", "countr_instnorm_relu_pool_bwd", (P, P, None, P, 1, 8, 8, 64, 0, BF16, None, 0, None), T_IN_B),
    ("in-bwd-C96", "countr_instnorm_relu_pool_bwd", (P, P, P, P, 1, 8, 8, 96, 0, F32, None, 0, None), T_IN_B),
    # ---- attention.hip
    ("softmax-null", "countr_softmax_fwd", (None, P, 8, 64, 1, None), T_SM_F),
    ("softmax-n0", "countr_softmax_fwd", (P, P, 8, 0, 0, None), T_SM_F),
    ("softmax-n1025", "countr_softmax_fwd", (P, P, 8, 1025, 1, None), T_SM_F),
    ("softmax-ld-null", "countr_softmax_fwd_ld", (P, None, 8, 64, 64, 1, None), T_SM_F),
    ("softmax-ld-short", "countr_softmax_fwd_ld", (P, P, 8, 64, 63, 0, None), T_SM_F),
    ("softmax-ld-1032", "countr_softmax_fwd_ld", (P, P, 8, 64, 1032, 1, None), T_SM_F),
    ("softmax-bwd-null", "countr_softmax_bwd", (P, None, P, 8, 64, 1.0, BF16, None), T_SM_B),
    ("softmax-bwd-n1025", "countr_softmax_bwd", (P, P, P, 8, 1025, 1.0, F32, None), T_SM_B),
    ("xattn-fwd-null", "countr_xattn_fwd", (P, P, None, P, 1, 16, 3, 512, 16, 512, 1.0, BF16, None), T_XA_F),
    ("xattn-fwd-S0", "countr_xattn_fwd", (P, P, P, P, 1, 16, 0, 512, 16, 512, 1.0, BF16, None), T_XA_F),
    ("xattn-fwd-D256", "countr_xattn_fwd", (P, P, P, P, 1, 16, 3, 256, 8, 256, 1.0, F32, None), T_XA_F),
    ("xattn-fwd-heads8", "countr_xattn_fwd", (P, P, P, P, 1, 16, 3, 512, 8, 512, 1.0, BF16, None), T_XA_F),
    ("xattn-bwd-null", "countr_xattn_bwd", (P, P, P, P, P, P, P, None, 1, 16, 3, 512, 16, 512, 1.0, BF16, None, None, None), T_XA_B),
    ("xattn-bwd-S0", "countr_xattn_bwd", (P, P, P, P, P, P, P, P, 1, 16, 0, 512, 16, 512, 1.0, F32, None, None, None), T_XA_B),
    ("xattn-bwd-D1024", "countr_xattn_bwd", (P, P, P, P, P, P, P, P, 1, 16, 9, 1024, 32, 1024, 1.0, BF16, None, None, None), T_XA_B),
    # ---- mae.hip
    ("mae-null", "countr_mae_indices", (P, P, P, P, P, P, None, 1, 16, 4, None), T_MAE),
    ("mae-K-above-N", "countr_mae_indices", (P, P, P, P, P, P, P, 1, 16, 17, None), T_MAE),
    ("mae-K0", "countr_mae_indices", (P, P, P, P, P, P, P, 1, 16, 0, None), T_MAE),
    ("mae-no-mask-src", "countr_mae_indices", (P, P, P, P, P, None, P, 1, 16, 4, None), T_MAE),
    ("gather-null", "countr_gather_rows", (None, P, P, None, None, 0, 4, 64, BF16, BF16, None), T_GATHER),
    ("gather-cols6", "countr_gather_rows", (P, P, P, None, None, 0, 4, 6, BF16, F32, None), T_GATHER),
    ("gather-cols0", "countr_gather_rows", (P, P, P, None, None, 0, 4, 0, F32, BF16, None), T_GATHER),
    ("gather-rows0", "countr_gather_rows", (P, P, P, None, None, 0, 0, 64, F32, F32, None), T_GATHER),
    ("patch-mse-null", "countr_patch_mse", (P, P, P, None, P, 1, 32, 32, 16, 0, 1.0, BF16, None), T_PMSE),
    ("patch-mse-H-rest", "countr_patch_mse", (P, P, P, P, P, 1, 40, 32, 16, 0, 1.0, F32, None), T_PMSE),
    ("patch-mse-patch19", "countr_patch_mse", (P, P, P, P, P, 1, 38, 38, 19, 1, 1.0, BF16, None), T_PMSE),
    ("patch-mse-amp-patch0", "countr_patch_mse_amp", (P, P, P, P, P, 1, 32, 32, 0, 0, 1.0, BF16, None, None), T_PMSE),
    ("patch-mse-amp-null", "countr_patch_mse_amp", (None, P, P, P, P, 1, 32, 32, 16, 0, 1.0, F32, P, None), T_PMSE),
    # ---- gemm.hip
    ("reduce-table-null", "countr_reduce_table", (None, 1, 1, None), "countr_reduce_table: bad args"),
    ("reduce-table-n0", "countr_reduce_table", (P, 0, 1, None), "countr_reduce_table: bad args"),
    ("reduce-table-blocks0", "countr_reduce_table", (P, 1, 0, None), "countr_reduce_table: bad args"),
    ("splitk-finish-null", "countr_splitk_finish", (P, None, None, 2, 8, 64, 1, None), T_SK_F),
    ("splitk-finish-N6", "countr_splitk_finish", (P, P, None, 2, 8, 6, 0, None), T_SK_F),
    ("splitk-finish-splitk0", "countr_splitk_finish", (P, P, None, 0, 8, 64, 1, None), T_SK_F),
    ("splitk-reduce-null", "countr_splitk_reduce", (None, P, 2, 8, 64, 0, 0, None, None, None), T_SK_R),
    ("splitk-reduce-rowsum", "countr_splitk_reduce", (P, P, 2, 8, 64, 0, 0, P, None, None), T_SK_R),
    ("gemm-group-null", "countr_gemm_group", (None, 1, BF16, 0, 0, None), T_GROUP),
    ("gemm-group-0", "countr_gemm_group", (_gemm(), 0, BF16, 0, 0, None), T_GROUP),
    ("gemm-group-11", "countr_gemm_group", (_gemm(), 11, BF16, 1, 1, None), T_GROUP),
    ("gemm-null", "countr_gemm", (None, BF16, 0, 0, None), "countr_gemm: null pointer"),
    ("gemm-no-output", "countr_gemm", (_gemm(C=None), F32, 0, 0, None), "countr_gemm: null pointer"),
    ("gemm-splitk", "countr_gemm", (_gemm(splitk=2), BF16, 0, 0, None), "countr_gemm: bad split-K setup"),
    ("gemm-rowsum-fp32", "countr_gemm", (_gemm(partial=P, rowsum_partial=P), F32, 1, 1, None),
     "countr_gemm: rowsum_partial needs the bf16 split-K path"),
    ("gemm-act", "countr_gemm", (_gemm(act=3), BF16, 0, 0, None),
     "countr_gemm: bad activation code (GELU_BWD needs the saved pre-activation in C2 and no split-K)"),
    ("gemm-N6", "countr_gemm", (_gemm(N=6), BF16, 0, 0, None), "countr_gemm: bad shape (need N % 4 == 0)"),
    ("gemm-K-chunk", "countr_gemm", (_gemm(K=132), BF16, 0, 0, None), "countr_gemm: K must be a multiple of the 16-byte chunk"),
    ("gemm-M-chunk", "countr_gemm", (_gemm(M=132), BF16, 1, 1, None), "countr_gemm: M must be a multiple of the chunk for COL A"),
    ("gemm-N-chunk", "countr_gemm", (_gemm(N=132), BF16, 1, 1, None), "countr_gemm: N must be a multiple of the chunk for COL B"),
    ("gemm-Cin", "countr_gemm", (_gemm(Cin=96, H=8, W=8), BF16, 2, 0, None), "countr_gemm: conv modes need Cin % 64 == 0"),
    ("gemm-gn-rows", "countr_gemm", (_gemm(gn_rows=P), BF16, 0, 0, None),
     "countr_gemm: gn_rows is an output of the bf16 (IM2ROW, ROW) convolution launches only"),
]
assert len({c[0] for c in CASES}) == len(CASES)


@pytest.mark.parametrize("variant", ["", "f16"], ids=["bf16", "f16"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_refusal_code_and_text(case, variant):
    _id, name, args, text = case
    L = _lib.lib(variant)
    assert len(args) == len(_lib.PROTOS[name][1]), name
    # another refusal first, so that the text read below is the one this call left
    other = ("countr_colsum_partials", (None, None, 1, 8, 0, None), b"countr_colsum_partials: null") if name != "countr_colsum_partials" \
        else ("countr_reduce_table", (None, 1, 1, None), b"countr_reduce_table: bad args")
    assert getattr(L, other[0])(*other[1]) == -1 and L.countr_last_error() == other[2]
    assert getattr(L, name)(*args) == -1
    assert L.countr_last_error() == text.encode()
