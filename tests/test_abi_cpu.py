"""CPU: include/countr_hip.h is the one statement of the C ABI.  countr_amd/_lib.py reads its binding from it and both libraries export
exactly it; checked here against the compiler (layout), the libraries' own dynamic symbols, and literal pins that keep a parser bug
from agreeing with itself."""
import ctypes as C
import glob
import os
import re
import subprocess

import pytest

from countr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")      # the compiler countr_amd/build.py uses


def test_struct_layout_equals_the_compilers(tmp_path):
    """sizeof of every struct and offsetof / sizeof of every field, printed by a C program that includes the header (which so is valid C)."""
    want, body = [], []
    for name, cls in _lib.STRUCTS.items():
        want.append("%s %d" % (name, C.sizeof(cls)))
        body.append('  printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        for field, _ctype in cls._fields_:
            want.append("%s.%s %d %d" % (name, field, getattr(cls, field).offset, getattr(cls, field).size))
            body.append('  printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (name, field, name, field, name, field))
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "countr_hip.h"\nint main(void) {\n%s\n  return 0;\n}\n' % "\n".join(body))
    subprocess.check_call([HIPCC, "-x", "c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")])
    got = subprocess.check_output([str(tmp_path / "layout")], text=True).splitlines()
    assert len(_lib.STRUCTS) == 10 and len(want) > 100
    assert got == want


@pytest.mark.parametrize("path", [_lib.LIB_PATH, _lib.LIB_PATH_F16])
def test_library_exports_the_header_and_nothing_else(path):
    readelf = subprocess.check_output([HIPCC, "-print-prog-name=llvm-readelf"], text=True).strip()      # the one beside the compiler
    rows = [line.split() for line in subprocess.check_output([readelf, "--dyn-syms", "-W", path], text=True).splitlines()]
    defined = [r[7].split("@")[0] for r in rows if len(r) == 8 and r[0][:-1].isdigit() and r[6] != "UND"]      # Num Value Size Type Bind Vis Ndx Name
    assert sorted(n for n in defined if n.startswith("countr_")) == _lib.exported_symbols()
    assert [n for n in defined if not n.startswith(("countr_", "__hip_cuid_"))] == []


def test_binding_pins_one_per_type_class():
    P, vp = _lib.PROTOS, C.c_void_p
    L = _lib.lib()
    assert L.countr_softmax_fwd.argtypes[2] is C.c_int64                                   # int64_t
    assert L.countr_aug_normal.argtypes[3:5] == [C.c_uint64, C.c_uint64]                   # uint64_t
    assert L.countr_layernorm_fwd.argtypes[8] is C.c_float                                 # float
    assert L.countr_layernorm_fwd.argtypes == [vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_float, C.c_int, vp]
    assert L.countr_xattn_bwd_workspace_floats.restype is C.c_int64                        # int64_t result
    assert L.countr_groupnorm_bwd_image_sums_offset.restype is C.c_int64                   # long long result
    assert L.countr_last_error.restype is C.c_char_p and L.countr_last_error.argtypes == []
    assert L.countr_version.restype is C.c_int and L.countr_version.argtypes == []
    assert L.countr_gemm.argtypes[0] is C.POINTER(_lib.GemmArgs)                           # pointer to a struct of the header
    assert L.countr_copy_multi.argtypes == [C.c_int, vp, vp, vp, vp]                       # pointers to pointers, to int64_t
    assert L.countr_reduce_table.argtypes[0] is vp                                         # const long long*
    fields = dict(_lib.AugImage._fields_)
    assert fields["affine"] is C.c_double * 6 and fields["kx"] is C.c_float * 7 and fields["counter"] is C.c_uint64
    assert dict(_lib.ReportImage._fields_)["maps"] is C.c_void_p * 9 and dict(_lib.ReportImage._fields_)["labels"] is _lib.ReportPatch
    assert dict(_lib.MosaicImage._fields_)["piece"] is _lib.MosaicPiece * 4
    assert [f for f, _t in _lib.GemmArgs._fields_[7:11]] == ["lda", "ldb", "ldc", "ldres"]                  # a declarator list
    assert [f for f, _t in _lib.MatchSet._fields_] == ["pred", "gt", "P", "G", "max_dist", "offset"]
    assert (C.sizeof(_lib.GemmArgs), C.sizeof(_lib.AugImage), C.sizeof(_lib.MatchSet)) == (272, 304, 32)
    assert len(P) == 87 == len(_lib.exported_symbols())
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    for name, (_restype, argtypes) in P.items():
        params = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, hdr).group(1).strip()
        assert getattr(L, name).argtypes == argtypes and len(argtypes) == (0 if params == "void" else params.count(",") + 1), name
    for variant in ("", "f16"):
        assert _lib.lib(variant).countr_version() == _lib.CONSTS["COUNTR_ABI_VERSION"] == _lib.ABI_VERSION == 9
    assert (_lib.F32, _lib.BF16, _lib.OP_ROW, _lib.OP_COL, _lib.OP_IM2ROW, _lib.OP_IM2COL) == (0, 1, 0, 1, 2, 3)
    assert (_lib.ACT_NONE, _lib.ACT_GELU, _lib.ACT_GELU_BWD) == (0, 1, 2)
    limits = {k[7:]: v for k, v in _lib.CONSTS.items() if "_MAX" in k}
    assert limits == {"AUG_MAX_IMAGES": 32, "PRETRAIN_MAX_IMAGES": 16, "REPORT_MAX_IMAGES": 16, "PEAKS_MAX_MAPS": 16, "PEAKS_MAX_RADIUS": 8,
                      "PEAKS_MAX_POINTS": 8192, "MATCH_MAX_SETS": 16, "MATCH_MAX_POINTS": 8192, "FRAMES_MAX": 16, "CARPK_MAX_FRAMES": 16,
                      "WINDOW_MAX_STARTS": 16}


def test_wrappers_take_their_limits_from_the_header():
    from countr_amd import carpk, frames, inference, match, peaks, pretrain_aug, report
    assert (peaks.MAX_MAPS, peaks.MAX_RADIUS, peaks.MAX_CAP) == (16, 8, 8192) and (match.MAX_SETS, match.MAX_POINTS) == (16, 8192)
    assert frames.MAX_BATCHED == carpk.MAX_FRAMES == report.MAX_GROUP == inference.MAX_BLEND_WINDOWS == pretrain_aug.GROUP == 16


def test_every_prototype_is_defined_extern_c_in_the_sources():
    src = "".join(open(p).read() for p in glob.glob(os.path.join(ROOT, "countr_amd", "csrc", "*.hip")))
    for name in _lib.exported_symbols():
        assert re.search(r'extern "C" [\w ]+\*? ?%s\(' % name, src), name
    assert re.search(r"countr_version\(void\) \{ return COUNTR_ABI_VERSION; \}", src)


@pytest.mark.parametrize("text", ["int countr_x(size_t n);\n}", "int countr_x(int);\n}", "int countr_x(const foo_t* p);\n}",
                                  "unsigned countr_x(void);\n}", "typedef struct countr_s { short a; } countr_s;\n}",
                                  "typedef struct countr_s { int a : 3; } countr_s;\n}", "int countr_x(int a)\n}", "#define COUNTR_X (1 << 4)\n}"])
def test_parser_refuses_what_it_does_not_know(text):
    assert _lib.parse_header("int countr_x(const float* p, int64_t n);\n}")[2] == {"countr_x": (C.c_int, [C.c_void_p, C.c_int64])}
    with pytest.raises((_lib.CountrError, ValueError)):
        _lib.parse_header(text)
