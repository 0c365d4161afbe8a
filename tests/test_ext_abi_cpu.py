"""CPU: include/countr_hip_ext.h is the one statement of the extension library's C ABI, as include/countr_hip.h is of the main
libraries'.  countr_amd/_lib.py reads the binding from it and libcountr_hip_ext.so exports exactly it; checked against the compiler
(layout), the library's own dynamic symbols and literal pins."""
import ctypes as C
import glob
import os
import re
import subprocess

from countr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")      # the compiler countr_amd/build.py uses


def test_struct_layout_equals_the_compilers(tmp_path):
    want, body = [], []
    for name, cls in _lib.EXT_STRUCTS.items():
        want.append("%s %d" % (name, C.sizeof(cls)))
        body.append('  printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        for field, _ctype in cls._fields_:
            want.append("%s.%s %d %d" % (name, field, getattr(cls, field).offset, getattr(cls, field).size))
            body.append('  printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (name, field, name, field, name, field))
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "countr_hip_ext.h"\nint main(void) {\n%s\n  return 0;\n}\n' % "\n".join(body))
    subprocess.check_call([HIPCC, "-x", "c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")])
    got = subprocess.check_output([str(tmp_path / "layout")], text=True).splitlines()
    assert list(_lib.EXT_STRUCTS) == ["countr_region_map", "countr_region"]
    assert got == want
    assert (C.sizeof(_lib.RegionMap), C.sizeof(_lib.Region)) == (24, 20)
    assert [f for f, _t in _lib.RegionMap._fields_] == ["map", "h", "w", "set", "place"]
    assert [f for f, _t in _lib.Region._fields_] == ["set", "nv", "gy", "gx", "data"]


def test_library_exports_the_header_and_nothing_else():
    readelf = subprocess.check_output([HIPCC, "-print-prog-name=llvm-readelf"], text=True).strip()
    rows = [line.split() for line in subprocess.check_output([readelf, "--dyn-syms", "-W", _lib.EXT_LIB_PATH], text=True).splitlines()]
    defined = [r[7].split("@")[0] for r in rows if len(r) == 8 and r[0][:-1].isdigit() and r[6] != "UND"]
    assert sorted(n for n in defined if n.startswith("countr_")) == _lib.ext_exported_symbols()
    assert _lib.ext_exported_symbols() == ["countr_ext_last_error", "countr_ext_version", "countr_region_sums", "countr_regions_workspace"]
    assert [n for n in defined if not n.startswith(("countr_", "__hip_cuid_"))] == []


def test_every_prototype_is_defined_extern_c_in_the_sources():
    paths = glob.glob(os.path.join(ROOT, "countr_amd", "csrc_ext", "*.hip"))
    src = "".join(open(p).read() for p in paths)
    for name in _lib.ext_exported_symbols():
        assert re.search(r'extern "C" [\w ]+\*? ?%s\(' % name, src), name
    assert re.search(r"countr_ext_version\(void\) \{ return COUNTR_EXT_ABI_VERSION; \}", src)
    # the extension's sources stay outside the glob the main libraries are built from
    assert paths and not set(os.path.basename(p) for p in paths) & set(os.path.basename(p) for p in glob.glob(os.path.join(ROOT, "countr_amd", "csrc", "*.hip")))


def test_version_limits_binding_and_errors():
    main = (dict(_lib.CONSTS), dict(_lib.STRUCTS), dict(_lib.PROTOS), _lib.exported_symbols())
    E = _lib.ext_lib()
    assert E.countr_ext_version() == _lib.EXT_CONSTS["COUNTR_EXT_ABI_VERSION"] == 1
    assert {k: v for k, v in _lib.EXT_CONSTS.items() if "_MAX" in k} == {
        "COUNTR_REGIONS_MAX_MAPS": 16, "COUNTR_REGIONS_MAX_REGIONS": 64, "COUNTR_REGIONS_MAX_VERTICES": 64, "COUNTR_REGIONS_MAX_CELLS": 256}
    vp = C.c_void_p
    assert E.countr_ext_last_error.restype is C.c_char_p and E.countr_ext_last_error.argtypes == []
    assert E.countr_region_sums.argtypes == [C.POINTER(_lib.RegionMap), C.c_int, C.POINTER(_lib.Region), C.c_int, C.c_int, vp, vp, C.c_int, vp, vp,
                                             vp, vp, vp]
    assert E.countr_regions_workspace.argtypes == [C.POINTER(_lib.RegionMap), C.c_int, C.POINTER(_lib.Region), C.c_int, C.c_int]
    # loading the extension leaves the main binding as the pinned test reads it
    assert (dict(_lib.CONSTS), dict(_lib.STRUCTS), dict(_lib.PROTOS), _lib.exported_symbols()) == main
    assert len(_lib.PROTOS) == 87 and len(_lib.STRUCTS) == 10 and not set(_lib.EXT_PROTOS) & set(_lib.PROTOS)
    assert not any(k.startswith(("REGIONS_", "EXT_ABI")) for k in vars(_lib))
    # the size export runs on the host: a strip is 4 rows (at most 256 strips a map), a partial is a float and an int per slot + the total
    maps = (_lib.RegionMap * 2)()
    regs = (_lib.Region * 2)()
    for m, (h, w) in zip(maps, ((33, 130), (5, 7))):
        m.h, m.w, m.set = h, w, 0
    regs[0].nv, regs[1].gy, regs[1].gx = 5, 4, 4
    assert E.countr_regions_workspace(maps, 2, regs, 2, 1) == (9 + 2) * (1 + 16 + 1) * 8
    regs[0].nv = 2
    assert E.countr_regions_workspace(maps, 2, regs, 2, 1) < 0 and b"3..64 vertices" in E.countr_ext_last_error()
    try:
        _lib.ext_check(-1, "probe")
    except _lib.CountrError as e:
        assert "3..64 vertices" in str(e)
    else:
        raise AssertionError("ext_check(-1) did not raise")
