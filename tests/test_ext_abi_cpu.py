"""CPU: include/countr_hip_ext.h is the one statement of the extension library's C ABI, as include/countr_hip.h is of the main
libraries'.  countr_amd/_lib.py reads the binding from it and libcountr_hip_ext.so exports exactly it; pinned here by literals (the
checks against the C compiler and the library's dynamic symbols are in tests/test_libraries_cpu.py, once per tag)."""
import ctypes as C

from countr_amd import _lib


def test_version_limits_binding_and_errors():
    # the literal pins of the header's names (what holds of every library by rule is in test_libraries_cpu.py)
    assert list(_lib.EXT_STRUCTS) == ["countr_region_map", "countr_region"]
    assert (C.sizeof(_lib.RegionMap), C.sizeof(_lib.Region)) == (24, 20)
    assert [f for f, _t in _lib.RegionMap._fields_] == ["map", "h", "w", "set", "place"]
    assert [f for f, _t in _lib.Region._fields_] == ["set", "nv", "gy", "gx", "data"]
    assert _lib.ext_exported_symbols() == ["countr_ext_last_error", "countr_ext_version", "countr_region_sums", "countr_regions_workspace"]
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
