"""CPU: include/countr_hip_classes.h is the one statement of the classes library's C ABI, as countr_hip.h and countr_hip_ext.h are of
theirs.  countr_amd/_lib.py reads the binding from it and libcountr_hip_classes.so exports exactly it; pinned here by literals (the
checks against the C compiler and the library's dynamic symbols are in tests/test_libraries_cpu.py, once per tag)."""
import ctypes as C

from countr_amd import _lib


def test_version_limits_binding_and_errors():
    # the literal pins of the header's names (what holds of every library by rule is in test_libraries_cpu.py)
    assert list(_lib.CLASSES_STRUCTS) == ["countr_class_set"]
    assert C.sizeof(_lib.ClassSet) == 216          # 16 pointers, a pointer, 16 floats, three ints, padded to 8
    assert [f for f, _t in _lib.ClassSet._fields_] == ["map", "labels", "scale", "nc", "h", "w"]
    assert _lib.classes_exported_symbols() == ["countr_class_fold", "countr_classes_last_error", "countr_classes_version", "countr_classes_workspace"]
    snapshot = lambda: (dict(_lib.CONSTS), dict(_lib.STRUCTS), dict(_lib.PROTOS), _lib.exported_symbols(),
                        dict(_lib.EXT_CONSTS), dict(_lib.EXT_STRUCTS), dict(_lib.EXT_PROTOS), _lib.ext_exported_symbols())
    before = snapshot()
    K = _lib.classes_lib()
    assert K.countr_classes_version() == _lib.CLASSES_CONSTS["COUNTR_CLASSES_ABI_VERSION"] == 1
    assert {k: v for k, v in _lib.CLASSES_CONSTS.items() if "_MAX" in k} == {"COUNTR_CLASSES_MAX_SETS": 16, "COUNTR_CLASSES_MAX": 16}
    vp = C.c_void_p
    assert K.countr_classes_last_error.restype is C.c_char_p and K.countr_classes_last_error.argtypes == []
    assert K.countr_classes_workspace.argtypes == [C.POINTER(_lib.ClassSet), C.c_int]
    assert K.countr_class_fold.argtypes == [C.POINTER(_lib.ClassSet), C.c_int, vp, C.c_float, vp, vp, vp, vp, vp]
    # loading the classes library leaves the two older bindings as their pinned tests read them
    assert snapshot() == before
    assert len(_lib.PROTOS) == 87 and len(_lib.STRUCTS) == 10 and len(_lib.EXT_PROTOS) == 4 and list(_lib.EXT_STRUCTS) == ["countr_region_map", "countr_region"]
    assert not set(_lib.CLASSES_PROTOS) & (set(_lib.PROTOS) | set(_lib.EXT_PROTOS))
    assert not any(k.startswith(("REGIONS_", "EXT_ABI", "CLASSES_MAX", "CLASSES_ABI")) for k in vars(_lib))
    # the size export runs on the host: a strip is 16 rows (at most 256 strips a set), a partial is 3 x 16 four-byte sums
    sets = (_lib.ClassSet * 3)()
    for d, (h, w, nc) in zip(sets, ((33, 130, 2), (5, 7, 16), (5000, 3, 1))):
        d.h, d.w, d.nc = h, w, nc
    assert K.countr_classes_workspace(sets, 2) == (3 + 1) * 48 * 4
    assert K.countr_classes_workspace(sets, 3) == (3 + 1 + 250) * 48 * 4       # 5000 rows: strips of ceil(5000 / 256) = 20 rows
    sets[1].nc = 17
    assert K.countr_classes_workspace(sets, 2) < 0 and b"1..16 classes" in K.countr_classes_last_error()
    try:
        _lib.classes_check(-1, "probe")
    except _lib.CountrError as e:
        assert "1..16 classes" in str(e)
    else:
        raise AssertionError("classes_check(-1) did not raise")
    sets[1].nc = 16
    assert K.countr_classes_workspace(sets, 17) < 0 and b"1..16 sets" in K.countr_classes_last_error()
    sets[0].h, sets[0].w = 1 << 14, (1 << 14) + 1
    assert K.countr_classes_workspace(sets, 1) < 0 and b"2^28 pixels" in K.countr_classes_last_error()
