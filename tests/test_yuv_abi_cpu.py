"""CPU: include/countr_hip_yuv.h is the one statement of the yuv library's C ABI, as the four older headers are of theirs.
countr_amd/_lib.py reads the binding from it and libcountr_hip_yuv.so exports exactly it; pinned here by literals (the checks against
the C compiler and the library's dynamic symbols are in tests/test_libraries_cpu.py, once per tag).  Every refusal runs on the host: a
refused call launches nothing."""
import ctypes as C

from countr_amd import _lib, build

NAMES = ("ABI_VERSION", "MAX_FRAMES", "MAX_SIDE", "NV12", "NV21", "I420", "P010", "BT601", "BT709", "LIMITED", "FULL", "NEAREST", "LINEAR")


def test_version_limits_binding_and_errors():
    # the literal pins of the header's names (what holds of every library by rule is in test_libraries_cpu.py)
    assert list(_lib.YUV_STRUCTS) == []            # plain pointers and sizes only
    assert list(_lib.YUV_CONSTS) == ["COUNTR_YUV_" + n for n in NAMES]
    assert _lib.yuv_exported_symbols() == ["countr_yuv_last_error", "countr_yuv_to_rgb", "countr_yuv_version"]
    # the one table of the side libraries, in the order they were added, up to this one
    assert list(build.SINGLE)[:4] == ["ext", "classes", "tiles", "yuv"]
    snapshot = lambda: (dict(_lib.CONSTS), dict(_lib.STRUCTS), dict(_lib.PROTOS), _lib.exported_symbols(),
                        dict(_lib.EXT_CONSTS), dict(_lib.EXT_STRUCTS), dict(_lib.EXT_PROTOS), _lib.ext_exported_symbols(),
                        dict(_lib.CLASSES_CONSTS), dict(_lib.CLASSES_STRUCTS), dict(_lib.CLASSES_PROTOS), _lib.classes_exported_symbols(),
                        dict(_lib.TILES_CONSTS), dict(_lib.TILES_STRUCTS), dict(_lib.TILES_PROTOS), _lib.tiles_exported_symbols())
    before = snapshot()
    Y = _lib.yuv_lib()
    assert Y.countr_yuv_version() == _lib.YUV_CONSTS["COUNTR_YUV_ABI_VERSION"] == 1
    assert _lib.YUV_CONSTS == {"COUNTR_YUV_ABI_VERSION": 1, "COUNTR_YUV_MAX_FRAMES": 16, "COUNTR_YUV_MAX_SIDE": 16384, "COUNTR_YUV_NV12": 0,
                               "COUNTR_YUV_NV21": 1, "COUNTR_YUV_I420": 2, "COUNTR_YUV_P010": 3, "COUNTR_YUV_BT601": 0, "COUNTR_YUV_BT709": 1,
                               "COUNTR_YUV_LIMITED": 0, "COUNTR_YUV_FULL": 1, "COUNTR_YUV_NEAREST": 0, "COUNTR_YUV_LINEAR": 1}
    vp, ci = C.c_void_p, C.c_int
    assert Y.countr_yuv_last_error.restype is C.c_char_p and Y.countr_yuv_last_error.argtypes == []
    assert Y.countr_yuv_to_rgb.restype is ci and Y.countr_yuv_to_rgb.argtypes == [vp, vp, vp, vp] + [ci] * 9 + [vp]
    # loading the yuv library leaves the four older bindings as their pinned tests read them
    assert snapshot() == before
    assert len(_lib.PROTOS) == 87 and len(_lib.EXT_PROTOS) == 4 and len(_lib.CLASSES_PROTOS) == 4 and len(_lib.TILES_PROTOS) == 5
    assert not set(_lib.YUV_PROTOS) & (set(_lib.PROTOS) | set(_lib.EXT_PROTOS) | set(_lib.CLASSES_PROTOS) | set(_lib.TILES_PROTOS))
    assert not any(k.startswith(("REGIONS_", "EXT_ABI", "CLASSES_MAX", "CLASSES_ABI", "TILES_MAX", "TILES_ABI", "TILES_SIZE", "YUV_ABI",
                                 "YUV_MAX", "YUV_NV", "YUV_BT")) for k in vars(_lib))
    try:
        _lib.yuv_check(-1, "probe")
    except _lib.CountrError as e:
        assert "probe failed" in str(e)
    else:
        raise AssertionError("yuv_check(-1) did not raise")


def ptrs(values):
    return (C.c_void_p * len(values))(*values)


def test_refusals_run_on_the_host():
    """Every refusal returns before a plane is read or a kernel is launched: the device pointers are aligned numbers, not buffers."""
    Y = _lib.yuv_lib()
    K = {k[len("COUNTR_YUV_"):]: v for k, v in _lib.YUV_CONSTS.items()}
    err = lambda: Y.countr_yuv_last_error().decode()
    ys, c0, c1, rgb = (ptrs([0x10000 * k + 0x100 * j for j in range(1, 18)]) for k in range(1, 5))

    def call(n=1, H=4, W=6, py=6, pc=6, fmt=K["NV12"], matrix=K["BT709"], rng=K["LIMITED"], chroma=K["NEAREST"], y=ys, a=c0, b=None, out=rgb):
        return Y.countr_yuv_to_rgb(y, a, b, out, n, H, W, py, pc, fmt, matrix, rng, chroma, None)

    # n out of range
    assert call(n=0) < 0 and "1..16 frames a call, got 0" in err()
    assert call(n=17) < 0 and "got 17" in err()
    assert call(n=-1) < 0 and "got -1" in err()
    # an unknown enum
    assert call(fmt=4) < 0 and "unknown format 4" in err()
    assert call(fmt=-1) < 0 and "unknown format -1" in err()
    assert call(matrix=2) < 0 and "unknown matrix 2" in err()
    assert call(rng=7) < 0 and "unknown range 7" in err()
    assert call(chroma=2) < 0 and "unknown chroma reconstruction 2" in err()
    # H or W outside 1..16384
    assert call(H=0) < 0 and "1..16384, got 0 x 6" in err()
    assert call(W=0) < 0 and "got 4 x 0" in err()
    assert call(H=16385, py=6) < 0 and "got 16385 x 6" in err()
    assert call(W=16385, py=16385, pc=16386) < 0 and "got 4 x 16385" in err()
    # a pitch below the row's bytes (an odd W: the chroma row has W + 1 bytes), or odd for p010
    assert call(py=5) < 0 and "pitch_y 5: a Y row has 6 bytes" in err()
    assert call(W=7, py=7, pc=7) < 0 and "pitch_c 7: a chroma row has 8 bytes" in err()
    assert call(fmt=K["I420"], W=7, py=7, pc=3, b=c1) < 0 and "pitch_c 3: a chroma row has 4 bytes" in err()
    assert call(fmt=K["P010"], py=11, pc=12) < 0 and "pitch_y 11: a Y row has 12 bytes" in err()
    assert call(fmt=K["P010"], py=13, pc=12) < 0 and "pitch_y 13" in err() and "even" in err()
    assert call(fmt=K["P010"], py=12, pc=15) < 0 and "pitch_c 15" in err() and "even" in err()
    # a null pointer: an array, c1 where it is required, c1 where it must not be, an element
    assert call(y=None) < 0 and "required" in err()
    assert call(a=None) < 0 and "required" in err()
    assert call(out=None) < 0 and "required" in err()
    assert call(fmt=K["I420"], pc=3) < 0 and "c1 (the V planes) is required for I420" in err()
    assert call(b=c1) < 0 and "c1 must be NULL" in err()
    holed = ptrs([0x1000, 0x2000, None])
    assert call(n=3, y=holed) < 0 and "frame 2 has a null pointer" in err()
    assert call(n=3, out=holed) < 0 and "frame 2 has a null pointer" in err()
    assert call(n=3, a=holed) < 0 and "frame 2 has a null pointer" in err()
    assert call(fmt=K["I420"], pc=3, n=3, b=holed) < 0 and "frame 2 has a null pointer" in err()
    assert call(fmt=K["P010"], py=12, pc=12, y=ptrs([0x1001])) < 0 and "frame 0: a P010 plane is 2-byte aligned" in err()
