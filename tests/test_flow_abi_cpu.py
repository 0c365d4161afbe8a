"""CPU: include/countr_hip_flow.h is the one statement of the flow library's C ABI, as the seven older headers are of theirs.
countr_amd/_lib.py reads the binding from it and libcountr_hip_flow.so exports exactly it; pinned here by literals (the checks against
the C compiler and the library's dynamic symbols are in tests/test_libraries_cpu.py, once per tag).  Every refusal runs on the host: a
refused call launches nothing."""
import ctypes as C

from countr_amd import _lib, build

NAMES = ("ABI_VERSION", "MAX_FRAMES", "MAX_LINES", "MAX_SEARCH", "MAX_INTERVAL", "CELL", "MAX_SIDE", "OUT_FLOATS")
FIELDS = ("map", "motion", "out", "sx", "tx", "sy", "ty")
EXPORTS = ["countr_flow_flux", "countr_flow_last_error", "countr_flow_luma", "countr_flow_motion", "countr_flow_version", "countr_flow_workspace"]


def test_version_limits_binding_and_errors():
    # the literal pins of the header's names (what holds of every library by rule is in test_libraries_cpu.py)
    assert list(_lib.FLOW_STRUCTS) == ["countr_flow_map"]
    assert [f[0] for f in _lib.FlowMap._fields_] == list(FIELDS) and C.sizeof(_lib.FlowMap) == 56
    assert list(_lib.FLOW_CONSTS) == ["COUNTR_FLOW_" + n for n in NAMES]
    assert _lib.flow_exported_symbols() == EXPORTS
    # the one table of the side libraries, in the order they were added, up to this one
    assert list(build.SINGLE)[:7] == ["ext", "classes", "tiles", "yuv", "overlay", "tracks", "flow"]
    snapshot = lambda: (dict(_lib.CONSTS), dict(_lib.STRUCTS), dict(_lib.PROTOS), _lib.exported_symbols(),
                        dict(_lib.EXT_CONSTS), dict(_lib.EXT_STRUCTS), dict(_lib.EXT_PROTOS), _lib.ext_exported_symbols(),
                        dict(_lib.CLASSES_CONSTS), dict(_lib.CLASSES_STRUCTS), dict(_lib.CLASSES_PROTOS), _lib.classes_exported_symbols(),
                        dict(_lib.TILES_CONSTS), dict(_lib.TILES_STRUCTS), dict(_lib.TILES_PROTOS), _lib.tiles_exported_symbols(),
                        dict(_lib.YUV_CONSTS), dict(_lib.YUV_STRUCTS), dict(_lib.YUV_PROTOS), _lib.yuv_exported_symbols(),
                        dict(_lib.OVERLAY_CONSTS), dict(_lib.OVERLAY_STRUCTS), dict(_lib.OVERLAY_PROTOS), _lib.overlay_exported_symbols(),
                        dict(_lib.TRACKS_CONSTS), dict(_lib.TRACKS_STRUCTS), dict(_lib.TRACKS_PROTOS), _lib.tracks_exported_symbols())
    before = snapshot()
    L = _lib.flow_lib()
    assert L.countr_flow_version() == _lib.FLOW_CONSTS["COUNTR_FLOW_ABI_VERSION"] == 1
    K = {k[len("COUNTR_FLOW_"):]: v for k, v in _lib.FLOW_CONSTS.items()}
    assert K == {"ABI_VERSION": 1, "MAX_FRAMES": 16, "MAX_LINES": 16, "MAX_SEARCH": 16, "MAX_INTERVAL": 8, "CELL": 8, "MAX_SIDE": 4096,
                 "OUT_FLOATS": 33}
    vp, ci, cd = C.c_void_p, C.c_int, C.c_double
    assert L.countr_flow_last_error.restype is C.c_char_p and L.countr_flow_last_error.argtypes == []
    assert L.countr_flow_workspace.restype is ci and L.countr_flow_workspace.argtypes == [ci, ci]
    assert L.countr_flow_luma.restype is ci and L.countr_flow_luma.argtypes == [vp, vp, ci, ci, ci, vp]
    assert L.countr_flow_motion.restype is ci and L.countr_flow_motion.argtypes == [vp, vp, vp, ci, ci, ci, ci, ci, vp]
    assert L.countr_flow_flux.restype is ci and L.countr_flow_flux.argtypes == [C.POINTER(_lib.FlowMap), ci, ci, ci, vp, ci, cd, ci, vp, vp]
    # loading the flow library leaves the seven older bindings as their pinned tests read them
    assert snapshot() == before
    assert (len(_lib.PROTOS) == 87 and len(_lib.EXT_PROTOS) == 4 and len(_lib.CLASSES_PROTOS) == 4 and len(_lib.TILES_PROTOS) == 5
            and len(_lib.YUV_PROTOS) == 3 and len(_lib.OVERLAY_PROTOS) == 3 and len(_lib.TRACKS_PROTOS) == 6)
    older = (set(_lib.PROTOS) | set(_lib.EXT_PROTOS) | set(_lib.CLASSES_PROTOS) | set(_lib.TILES_PROTOS) | set(_lib.YUV_PROTOS)
             | set(_lib.OVERLAY_PROTOS) | set(_lib.TRACKS_PROTOS))
    assert not set(_lib.FLOW_PROTOS) & older
    assert not any(k.startswith(("FLOW_ABI", "FLOW_MAX", "FLOW_CELL", "FLOW_OUT")) for k in vars(_lib))
    try:
        _lib.flow_check(-1, "probe")
    except _lib.CountrError as e:
        assert "probe failed" in str(e)
    else:
        raise AssertionError("flow_check(-1) did not raise")
    # the scratch of a flux call: 33 floats per cell row of every map
    assert L.countr_flow_workspace(1, 8) == 33 * 4 and L.countr_flow_workspace(16, 384) == 16 * 48 * 33 * 4
    assert L.countr_flow_workspace(3, 96) == 3 * 12 * 33 * 4


def test_refusals_run_on_the_host():
    """Every refusal returns before anything is read on the device or a kernel is launched: the device pointers are aligned numbers, not
    buffers."""
    L = _lib.flow_lib()
    err = lambda: L.countr_flow_last_error().decode()
    WS = 0x7000000
    ptrs = lambda base=0x1000000, n=17: (C.c_void_p * n)(*[base * (j + 1) for j in range(n)])
    A, B, M = ptrs(0x1000000), ptrs(0x1100000), ptrs(0x1200000)

    # ---- luma
    assert L.countr_flow_luma(A, B, 0, 384, 64, None) < 0 and "1..16 frames a call, got 0" in err()
    assert L.countr_flow_luma(A, B, 17, 384, 64, None) < 0 and "got 17" in err()
    for h, w in ((0, 64), (384, 60), (380, 64), (4104, 64), (384, 4104), (384, -8)):
        assert L.countr_flow_luma(A, B, 1, h, w, None) < 0 and "multiples of 8 in 8..4096, got %d x %d" % (h, w) in err()
    assert L.countr_flow_luma(None, B, 1, 384, 64, None) < 0 and "arrays are required" in err()
    assert L.countr_flow_luma(A, None, 1, 384, 64, None) < 0 and "arrays are required" in err()
    bad = ptrs(0x1000000)
    bad[1] = None
    assert L.countr_flow_luma(bad, B, 2, 384, 64, None) < 0 and "frame 1 has a null pointer" in err()
    assert L.countr_flow_luma(A, bad, 2, 384, 64, None) < 0 and "frame 1 has a null pointer" in err()
    bad[1] = 0x2000008
    assert L.countr_flow_luma(bad, B, 2, 384, 64, None) < 0 and "frame 1: the image is 16-byte aligned" in err()
    bad[1] = 0x2000002
    assert L.countr_flow_luma(A, bad, 2, 384, 64, None) < 0 and "the luma 4-byte aligned" in err()

    # ---- motion
    assert L.countr_flow_motion(A, B, M, 0, 384, 64, 4, 256, None) < 0 and "1..16 frames a call, got 0" in err()
    assert L.countr_flow_motion(A, B, M, 17, 384, 64, 4, 256, None) < 0 and "got 17" in err()
    assert L.countr_flow_motion(A, B, M, 1, 384, 12, 4, 256, None) < 0 and "got 384 x 12" in err()
    assert L.countr_flow_motion(A, B, M, 1, 384, 64, 0, 256, None) < 0 and "search is 1..16, got 0" in err()
    assert L.countr_flow_motion(A, B, M, 1, 384, 64, 17, 256, None) < 0 and "got 17" in err()
    assert L.countr_flow_motion(A, B, M, 1, 384, 64, 4, -1, None) < 0 and "min_gain is >= 0, got -1" in err()
    for k in range(3):
        args = [A, B, M]
        args[k] = None
        assert L.countr_flow_motion(*args, 1, 384, 64, 4, 256, None) < 0 and "arrays are required" in err()
        args = [A, B, M]
        args[k] = ptrs(0x1000000)
        args[k][2] = None
        assert L.countr_flow_motion(*args, 3, 384, 64, 4, 256, None) < 0 and "pair 2 has a null pointer" in err()
    bad = ptrs(0x1200000)
    bad[0] = 0x1200002
    assert L.countr_flow_motion(A, B, bad, 1, 384, 64, 4, 256, None) < 0 and "pair 0: the motion field is 4-byte aligned" in err()

    # ---- flux
    lines = (C.c_double * 68)(*([10.0, 0.0, 10.0, 100.0] * 17))

    def records(n=17, **fields):
        recs = (_lib.FlowMap * n)()
        for j in range(n):
            base = 0x1000000 * (j + 1)
            recs[j].map, recs[j].motion, recs[j].out = base, base + 0x100000, base + 0x200000
            recs[j].sx, recs[j].tx, recs[j].sy, recs[j].ty = 2.8125, 0.90625, 2.8125, 0.90625
            for k, v in fields.items():
                setattr(recs[j], k, v)
        return recs

    def call(recs=None, n=1, h=384, w=64, ln=lines, nl=2, band=8.0, interval=1, ws=WS):
        return L.countr_flow_flux(records() if recs is None else recs, n, h, w, ln, nl, band, interval, ws, None)

    def one(field, value, j=1, n=3):
        recs = records()
        setattr(recs[j], field, value)
        return call(recs, n=n)

    assert call(n=0) < 0 and "1..16 frames a call, got 0" in err()
    assert call(n=17) < 0 and "got 17" in err()
    assert call(h=388) < 0 and "got 388 x 64" in err()
    assert call(nl=17) < 0 and "0..16 lines, got 17" in err()
    assert call(nl=-1) < 0 and "got -1" in err()
    assert call(interval=0) < 0 and "interval is 1..8, got 0" in err()
    assert call(interval=9) < 0 and "got 9" in err()
    for bad_band in (0.0, -1.0, float("inf"), float("nan")):
        assert call(band=bad_band) < 0 and "band is finite and > 0" in err(), bad_band
    assert L.countr_flow_flux(None, 1, 384, 64, lines, 2, 8.0, 1, WS, None) < 0 and "maps array is required" in err()
    assert call(ln=None) < 0 and "lines array is required" in err()
    assert call(ws=None) < 0 and "workspace is required and 4-byte aligned" in err()
    assert call(ws=WS + 2) < 0 and "workspace is required and 4-byte aligned" in err()
    for field in ("map", "motion", "out"):
        assert one(field, None, j=2) < 0 and "map 2 has a null pointer" in err(), field
        assert one(field, 0x2000002) < 0 and "map 1: map, motion and out are 4-byte aligned" in err(), field
    for field, value in (("sx", 0.0), ("sy", -1.0), ("sx", float("nan")), ("tx", float("inf")), ("ty", float("nan")), ("sy", float("inf"))):
        assert one(field, value) < 0 and "map 1: a placement is finite with sx > 0 and sy > 0" in err(), (field, value)
    for k, value in ((0, float("nan")), (5, float("inf")), (7, float("-inf"))):
        ln = (C.c_double * 8)(10.0, 0.0, 10.0, 100.0, 20.0, 0.0, 20.0, 100.0)
        ln[k] = value
        assert call(ln=ln) < 0 and "line %d: a coordinate is not finite" % (k // 4) in err()
    ln = (C.c_double * 4)(-1e200, 0.0, 1e200, 0.0)
    assert call(ln=ln, nl=1) < 0 and "line 0: its squared length and band are finite" in err()
    # the workspace query
    assert L.countr_flow_workspace(0, 384) < 0 and "got 0 of 384" in err()
    assert L.countr_flow_workspace(17, 384) < 0 and L.countr_flow_workspace(1, 4) < 0 and L.countr_flow_workspace(1, 4104) < 0
    assert "got 1 of 4104" in err()
