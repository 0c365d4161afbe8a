"""CPU: include/countr_hip_tracks.h is the one statement of the tracks library's C ABI, as the six older headers are of theirs.
countr_amd/_lib.py reads the binding from it and libcountr_hip_tracks.so exports exactly it; pinned here by literals (the checks against
the C compiler and the library's dynamic symbols are in tests/test_libraries_cpu.py, once per tag).  Every refusal runs on the host: a
refused call launches nothing."""
import ctypes as C

from countr_amd import _lib, build

NAMES = ("ABI_VERSION", "MAX_STREAMS", "MAX_TRACKS", "MAX_POINTS", "MAX_LINES", "HEAD_INTS", "FIELDS", "SUMMARY_INTS")
FIELDS = ("state", "points", "ids", "events", "summary", "lines", "N", "L", "max_dist", "beta", "max_missed", "min_hits")
EXPORTS = ["countr_tracks_last_error", "countr_tracks_reset", "countr_tracks_state_bytes", "countr_tracks_step", "countr_tracks_version",
           "countr_tracks_workspace"]


def test_version_limits_binding_and_errors():
    # the literal pins of the header's names (what holds of every library by rule is in test_libraries_cpu.py)
    assert list(_lib.TRACKS_STRUCTS) == ["countr_tracks_stream"]
    assert [f[0] for f in _lib.TracksStream._fields_] == list(FIELDS) and C.sizeof(_lib.TracksStream) == 72
    assert list(_lib.TRACKS_CONSTS) == ["COUNTR_TRACKS_" + n for n in NAMES]
    assert _lib.tracks_exported_symbols() == EXPORTS
    # the one table of the side libraries, in the order they were added, up to this one
    assert list(build.SINGLE)[:6] == ["ext", "classes", "tiles", "yuv", "overlay", "tracks"]
    snapshot = lambda: (dict(_lib.CONSTS), dict(_lib.STRUCTS), dict(_lib.PROTOS), _lib.exported_symbols(),
                        dict(_lib.EXT_CONSTS), dict(_lib.EXT_STRUCTS), dict(_lib.EXT_PROTOS), _lib.ext_exported_symbols(),
                        dict(_lib.CLASSES_CONSTS), dict(_lib.CLASSES_STRUCTS), dict(_lib.CLASSES_PROTOS), _lib.classes_exported_symbols(),
                        dict(_lib.TILES_CONSTS), dict(_lib.TILES_STRUCTS), dict(_lib.TILES_PROTOS), _lib.tiles_exported_symbols(),
                        dict(_lib.YUV_CONSTS), dict(_lib.YUV_STRUCTS), dict(_lib.YUV_PROTOS), _lib.yuv_exported_symbols(),
                        dict(_lib.OVERLAY_CONSTS), dict(_lib.OVERLAY_STRUCTS), dict(_lib.OVERLAY_PROTOS), _lib.overlay_exported_symbols())
    before = snapshot()
    L = _lib.tracks_lib()
    assert L.countr_tracks_version() == _lib.TRACKS_CONSTS["COUNTR_TRACKS_ABI_VERSION"] == 1
    K = {k[len("COUNTR_TRACKS_"):]: v for k, v in _lib.TRACKS_CONSTS.items()}
    assert K == {"ABI_VERSION": 1, "MAX_STREAMS": 16, "MAX_TRACKS": 4096, "MAX_POINTS": 4096, "MAX_LINES": 16, "HEAD_INTS": 64, "FIELDS": 9,
                 "SUMMARY_INTS": 40}
    assert L.countr_tracks_state_bytes() == 4 * (64 + 9 * 4096) and L.countr_tracks_state_bytes() % 16 == 0
    vp, ci = C.c_void_p, C.c_int
    assert L.countr_tracks_last_error.restype is C.c_char_p and L.countr_tracks_last_error.argtypes == []
    assert L.countr_tracks_state_bytes.restype is ci and L.countr_tracks_state_bytes.argtypes == []
    assert L.countr_tracks_workspace.restype is ci and L.countr_tracks_workspace.argtypes == [ci, ci]
    assert L.countr_tracks_reset.restype is ci and L.countr_tracks_reset.argtypes == [vp, ci, vp]
    assert L.countr_tracks_step.restype is ci and L.countr_tracks_step.argtypes == [C.POINTER(_lib.TracksStream), ci, vp, vp]
    # loading the tracks library leaves the six older bindings as their pinned tests read them
    assert snapshot() == before
    assert (len(_lib.PROTOS) == 87 and len(_lib.EXT_PROTOS) == 4 and len(_lib.CLASSES_PROTOS) == 4 and len(_lib.TILES_PROTOS) == 5
            and len(_lib.YUV_PROTOS) == 3 and len(_lib.OVERLAY_PROTOS) == 3)
    older = (set(_lib.PROTOS) | set(_lib.EXT_PROTOS) | set(_lib.CLASSES_PROTOS) | set(_lib.TILES_PROTOS) | set(_lib.YUV_PROTOS)
             | set(_lib.OVERLAY_PROTOS))
    assert not set(_lib.TRACKS_PROTOS) & older
    assert not any(k.startswith(("TRACKS_ABI", "TRACKS_MAX", "TRACKS_HEAD_", "TRACKS_FIELDS", "TRACKS_SUMMARY")) for k in vars(_lib))
    try:
        _lib.tracks_check(-1, "probe")
    except _lib.CountrError as e:
        assert "probe failed" in str(e)
    else:
        raise AssertionError("tracks_check(-1) did not raise")
    # the scratch of a call: the predictions and the tracks' bests of every tracker, and the detections' bests
    assert L.countr_tracks_workspace(1, 0) == 4096 * 10 and L.countr_tracks_workspace(16, 4096) == 16 * 4096 * 12
    assert L.countr_tracks_workspace(3, 5) == 3 * (4096 * 10 + 16)


def test_refusals_run_on_the_host():
    """Every refusal returns before anything is read on the device or a kernel is launched: the device pointers are aligned numbers, not
    buffers."""
    L = _lib.tracks_lib()
    err = lambda: L.countr_tracks_last_error().decode()
    WS = 0x7000000

    def records(n=17, **fields):
        recs = (_lib.TracksStream * n)()
        for j in range(n):
            base = 0x1000000 * (j + 1)
            recs[j].state, recs[j].points, recs[j].ids, recs[j].events = base, base + 0x100000, base + 0x200000, base + 0x300000
            recs[j].summary, recs[j].lines = base + 0x400000, base + 0x500000
            recs[j].N, recs[j].L, recs[j].max_dist, recs[j].beta, recs[j].max_missed, recs[j].min_hits = 5, 1, 8.0, 0.5, 2, 3
            for k, v in fields.items():
                setattr(recs[j], k, v)
        return recs

    def call(recs=None, n=1, ws=WS):
        return L.countr_tracks_step(records() if recs is None else recs, n, ws, None)

    def one(field, value, j=1, n=3):
        recs = records()
        setattr(recs[j], field, value)
        return call(recs, n=n)

    # n out of range
    assert call(n=0) < 0 and "1..16 trackers a call, got 0" in err()
    assert call(n=17) < 0 and "got 17" in err()
    assert call(n=-1) < 0 and "got -1" in err()
    # the arrays
    assert L.countr_tracks_step(None, 1, WS, None) < 0 and "streams array is required" in err()
    assert call(ws=None) < 0 and "workspace is required and 16-byte aligned" in err()
    assert call(ws=WS + 8) < 0 and "workspace is required and 16-byte aligned" in err()
    # ranges
    assert one("N", -1) < 0 and "tracker 1: 0..4096 points, got -1" in err()
    assert one("N", 4097) < 0 and "got 4097" in err()
    assert one("L", 17) < 0 and "tracker 1: 0..16 lines, got 17" in err()
    assert one("L", -1) < 0 and "got -1" in err()
    assert one("max_missed", 256) < 0 and "max_missed is 0..255, got 256" in err()
    assert one("max_missed", -1) < 0 and "got -1" in err()
    assert one("min_hits", 0) < 0 and "min_hits is 1..255, got 0" in err()
    assert one("min_hits", 256) < 0 and "got 256" in err()
    # non-finite or out-of-range parameters
    for bad in (0.0, -1.0, float("inf"), float("nan"), 1e30):      # (the fp32 square of 1e30 is not finite)
        assert one("max_dist", bad, j=2) < 0 and "tracker 2: max_dist is finite and > 0" in err(), bad
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        assert one("beta", bad) < 0 and "tracker 1: beta is 0..1" in err(), bad
    # null pointers: required always, or only with N > 0 / L > 0
    for field in ("state", "summary", "points", "ids", "events", "lines"):
        assert one(field, None, j=2) < 0 and "tracker 2 has a null pointer" in err(), field
    # alignment
    assert one("state", 0x2000008) < 0 and "the state and the lines are 16-byte aligned" in err()
    assert one("lines", 0x2500004) < 0 and "the state and the lines are 16-byte aligned" in err()
    assert one("points", 0x2100004) < 0 and "the points are 8-byte aligned" in err()
    for field in ("ids", "events", "summary"):
        assert one(field, 0x2200002) < 0 and "4-byte aligned" in err(), field
    # two trackers of a call share no state
    recs = records()
    recs[2].state = recs[0].state
    assert call(recs, n=3) < 0 and "trackers 0 and 2 share a state" in err()
    # the reset and the workspace
    ptrs = (C.c_void_p * 17)(*[0x1000000 * (j + 1) for j in range(17)])
    assert L.countr_tracks_reset(ptrs, 0, None) < 0 and "1..16 trackers a call, got 0" in err()
    assert L.countr_tracks_reset(ptrs, 17, None) < 0 and "got 17" in err()
    assert L.countr_tracks_reset(None, 1, None) < 0 and "states array is required" in err()
    ptrs[1] = None
    assert L.countr_tracks_reset(ptrs, 2, None) < 0 and "tracker 1: the state is required and 16-byte aligned" in err()
    ptrs[1] = 0x2000004
    assert L.countr_tracks_reset(ptrs, 2, None) < 0 and "tracker 1" in err()
    assert L.countr_tracks_workspace(0, 5) < 0 and "got 0 of 5" in err()
    assert L.countr_tracks_workspace(17, 5) < 0 and L.countr_tracks_workspace(1, -1) < 0 and L.countr_tracks_workspace(1, 4097) < 0
    assert "got 1 of 4097" in err()
