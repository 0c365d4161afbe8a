"""CPU: include/countr_hip_cam.h is the one statement of the camera library's C ABI, as the eight older headers are of theirs.
countr_amd/_lib.py reads the binding from it and libcountr_hip_cam.so exports exactly it; pinned here by literals (the checks against
the C compiler and the library's dynamic symbols are in tests/test_libraries_cpu.py, once per tag).  Every refusal runs on the host: a
refused call launches nothing.  The library is the last entry of the one list of side libraries (build.TAGS)."""
import ctypes as C
import glob
import io
import os
import re
from contextlib import redirect_stdout

from countr_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ABI_VERSION", "MAX_FRAMES", "CELL", "MAX_SIDE", "RANGE", "BINS", "RECORD_INTS")
EXPORTS = ["countr_cam_compensate", "countr_cam_estimate", "countr_cam_last_error", "countr_cam_version", "countr_cam_workspace"]
OLDER = ["ext", "classes", "tiles", "yuv", "overlay", "tracks", "flow"]


def test_later_is_stated_once_and_by_the_rule_of_the_first_list():
    paths = glob.glob(os.path.join(ROOT, "countr_amd", "csrc_cam", "*.hip"))
    # one list, whole and in the order the libraries were added; the camera library is its last entry, in the same three-part form
    assert list(build.TAGS) == list(build.SINGLE) == list(_lib.LIBRARIES) == OLDER + ["cam"]
    assert paths and build.SINGLE["cam"][1]() == sorted(paths)
    assert build.SINGLE["cam"][0] == os.path.join(ROOT, "countr_amd", "libcountr_hip_cam.so") == os.path.normpath(_lib.CAM_LIB_PATH)
    assert os.path.samefile(build.SINGLE["cam"][2], _lib.CAM_HEADER)
    assert isinstance(_lib.LIBRARIES["cam"], _lib.Library) and _lib.LIBRARIES["cam"].tag == "cam"
    assert len(re.findall(r"^TAGS\s*=", open(os.path.join(ROOT, "countr_amd", "build.py")).read(), re.M)) == 1
    # the library is a build product: git ignores it like its siblings
    ignored = open(os.path.join(ROOT, ".gitignore")).read().split()
    assert "*.so" in ignored and "*.sha256" in ignored and "build/" in ignored


def test_build_load_checks_the_later_libraries():
    import __graft_entry__ as entry
    out = io.StringIO()
    with redirect_stdout(out):
        entry.check_side_libraries()
    lines = out.getvalue().splitlines()
    assert len(lines) == 8 and all(line.startswith("build ok: ") for line in lines)
    assert "libcountr_hip_cam.so (5 exported symbols)" in lines[-1] and not any("libcountr_hip_cam.so" in line for line in lines[:-1])
    text = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    body = text[text.index("def build():"):text.index("def smoke():")]
    assert body.count("check_side_libraries()") == 1


def test_version_limits_binding_and_errors():
    # the literal pins of the header's names (what holds of every library by rule is in test_libraries_cpu.py)
    assert list(_lib.CAM_STRUCTS) == []
    assert list(_lib.CAM_CONSTS) == ["COUNTR_CAM_" + n for n in NAMES]
    assert _lib.cam_exported_symbols() == EXPORTS
    tags = ["", "EXT_", "CLASSES_", "TILES_", "YUV_", "OVERLAY_", "TRACKS_", "FLOW_"]
    snapshot = lambda: [(dict(getattr(_lib, t + "CONSTS")), dict(getattr(_lib, t + "STRUCTS")), dict(getattr(_lib, t + "PROTOS")),
                         getattr(_lib, (t.lower() if t else "") + "exported_symbols")()) for t in tags]
    before = snapshot()
    L = _lib.cam_lib()
    assert L.countr_cam_version() == _lib.CAM_CONSTS["COUNTR_CAM_ABI_VERSION"] == 1
    K = {k[len("COUNTR_CAM_"):]: v for k, v in _lib.CAM_CONSTS.items()}
    assert K == {"ABI_VERSION": 1, "MAX_FRAMES": 16, "CELL": 8, "MAX_SIDE": 4096, "RANGE": 264, "BINS": 529, "RECORD_INTS": 8}
    F = _lib.FLOW_CONSTS
    assert K["RANGE"] == 16 * F["COUNTR_FLOW_MAX_SEARCH"] + 8 and K["BINS"] == 2 * K["RANGE"] + 1
    assert (K["MAX_FRAMES"], K["CELL"], K["MAX_SIDE"]) == (F["COUNTR_FLOW_MAX_FRAMES"], F["COUNTR_FLOW_CELL"], F["COUNTR_FLOW_MAX_SIDE"])
    vp, ci = C.c_void_p, C.c_int
    assert L.countr_cam_version.restype is ci and L.countr_cam_version.argtypes == []
    assert L.countr_cam_last_error.restype is C.c_char_p and L.countr_cam_last_error.argtypes == []
    assert L.countr_cam_workspace.restype is ci and L.countr_cam_workspace.argtypes == [ci, ci, ci]
    assert L.countr_cam_estimate.restype is ci and L.countr_cam_estimate.argtypes == [vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, vp, vp]
    assert L.countr_cam_compensate.restype is ci and L.countr_cam_compensate.argtypes == [vp, vp, vp, vp, ci, ci, ci, vp]
    # loading the camera library leaves the eight older bindings as their pinned tests read them
    assert snapshot() == before
    assert (len(_lib.PROTOS) == 87 and len(_lib.EXT_PROTOS) == 4 and len(_lib.CLASSES_PROTOS) == 4 and len(_lib.TILES_PROTOS) == 5
            and len(_lib.YUV_PROTOS) == 3 and len(_lib.OVERLAY_PROTOS) == 3 and len(_lib.TRACKS_PROTOS) == 6 and len(_lib.FLOW_PROTOS) == 6)
    older = set(_lib.PROTOS).union(*(getattr(_lib, t.upper() + "_PROTOS") for t in OLDER))
    assert not set(_lib.CAM_PROTOS) & older
    assert not any(k.startswith(("CAM_ABI", "CAM_MAX", "CAM_CELL", "CAM_RANGE", "CAM_BINS", "CAM_RECORD")) for k in vars(_lib))
    try:
        _lib.cam_check(-1, "probe")
    except _lib.CountrError as e:
        assert "probe failed" in str(e)
    else:
        raise AssertionError("cam_check(-1) did not raise")
    # the scratch of an estimate call: two histograms of 529 int32 per field, whatever its size
    assert L.countr_cam_workspace(1, 8, 8) == 2 * 529 * 4 and L.countr_cam_workspace(16, 384, 672) == 16 * 2 * 529 * 4
    assert L.countr_cam_workspace(3, 96, 192) == 3 * 2 * 529 * 4


def test_refusals_run_on_the_host():
    """Every refusal returns before anything is read on the device or a kernel is launched: the device pointers are aligned numbers, not
    buffers."""
    L = _lib.cam_lib()
    err = lambda: L.countr_cam_last_error().decode()
    ptrs = lambda base=0x1000000, n=17: (C.c_void_p * n)(*[base * (j + 1) for j in range(n)])
    F, P, O = ptrs(0x1000000), ptrs(0x1100000), ptrs(0x1200000)
    REC, FL, WS = 0x5000000, 0x6000000, 0x7000000

    def est(f=F, p=P, rec=REC, fl=FL, n=1, h=384, w=64, tex=128, tol=8, voters=16, ws=WS):
        return L.countr_cam_estimate(f, p, rec, fl, n, h, w, tex, tol, voters, ws, None)

    def comp(f=F, rec=REC, fl=FL, o=O, n=1, h=384, w=64):
        return L.countr_cam_compensate(f, rec, fl, o, n, h, w, None)

    for call, who in ((est, "countr_cam_estimate"), (comp, "countr_cam_compensate")):
        assert call(n=0) < 0 and who + ": 1..16 frames a call, got 0" in err()
        assert call(n=17) < 0 and "got 17" in err()
        for h, w in ((0, 64), (384, 60), (380, 64), (4104, 64), (384, 4104), (384, -8)):
            assert call(h=h, w=w) < 0 and "multiples of 8 in 8..4096, got %d x %d" % (h, w) in err()
        assert call(rec=None) < 0 and "records are required and 4-byte aligned" in err()
        assert call(rec=REC + 2) < 0 and "records are required and 4-byte aligned" in err()
        assert call(fl=None) < 0 and "flags are required" in err()
    # ---- estimate
    assert est(tex=-1) < 0 and "min_texture is >= 0, got -1" in err()
    assert est(tol=-1) < 0 and "tol is >= 0, got -1" in err()
    assert est(voters=0) < 0 and "min_voters is >= 1, got 0" in err()
    assert est(f=None) < 0 and "fields and lumas arrays are required" in err()
    assert est(p=None) < 0 and "fields and lumas arrays are required" in err()
    assert est(ws=None) < 0 and "workspace is required and 4-byte aligned" in err()
    assert est(ws=WS + 1) < 0 and "workspace is required and 4-byte aligned" in err()
    for k in range(2):
        args = [F, P]
        args[k] = ptrs(0x1000000)
        args[k][2] = None
        assert est(f=args[0], p=args[1], n=3) < 0 and "pair 2 has a null pointer" in err()
    bad = ptrs(0x1000000)
    bad[1] = 0x2000002
    assert est(f=bad, n=2) < 0 and "pair 1: the motion field is 4-byte aligned" in err()
    # ---- compensate
    assert comp(f=None) < 0 and "fields and out_fields arrays are required" in err()
    assert comp(o=None) < 0 and "fields and out_fields arrays are required" in err()
    for k in range(2):
        args = [F, O]
        args[k] = ptrs(0x1000000)
        args[k][1] = None
        assert comp(f=args[0], o=args[1], n=2) < 0 and "field 1 has a null pointer" in err()
        args[k][1] = 0x2000002
        assert comp(f=args[0], o=args[1], n=2) < 0 and "field 1: the field and its output are 4-byte aligned" in err()
    # ---- the workspace query
    assert L.countr_cam_workspace(0, 384, 64) < 0 and "countr_cam_workspace: 1..16 frames a call, got 0" in err()
    assert L.countr_cam_workspace(17, 384, 64) < 0 and L.countr_cam_workspace(1, 4, 64) < 0 and L.countr_cam_workspace(1, 384, 4104) < 0
    assert "got 384 x 4104" in err()
