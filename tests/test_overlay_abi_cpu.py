"""CPU: include/countr_hip_overlay.h is the one statement of the overlay library's C ABI, as the five older headers are of theirs.
countr_amd/_lib.py reads the binding from it and libcountr_hip_overlay.so exports exactly it; pinned here by literals (the checks
against the C compiler and the library's dynamic symbols are in tests/test_libraries_cpu.py, once per tag).  Every refusal runs on the
host: a refused call launches nothing."""
import ctypes as C

from countr_amd import _lib, build

NAMES = ("ABI_VERSION", "MAX_FRAMES", "MAX_SIDE", "MAX_POINTS", "MAX_POLYGONS", "MAX_VERTICES", "MAX_RADIUS", "PATCH_H", "PATCH_W", "PACK_GAINS",
         "PACK_LUT", "PACK_HEAD", "RGB", "NV12", "NV21", "I420", "BT601", "BT709", "LIMITED", "FULL")
FIELDS = ("rgb", "map", "out", "yuv", "poly_verts", "gain_max", "n_points", "points_off", "n_polys", "n_edges", "edges_off", "lh", "lw", "lx", "ly",
          "patch_off")


def test_version_limits_binding_and_errors():
    # the literal pins of the header's names (what holds of every library by rule is in test_libraries_cpu.py)
    assert list(_lib.OVERLAY_STRUCTS) == ["countr_overlay_frame"]
    assert [f[0] for f in _lib.OverlayFrame._fields_] == list(FIELDS)
    assert list(_lib.OVERLAY_CONSTS) == ["COUNTR_OVERLAY_" + n for n in NAMES]
    assert _lib.overlay_exported_symbols() == ["countr_overlay_last_error", "countr_overlay_render", "countr_overlay_version"]
    # the one table of the side libraries, in the order they were added, up to this one
    assert list(build.SINGLE)[:5] == ["ext", "classes", "tiles", "yuv", "overlay"]
    snapshot = lambda: (dict(_lib.CONSTS), dict(_lib.STRUCTS), dict(_lib.PROTOS), _lib.exported_symbols(),
                        dict(_lib.EXT_CONSTS), dict(_lib.EXT_STRUCTS), dict(_lib.EXT_PROTOS), _lib.ext_exported_symbols(),
                        dict(_lib.CLASSES_CONSTS), dict(_lib.CLASSES_STRUCTS), dict(_lib.CLASSES_PROTOS), _lib.classes_exported_symbols(),
                        dict(_lib.TILES_CONSTS), dict(_lib.TILES_STRUCTS), dict(_lib.TILES_PROTOS), _lib.tiles_exported_symbols(),
                        dict(_lib.YUV_CONSTS), dict(_lib.YUV_STRUCTS), dict(_lib.YUV_PROTOS), _lib.yuv_exported_symbols())
    before = snapshot()
    L = _lib.overlay_lib()
    assert L.countr_overlay_version() == _lib.OVERLAY_CONSTS["COUNTR_OVERLAY_ABI_VERSION"] == 1
    K = {k[len("COUNTR_OVERLAY_"):]: v for k, v in _lib.OVERLAY_CONSTS.items()}
    assert K == {"ABI_VERSION": 1, "MAX_FRAMES": 16, "MAX_SIDE": 16384, "MAX_POINTS": 4096, "MAX_POLYGONS": 64, "MAX_VERTICES": 64, "MAX_RADIUS": 16,
                 "PATCH_H": 64, "PATCH_W": 256, "PACK_GAINS": 0, "PACK_LUT": 64, "PACK_HEAD": 1088, "RGB": 0, "NV12": 1, "NV21": 2, "I420": 3,
                 "BT601": 0, "BT709": 1, "LIMITED": 0, "FULL": 1}
    vp, ci = C.c_void_p, C.c_int
    assert L.countr_overlay_last_error.restype is C.c_char_p and L.countr_overlay_last_error.argtypes == []
    assert L.countr_overlay_render.restype is ci
    assert L.countr_overlay_render.argtypes == [C.POINTER(_lib.OverlayFrame)] + [ci] * 5 + [vp] + [ci] * 7 + [vp, vp]
    # loading the overlay library leaves the five older bindings as their pinned tests read them
    assert snapshot() == before
    assert len(_lib.PROTOS) == 87 and len(_lib.EXT_PROTOS) == 4 and len(_lib.CLASSES_PROTOS) == 4 and len(_lib.TILES_PROTOS) == 5 and len(_lib.YUV_PROTOS) == 3
    older = set(_lib.PROTOS) | set(_lib.EXT_PROTOS) | set(_lib.CLASSES_PROTOS) | set(_lib.TILES_PROTOS) | set(_lib.YUV_PROTOS)
    assert not set(_lib.OVERLAY_PROTOS) & older
    assert not any(k.startswith(("OVERLAY_ABI", "OVERLAY_MAX", "OVERLAY_PATCH", "OVERLAY_PACK", "OVERLAY_NV", "OVERLAY_BT")) for k in vars(_lib))
    try:
        _lib.overlay_check(-1, "probe")
    except _lib.CountrError as e:
        assert "probe failed" in str(e)
    else:
        raise AssertionError("overlay_check(-1) did not raise")


def test_refusals_run_on_the_host():
    """Every refusal returns before anything is read on the device or a kernel is launched: the device pointers are aligned numbers, not
    buffers."""
    L = _lib.overlay_lib()
    K = {k[len("COUNTR_OVERLAY_"):]: v for k, v in _lib.OVERLAY_CONSTS.items()}
    err = lambda: L.countr_overlay_last_error().decode()
    PACK, BYTES = 0x7000000, 1 << 20

    def records(n=17, **fields):
        recs = (_lib.OverlayFrame * n)()
        for j in range(n):
            recs[j].rgb, recs[j].map, recs[j].out = 0x100000 * (j + 1), 0x100000 * (j + 1) + 0x40000, 0x100000 * (j + 1) + 0x80000
            for k, v in fields.items():
                setattr(recs[j], k, v)
        return recs

    def call(recs=None, n=1, H=4, W=6, mh=2, mw=3, pack=PACK, nbytes=BYTES, radius=2, fmt=K["RGB"], matrix=K["BT709"], rng=K["LIMITED"],
             maxbits=None):
        return L.countr_overlay_render(records() if recs is None else recs, n, H, W, mh, mw, pack, nbytes, radius, 0x00ff00, 0xffff00, fmt, matrix,
                                       rng, maxbits, None)

    # n out of range
    assert call(n=0) < 0 and "1..16 frames a call, got 0" in err()
    assert call(n=17) < 0 and "got 17" in err()
    assert call(n=-1) < 0 and "got -1" in err()
    # an unknown enum
    assert call(fmt=4) < 0 and "unknown format 4" in err()
    assert call(fmt=-1) < 0 and "unknown format -1" in err()
    assert call(matrix=2) < 0 and "unknown matrix 2" in err()
    assert call(rng=7) < 0 and "unknown range 7" in err()
    # H, W, mh or mw outside 1..16384
    assert call(H=0) < 0 and "H and W are 1..16384, got 0 x 6" in err()
    assert call(W=16385) < 0 and "got 4 x 16385" in err()
    assert call(mh=0) < 0 and "mh and mw are 1..16384, got 0 x 3" in err()
    assert call(mw=16385) < 0 and "got 2 x 16385" in err()
    assert call(radius=17) < 0 and "point_radius is 0..16, got 17" in err()
    assert call(radius=-1) < 0 and "got -1" in err()
    # the marks' limits
    assert call(records(n_points=4097, points_off=1088)) < 0 and "0..4096 points, got 4097" in err()
    verts = (C.c_int * 65)(*([3] * 65))
    assert call(records(n_polys=65, poly_verts=C.addressof(verts), n_edges=195, edges_off=1088)) < 0 and "0..64 polygons, got 65" in err()
    verts[1] = 65
    assert call(records(n_polys=2, poly_verts=C.addressof(verts), n_edges=68, edges_off=1088)) < 0 and "polygon 1: 1..64 vertices, got 65" in err()
    verts[1] = 0
    assert call(records(n_polys=2, poly_verts=C.addressof(verts), n_edges=3, edges_off=1088)) < 0 and "got 0" in err()
    verts[1] = 4
    assert call(records(n_polys=2, poly_verts=C.addressof(verts), n_edges=8, edges_off=1088)) < 0 and "n_edges 8, its polygons have 7 vertices" in err()
    assert call(records(n_polys=2, n_edges=7, edges_off=1088)) < 0 and "polygons and no poly_verts" in err()
    assert call(records(lh=65, lw=4, patch_off=1088)) < 0 and "at most 64 x 256" in err() and "got 65 x 4" in err()
    assert call(records(lh=4, lw=257, patch_off=1088)) < 0 and "got 4 x 257" in err()
    assert call(records(lh=0, lw=4)) < 0 and "got 0 x 4" in err()
    # offsets outside the packed upload, or in front of its fixed part
    assert call(records(n_points=2, points_off=BYTES - 8)) < 0 and "outside the packed upload" in err()
    assert call(records(n_points=2, points_off=64)) < 0 and "outside the packed upload" in err()
    assert call(records(n_points=2, points_off=1090)) < 0 and "4-byte aligned" in err()
    assert call(records(lh=4, lw=4, patch_off=BYTES - 15)) < 0 and "outside the packed upload" in err()
    assert call(nbytes=1087) < 0 and "at least 1088 bytes" in err()
    # a null pointer: an array, an element, the 4:2:0 buffer where it is required and where it must not be, the maxima's workspace
    assert L.countr_overlay_render(None, 1, 4, 6, 2, 3, PACK, BYTES, 2, 0, 0, 0, 1, 0, None, None) < 0 and "frames array is required" in err()
    assert call(pack=None) < 0 and "packed upload is required" in err()
    assert call(pack=PACK + 4) < 0 and "16-byte aligned" in err()
    for field in ("rgb", "map", "out"):
        recs = records()
        setattr(recs[2], field, None)
        assert call(recs, n=3) < 0 and "frame 2 has a null pointer" in err(), field
    assert call(fmt=K["NV12"]) < 0 and "frame 0 has a null pointer" in err()
    assert call(records(yuv=0x9000000)) < 0 and "yuv must be NULL when the format is RGB" in err()
    assert call(records(gain_max=1)) < 0 and "maxbits" in err()
    recs = records()
    recs[0].map = 0x140002
    assert call(recs) < 0 and "the map is 4-byte aligned" in err()
