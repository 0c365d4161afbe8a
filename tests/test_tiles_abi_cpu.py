"""CPU: include/countr_hip_tiles.h is the one statement of the tiles library's C ABI, as the three older headers are of theirs.
countr_amd/_lib.py reads the binding from it and libcountr_hip_tiles.so exports exactly it; pinned here by literals (the checks against
the C compiler and the library's dynamic symbols are in tests/test_libraries_cpu.py, once per tag).  The size query and every refusal
run on the host: a refused call launches nothing."""
import ctypes as C

from countr_amd import _lib, build


def test_version_limits_binding_and_errors():
    # the literal pins of the header's names (what holds of every library by rule is in test_libraries_cpu.py)
    assert list(_lib.TILES_STRUCTS) == []          # plain pointers and sizes only
    assert list(_lib.TILES_CONSTS)[:5] == ["COUNTR_TILES_ABI_VERSION", "COUNTR_TILES_SIZE", "COUNTR_TILES_MAX_STARTS", "COUNTR_TILES_MAX_RECTS",
                                           "COUNTR_TILES_MAX_ZOOM"]
    assert _lib.tiles_exported_symbols() == ["countr_tile_blend", "countr_tile_gather", "countr_tiles_last_error", "countr_tiles_version",
                                             "countr_tiles_workspace"]
    assert list(build.SINGLE)[:3] == ["ext", "classes", "tiles"]
    snapshot = lambda: (dict(_lib.CONSTS), dict(_lib.STRUCTS), dict(_lib.PROTOS), _lib.exported_symbols(),
                        dict(_lib.EXT_CONSTS), dict(_lib.EXT_STRUCTS), dict(_lib.EXT_PROTOS), _lib.ext_exported_symbols(),
                        dict(_lib.CLASSES_CONSTS), dict(_lib.CLASSES_STRUCTS), dict(_lib.CLASSES_PROTOS), _lib.classes_exported_symbols())
    before = snapshot()
    T = _lib.tiles_lib()
    assert T.countr_tiles_version() == _lib.TILES_CONSTS["COUNTR_TILES_ABI_VERSION"] == 1
    assert _lib.TILES_CONSTS == {"COUNTR_TILES_ABI_VERSION": 1, "COUNTR_TILES_SIZE": 384, "COUNTR_TILES_MAX_STARTS": 64,
                                 "COUNTR_TILES_MAX_RECTS": 8, "COUNTR_TILES_MAX_ZOOM": 4}
    vp, ci = C.c_void_p, C.c_int
    assert T.countr_tiles_last_error.restype is C.c_char_p and T.countr_tiles_last_error.argtypes == []
    assert T.countr_tiles_workspace.argtypes == [ci, ci]
    assert T.countr_tile_gather.argtypes == [vp, ci, ci, vp, vp, ci, vp, vp]
    assert T.countr_tile_blend.argtypes == [vp, ci, ci, vp, vp, ci, ci, vp, ci, vp, vp, vp, vp]
    # loading the tiles library leaves the three older bindings as their pinned tests read them
    assert snapshot() == before
    assert len(_lib.PROTOS) == 87 and len(_lib.STRUCTS) == 10 and len(_lib.EXT_PROTOS) == 4 and len(_lib.CLASSES_PROTOS) == 4
    assert list(_lib.EXT_STRUCTS) == ["countr_region_map", "countr_region"] and list(_lib.CLASSES_STRUCTS) == ["countr_class_set"]
    assert not set(_lib.TILES_PROTOS) & (set(_lib.PROTOS) | set(_lib.EXT_PROTOS) | set(_lib.CLASSES_PROTOS))
    assert not any(k.startswith(("REGIONS_", "EXT_ABI", "CLASSES_MAX", "CLASSES_ABI", "TILES_MAX", "TILES_ABI", "TILES_SIZE")) for k in vars(_lib))


def ints(values):
    return (C.c_int * len(values))(*values)


def test_size_query_and_refusals_run_on_the_host():
    T = _lib.tiles_lib()
    err = lambda: T.countr_tiles_last_error().decode()
    # a workgroup of the blend is 4 rows x 1024 columns and writes 9 four-byte partials
    assert T.countr_tiles_workspace(768, 640) == 1 * 192 * 9 * 4
    assert T.countr_tiles_workspace(768, 1040) == 2 * 192 * 9 * 4
    assert T.countr_tiles_workspace(1536, 2720) == 3 * 384 * 9 * 4
    assert T.countr_tiles_workspace(386, 384) == 97 * 9 * 4
    assert T.countr_tiles_workspace(383, 640) < 0 and "384 .." in err()
    assert T.countr_tiles_workspace(768, 642) < 0 and "multiple of 4" in err()
    assert T.countr_tiles_workspace(768, 64 * 384 + 4) < 0
    try:
        _lib.tiles_check(-1, "probe")
    except _lib.CountrError as e:
        assert "probe failed" in str(e) and "countr_tiles_workspace" in str(e)
    else:
        raise AssertionError("tiles_check(-1) did not raise")
    # every refusal below returns before a pointer is read or a kernel is launched: the pointers are aligned numbers, not buffers
    img, wins, outs, dm, sums, ws = (C.c_void_p(0x1000 * k) for k in range(1, 7))
    assert T.countr_tile_gather(img, 768, 400, ints([0] * 65), ints([0] * 65), 65, wins, None) < 0 and "1..64 tiles" in err()
    assert T.countr_tile_gather(img, 768, 400, ints([0]), ints([0]), 0, wins, None) < 0
    assert T.countr_tile_gather(img, 768, 400, ints([0, 385]), ints([0, 0]), 2, wins, None) < 0 and "tile 1 at (385, 0) lies outside the 768 x 400 image" in err()
    assert T.countr_tile_gather(img, 768, 400, ints([0]), ints([32]), 1, wins, None) < 0 and "outside" in err()
    assert T.countr_tile_gather(img, 768, 400, ints([-1]), ints([0]), 1, wins, None) < 0 and "outside" in err()
    assert T.countr_tile_gather(img, 768, 400, ints([0]), ints([6]), 1, wins, None) < 0 and "multiple of 4" in err()
    assert T.countr_tile_gather(C.c_void_p(0x1004), 768, 400, ints([0]), ints([0]), 1, wins, None) < 0 and "16-byte" in err()
    assert T.countr_tile_gather(None, 768, 400, ints([0]), ints([0]), 1, wins, None) < 0

    def blend(rows, cols, hk, wk, rects=(), o=outs):
        flat = [v for r in rects for v in r]
        return T.countr_tile_blend(o, len(rows), len(cols), ints(list(rows)), ints(list(cols)), hk, wk, ints(flat) if flat else None, len(rects),
                                   dm, sums, ws, None)

    assert blend(range(65), [0, 16], 448, 400) < 0 and "1..64 row starts, got 65" in err()
    assert blend([0, 384], range(0, 65 * 4, 4), 768, 640) < 0 and "1..64 column starts, got 65" in err()
    assert blend([0, 128, 256, 384], [0, 16], 768, 400, [(0, 0, 1, 1)] * 9) < 0 and "0..8 rectangles, got 9" in err()
    assert blend([0, 128, 256, 384], [0, 16], 768, 400, [(5, 5, 4, 9)]) < 0 and "rectangle 0" in err()
    assert blend([0, 128, 256], [0, 16], 768, 400) < 0 and "the last row tile ends at 640, the map at 768" in err()
    assert blend([0, 385], [0, 16], 769, 400) < 0 and "row start 1 = 385" in err()                 # a gap
    assert blend([128, 384], [0, 16], 768, 400) < 0 and "row start 0 = 128" in err()               # does not begin at 0
    assert blend([0, 0, 384], [0, 16], 768, 400) < 0 and "row start 1 = 0" in err()                # does not increase
    assert blend([0, 384], [0, 18], 768, 402) < 0                                                  # width is no multiple of 4
    assert blend([0, 384], [0, 10, 16], 768, 400) < 0 and "column start 1 = 10" in err()
    assert blend([0, 384], [0, 16], 768, 400, o=None) < 0 and "required" in err()
