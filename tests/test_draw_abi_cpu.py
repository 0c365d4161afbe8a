"""CPU: include/countr_hip_draw.h is the one statement of the draw library's C ABI, the first library of the later table
(build.LATER_TAGS, _lib.LATER_LIBRARIES): the table of eight side libraries is closed by its tests.  Pinned here by literals, together
with what tests/test_libraries_cpu.py checks once per tag of the closed table: the naming rule, the header against the C compiler, the
library's dynamic symbols against the header, the sources against the prototypes.  Every refusal runs on the host: a refused call
launches nothing."""
import ctypes as C
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from countr_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
LATER = ["draw"]
CONSTS = {"ABI_VERSION": 1, "MAX_FRAMES": 16, "MAX_SIDE": 16384, "MAX_SEGMENTS": 65600, "MAX_DISCS": 4096, "MAX_TEXTS": 4160, "MAX_HALF_WIDTH": 8,
          "MAX_RADIUS": 16, "MAX_SCALE": 8, "TEXT_BYTES": 32, "MAX_COORD": 1 << 20, "SEGMENT_WORDS": 6, "DISC_WORDS": 4, "TEXT_WORDS": 14,
          "FONT_FIRST": 32, "FONT_GLYPHS": 95, "FONT_ROWS": 7, "FONT_COLS": 5, "RGB": 0, "NV12": 1, "NV21": 2, "I420": 3, "BT601": 0, "BT709": 1,
          "LIMITED": 0, "FULL": 1}
FIELDS = ("rgb", "owner", "yuv", "n_segments", "segments_off", "n_discs", "discs_off", "n_texts", "texts_off")


def test_header_pins_and_the_later_table():
    assert {k[len("COUNTR_DRAW_"):]: v for k, v in _lib.DRAW_CONSTS.items()} == CONSTS and list(_lib.DRAW_CONSTS) == ["COUNTR_DRAW_" + n for n in CONSTS]
    assert list(_lib.DRAW_STRUCTS) == ["countr_draw_frame"] and [f[0] for f in _lib.DrawFrame._fields_] == list(FIELDS)
    assert _lib.draw_exported_symbols() == ["countr_draw_font", "countr_draw_last_error", "countr_draw_paint", "countr_draw_version"]
    # a full tracker fits one frame: 4096 tracks with a 16-step trail, a disc and a tag each, and 64 more texts
    assert CONSTS["MAX_SEGMENTS"] >= 4096 * 16 and CONSTS["MAX_DISCS"] >= 4096 and CONSTS["MAX_TEXTS"] >= 4096 + 64
    L = _lib.draw_lib()
    vp, ci = C.c_void_p, C.c_int
    assert L.countr_draw_version() == 1 and L.countr_draw_last_error.restype is C.c_char_p
    assert L.countr_draw_paint.restype is ci and L.countr_draw_paint.argtypes == [C.POINTER(_lib.DrawFrame), ci, ci, ci, vp, vp, ci, ci, ci, ci, vp]
    assert L.countr_draw_font.argtypes == [vp]
    # the later table follows the naming rule of the closed one, and is no part of it
    assert list(build.LATER_TAGS) == list(build.LATER) == list(_lib.LATER_LIBRARIES) == LATER
    assert not set(LATER) & set(build.TAGS) and not set(LATER) & set(build.SINGLE) and not set(LATER) & set(_lib.LIBRARIES)
    assert len(build.TAGS) == 8 and len(_lib.PROTOS) == 87
    for tag, side in _lib.LATER_LIBRARIES.items():
        lib, _sources, header = build.LATER[tag]
        assert side.path == lib == os.path.join(ROOT, "countr_amd", "libcountr_hip_%s.so" % tag)
        assert os.path.samefile(side.header, header) and os.path.basename(header) == "countr_hip_%s.h" % tag
        assert "countr_%s_version" % tag in side.exported_symbols() and "countr_%s_last_error" % tag in side.exported_symbols()
        T = tag.upper()
        assert getattr(_lib, T + "_LIB_PATH") == side.path and getattr(_lib, T + "_HEADER") == side.header
        assert getattr(_lib, T + "_CONSTS") is side.consts and getattr(_lib, T + "_STRUCTS") is side.structs
        assert getattr(_lib, T + "_PROTOS") is side.protos and getattr(_lib, tag + "_lib")() is side.load()
        assert getattr(_lib, tag + "_exported_symbols")() == side.exported_symbols()
        assert {k for k in vars(_lib) if k.startswith(T + "_")} == {T + s for s in ("_LIB_PATH", "_HEADER", "_CONSTS", "_STRUCTS", "_PROTOS")}
        older = set(_lib.PROTOS).union(*(set(o.protos) for o in _lib.LIBRARIES.values()))
        assert not set(side.protos) & older
        check = getattr(_lib, tag + "_check")
        assert check(0) is None
        with pytest.raises(_lib.CountrError, match=r"probe failed \(rc=-1\)"):
            check(-1, "probe")
        with pytest.raises(_lib.CountrError, match=r"countr_%s call failed \(rc=-7\)" % tag):
            check(-7)


def test_environment_overrides_the_path():
    env = dict(os.environ, COUNTR_LIB_DRAW="/elsewhere/draw.so")
    code = "from countr_amd import _lib\nprint(_lib.LATER_LIBRARIES['draw'].path, _lib.DRAW_LIB_PATH)"
    assert subprocess.check_output([sys.executable, "-c", code], cwd=ROOT, env=env, text=True).split() == ["/elsewhere/draw.so"] * 2


def test_build_load_checks_the_later_libraries_after_the_eight(capsys):
    import __graft_entry__ as G
    G.check_later_libraries()
    lines = capsys.readouterr().out.splitlines()
    assert lines == ["build ok: %s (%d exported symbols)" % (side.path, len(side.protos)) for side in _lib.LATER_LIBRARIES.values()]
    assert len(lines) == 1 and "libcountr_hip_draw.so (4 exported symbols)" in lines[0]
    G.check_side_libraries()
    assert len(capsys.readouterr().out.splitlines()) == 8


@pytest.mark.parametrize("tag", LATER)
def test_header_compiles_as_c_with_the_binding_s_constants_and_layout(tag, tmp_path):
    side = _lib.LATER_LIBRARIES[tag]
    prints, want = list(side.consts), list(side.consts.values())
    for name, cls in side.structs.items():
        prints.append("sizeof(%s)" % name)
        want.append(C.sizeof(cls))
        for field, _ctype in cls._fields_:
            prints += ["offsetof(%s, %s)" % (name, field), "sizeof(((%s*)0)->%s)" % (name, field)]
            want += [getattr(cls, field).offset, getattr(cls, field).size]
    assert "COUNTR_%s_ABI_VERSION" % tag.upper() in side.consts
    src = tmp_path / "use.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "countr_hip_%s.h"\nint main(void) {\n%s  return 0;\n}\n'
                   % (tag, "".join('  printf("%%lld\\n", (long long)(%s));\n' % p for p in prints)))
    subprocess.check_call([HIPCC, "-x", "c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "use")])
    assert [int(v) for v in subprocess.check_output([str(tmp_path / "use")], text=True).split()] == want


@pytest.mark.parametrize("tag", LATER)
def test_library_exports_the_header_and_nothing_else(tag):
    side = _lib.LATER_LIBRARIES[tag]
    readelf = subprocess.check_output([HIPCC, "-print-prog-name=llvm-readelf"], text=True).strip()
    rows = [line.split() for line in subprocess.check_output([readelf, "--dyn-syms", "-W", side.path], text=True).splitlines()]
    defined = [r[7].split("@")[0] for r in rows if len(r) == 8 and r[0][:-1].isdigit() and r[6] != "UND"]
    assert sorted(n for n in defined if n.startswith("countr_")) == side.exported_symbols()
    assert [n for n in defined if not n.startswith(("countr_", "__hip_cuid_"))] == []


@pytest.mark.parametrize("tag", LATER)
def test_every_prototype_is_defined_extern_c_in_the_sources(tag):
    side = _lib.LATER_LIBRARIES[tag]
    paths = glob.glob(os.path.join(ROOT, "countr_amd", "csrc_" + tag, "*.hip"))
    src = "".join(open(p).read() for p in paths)
    for name in side.exported_symbols():
        assert re.search(r'extern "C" [\w ]+\*? ?%s\(' % name, src), name
    assert re.search(r"countr_%s_version\(void\) \{ return COUNTR_%s_ABI_VERSION; \}" % (tag, tag.upper()), src)
    assert paths and build.LATER[tag][1]() == sorted(paths)
    others = [os.path.basename(p) for d in ["csrc"] + ["csrc_" + t for t in build.TAGS + build.LATER_TAGS if t != tag]
              for p in glob.glob(os.path.join(ROOT, "countr_amd", d, "*.hip"))]
    assert not set(os.path.basename(p) for p in paths) & set(others)


def test_the_shared_conversion_is_stated_once():
    """yuv_kernel, its helpers and rdiv live in csrc/rgb420.hpp; both libraries include it and neither states them again."""
    shared = open(os.path.join(ROOT, "countr_amd", "csrc", "rgb420.hpp")).read()
    for name in ("void yuv_kernel(", "void load_px(", "uint32_t byte_of(", "int64_t rdiv(", "COEF[2][2][10]"):
        assert name in shared, name
        for lib in ("overlay", "draw"):
            src = open(os.path.join(ROOT, "countr_amd", "csrc_" + lib, lib + ".hip")).read()
            assert name not in src and '#include "../csrc/rgb420.hpp"' in src, (lib, name)


def test_refusals_run_on_the_host():
    """Every refusal returns before anything is read on the device or a kernel is launched: the device pointers are aligned numbers, not
    buffers; the packed upload's host copy is real, as the call reads it."""
    L = _lib.draw_lib()
    K = CONSTS
    err = lambda: L.countr_draw_last_error().decode()
    PACK = 0x7000000
    SEG, DISC, TEXT = [0, 0, 5, 5, 1, 0xff0000], [3, 3, 2, 0x00ff00], [1, 1, 1, 0xffffff, -1, 2] + [0x4948] + [0] * 7

    def records(n=17, **fields):
        recs = (_lib.DrawFrame * n)()
        for j in range(n):
            recs[j].rgb, recs[j].owner = 0x100000 * (j + 1), 0x100000 * (j + 1) + 0x80000
            for k, v in fields.items():
                setattr(recs[j], k, v)
        return recs

    def call(recs=None, n=1, H=4, W=6, words=(), host=True, pack=PACK, nbytes=None, fmt=K["RGB"], matrix=K["BT709"], rng=K["LIMITED"]):
        buf = np.asarray(list(words) + [0] * 4, np.int32)
        return L.countr_draw_paint(records() if recs is None else recs, n, H, W, buf.ctypes.data if host else None, pack,
                                   4 * len(words) if nbytes is None else nbytes, fmt, matrix, rng, None)

    # n out of range
    assert call(n=0) < 0 and "1..16 frames a call, got 0" in err()
    assert call(n=17) < 0 and "got 17" in err()
    # an unknown format, matrix or range
    assert call(fmt=4) < 0 and "unknown format 4" in err()
    assert call(fmt=-1) < 0 and "unknown format -1" in err()
    assert call(matrix=2) < 0 and "unknown matrix 2" in err()
    assert call(rng=2) < 0 and "unknown range 2" in err()
    # H or W outside 1..16384
    assert call(H=0) < 0 and "H and W are 1..16384, got 0 x 6" in err()
    assert call(W=16385) < 0 and "got 4 x 16385" in err()
    # every limit + 1
    assert call(records(n_segments=65601)) < 0 and "0..65600 segments, got 65601" in err()
    assert call(records(n_discs=4097)) < 0 and "0..4096 discs, got 4097" in err()
    assert call(records(n_texts=4161)) < 0 and "0..4160 texts, got 4161" in err()
    assert call(records(n_discs=-1)) < 0 and "got -1" in err()
    # a mark out of range, read from the host copy of the pack
    bad = lambda rec, k, v: rec[:k] + [v] + rec[k + 1:]
    assert call(records(n_segments=1), words=bad(SEG, 4, 9)) < 0 and "segment 0: half_width is 0..8, got 9" in err()
    assert call(records(n_segments=1), words=bad(SEG, 4, -1)) < 0 and "got -1" in err()
    assert call(records(n_segments=2, segments_off=0), words=SEG + bad(SEG, 2, (1 << 20) + 1)) < 0 and "segment 1: coordinates are within +-1048576" in err()
    assert call(records(n_segments=1), words=bad(SEG, 1, -(1 << 20) - 1)) < 0 and "coordinates are within" in err()
    assert call(records(n_segments=1), words=bad(SEG, 5, 1 << 24)) < 0 and "a colour is 0..0xffffff" in err()
    assert call(records(n_discs=1), words=bad(DISC, 2, 17)) < 0 and "disc 0: r is 0..16, got 17" in err()
    assert call(records(n_discs=1), words=bad(DISC, 0, (1 << 20) + 1)) < 0 and "disc 0: coordinates are within" in err()
    assert call(records(n_texts=1), words=bad(TEXT, 2, 0)) < 0 and "text 0: scale is 1..8, got 0" in err()
    assert call(records(n_texts=1), words=bad(TEXT, 2, 9)) < 0 and "got 9" in err()
    assert call(records(n_texts=1), words=bad(TEXT, 5, 33)) < 0 and "0..32 bytes of text, got 33" in err()
    assert call(records(n_texts=1), words=bad(TEXT, 1, (1 << 20) + 1)) < 0 and "text 0: coordinates are within" in err()
    assert call(records(n_texts=1), words=bad(TEXT, 4, -2)) < 0 and "background -1: none" in err()
    # offsets outside the pack, or misaligned in it
    assert call(records(n_segments=1, segments_off=4), words=SEG) < 0 and "outside the packed upload of 24 bytes" in err()
    assert call(records(n_segments=1, segments_off=-4), words=SEG) < 0 and "outside the packed upload" in err()
    assert call(records(n_discs=1, discs_off=2), words=DISC + [0]) < 0 and "4-byte aligned" in err()
    assert call(records(n_texts=1, texts_off=0), words=TEXT, nbytes=55) < 0 and "outside the packed upload of 55 bytes" in err()
    assert call(nbytes=-1) < 0 and "pack_bytes is >= 0" in err()
    # null pointers: the array, an element, the packs, the 4:2:0 buffer where it is required and where it must not be
    assert L.countr_draw_paint(None, 1, 4, 6, None, None, 0, 0, 1, 0, None) < 0 and "frames array is required" in err()
    for field in ("rgb", "owner"):
        recs = records()
        setattr(recs[2], field, None)
        assert call(recs, n=3) < 0 and "frame 2 has a null pointer" in err(), field
    assert call(records(n_segments=1), words=SEG, host=False) < 0 and "needs the packed upload" in err()
    assert call(records(n_segments=1), words=SEG, pack=None) < 0 and "needs the packed upload" in err()
    assert call(records(n_segments=1), words=SEG, pack=PACK + 4) < 0 and "16-byte aligned" in err()
    assert call(fmt=K["NV12"]) < 0 and "frame 0 has a null pointer" in err()
    assert call(records(yuv=0x9000000)) < 0 and "yuv must be NULL when the format is RGB" in err()
    recs = records()
    recs[0].owner = 0x180002
    assert call(recs) < 0 and "the owner plane is 4-byte aligned" in err()
    assert L.countr_draw_font(None) < 0 and "out is required" in err()
