"""CPU: the side libraries are stated by one ordered list of tags.  countr_amd/build.py (what is built), countr_amd/_lib.py (what is
bound) and __graft_entry__.build() (what is load-checked) follow it by one naming rule, and the sources share one host-side error
path (csrc/host_api.hpp).  What holds of every library by that rule is checked here once per tag: the header against the C compiler,
the library's dynamic symbols against the header, the sources against the prototypes.  The per-library literal pins stay in the
test_<tag>_abi_cpu.py files."""
import ctypes as C
import glob
import os
import re
import subprocess
import sys
import threading

import pytest

from countr_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")      # the compiler countr_amd/build.py uses
TAGS = ["ext", "classes", "tiles", "yuv", "overlay", "tracks", "flow", "cam"]


def test_one_list_of_tags_states_build_and_binding():
    assert list(build.TAGS) == list(build.SINGLE) == list(_lib.LIBRARIES) == TAGS
    for tag, side in _lib.LIBRARIES.items():
        lib, _sources, header = build.SINGLE[tag]
        assert side.path == lib == os.path.join(ROOT, "countr_amd", "libcountr_hip_%s.so" % tag)
        assert os.path.samefile(side.header, header) and os.path.basename(header) == "countr_hip_%s.h" % tag
        assert "countr_%s_version" % tag in side.exported_symbols() and "countr_%s_last_error" % tag in side.exported_symbols()
        # the module-level names the wrappers read are this instance's
        T = tag.upper()
        assert getattr(_lib, T + "_LIB_PATH") == side.path and getattr(_lib, T + "_HEADER") == side.header
        assert getattr(_lib, T + "_CONSTS") is side.consts and getattr(_lib, T + "_STRUCTS") is side.structs
        assert getattr(_lib, T + "_PROTOS") is side.protos and getattr(_lib, tag + "_lib")() is side.load()
        assert getattr(_lib, tag + "_exported_symbols")() == side.exported_symbols()
        # and nothing else of the library is a global of the module: none of its COUNTR_<TAG>_* constants
        assert {k for k in vars(_lib) if k.startswith(T + "_")} == {T + s for s in ("_LIB_PATH", "_HEADER", "_CONSTS", "_STRUCTS", "_PROTOS")}


def test_environment_overrides_each_path():
    env = dict(os.environ, **{"COUNTR_LIB_" + tag.upper(): "/elsewhere/%s.so" % tag for tag in TAGS})
    code = "from countr_amd import _lib\nfor t, l in _lib.LIBRARIES.items(): print(t, l.path, getattr(_lib, t.upper() + '_LIB_PATH'))"
    out = subprocess.check_output([sys.executable, "-c", code], cwd=ROOT, env=env, text=True)
    assert out.split() == [w for tag in TAGS for w in (tag, "/elsewhere/%s.so" % tag, "/elsewhere/%s.so" % tag)]


@pytest.mark.parametrize("tag", TAGS)
def test_check_passes_zero_and_raises_with_the_library_s_text(tag):
    check = getattr(_lib, tag + "_check")
    assert check(0) is None and check(0, "probe") is None
    with pytest.raises(_lib.CountrError, match=r"probe failed \(rc=-1\)"):
        check(-1, "probe")
    with pytest.raises(_lib.CountrError, match=r"countr_%s call failed \(rc=-7\)" % tag):
        check(-7)


def test_error_text_is_per_thread():
    """A refusal on one thread (host-side: it launches nothing) is not seen from another; both threads are alive at once."""
    L = _lib.flow_lib()
    refused, read = threading.Event(), threading.Event()
    seen = {}

    def first():
        seen["rc"] = L.countr_flow_workspace(0, 384)
        refused.set()
        read.wait(30)
        seen["first"] = L.countr_flow_last_error()

    def second():
        refused.wait(30)
        seen["second"] = L.countr_flow_last_error()
        read.set()

    threads = [threading.Thread(target=f) for f in (first, second)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(60)
    assert seen["rc"] == -1 and seen["second"] == b""
    assert seen["first"] == b"countr_flow_workspace: 1..16 maps of a height that is a multiple of 8 in 8..4096, got 0 of 384"


def test_build_load_checks_every_side_library(capsys):
    import __graft_entry__ as G
    G.check_side_libraries()
    lines = capsys.readouterr().out.splitlines()
    assert lines == ["build ok: %s (%d exported symbols)" % (side.path, len(side.protos)) for side in _lib.LIBRARIES.values()]
    assert len(lines) == 8 and any("libcountr_hip_overlay.so" in line for line in lines)


def test_a_missing_symbol_fails_the_load_check(monkeypatch):
    import __graft_entry__ as G
    side = _lib.LIBRARIES["overlay"]
    side.load()
    monkeypatch.setitem(side.protos, "countr_overlay_absent", (C.c_int, []))
    with pytest.raises(RuntimeError, match=r"libcountr_hip_overlay\.so lacks symbols declared in include/countr_hip_overlay\.h: \['countr_overlay_absent'\]"):
        G.check_side_libraries()


@pytest.mark.parametrize("tag", build.TAGS)
def test_header_compiles_as_c_with_the_binding_s_constants_and_layout(tag, tmp_path):
    """The C program is generated from the header's own lists: every constant, and of every struct the size and each field's offset
    and size, as a C compiler sees them and as the binding read them."""
    side = _lib.LIBRARIES[tag]
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


@pytest.mark.parametrize("tag", build.TAGS)
def test_library_exports_the_header_and_nothing_else(tag):
    side = _lib.LIBRARIES[tag]
    readelf = subprocess.check_output([HIPCC, "-print-prog-name=llvm-readelf"], text=True).strip()
    rows = [line.split() for line in subprocess.check_output([readelf, "--dyn-syms", "-W", side.path], text=True).splitlines()]
    defined = [r[7].split("@")[0] for r in rows if len(r) == 8 and r[0][:-1].isdigit() and r[6] != "UND"]
    assert sorted(n for n in defined if n.startswith("countr_")) == side.exported_symbols()
    assert [n for n in defined if not n.startswith(("countr_", "__hip_cuid_"))] == []


@pytest.mark.parametrize("tag", build.TAGS)
def test_every_prototype_is_defined_extern_c_in_the_sources(tag):
    side = _lib.LIBRARIES[tag]
    paths = glob.glob(os.path.join(ROOT, "countr_amd", "csrc_" + tag, "*.hip"))
    src = "".join(open(p).read() for p in paths)
    for name in side.exported_symbols():
        assert re.search(r'extern "C" [\w ]+\*? ?%s\(' % name, src), name
    assert re.search(r"countr_%s_version\(void\) \{ return COUNTR_%s_ABI_VERSION; \}" % (tag, tag.upper()), src)
    # the library is built from exactly these, and their names stay outside the globs every other library is built from
    assert paths and build.SINGLE[tag][1]() == sorted(paths)
    others = [os.path.basename(p) for d in ["csrc"] + ["csrc_" + t for t in build.TAGS if t != tag]
              for p in glob.glob(os.path.join(ROOT, "countr_amd", d, "*.hip"))]
    assert not set(os.path.basename(p) for p in paths) & set(others)
