"""CPU: the side libraries are stated by one ordered list of tags.  countr_amd/build.py (what is built), countr_amd/_lib.py (what is
bound) and __graft_entry__.build() (what is load-checked) follow it by one naming rule, and the seven sources share one host-side error
path (csrc/host_api.hpp).  The per-library literal pins stay in the test_<tag>_abi_cpu.py files."""
import ctypes as C
import os
import subprocess
import sys
import threading

import pytest

from countr_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = ["ext", "classes", "tiles", "yuv", "overlay", "tracks", "flow"]


def test_one_list_of_tags_states_build_and_binding():
    assert list(build.SINGLE) == list(_lib.LIBRARIES) == TAGS
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
    assert len(lines) == 7 and any("libcountr_hip_overlay.so" in line for line in lines)


def test_a_missing_symbol_fails_the_load_check(monkeypatch):
    import __graft_entry__ as G
    side = _lib.LIBRARIES["overlay"]
    side.load()
    monkeypatch.setitem(side.protos, "countr_overlay_absent", (C.c_int, []))
    with pytest.raises(RuntimeError, match=r"libcountr_hip_overlay\.so lacks symbols declared in include/countr_hip_overlay\.h: \['countr_overlay_absent'\]"):
        G.check_side_libraries()
