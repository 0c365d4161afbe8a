"""ctypes binding of libcountr_hip.so, read from include/countr_hip.h: the header is the only statement of the C ABI.

There is no CPU fallback: if the shared library is missing or a call fails, this raises.
"""
import ctypes as C
import os
import re

from .build import LATER_TAGS, TAGS

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("COUNTR_LIB", os.path.join(_HERE, "libcountr_hip.so"))
# the same sources built with IEEE fp16 as the 16-bit storage / matrix-operand type (precision="fp16"; csrc/common.hpp, build.py)
LIB_PATH_F16 = os.environ.get("COUNTR_LIB_F16", os.path.join(_HERE, "libcountr_hip_f16.so"))
HEADER = os.path.join(_HERE, "..", "include", "countr_hip.h")


class CountrError(RuntimeError):
    pass


# ---- the header's dialect: comments, `#define COUNTR_X <integer>`, `typedef struct name { ... } name;` and prototypes, over the types
# below, pointers to them and fixed arrays.  Anything else is an error, never a guess: a wrong guess loads and then corrupts arguments.
_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "long long": C.c_int64, "uint64_t": C.c_uint64,
            "float": C.c_float, "double": C.c_double}
_DECLARATOR = r"\w+(?:\[\d+\])?"


def _ctype(text, structs, result=False):
    """The ctypes type of a C type: a struct pointer is POINTER(its class), `const char*` as a result c_char_p, other pointers c_void_p."""
    words = [w for w in text.replace("*", " * ").split() if w != "const"]
    stars = words.count("*")
    base = " ".join(words[:len(words) - stars])
    if "*" in words[:len(words) - stars] or not (base in _SCALARS or base in structs or (stars and base in ("void", "char"))):
        raise CountrError("include/countr_hip.h: unknown type %r" % text)
    if stars == 0:
        return _SCALARS.get(base) or structs[base]
    if base == "char":
        if not (result and stars == 1):
            raise CountrError("include/countr_hip.h: char pointers are results only: %r" % text)
        return C.c_char_p
    return C.POINTER(structs[base]) if stars == 1 and base in structs else C.c_void_p


def _split(decl, what):
    """`<type> <rest>` -> (type, rest), rest being a name, a declarator list or `name(parameters)`."""
    m = re.fullmatch(r"(.+?[\s*])\s*(%s(?:\s*,\s*%s)*|\w+\s*\(.*\))" % (_DECLARATOR, _DECLARATOR), decl, re.S)
    if not m:
        raise CountrError("include/countr_hip.h: cannot read %s %r" % (what, decl))
    return m.group(1), m.group(2)


def parse_header(text):
    """-> (constants {COUNTR_X: int}, structs {name: ctypes.Structure class}, prototypes {name: (restype, argtypes)}), each in the
    header's order."""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    consts = {name: int(value, 0) for name, value in re.findall(r"^#define[ \t]+(COUNTR_\w+)[ \t]+(\S.*?)[ \t]*$", text, re.M)}
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M).replace('extern "C" {', "", 1)
    structs = {}

    def struct(m):
        if m.group(1) != m.group(3):
            raise CountrError("include/countr_hip.h: struct %s is typedef'd as %s" % (m.group(1), m.group(3)))
        fields = []
        for decl in filter(None, (d.strip() for d in m.group(2).split(";"))):
            ctype, names = _split(decl, "field")
            ctype = _ctype(ctype, structs)
            for name in names.split(","):
                name, _, count = name.strip().rstrip("]").partition("[")
                fields.append((name, ctype * int(count) if count else ctype))
        structs[m.group(1)] = type(m.group(1), (C.Structure,), {"_fields_": fields})
        return ""

    text = re.sub(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", struct, text, flags=re.S)
    decls = [d.strip() for d in text.split(";")]
    if decls.pop() != "}":
        raise CountrError("include/countr_hip.h: text behind the last declaration")
    protos = {}
    for decl in decls:
        restype, rest = _split(decl, "prototype")
        name, _, params = rest.rstrip(")").partition("(")
        if not name.strip().startswith("countr_") or not params.strip():
            raise CountrError("include/countr_hip.h: cannot read prototype %r" % decl)
        params = [] if params.strip() == "void" else [_split(p.strip(), "parameter")[0] for p in params.split(",")]
        protos[name.strip()] = (_ctype(restype, structs, result=True), [_ctype(p, structs) for p in params])
    return consts, structs, protos


CONSTS, STRUCTS, PROTOS = parse_header(open(HEADER).read())
# every COUNTR_X of the header is X here: F32, BF16, OP_*, ACT_*, ABI_VERSION, AUG_MAX_IMAGES, PEAKS_MAX_MAPS, MATCH_MAX_SETS, ...
globals().update({name[len("COUNTR_"):]: value for name, value in CONSTS.items()})
GemmArgs, AugImage, MosaicPiece, MosaicImage, PretrainImage = (STRUCTS["countr_" + n] for n in (
    "gemm_args", "aug_image", "mosaic_piece", "mosaic_image", "pretrain_image"))
ReportPatch, ReportImage, ReportStrip, PeakMap, MatchSet = (STRUCTS["countr_" + n] for n in (
    "report_patch", "report_image", "report_strip", "peak_map", "match_set"))
_libs = {}


def _load(path, protos, version, want):
    """The ctypes handle of the library at `path`, bound from its header's prototypes; raises CountrError if it is not built or was
    built from another version of the header (its `version` export does not return `want`)."""
    if not os.path.exists(path):
        raise CountrError(
            "%s is not built (run `python -m countr_amd.build` or __graft_entry__.build()); "
            "the HIP path has no CPU fallback" % os.path.basename(path))
    L = C.CDLL(path)
    for name, (restype, argtypes) in protos.items():
        fn = getattr(L, name)  # AttributeError here means the .so is stale: rebuild
        fn.restype, fn.argtypes = restype, argtypes
    if getattr(L, version)() != want:      # a stale build: its structs (countr_gemm_args, ...) are not the header's
        raise CountrError("%s has ABI version %d, this package needs %d: rebuild (python -m countr_amd.build)"
                          % (os.path.basename(path), getattr(L, version)(), want))
    return L


def lib(variant=""):
    """Load (once) and return the ctypes handle of a library variant ("" = bf16 build, "f16" = fp16 build); raises CountrError if it
    is not built."""
    L = _libs.get(variant)
    if L is None:
        L = _libs[variant] = _load(LIB_PATH_F16 if variant == "f16" else LIB_PATH, PROTOS, "countr_version", ABI_VERSION)
    return L


def variant_of(precision):
    return "f16" if precision == "fp16" else ""


def check(rc, what=""):
    if rc != 0:
        msgs = [m.decode() for m in (L.countr_last_error() for L in _libs.values()) if m]      # (the error text is per library and thread)
        raise CountrError("%s failed (rc=%d): %s" % (what or "countr call", rc, " | ".join(msgs)))


def exported_symbols():
    """Names declared in include/countr_hip.h, which are the names the library exports."""
    return sorted(PROTOS)


# ---- the side libraries: exports that came after the ABI of countr_hip.h was closed.  Each is stated by its tag alone (build.py builds
# them by the same rule): header include/countr_hip_<tag>.h, in the same dialect, is its one statement; nothing of it enters CONSTS /
# STRUCTS / PROTOS or this module's COUNTR_* globals.
class Library:
    """The binding of libcountr_hip_<tag>.so (COUNTR_LIB_<TAG> overrides the path), read from its header."""

    def __init__(self, tag):
        self.tag = tag
        self.path = os.environ.get("COUNTR_LIB_" + tag.upper(), os.path.join(_HERE, "libcountr_hip_%s.so" % tag))
        self.header = os.path.join(_HERE, "..", "include", "countr_hip_%s.h" % tag)
        self.consts, self.structs, self.protos = parse_header(open(self.header).read())
        self._handle = None

    def load(self):
        """Load (once) and return the ctypes handle, bound from the header; raises CountrError if the library is not built or was built
        from another version of the header."""
        if self._handle is None:
            self._handle = _load(self.path, self.protos, "countr_%s_version" % self.tag,
                                 self.consts["COUNTR_%s_ABI_VERSION" % self.tag.upper()])
        return self._handle

    def check(self, rc, what=""):
        if rc != 0:
            text = getattr(self.load(), "countr_%s_last_error" % self.tag)() or b""
            raise CountrError("%s failed (rc=%d): %s" % (what or "countr_%s call" % self.tag, rc, text.decode()))

    def exported_symbols(self):
        """Names declared in the header, which are the names the library exports."""
        return sorted(self.protos)


# build.TAGS, in the order they were added: regional counts, the fold of class maps into a label map, frames counted on a 2-D grid of
# tiles, 4:2:0 decoder surfaces to packed RGB, annotated frames, points joined into tracks, line counts from density flux, the camera's
# motion from the flow field
LIBRARIES = {tag: Library(tag) for tag in TAGS}
# build.LATER_TAGS: the libraries that came after that table was closed, stated and bound by the same rule: marks drawn onto frames
LATER_LIBRARIES = {tag: Library(tag) for tag in LATER_TAGS}
# what the wrappers read: EXT_LIB_PATH, EXT_HEADER, EXT_CONSTS, EXT_STRUCTS, EXT_PROTOS, ext_lib(), ext_check(rc, what), ext_exported_symbols()
# and the same for every other tag, of either table
for _tag, _l in list(LIBRARIES.items()) + list(LATER_LIBRARIES.items()):
    globals().update({_tag.upper() + "_LIB_PATH": _l.path, _tag.upper() + "_HEADER": _l.header, _tag.upper() + "_CONSTS": _l.consts,
                      _tag.upper() + "_STRUCTS": _l.structs, _tag.upper() + "_PROTOS": _l.protos, _tag + "_lib": _l.load,
                      _tag + "_check": _l.check, _tag + "_exported_symbols": _l.exported_symbols})
RegionMap, Region = EXT_STRUCTS["countr_region_map"], EXT_STRUCTS["countr_region"]
ClassSet, OverlayFrame = CLASSES_STRUCTS["countr_class_set"], OVERLAY_STRUCTS["countr_overlay_frame"]
TracksStream, FlowMap = TRACKS_STRUCTS["countr_tracks_stream"], FLOW_STRUCTS["countr_flow_map"]
DrawFrame = DRAW_STRUCTS["countr_draw_frame"]
