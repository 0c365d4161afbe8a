"""ctypes binding of libcountr_hip.so, read from include/countr_hip.h: the header is the only statement of the C ABI.

There is no CPU fallback: if the shared library is missing or a call fails, this raises.
"""
import ctypes as C
import os
import re

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


def lib(variant=""):
    """Load (once) and return the ctypes handle of a library variant ("" = bf16 build, "f16" = fp16 build); raises CountrError if it
    is not built."""
    L = _libs.get(variant)
    if L is None:
        path = LIB_PATH_F16 if variant == "f16" else LIB_PATH
        if not os.path.exists(path):
            raise CountrError(
                "%s is not built (run `python -m countr_amd.build` or __graft_entry__.build()); "
                "the HIP path has no CPU fallback" % os.path.basename(path))
        L = C.CDLL(path)
        for name, (restype, argtypes) in PROTOS.items():
            fn = getattr(L, name)  # AttributeError here means the .so is stale: rebuild
            fn.restype, fn.argtypes = restype, argtypes
        if L.countr_version() != ABI_VERSION:      # a stale build: its countr_gemm_args is shorter than GemmArgs
            raise CountrError("%s has ABI version %d, this package needs %d: rebuild (python -m countr_amd.build)"
                              % (os.path.basename(path), L.countr_version(), ABI_VERSION))
        _libs[variant] = L
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


# ---- the extension library: exports that came after the ABI of countr_hip.h was closed.  include/countr_hip_ext.h is its one statement,
# in the same dialect; nothing of it enters CONSTS / STRUCTS / PROTOS or this module's COUNTR_* globals.
EXT_LIB_PATH = os.environ.get("COUNTR_LIB_EXT", os.path.join(_HERE, "libcountr_hip_ext.so"))
EXT_HEADER = os.path.join(_HERE, "..", "include", "countr_hip_ext.h")
EXT_CONSTS, EXT_STRUCTS, EXT_PROTOS = parse_header(open(EXT_HEADER).read())
RegionMap, Region = EXT_STRUCTS["countr_region_map"], EXT_STRUCTS["countr_region"]
_ext = None


def ext_lib():
    """Load (once) and return the ctypes handle of libcountr_hip_ext.so, bound from its header; raises CountrError if it is not built or
    was built from another version of the header."""
    global _ext
    if _ext is None:
        if not os.path.exists(EXT_LIB_PATH):
            raise CountrError(
                "%s is not built (run `python -m countr_amd.build` or __graft_entry__.build()); "
                "the HIP path has no CPU fallback" % os.path.basename(EXT_LIB_PATH))
        L = C.CDLL(EXT_LIB_PATH)
        for name, (restype, argtypes) in EXT_PROTOS.items():
            fn = getattr(L, name)  # AttributeError here means the .so is stale: rebuild
            fn.restype, fn.argtypes = restype, argtypes
        if L.countr_ext_version() != EXT_CONSTS["COUNTR_EXT_ABI_VERSION"]:
            raise CountrError("%s has ABI version %d, this package needs %d: rebuild (python -m countr_amd.build)"
                              % (os.path.basename(EXT_LIB_PATH), L.countr_ext_version(), EXT_CONSTS["COUNTR_EXT_ABI_VERSION"]))
        _ext = L
    return _ext


def ext_check(rc, what=""):
    if rc != 0:
        raise CountrError("%s failed (rc=%d): %s" % (what or "countr_ext call", rc, (ext_lib().countr_ext_last_error() or b"").decode()))


def ext_exported_symbols():
    """Names declared in include/countr_hip_ext.h, which are the names the extension library exports."""
    return sorted(EXT_PROTOS)


# ---- the classes library: the fold of a frame's class maps into a label map.  include/countr_hip_classes.h is its one statement, in
# the same dialect; nothing of it enters the bindings above or this module's COUNTR_* globals.
CLASSES_LIB_PATH = os.environ.get("COUNTR_LIB_CLASSES", os.path.join(_HERE, "libcountr_hip_classes.so"))
CLASSES_HEADER = os.path.join(_HERE, "..", "include", "countr_hip_classes.h")
CLASSES_CONSTS, CLASSES_STRUCTS, CLASSES_PROTOS = parse_header(open(CLASSES_HEADER).read())
ClassSet = CLASSES_STRUCTS["countr_class_set"]
_classes = None


def classes_lib():
    """Load (once) and return the ctypes handle of libcountr_hip_classes.so, bound from its header; raises CountrError if it is not built
    or was built from another version of the header."""
    global _classes
    if _classes is None:
        if not os.path.exists(CLASSES_LIB_PATH):
            raise CountrError(
                "%s is not built (run `python -m countr_amd.build` or __graft_entry__.build()); "
                "the HIP path has no CPU fallback" % os.path.basename(CLASSES_LIB_PATH))
        L = C.CDLL(CLASSES_LIB_PATH)
        for name, (restype, argtypes) in CLASSES_PROTOS.items():
            fn = getattr(L, name)  # AttributeError here means the .so is stale: rebuild
            fn.restype, fn.argtypes = restype, argtypes
        if L.countr_classes_version() != CLASSES_CONSTS["COUNTR_CLASSES_ABI_VERSION"]:
            raise CountrError("%s has ABI version %d, this package needs %d: rebuild (python -m countr_amd.build)"
                              % (os.path.basename(CLASSES_LIB_PATH), L.countr_classes_version(), CLASSES_CONSTS["COUNTR_CLASSES_ABI_VERSION"]))
        _classes = L
    return _classes


def classes_check(rc, what=""):
    if rc != 0:
        raise CountrError("%s failed (rc=%d): %s" % (what or "countr_classes call", rc, (classes_lib().countr_classes_last_error() or b"").decode()))


def classes_exported_symbols():
    """Names declared in include/countr_hip_classes.h, which are the names the classes library exports."""
    return sorted(CLASSES_PROTOS)


# ---- the tiles library: a frame counted on a 2-D grid of 384 x 384 tiles (count_frames(zoom=k)).  include/countr_hip_tiles.h is its one
# statement, in the same dialect; nothing of it enters the bindings above or this module's COUNTR_* globals.
TILES_LIB_PATH = os.environ.get("COUNTR_LIB_TILES", os.path.join(_HERE, "libcountr_hip_tiles.so"))
TILES_HEADER = os.path.join(_HERE, "..", "include", "countr_hip_tiles.h")
TILES_CONSTS, TILES_STRUCTS, TILES_PROTOS = parse_header(open(TILES_HEADER).read())
_tiles = None


def tiles_lib():
    """Load (once) and return the ctypes handle of libcountr_hip_tiles.so, bound from its header; raises CountrError if it is not built
    or was built from another version of the header."""
    global _tiles
    if _tiles is None:
        if not os.path.exists(TILES_LIB_PATH):
            raise CountrError(
                "%s is not built (run `python -m countr_amd.build` or __graft_entry__.build()); "
                "the HIP path has no CPU fallback" % os.path.basename(TILES_LIB_PATH))
        L = C.CDLL(TILES_LIB_PATH)
        for name, (restype, argtypes) in TILES_PROTOS.items():
            fn = getattr(L, name)  # AttributeError here means the .so is stale: rebuild
            fn.restype, fn.argtypes = restype, argtypes
        if L.countr_tiles_version() != TILES_CONSTS["COUNTR_TILES_ABI_VERSION"]:
            raise CountrError("%s has ABI version %d, this package needs %d: rebuild (python -m countr_amd.build)"
                              % (os.path.basename(TILES_LIB_PATH), L.countr_tiles_version(), TILES_CONSTS["COUNTR_TILES_ABI_VERSION"]))
        _tiles = L
    return _tiles


def tiles_check(rc, what=""):
    if rc != 0:
        raise CountrError("%s failed (rc=%d): %s" % (what or "countr_tiles call", rc, (tiles_lib().countr_tiles_last_error() or b"").decode()))


def tiles_exported_symbols():
    """Names declared in include/countr_hip_tiles.h, which are the names the tiles library exports."""
    return sorted(TILES_PROTOS)


# ---- the yuv library: 4:2:0 decoder surfaces (NV12, NV21, I420, P010) converted to the packed RGB the raw-frame entry points take.
# include/countr_hip_yuv.h is its one statement, in the same dialect; nothing of it enters the bindings above or this module's COUNTR_*
# globals.
YUV_LIB_PATH = os.environ.get("COUNTR_LIB_YUV", os.path.join(_HERE, "libcountr_hip_yuv.so"))
YUV_HEADER = os.path.join(_HERE, "..", "include", "countr_hip_yuv.h")
YUV_CONSTS, YUV_STRUCTS, YUV_PROTOS = parse_header(open(YUV_HEADER).read())
_yuv = None


def yuv_lib():
    """Load (once) and return the ctypes handle of libcountr_hip_yuv.so, bound from its header; raises CountrError if it is not built or
    was built from another version of the header."""
    global _yuv
    if _yuv is None:
        if not os.path.exists(YUV_LIB_PATH):
            raise CountrError(
                "%s is not built (run `python -m countr_amd.build` or __graft_entry__.build()); "
                "the HIP path has no CPU fallback" % os.path.basename(YUV_LIB_PATH))
        L = C.CDLL(YUV_LIB_PATH)
        for name, (restype, argtypes) in YUV_PROTOS.items():
            fn = getattr(L, name)  # AttributeError here means the .so is stale: rebuild
            fn.restype, fn.argtypes = restype, argtypes
        if L.countr_yuv_version() != YUV_CONSTS["COUNTR_YUV_ABI_VERSION"]:
            raise CountrError("%s has ABI version %d, this package needs %d: rebuild (python -m countr_amd.build)"
                              % (os.path.basename(YUV_LIB_PATH), L.countr_yuv_version(), YUV_CONSTS["COUNTR_YUV_ABI_VERSION"]))
        _yuv = L
    return _yuv


def yuv_check(rc, what=""):
    if rc != 0:
        raise CountrError("%s failed (rc=%d): %s" % (what or "countr_yuv call", rc, (yuv_lib().countr_yuv_last_error() or b"").decode()))


def yuv_exported_symbols():
    """Names declared in include/countr_hip_yuv.h, which are the names the yuv library exports."""
    return sorted(YUV_PROTOS)


# ---- the overlay library: annotated frames composed on the device (density overlay, marks, RGB or 4:2:0 out).
# include/countr_hip_overlay.h is its one statement, in the same dialect; nothing of it enters the bindings above or this module's
# COUNTR_* globals.
OVERLAY_LIB_PATH = os.environ.get("COUNTR_LIB_OVERLAY", os.path.join(_HERE, "libcountr_hip_overlay.so"))
OVERLAY_HEADER = os.path.join(_HERE, "..", "include", "countr_hip_overlay.h")
OVERLAY_CONSTS, OVERLAY_STRUCTS, OVERLAY_PROTOS = parse_header(open(OVERLAY_HEADER).read())
OverlayFrame = OVERLAY_STRUCTS["countr_overlay_frame"]
_overlay = None


def overlay_lib():
    """Load (once) and return the ctypes handle of libcountr_hip_overlay.so, bound from its header; raises CountrError if it is not built
    or was built from another version of the header."""
    global _overlay
    if _overlay is None:
        if not os.path.exists(OVERLAY_LIB_PATH):
            raise CountrError(
                "%s is not built (run `python -m countr_amd.build` or __graft_entry__.build()); "
                "the HIP path has no CPU fallback" % os.path.basename(OVERLAY_LIB_PATH))
        L = C.CDLL(OVERLAY_LIB_PATH)
        for name, (restype, argtypes) in OVERLAY_PROTOS.items():
            fn = getattr(L, name)  # AttributeError here means the .so is stale: rebuild
            fn.restype, fn.argtypes = restype, argtypes
        if L.countr_overlay_version() != OVERLAY_CONSTS["COUNTR_OVERLAY_ABI_VERSION"]:
            raise CountrError("%s has ABI version %d, this package needs %d: rebuild (python -m countr_amd.build)"
                              % (os.path.basename(OVERLAY_LIB_PATH), L.countr_overlay_version(), OVERLAY_CONSTS["COUNTR_OVERLAY_ABI_VERSION"]))
        _overlay = L
    return _overlay


def overlay_check(rc, what=""):
    if rc != 0:
        raise CountrError("%s failed (rc=%d): %s" % (what or "countr_overlay call", rc, (overlay_lib().countr_overlay_last_error() or b"").decode()))


def overlay_exported_symbols():
    """Names declared in include/countr_hip_overlay.h, which are the names the overlay library exports."""
    return sorted(OVERLAY_PROTOS)


# ---- the tracks library: the frames' points joined over time (track ids, line crossings, distinct count).
# include/countr_hip_tracks.h is its one statement, in the same dialect; nothing of it enters the bindings above or this module's
# COUNTR_* globals.
TRACKS_LIB_PATH = os.environ.get("COUNTR_LIB_TRACKS", os.path.join(_HERE, "libcountr_hip_tracks.so"))
TRACKS_HEADER = os.path.join(_HERE, "..", "include", "countr_hip_tracks.h")
TRACKS_CONSTS, TRACKS_STRUCTS, TRACKS_PROTOS = parse_header(open(TRACKS_HEADER).read())
TracksStream = TRACKS_STRUCTS["countr_tracks_stream"]
_tracks = None


def tracks_lib():
    """Load (once) and return the ctypes handle of libcountr_hip_tracks.so, bound from its header; raises CountrError if it is not built
    or was built from another version of the header."""
    global _tracks
    if _tracks is None:
        if not os.path.exists(TRACKS_LIB_PATH):
            raise CountrError(
                "%s is not built (run `python -m countr_amd.build` or __graft_entry__.build()); "
                "the HIP path has no CPU fallback" % os.path.basename(TRACKS_LIB_PATH))
        L = C.CDLL(TRACKS_LIB_PATH)
        for name, (restype, argtypes) in TRACKS_PROTOS.items():
            fn = getattr(L, name)  # AttributeError here means the .so is stale: rebuild
            fn.restype, fn.argtypes = restype, argtypes
        if L.countr_tracks_version() != TRACKS_CONSTS["COUNTR_TRACKS_ABI_VERSION"]:
            raise CountrError("%s has ABI version %d, this package needs %d: rebuild (python -m countr_amd.build)"
                              % (os.path.basename(TRACKS_LIB_PATH), L.countr_tracks_version(), TRACKS_CONSTS["COUNTR_TRACKS_ABI_VERSION"]))
        _tracks = L
    return _tracks


def tracks_check(rc, what=""):
    if rc != 0:
        raise CountrError("%s failed (rc=%d): %s" % (what or "countr_tracks call", rc, (tracks_lib().countr_tracks_last_error() or b"").decode()))


def tracks_exported_symbols():
    """Names declared in include/countr_hip_tracks.h, which are the names the tracks library exports."""
    return sorted(TRACKS_PROTOS)


# ---- the flow library: line counts from density flux (luma, block-matching motion, flux of a density map through counting lines).
# include/countr_hip_flow.h is its one statement, in the same dialect; nothing of it enters the bindings above or this module's
# COUNTR_* globals.
FLOW_LIB_PATH = os.environ.get("COUNTR_LIB_FLOW", os.path.join(_HERE, "libcountr_hip_flow.so"))
FLOW_HEADER = os.path.join(_HERE, "..", "include", "countr_hip_flow.h")
FLOW_CONSTS, FLOW_STRUCTS, FLOW_PROTOS = parse_header(open(FLOW_HEADER).read())
FlowMap = FLOW_STRUCTS["countr_flow_map"]
_flow = None


def flow_lib():
    """Load (once) and return the ctypes handle of libcountr_hip_flow.so, bound from its header; raises CountrError if it is not built or
    was built from another version of the header."""
    global _flow
    if _flow is None:
        if not os.path.exists(FLOW_LIB_PATH):
            raise CountrError(
                "%s is not built (run `python -m countr_amd.build` or __graft_entry__.build()); "
                "the HIP path has no CPU fallback" % os.path.basename(FLOW_LIB_PATH))
        L = C.CDLL(FLOW_LIB_PATH)
        for name, (restype, argtypes) in FLOW_PROTOS.items():
            fn = getattr(L, name)  # AttributeError here means the .so is stale: rebuild
            fn.restype, fn.argtypes = restype, argtypes
        if L.countr_flow_version() != FLOW_CONSTS["COUNTR_FLOW_ABI_VERSION"]:
            raise CountrError("%s has ABI version %d, this package needs %d: rebuild (python -m countr_amd.build)"
                              % (os.path.basename(FLOW_LIB_PATH), L.countr_flow_version(), FLOW_CONSTS["COUNTR_FLOW_ABI_VERSION"]))
        _flow = L
    return _flow


def flow_check(rc, what=""):
    if rc != 0:
        raise CountrError("%s failed (rc=%d): %s" % (what or "countr_flow call", rc, (flow_lib().countr_flow_last_error() or b"").decode()))


def flow_exported_symbols():
    """Names declared in include/countr_hip_flow.h, which are the names the flow library exports."""
    return sorted(FLOW_PROTOS)
