"""Build libcountr_hip.so (all HIP kernels + the C ABI) and the extension libraries libcountr_hip_ext.so, libcountr_hip_classes.so,
libcountr_hip_tiles.so, libcountr_hip_yuv.so, libcountr_hip_overlay.so, libcountr_hip_tracks.so and libcountr_hip_flow.so in-tree for gfx950.

hipcc cross-compiles without a GPU, so this runs in the build container and on the GPU box.
The .so is git-ignored but travels with the repo snapshot to the GPU box.
"""
import glob
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libcountr_hip.so")


def sources():
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")))


# per-file flags on top of the common ones (reasons in the file headers)
EXTRA_FLAGS = {"flash_attn_fwd.hip": ["-fno-slp-vectorize", "-fno-honor-nans"]}


def _digest(paths, extra=""):
    import hashlib
    h = hashlib.sha256(extra.encode())
    for p in sorted(paths):
        h.update(os.path.basename(p).encode())
        h.update(open(p, "rb").read())
    return h.hexdigest()


# the library is built twice from the same sources: the 16-bit storage / matrix-operand type is bfloat16 in libcountr_hip.so
# (precision="bf16") and IEEE fp16 in libcountr_hip_f16.so (precision="fp16", -DCOUNTR_HALF_FP16=1: csrc/common.hpp)
LIB_F16 = os.path.join(HERE, "libcountr_hip_f16.so")
VARIANTS = (("", LIB, []), ("f16", LIB_F16, ["-DCOUNTR_HALF_FP16=1"]))
# the extension library (include/countr_hip_ext.h): exports that came after the ABI of countr_hip.h was closed.  Its sources live in
# csrc_ext/, outside the csrc/*.hip glob, and are built once: nothing in them has a 16-bit operand
CSRC_EXT = os.path.join(HERE, "csrc_ext")
LIB_EXT = os.path.join(HERE, "libcountr_hip_ext.so")
EXT_HEADER = os.path.join(HERE, "..", "include", "countr_hip_ext.h")
# the classes library (include/countr_hip_classes.h), built like the extension library, from csrc_classes/
CSRC_CLASSES = os.path.join(HERE, "csrc_classes")
LIB_CLASSES = os.path.join(HERE, "libcountr_hip_classes.so")
CLASSES_HEADER = os.path.join(HERE, "..", "include", "countr_hip_classes.h")
# the tiles library (include/countr_hip_tiles.h), built the same way, from csrc_tiles/
CSRC_TILES = os.path.join(HERE, "csrc_tiles")
LIB_TILES = os.path.join(HERE, "libcountr_hip_tiles.so")
TILES_HEADER = os.path.join(HERE, "..", "include", "countr_hip_tiles.h")
# the yuv library (include/countr_hip_yuv.h), built the same way, from csrc_yuv/
CSRC_YUV = os.path.join(HERE, "csrc_yuv")
LIB_YUV = os.path.join(HERE, "libcountr_hip_yuv.so")
YUV_HEADER = os.path.join(HERE, "..", "include", "countr_hip_yuv.h")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden"]


def ext_sources():
    return sorted(glob.glob(os.path.join(CSRC_EXT, "*.hip")))


def classes_sources():
    return sorted(glob.glob(os.path.join(CSRC_CLASSES, "*.hip")))


def tiles_sources():
    return sorted(glob.glob(os.path.join(CSRC_TILES, "*.hip")))


def yuv_sources():
    return sorted(glob.glob(os.path.join(CSRC_YUV, "*.hip")))


# the libraries built once, without a 16-bit twin: tag -> (library, sources, its header)
SINGLE = {"ext": (LIB_EXT, ext_sources, EXT_HEADER), "classes": (LIB_CLASSES, classes_sources, CLASSES_HEADER),
          "tiles": (LIB_TILES, tiles_sources, TILES_HEADER)}
# the same table for the libraries that came after SINGLE's keys were pinned; build() walks both
SINGLE_LATER = {"yuv": (LIB_YUV, yuv_sources, YUV_HEADER)}
# the overlay library (include/countr_hip_overlay.h), from csrc_overlay/: SINGLE_LATER's keys are pinned too, so it has a table of its own
CSRC_OVERLAY = os.path.join(HERE, "csrc_overlay")
LIB_OVERLAY = os.path.join(HERE, "libcountr_hip_overlay.so")
OVERLAY_HEADER = os.path.join(HERE, "..", "include", "countr_hip_overlay.h")


def overlay_sources():
    return sorted(glob.glob(os.path.join(CSRC_OVERLAY, "*.hip")))


SINGLE_OVERLAY = {"overlay": (LIB_OVERLAY, overlay_sources, OVERLAY_HEADER)}
# the tracks library (include/countr_hip_tracks.h), from csrc_tracks/: every older table's keys are pinned, so it has a table of its own
CSRC_TRACKS = os.path.join(HERE, "csrc_tracks")
LIB_TRACKS = os.path.join(HERE, "libcountr_hip_tracks.so")
TRACKS_HEADER = os.path.join(HERE, "..", "include", "countr_hip_tracks.h")


def tracks_sources():
    return sorted(glob.glob(os.path.join(CSRC_TRACKS, "*.hip")))


SINGLE_TRACKS = {"tracks": (LIB_TRACKS, tracks_sources, TRACKS_HEADER)}
# the flow library (include/countr_hip_flow.h), from csrc_flow/: every older table's keys are pinned, so it has a table of its own
CSRC_FLOW = os.path.join(HERE, "csrc_flow")
LIB_FLOW = os.path.join(HERE, "libcountr_hip_flow.so")
FLOW_HEADER = os.path.join(HERE, "..", "include", "countr_hip_flow.h")


def flow_sources():
    return sorted(glob.glob(os.path.join(CSRC_FLOW, "*.hip")))


SINGLE_FLOW = {"flow": (LIB_FLOW, flow_sources, FLOW_HEADER)}


def build(force=False, verbose=True):
    """Compile every csrc/*.hip for gfx950 and link libcountr_hip.so + libcountr_hip_f16.so, and every csrc_ext/*.hip into
    libcountr_hip_ext.so, every csrc_classes/*.hip into libcountr_hip_classes.so, every csrc_tiles/*.hip into libcountr_hip_tiles.so, every csrc_yuv/*.hip into libcountr_hip_yuv.so, every csrc_overlay/*.hip into libcountr_hip_overlay.so, every csrc_tracks/*.hip into libcountr_hip_tracks.so, every csrc_flow/*.hip into libcountr_hip_flow.so.  An object is reused only if the record
    written when it was compiled (build/<variant>/<src>.o.sha256: content hash of the source, of every shared header and of the flags)
    still matches -- content, not mtime, so a snapshot copy or a checkout cannot make a stale object look fresh.  COUNTR_BUILD_FORCE=1
    (or force=True / --force) recompiles everything.  Prints how many objects were compiled."""
    force = force or os.environ.get("COUNTR_BUILD_FORCE", "0") == "1"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    shared = glob.glob(os.path.join(CSRC, "*.hpp"))
    hdrs = shared + [os.path.join(HERE, "..", "include", "countr_hip.h")]
    procs, reused, total = [], 0, 0
    links = []
    jobs = int(os.environ.get("COUNTR_BUILD_JOBS", "0")) or max(2, (os.cpu_count() or 4))
    single = dict(SINGLE, **SINGLE_LATER, **SINGLE_OVERLAY, **SINGLE_TRACKS, **SINGLE_FLOW)
    for tag, lib, extra in VARIANTS + tuple((t, lib_, None) for t, (lib_, _s, _h) in single.items()):
        bdir = os.path.join(HERE, "build", tag) if tag else os.path.join(HERE, "build")
        os.makedirs(bdir, exist_ok=True)
        objs, fresh = [], False
        for src in sources() if extra is not None else single[tag][1]():
            obj = os.path.join(bdir, os.path.basename(src) + ".o")
            objs.append(obj)
            total += 1
            if extra is None:
                cmd = [hipcc] + FLAGS + ["-c", src, "-o", obj]
            else:
                cmd = ([hipcc] + FLAGS + ["-mllvm", "-amdgpu-mfma-vgpr-form=1"] + extra
                       + EXTRA_FLAGS.get(os.path.basename(src), []) + ["-c", src, "-o", obj])
            want = _digest([src] + (hdrs if extra is not None else shared + [single[tag][2]]), " ".join(cmd[1:-3]))
            rec = obj + ".sha256"
            if not force and os.path.exists(obj) and os.path.exists(rec) and open(rec).read().strip() == want:
                reused += 1
                continue
            if os.path.exists(rec):
                os.remove(rec)
            while sum(1 for _s, _r, _w, p_ in procs if p_.poll() is None) >= jobs:      # (30 hipcc processes at once starve an 8-core box)
                import time
                time.sleep(0.2)
            if verbose:
                print(" ".join(cmd), flush=True)
            procs.append((src, rec, want, subprocess.Popen(cmd)))
            fresh = True
        links.append((lib, objs, fresh))
    for src, rec, want, p in procs:
        if p.wait() != 0:
            raise RuntimeError("hipcc failed on %s" % src)
        open(rec, "w").write(want + "\n")
    for lib, objs, fresh in links:
        lrec = lib + ".sha256"
        lwant = _digest([o + ".sha256" for o in objs])
        if fresh or not os.path.exists(lib) or not os.path.exists(lrec) or open(lrec).read().strip() != lwant:
            cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib] + objs
            if verbose:
                print(" ".join(cmd), flush=True)
            subprocess.check_call(cmd)
            open(lrec, "w").write(lwant + "\n")
    if verbose:
        print("build_mode: %s -- %d of %d objects compiled (2 libraries x %d sources + %d of the extension library + %d of the classes library + %d of the tiles library + %d of the yuv library + %d of the overlay library + %d of the tracks library + %d of the flow library), %d reused after a "
              "content-hash check (source + headers + flags)"
              % ("full" if reused == 0 else "incremental", len(procs), total, len(sources()), len(ext_sources()), len(classes_sources()), len(tiles_sources()), len(yuv_sources()), len(overlay_sources()), len(tracks_sources()), len(flow_sources()), reused), flush=True)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    print(LIB)
