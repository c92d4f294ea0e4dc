"""In-tree build of the HIP library (hipcc cross-compiles gfx950 without a GPU)."""
import os
import shutil
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_DIR = os.path.join(_HERE, "_lib")
LIB = os.path.join(LIB_DIR, "libslslam_hip.so")
SOURCES = ["lba_api.hip", "lba_stream.hip", "lba_host_util.hip", "lba_pack.cpp", "po_api.hip", "ransac_api.hip", "frame_api.hip", "match_api.hip", "triangulate_api.hip", "place_api.hip", "voctree_train_api.hip", "descriptor_api.hip", "line_descriptor_api.hip", "line_detect_api.hip", "stereo_api.hip", "track_api.hip", "rectify_api.hip",
           os.path.join("..", "host", "place_filter.cpp"),      # (the place recogniser's Bayes filter: host C++, exported with the rest)
           os.path.join("..", "host", "voctree_host.cpp")]      # (the tree trainer's host half: keys, centres, partition, save)
HEADERS = sorted(f for f in os.listdir(CSRC) if f.endswith(".h")) + [os.path.join("..", "..", "include", "slslam_hip.h"), os.path.join("..", "host", "place_filter.h"), os.path.join("..", "host", "voctree_host.h")]   # every header: a new one must not leave a stale library behind
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-munsafe-fp-atomics"]


def _stale(lib=LIB):
    if not os.path.exists(lib):
        return True
    t = os.path.getmtime(lib)
    for f in SOURCES + HEADERS:
        p = os.path.join(CSRC, f)
        if os.path.exists(p) and os.path.getmtime(p) > t:
            return True
    return False


def _compile(lib, flags, force, verbose):
    if not force and not _stale(lib):
        return lib
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    os.makedirs(LIB_DIR, exist_ok=True)
    cmd = [hipcc] + FLAGS + list(flags) + [os.path.join(CSRC, s) for s in SOURCES] + ["-o", lib]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return lib


def build_lib(force=False, verbose=False):
    """Compile every HIP translation unit for gfx950 into slslam_amd/_lib/libslslam_hip.so."""
    return _compile(LIB, [], force, verbose)


def build_variant(name, flags, force=False, verbose=False):
    """The same sources with extra compiler flags (the timing builds of tools/: -DSLSLAM_K1_TIMING=1, ...) as a library of its own,
    slslam_amd/_lib/libslslam_hip.<name>.so; the product library is never touched.  Returns the path (for SLSLAM_HIP_LIBRARY).
    The name stands for the flags: one name, one set of flags."""
    return _compile(os.path.join(LIB_DIR, "libslslam_hip.%s.so" % name), flags, force, verbose)


if __name__ == "__main__":
    print(build_lib(force=True, verbose=True))
