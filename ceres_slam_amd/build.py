"""Builds the HIP library in-tree: hipcc --offload-arch=gfx950 -> ceres_slam_amd/libssba.so.

hipcc cross-compiles for gfx950 without a GPU, so this runs on the CPU-only build box;
the resulting .so travels to the GPU box with the repo snapshot.
"""
from __future__ import annotations

import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libssba.so")
SOURCES = ["ssba_api.hip", "ssba_kernels.hip", "ssba_bcr.hip", "ssba_bcr_mfma.hip", "ssba_phong.hip", "ssba_phong_solver.hip", "ssba_border.hip", "ssba_frontend.hip", "ssba_dense.hip", "ssba_pool.hip", "ssba_wide.hip", "ssba_wide_covariance.hip", "ssba_covariance.hip", "ssba_image.hip", "ssba_image_pyramid.hip", "ssba_sgbm.hip", "ssba_wide_layout.cpp", "ssba_layout.cpp"]
HEADERS = ["ssba_types.h", "ssba_wide_device.h", "ssba_wide_layout.h", "ssba_pool.h", "ssba_launch.h", "ssba_device.h", "ssba_phong_device.h", "ssba_linesearch.h", "ssba_posefactor_device.h", "ssba_check.h", "ssba_solve6.h", "ssba_align3.h", "ssba_image_pyramid.h", "ssba_sgbm.h", "libssba.map", os.path.join("..", "..", "include", "ssba.h")]
# -fvisibility=hidden + the version script below: the dynamic symbol table of libssba.so holds the entry points of
# include/ssba.h (SSBA_API) and nothing else -- no unprefixed helpers, no ssba:: C++ symbols next to torch's RCCL or user code
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-fvisibility-inlines-hidden", "-Wall", "-Wno-unused-function", *os.environ.get("SSBA_EXTRA_FLAGS", "").split(),
         "-Wno-unused-value", "-Wno-unused-variable", "-Wno-unused-result"]


# per-file flags: the factor kernel's accumulator tiles are also VALU operands (pivot rows, row scaling), so the matrix
# instructions take them from the architectural registers instead of bouncing them through v_accvgpr_read / _write
FILE_FLAGS = {"ssba_bcr_mfma.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form"]}

# libssba_tracks.so (include/ssba_tracks.h): the feature tracker, a library of its own with its own version script.  It compiles
# the pool in once more (its buffers and streams are its own); the objects carry the library's prefix so the two builds never
# share a file.
TRACKS_LIB = os.path.join(HERE, "libssba_tracks.so")
TRACKS_SOURCES = ["ssba_tracks.hip", "ssba_pool.hip"]
TRACKS_HEADERS = ["ssba_pool.h", "ssba_brief_pattern.h", "ssba_align3.h", "ssba_solve6.h", "ssba_device.h", "ssba_types.h", "ssba_tracks_odometry.h", "libssba_tracks.map", os.path.join("..", "..", "include", "ssba.h"),
                  os.path.join("..", "..", "include", "ssba_tracks.h")]


def _stale(lib: str = LIB, sources=None, headers=None) -> bool:
    if not os.path.exists(lib):
        return True
    t = os.path.getmtime(lib)
    deps = [os.path.join(CSRC, s) for s in (SOURCES if sources is None else sources) + (HEADERS if headers is None else headers)] + [os.path.abspath(__file__)]
    return any(os.path.getmtime(d) > t for d in deps if os.path.exists(d))


def build_library(force: bool = False, verbose: bool = False) -> str:
    """libssba.so, and libssba_tracks.so next to it (build_tracks_library): every route that builds the project builds both."""
    build_tracks_library(force, verbose)
    if not force and not _stale():
        return LIB
    return _compile_and_link(LIB, SOURCES, "libssba.map", "", verbose)


def build_tracks_library(force: bool = False, verbose: bool = False) -> str:
    if not force and not _stale(TRACKS_LIB, TRACKS_SOURCES, TRACKS_HEADERS):
        return TRACKS_LIB
    return _compile_and_link(TRACKS_LIB, TRACKS_SOURCES, "libssba_tracks.map", "tracks_", verbose)


def _compile_and_link(lib: str, sources, version_script: str, obj_prefix: str, verbose: bool) -> str:
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objs = []
    procs = []
    for s in sources:
        obj = os.path.join(CSRC, obj_prefix + os.path.splitext(s)[0] + ".o")
        cmd = [hipcc, *[f for f in FLAGS if f], *FILE_FLAGS.get(s, []), "-c", os.path.join(CSRC, s), "-o", obj]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        procs.append((cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
        objs.append(obj)
    for cmd, pr in procs:
        out, _ = pr.communicate()
        if pr.returncode != 0:
            raise RuntimeError("hipcc failed:\n" + " ".join(cmd) + "\n" + out.decode(errors="replace"))
        if verbose and out:
            print(out.decode(errors="replace"), file=sys.stderr)
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,--version-script=" + os.path.join(CSRC, version_script), "-o", lib, *objs]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0:
        raise RuntimeError("link failed:\n" + r.stdout.decode(errors="replace"))
    return lib


def build_examples(name: str = "dataset_vo_gpu", extra_library: str = "") -> str:
    """C++ drivers written against the Ceres-shaped shim (include/ceres_slam_amd/ceres_shim.hpp):
    dataset_vo_gpu (tests/dataset_vo.cpp), dataset_ba_phong_gpu (tests/dataset_ba_phong.cpp) and dataset_vo_sun_gpu
    (tests/dataset_vo_sun.cpp).  extra_library: one more library of this package to link, by its -l name ("ssba_tracks")."""
    root = os.path.dirname(HERE)
    src = os.path.join(root, "examples", name + ".cpp")
    out = os.path.join(root, "examples", name)
    build_library()
    inc = os.path.join(root, "include", "ceres_slam_amd")
    deps = [src, os.path.join(root, "include", "ssba.h"), LIB] + [os.path.join(inc, h) for h in sorted(os.listdir(inc)) if h.endswith(".hpp")]
    if extra_library:
        deps += [os.path.join(HERE, "lib" + extra_library + ".so"), os.path.join(root, "include", extra_library + ".h")]
    if os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in deps):
        return out
    cmd = ["g++", "-std=c++11", "-O2", "-Wall", "-I" + os.path.join(root, "include"), src, "-o", out,
           "-L" + HERE, *(["-l" + extra_library] if extra_library else []), "-lssba", "-Wl,-rpath,$ORIGIN/../ceres_slam_amd", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0:
        raise RuntimeError("g++ failed:\n" + r.stdout.decode(errors="replace"))
    return out


if __name__ == "__main__":
    print(build_library(force="--force" in sys.argv, verbose=True))
    print(TRACKS_LIB)
