"""What ceres::SolveBatch of the C++ shim (include/ceres_slam_amd/ceres_shim.hpp) refuses: tests/host/image_batch_shim_check.cpp
holds the cases (an empty vector, a NULL entry, the same problem twice, a problem with stereo blocks, DOGLEG).  Every case throws
std::invalid_argument before the back end is called, so the program runs without a device."""
import os
import subprocess

from ceres_slam_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_solve_batch_refusals_of_the_shim(tmp_path):
    lib = build.build_library()
    exe = str(tmp_path / "image_batch_shim_check")
    cmd = ["g++", "-std=c++11", "-O1", "-g", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "host", "image_batch_shim_check.cpp"),
           "-o", exe, "-L" + os.path.dirname(lib), "-lssba", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all refusals hold" in r.stdout and "FAIL" not in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
