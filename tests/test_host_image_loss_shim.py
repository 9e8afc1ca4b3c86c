"""The loss of ImageError blocks in the C++ shim (include/ceres_slam_amd/ceres_shim.hpp): tests/host/image_loss_shim_check.cpp
holds the cases (ImageError::Create takes a trailing huber_a, two widths in one problem throw, one width on every block does
not).  Every case ends before the back end is called, so the program runs without a device."""
import os
import subprocess

from ceres_slam_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_image_error_loss_width_of_the_shim(tmp_path):
    lib = build.build_library()
    exe = str(tmp_path / "image_loss_shim_check")
    cmd = ["g++", "-std=c++11", "-O1", "-g", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "host", "image_loss_shim_check.cpp"),
           "-o", exe, "-L" + os.path.dirname(lib), "-lssba", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all loss checks hold" in r.stdout and "FAIL" not in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
