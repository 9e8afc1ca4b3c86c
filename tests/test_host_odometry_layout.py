"""Relative-pose blocks between neighbouring free poses stay on the windowed layout (the host phase of ssba_finalize,
ceres_slam_amd/csrc/ssba_layout.cpp).  tests/host/odometry_layout_check.cpp holds the cases: a chain over two super-block
boundaries, blocks that must still take the general layout, pairs made consecutive by a constant pose.  Built and run like
tests/test_host_layout.py: g++ with -fsanitize=address,undefined and once with -fsanitize=thread, the binary run directly."""
import os
import subprocess

import pytest

from test_host_layout import CSRC, ROOT, _run


@pytest.mark.parametrize("san", ["address,undefined", "thread"])
def test_odometry_blocks_keep_the_windowed_layout(tmp_path, san):
    exe = str(tmp_path / ("odometry_layout_check_" + san.replace(",", "_")))
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=" + san, "-fno-sanitize-recover=all", "-pthread", "-I" + CSRC,
           os.path.join(ROOT, "tests", "host", "odometry_layout_check.cpp"), os.path.join(CSRC, "ssba_layout.cpp"), os.path.join(CSRC, "ssba_wide_layout.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = _run(exe, san, 300)
    assert r.returncode == 0 and "all invariants hold" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
