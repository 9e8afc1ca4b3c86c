"""Constant point blocks in the host phase of ssba_finalize (ceres_slam_amd/csrc/ssba_layout.cpp): the flag bit in the landmark
masks, an unchanged layout around it, every observation present exactly once with its own values (the cost-only blocks of a
constant point on a constant pose among them), and the combinations that are refused.  tests/host/const_points_check.cpp holds
the cases; built and run like tests/test_host_layout.py: g++ with -fsanitize=address,undefined, the binary run directly."""
import os
import subprocess

from test_host_layout import CSRC, ROOT, _run


def test_constant_point_flags_under_sanitizers(tmp_path):
    san = "address,undefined"
    exe = str(tmp_path / "const_points_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=" + san, "-fno-sanitize-recover=all", "-pthread", "-I" + CSRC,
           os.path.join(ROOT, "tests", "host", "const_points_check.cpp"), os.path.join(CSRC, "ssba_layout.cpp"), os.path.join(CSRC, "ssba_wide_layout.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = _run(exe, san, 300)
    assert r.returncode == 0 and "all invariants hold" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
