"""ssba_covariance_blocks on a machine without a GPU: the request struct, the header, the export and the shim example."""
import ctypes
import os
import re
import subprocess

from ceres_slam_amd import build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_request_struct_is_16_bytes():
    assert ctypes.sizeof(capi.CovBlock) == 16
    assert (capi.COV_POSE, capi.COV_POINT) == (0, 1)


def test_symbol_is_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ssba.h")).read()
    assert re.search(r"SSBA_API int ssba_covariance_blocks\(ssba_problem \*p, const ssba_cov_block \*blocks, uint64_t num, double \*out\);", hdr)
    assert "#define SSBA_COV_POSE 0" in hdr and "#define SSBA_COV_POINT 1" in hdr
    assert "ssba_covariance_blocks" in capi.SYMBOLS
    lib = build.build_library()
    out = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, check=True).stdout.decode()
    assert re.search(r"\bT ssba_covariance_blocks\b", out)


def test_example_compiles():
    exe = build.build_examples("covariance_blocks_gpu")
    assert os.path.exists(exe) and os.access(exe, os.X_OK)
