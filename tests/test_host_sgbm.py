"""CPU-side checks of the semi-global matcher's entry points: the example builds against the shim; ssba_stereo_sgbm and
ssba_image_pyramid_create_stereo judge their arguments before they look for a device, so the shim's StereoSGBM and its ImagePyramid
constructor for a stereo triple throw std::invalid_argument where the C call refuses (tests/host/sgbm_shim_check.cpp holds the
cases) without a GPU; with valid arguments and no GPU the calls report SSBA_ERR_NO_DEVICE -- there is no CPU fallback."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from ceres_slam_amd import build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_u8p = C.POINTER(C.c_uint8)


def test_the_sgbm_driver_compiles_against_the_shim():
    assert os.path.exists(build.build_examples("dense_stereo_sgbm_gpu"))


def test_refusals_of_the_shim(tmp_path):
    lib = build.build_library()
    exe = str(tmp_path / "sgbm_shim_check")
    cmd = ["g++", "-std=c++11", "-O1", "-g", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "host", "sgbm_shim_check.cpp"),
           "-o", exe, "-L" + os.path.dirname(lib), "-lssba", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all refusals hold" in r.stdout and "FAIL" not in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_the_c_calls_refuse_before_they_need_a_device(torch_sees_a_gpu):
    lib = capi.load()
    img = np.zeros((40, 64), np.uint8)
    p = img.ctypes.data_as(_u8p)
    h = C.c_void_p()
    q = capi.sgbm_params(num_disparities=16, block_size=5)
    assert [getattr(capi.sgbm_params(), n) for n, _ in capi.SgbmParams._fields_] == [0, 64, 15] + [0] * 8
    for bad, status in ((dict(num_disparities=24), -1), (dict(block_size=2), -1), (dict(min_disparity=-1), -1), (dict(full_dp=1), -1),
                        (dict(speckle_window_size=50), -6), (dict(min_disparity=50), -1)):
        b = capi.sgbm_params(**dict(dict(num_disparities=16, block_size=5), **bad))
        assert lib.ssba_stereo_sgbm(p, p, 40, 64, C.byref(b), -1, None, None) == status, bad
        assert "ssba_stereo_sgbm" in lib.ssba_last_error().decode()
        assert lib.ssba_image_pyramid_create_stereo(p, p, p, 40, 64, 2, 0, C.byref(b), 1, 0.125, -1, C.byref(h)) == status and not h, bad
        assert "ssba_image_pyramid_create_stereo" in lib.ssba_last_error().decode()
    assert lib.ssba_stereo_sgbm(None, p, 40, 64, C.byref(q), -1, None, None) == -1
    assert lib.ssba_stereo_sgbm(p, p, 40, 64, None, -1, None, None) == -1
    assert lib.ssba_stereo_sgbm(p, p, 1, 64, C.byref(q), -1, None, None) == -1
    assert lib.ssba_image_pyramid_create_stereo(p, None, p, 40, 64, 2, 0, C.byref(q), 1, 0.125, -1, C.byref(h)) == -1
    assert lib.ssba_image_pyramid_create_stereo(p, p, p, 40, 64, 2, 0, C.byref(q), 1, 0.125, -1, None) == -1
    assert lib.ssba_image_pyramid_create_stereo(p, p, p, 40, 32, 2, 1, C.byref(q), 1, 0.125, -1, C.byref(h)) == -1      # level 1 is 20 x 16: no computable column
    lib.ssba_sgbm_default_params(None)                                                                                # tolerated
    if not torch_sees_a_gpu:
        assert lib.ssba_stereo_sgbm(p, p, 40, 64, C.byref(q), -1, None, None) == -5
        assert lib.ssba_image_pyramid_create_stereo(p, p, p, 40, 64, 2, 0, C.byref(q), 1, 0.125, -1, C.byref(h)) == -5 and not h


def test_the_python_wrappers_check_shapes_before_the_library_sees_them():
    from ceres_slam_amd.solver import ImagePyramid, stereo_sgbm
    a = np.zeros((40, 64), np.uint8)
    with pytest.raises(ValueError):
        stereo_sgbm(a, a.astype(np.float64))
    with pytest.raises(ValueError):
        stereo_sgbm(a, a[:, :60])
    with pytest.raises(ValueError):
        ImagePyramid.create_stereo(a, a[:30], a, 2)
    with pytest.raises(AttributeError):
        stereo_sgbm(a, a, no_such_parameter=1)
