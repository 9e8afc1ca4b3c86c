"""CPU-side checks of the stereo-sequence entry points (ssba_stereo_sgbm_batch, ssba_image_sequence_create, _pyramid, _destroy):
the example and tests/host/image_sequence_shim_check.cpp build against the shim; the four C calls judge their arguments before they
look for a device, so the shim's ImageSequence and the batched StereoSGBM throw std::invalid_argument where the C call refuses
without a GPU; with valid arguments and no GPU the calls report SSBA_ERR_NO_DEVICE -- there is no CPU fallback."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from ceres_slam_amd import build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_u8p = C.POINTER(C.c_uint8)
NEW = ["ssba_stereo_sgbm_batch", "ssba_image_sequence_create", "ssba_image_sequence_pyramid", "ssba_image_sequence_destroy"]


def test_the_sequence_driver_compiles_against_the_shim():
    assert os.path.exists(build.build_examples("dense_stereo_sequence_gpu"))
    src = open(os.path.join(ROOT, "examples", "dense_stereo_sequence_gpu.cpp")).read()
    assert "--sequence" in src and "ceres_slam::ImageSequence" in src


def test_refusals_of_the_shim(tmp_path):
    lib = build.build_library()
    exe = str(tmp_path / "image_sequence_shim_check")
    cmd = ["g++", "-std=c++11", "-O1", "-g", "-Wall", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "host", "image_sequence_shim_check.cpp"), "-o", exe, "-L" + os.path.dirname(lib), "-lssba",
           "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all refusals hold" in r.stdout and "FAIL" not in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_the_header_declares_74_names_and_the_binding_lists_them():
    hdr = open(os.path.join(ROOT, "include", "ssba.h")).read()
    declared = set(re.findall(r"\b(ssba_[a-z_0-9]+)\s*\(", hdr)) - {"ssba_exchange_fn"}
    assert len(declared) == 74 and declared == set(capi.SYMBOLS) and len(capi.SYMBOLS) == 74
    assert set(NEW) <= declared
    lib = capi.load()
    for name in NEW:
        assert hasattr(lib, name), name
    assert capi.SGBM_DEFAULT_WORKSPACE_BYTES == 1 << 30 and "SSBA_SGBM_DEFAULT_WORKSPACE_BYTES (1ull << 30)" in hdr


def test_the_c_calls_refuse_before_they_need_a_device(torch_sees_a_gpu):
    lib = capi.load()
    stack = np.zeros((3, 40, 64), np.uint8)
    p = stack.ctypes.data_as(_u8p)
    h = C.c_void_p()
    q = capi.sgbm_params(num_disparities=16, block_size=5)
    need = capi.sgbm_pair_bytes(40, 64, 16)
    assert need == 12 * 40 * 48 * 16

    def batch(*a):
        rc = lib.ssba_stereo_sgbm_batch(*a, None, None)
        return rc, lib.ssba_last_error().decode()

    def create(*a):
        rc = lib.ssba_image_sequence_create(*a, -1, C.byref(h))
        assert rc != 0 and not h
        return rc, lib.ssba_last_error().decode()

    for bad, status in ((dict(num_disparities=24), -1), (dict(block_size=2), -1), (dict(min_disparity=-1), -1), (dict(full_dp=1), -1),
                        (dict(uniqueness_ratio=101), -1), (dict(pre_filter_cap=128), -1), (dict(speckle_window_size=50), -6),
                        (dict(speckle_range=2), -6), (dict(min_disparity=50), -1)):
        b = capi.sgbm_params(**dict(dict(num_disparities=16, block_size=5), **bad))
        rc, msg = batch(p, p, 3, 40, 64, C.byref(b), 0, -1)
        assert rc == status and "ssba_stereo_sgbm_batch: " in msg, (bad, rc, msg)
        rc, msg = create(p, p, 3, 40, 64, 2, 0, C.byref(b), 0, 1, 0.125)
        assert rc == status and "ssba_image_sequence_create: " in msg, (bad, rc, msg)
    for args, word in [((None, p, 3, 40, 64, C.byref(q), 0, -1), "NULL"), ((p, None, 3, 40, 64, C.byref(q), 0, -1), "NULL"),
                       ((p, p, 3, 40, 64, None, 0, -1), "NULL"), ((p, p, 0, 40, 64, C.byref(q), 0, -1), "n = 0"),
                       ((p, p, 3, 1, 64, C.byref(q), 0, -1), "rows"), ((p, p, 3, 40, 16, C.byref(q), 0, -1), "computable"),
                       ((p, p, 3, 40, 64, C.byref(q), need - 1, -1), str(need))]:
        rc, msg = batch(*args)
        assert rc == -1 and "ssba_stereo_sgbm_batch: " in msg and word in msg, (rc, msg, word)
    rc, msg = batch(p, p, 3, 8, 5462, C.byref(q), 0, -1)
    assert rc == -6 and "ssba_stereo_sgbm_batch: " in msg
    for args, word in [((None, p, 3, 40, 64, 2, 0, C.byref(q), 0, 1, 0.125), "NULL"), ((p, None, 3, 40, 64, 2, 0, C.byref(q), 0, 1, 0.125), "NULL"),
                       ((p, p, 3, 40, 64, 2, 0, None, 0, 1, 0.125), "NULL"), ((p, p, 1, 40, 64, 2, 0, C.byref(q), 0, 1, 0.125), "2 frames"),
                       ((p, p, 0, 40, 64, 2, 0, C.byref(q), 0, 1, 0.125), "2 frames"), ((p, p, 3, 40, 64, 0, 0, C.byref(q), 0, 1, 0.125), "levels"),
                       ((p, p, 3, 40, 64, 2, 2, C.byref(q), 0, 1, 0.125), "disparity_level"), ((p, p, 3, 40, 64, 4, 0, C.byref(q), 0, 1, 0.125), "8 rows"),
                       ((p, p, 3, 40, 64, 2, 0, C.byref(q), 0, 2, 0.125), "gradient source"), ((p, p, 3, 40, 64, 2, 0, C.byref(q), 0, 1, 0.0), "gradient_scale"),
                       ((p, p, 3, 40, 32, 2, 1, C.byref(q), 0, 1, 0.125), "computable"),                  # level 1 is 20 x 16
                       ((p, p, 3, 40, 64, 2, 0, C.byref(q), need - 1, 1, 0.125), str(need))]:
        rc, msg = create(*args)
        assert rc == -1 and "ssba_image_sequence_create: " in msg and word in msg, (rc, msg, word)
    assert lib.ssba_image_sequence_create(p, p, 3, 40, 64, 2, 0, C.byref(q), 0, 1, 0.125, -1, None) == -1
    pyr = C.c_void_p()
    assert lib.ssba_image_sequence_pyramid(None, 0, C.byref(pyr)) == -1 and "ssba_image_sequence_pyramid: " in lib.ssba_last_error().decode()
    assert lib.ssba_image_sequence_destroy(None) == -1 and "ssba_image_sequence_destroy: " in lib.ssba_last_error().decode()
    if not torch_sees_a_gpu:
        assert batch(p, p, 3, 40, 64, C.byref(q), 0, -1)[0] == -5
        assert create(p, p, 3, 40, 64, 2, 0, C.byref(q), 0, 1, 0.125)[0] == -5
