"""CPU-side checks of the image-pyramid entry points: the example builds against the shim, and ssba_image_pyramid_create judges
its arguments before it looks for a device, so its refusals (status and a message that names the call) hold without a GPU; with
valid arguments and no GPU the call reports SSBA_ERR_NO_DEVICE like ssba_create -- there is no CPU fallback."""
import ctypes as C
import os

import numpy as np

from ceres_slam_amd import build, capi

_u8p = C.POINTER(C.c_uint8)


def test_the_pyramid_driver_compiles_against_the_shim():
    assert os.path.exists(build.build_examples("dense_stereo_pyramid_gpu"))


def test_create_refuses_bad_arguments_before_it_needs_a_device(torch_sees_a_gpu):
    lib = capi.load()
    a, b, d = np.zeros((37, 50), np.uint8), np.zeros((37, 50), np.uint8), np.ones((18, 25))
    pa, pb, pd = a.ctypes.data_as(_u8p), b.ctypes.data_as(_u8p), capi.dptr(d)
    h = C.c_void_p()
    for args in [(None, pb, pd, 37, 50, 3, 1, 1, 1.0), (pa, None, pd, 37, 50, 3, 1, 1, 1.0), (pa, pb, None, 37, 50, 3, 1, 1, 1.0),
                 (pa, pb, pd, 37, 50, 0, 0, 1, 1.0), (pa, pb, pd, 37, 50, 3, 3, 1, 1.0), (pa, pb, pd, 37, 50, 3, 1, 7, 1.0),
                 (pa, pb, pd, 37, 50, 3, 1, 1, 0.0), (pa, pb, pd, 37, 50, 3, 1, 1, float("nan")), (pa, pb, pd, 37, 50, 4, 1, 1, 1.0),
                 (pa, pb, pd, 37, 50, 40, 1, 1, 1.0)]:
        assert lib.ssba_image_pyramid_create(*args, -1, C.byref(h)) == -1, args
        assert "ssba_image_pyramid_create" in lib.ssba_last_error().decode() and not h
    assert lib.ssba_image_pyramid_create(pa, pb, pd, 37, 50, 3, 1, 1, 1.0, -1, None) == -1
    if not torch_sees_a_gpu:
        assert lib.ssba_image_pyramid_create(pa, pb, pd, 37, 50, 3, 1, 1, 1.0, -1, C.byref(h)) == -5 and not h
    # NULL handles are refused by name
    for name, rc in (("ssba_image_pyramid_destroy", lib.ssba_image_pyramid_destroy(None)),
                     ("ssba_image_pyramid_level", lib.ssba_image_pyramid_level(None, 0, None, None, None, None, None, None, None, None, None)),
                     ("ssba_image_pyramid_align", lib.ssba_image_pyramid_align(None, None, None, None, 0, 1, 1, None, None))):
        assert rc == -1, name


def test_the_python_wrapper_checks_shapes_before_the_library_sees_them():
    import pytest
    from ceres_slam_amd.solver import ImagePyramid
    a = np.zeros((37, 50), np.uint8)
    with pytest.raises(ValueError):
        ImagePyramid(a, a.astype(np.float64), np.ones((37, 50)), 2)
    with pytest.raises(ValueError):
        ImagePyramid(a, a, np.ones((37, 50)), 2, disparity_level=1)
