"""The semi-global matcher on the device (ssba_stereo_sgbm, ssba_image_pyramid_create_stereo; ceres_slam_amd/csrc/ssba_sgbm.hip).

Reference: the numpy statement tests/sgbm_reference.py (tests/test_sgbm_reference.py pins it by known answers).  The matcher is
integer arithmetic throughout, so every bar here is bit-equality: disp16, the double map with its NaN positions, and whatever is
computed from them by code that both routes share.

Shapes: lane = disparity in the path kernel, K = ceil(D / 64) disparities per lane.  D 16 / 32 / 48 leave lanes idle, 64 is one
full wave, 80 and 128 are K = 2 (80: with idle lanes), 192 is K = 3 (the path without packed loads), 256 is K = 4; 37 x 131 has a
block wider than a third of the rows and both sides odd; 9 x 17 has one computable column; 2 rows is the least the pre-filter
can reflect (one row is refused); 12 x 200 and 12 x 330 split a row into several work-groups of the cost kernel.

End to end: the 96 x 128 triple with about 8 pixels of motion (make_stereo_triple(96, 128, seed, motion=10, min_wavelength_px=8)).
With seed 3, the seed of the coarse-to-fine case of tests/pyramid_reference.py, the numpy loop itself stalls on the matcher's map:
it ends 2.2 from the true pose (on the exact map: 6.4e-4; with exact values on the matcher's valid pixels: 4.2e-4 -- the matcher's
error of up to 0.6 px derails it, not the missing columns), so that seed can show nothing.  Seeds 10, 11, 12 end 4.3e-3, 2.9e-3 and
4.2e-3 from it (max |pose - true| over the 12 entries; 7.3e-4 ... 8.0e-4 on the exact map).  The test uses seed 10: measured
4.32e-3 with the numpy loop on the reference's map, bar 2 x that = 8.65e-3.  The factor covers what another seed changes, not
device error: the two device routes must agree to the bit."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

import image_reference as ir
import pyramid_reference as pr
import sgbm_reference as sr
from ceres_slam_amd import build, capi, synth
from ceres_slam_amd.solver import ImagePyramid, stereo_sgbm

pytestmark = pytest.mark.gpu

_u8p, _i16p = C.POINTER(C.c_uint8), C.POINTER(C.c_int16)
POSE_NUMPY, POSE_BAR = 4.324e-3, 8.65e-3


def _same_values(a, b):
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and a.dtype == b.dtype and (na == nb).all() and a[~na].tobytes() == b[~nb].tobytes()


@functools.lru_cache(maxsize=None)
def _pair(rows, cols, shift):
    """A textured 8-bit pair: smooth waves plus noise, the right image the left one moved by `shift` columns in the upper half and
    by shift + 2 in the lower half, with its own noise: winners, rivals and left-right failures all occur.  Never written."""
    rng = np.random.Generator(np.random.PCG64(rows * 1000 + cols))
    y, x = np.mgrid[0:rows, 0:cols + shift + 2]
    wide = 127.5 + 70.0 * np.sin(0.35 * x + 0.2 * y) * np.cos(0.11 * x - 0.3 * y) + rng.integers(-40, 41, x.shape)
    left = wide[:, shift + 2:]
    right = np.where(np.arange(rows)[:, None] < rows // 2, wide[:, 2:cols + 2], wide[:, :cols]) + rng.integers(-4, 5, (rows, cols))
    out = tuple(np.clip(np.rint(a), 0, 255).astype(np.uint8) for a in (left, right))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _reference(rows, cols, shift, params):
    left, right = _pair(rows, cols, shift)
    out = sr.sgbm(left, right, **dict(params))
    for a in out:
        a.setflags(write=False)
    return out


def _check(rows, cols, shift, **params):
    left, right = _pair(rows, cols, shift)
    want16, want = _reference(rows, cols, shift, tuple(sorted(params.items())))
    got16, got = stereo_sgbm(left, right, **params)
    bad = int((got16 != want16).sum())
    valid = float(np.isfinite(want[:, params.get("min_disparity", 0) + params["num_disparities"]:]).mean())
    print(f"{rows}x{cols} {params}: {bad} of {want16.size} disp16 differ; {valid:.3f} of the computable pixels valid, "
          f"{np.unique(want16).size} distinct values")
    assert got16.dtype == np.int16 and got16.tobytes() == want16.tobytes()
    assert _same_values(got, want)
    return got16, got


SHAPES = [(24, 80, 6, dict(num_disparities=16, block_size=5)),
          (37, 131, 11, dict(num_disparities=32, block_size=15)),
          (16, 48, 5, dict(num_disparities=16, block_size=1)),
          (20, 150, 23, dict(num_disparities=64, block_size=9)),
          (12, 200, 70, dict(num_disparities=128, block_size=3)),
          (12, 330, 130, dict(num_disparities=256, block_size=3)),
          (18, 120, 21, dict(num_disparities=48, block_size=7, min_disparity=4)),
          (9, 17, 3, dict(num_disparities=16, block_size=3)),
          (2, 40, 4, dict(num_disparities=16, block_size=3)),
          (10, 120, 40, dict(num_disparities=80, block_size=3)),
          (10, 250, 100, dict(num_disparities=192, block_size=5))]


@pytest.mark.parametrize("rows,cols,shift,params", SHAPES, ids=[f"{r}x{c}-D{p['num_disparities']}-b{p['block_size']}" for r, c, _, p in SHAPES])
def test_matcher_against_the_numpy_statement(rows, cols, shift, params):
    _check(rows, cols, shift, **params)


@pytest.mark.parametrize("extra", [dict(p1=8 * 25, p2=32 * 25), dict(uniqueness_ratio=10), dict(disp12_max_diff=-1), dict(disp12_max_diff=1),
                                   dict(pre_filter_cap=31), dict(p1=8 * 25, p2=32 * 25, uniqueness_ratio=10, disp12_max_diff=1, pre_filter_cap=63)],
                         ids=["p1p2", "uniqueness", "lr-off", "lr-1", "cap31", "all"])
def test_parameter_variants(extra):
    base16, _ = _check(20, 150, 23, num_disparities=64, block_size=9)
    got16, _ = _check(20, 150, 23, num_disparities=64, block_size=9, **extra)
    assert (got16 != base16).any()          # the variant changes the answer on this pair: the parameter reaches the kernels


def test_two_runs_are_bit_equal_and_either_output_may_be_null():
    left, right = _pair(37, 131, 11)
    a16, a = stereo_sgbm(left, right, num_disparities=32, block_size=15)
    b16, b = stereo_sgbm(left, right, num_disparities=32, block_size=15)
    assert a16.tobytes() == b16.tobytes() and a.tobytes() == b.tobytes()
    lib, q = capi.load(), capi.sgbm_params(num_disparities=32, block_size=15)
    only16, only = np.zeros((37, 131), np.int16), np.zeros((37, 131))
    pl, prr = left.ctypes.data_as(_u8p), right.ctypes.data_as(_u8p)
    assert lib.ssba_stereo_sgbm(pl, prr, 37, 131, C.byref(q), -1, only16.ctypes.data_as(_i16p), None) == 0
    assert lib.ssba_stereo_sgbm(pl, prr, 37, 131, C.byref(q), -1, None, capi.dptr(only)) == 0
    assert lib.ssba_stereo_sgbm(pl, prr, 37, 131, C.byref(q), -1, None, None) == 0
    assert only16.tobytes() == a16.tobytes() and _same_values(only, a)


def test_default_params_are_the_drivers():
    q = capi.sgbm_params()
    assert [getattr(q, n) for n, _ in capi.SgbmParams._fields_] == [0, 64, 15] + [0] * 8


REFUSALS = [(dict(min_disparity=-1), -1), (dict(num_disparities=0), -1), (dict(num_disparities=24), -1), (dict(num_disparities=272), -1),
            (dict(block_size=0), -1), (dict(block_size=4), -1), (dict(block_size=17), -1), (dict(uniqueness_ratio=-1), -1),
            (dict(uniqueness_ratio=101), -1), (dict(pre_filter_cap=128), -1), (dict(full_dp=1), -1), (dict(min_disparity=300), -1),
            (dict(block_size=15, p2=65535 - 20925 + 1), -1), (dict(block_size=15, pre_filter_cap=63, p2=23011), -1),
            (dict(speckle_window_size=50), -6), (dict(speckle_range=1), -6)]


def test_refusals():
    """Every refusal of the parameter check, where tests/sgbm_reference.py refuses (tests/test_sgbm_reference.py runs the same list)."""
    lib = capi.load()
    img = np.zeros((8, 300), np.uint8)
    p = img.ctypes.data_as(_u8p)
    d16, d = np.full((8, 300), 7, np.int16), np.full((8, 300), 7.0)
    out = (d16.ctypes.data_as(_i16p), capi.dptr(d))

    def refused(rc, status):
        msg = lib.ssba_last_error().decode()
        assert rc == status, (rc, status, msg)
        assert "ssba_stereo_sgbm" in msg and len(msg) > len("ssba_stereo_sgbm: ")

    for kw, status in REFUSALS:
        kw = dict(dict(num_disparities=16, block_size=3), **kw)
        with pytest.raises(sr.Unsupported if status == -6 else ValueError):
            sr.derive(8, 300, **kw)
        q = capi.sgbm_params(**kw)
        refused(lib.ssba_stereo_sgbm(p, p, 8, 300, C.byref(q), -1, *out), status)
    q = capi.sgbm_params(num_disparities=16, block_size=3)
    refused(lib.ssba_stereo_sgbm(None, p, 8, 300, C.byref(q), -1, *out), -1)
    refused(lib.ssba_stereo_sgbm(p, None, 8, 300, C.byref(q), -1, *out), -1)
    refused(lib.ssba_stereo_sgbm(p, p, 8, 300, None, -1, *out), -1)
    refused(lib.ssba_stereo_sgbm(p, p, 1, 300, C.byref(q), -1, *out), -1)              # one row cannot be reflected
    refused(lib.ssba_stereo_sgbm(p, p, 8, 16, C.byref(q), -1, *out), -1)               # no computable column
    refused(lib.ssba_stereo_sgbm(p, p, 8, 5462, C.byref(q), -1, *out), -6)             # (refused before anything is read)
    refused(lib.ssba_stereo_sgbm(p, p, 8, 300, C.byref(q), 1 << 20, *out), -1)         # no such device
    assert (d16 == 7).all() and (d == 7.0).all()                                        # a refusal writes nothing
    with pytest.raises(capi.SsbaError) as e:
        stereo_sgbm(img, img, speckle_window_size=50)
    assert e.value.status == -6
    with pytest.raises(ValueError):
        stereo_sgbm(img, img[:, :100])
    assert lib.ssba_stereo_sgbm(p, p, 8, 300, C.byref(q), -1, *out) == 0               # the refusals left the library usable
    assert (d16[:, 16:] == 0).all() and (d16[:, :16] == -16).all()


# ---- the pyramid from a stereo triple ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _triple(rows, cols, seed, motion):
    t = synth.make_stereo_triple(rows, cols, seed=seed, motion=motion, min_wavelength_px=8.0)
    for a in (t.left0, t.right0, t.left1, t.pair.pose_init, t.pair.pose_true, t.pair.disparity):
        a.setflags(write=False)
    return t


def _halved(img, level):
    for _ in range(level):
        img = pr.pyr_down(img)
    return img


@pytest.mark.parametrize("rows,cols,levels,dl,bs", [(96, 128, 3, 0, 15), (65, 131, 3, 1, 5), (64, 64, 3, 0, 7)])
def test_create_stereo_against_the_reference_on_the_pyramids_own_levels(rows, cols, levels, dl, bs):
    t = _triple(rows, cols, 3, 1.0)
    params = dict(num_disparities=16, block_size=bs)
    _, want = sr.sgbm(_halved(t.left0, dl), _halved(t.right0, dl), **params)
    for source, scale in ((capi.GRADIENT_OF_TRACKED, 0.125), (capi.GRADIENT_OF_REFERENCE, 1.0)):
        kw = dict(disparity_level=dl, gradient_source=source, gradient_scale=scale)
        got = ImagePyramid.create_stereo(t.left0, t.right0, t.left1, levels, params=params, **kw)
        fed = ImagePyramid(t.left0, t.left1, want, levels, **kw)
        d = want
        for l in range(levels):
            g, f = got.level(l), fed.level(l)
            assert g.ref_u8.shape == (rows >> l, cols >> l)
            for name in ("ref_u8", "track_u8", "ref", "track", "gradx", "grady"):
                assert getattr(g, name).tobytes() == getattr(f, name).tobytes(), (l, name)
            if l < dl:
                assert g.disparity is None
                continue
            if l > dl:
                d = pr.disparity_down(d)
            assert _same_values(g.disparity, d) and _same_values(g.disparity, f.disparity), l
        share = float(np.isfinite(want[:, 16:]).mean())
        print(f"{rows}x{cols} level {dl}: {share:.3f} of the computable pixels valid")
        assert share > 0.9


def test_create_stereo_refusals():
    t = _triple(64, 64, 3, 1.0)
    lib = capi.load()
    a, b, c = (x.ctypes.data_as(_u8p) for x in (t.left0, t.right0, t.left1))
    h = C.c_void_p()
    q = capi.sgbm_params(num_disparities=16, block_size=5)
    create = lambda *x: lib.ssba_image_pyramid_create_stereo(*x, -1, C.byref(h))

    def refused(rc, status):
        msg = lib.ssba_last_error().decode()
        assert rc == status and "ssba_image_pyramid_create_stereo" in msg and not h, (rc, status, msg)

    for args in [(None, b, c, 64, 64, 3, 0, C.byref(q), 1, 0.125), (a, None, c, 64, 64, 3, 0, C.byref(q), 1, 0.125), (a, b, None, 64, 64, 3, 0, C.byref(q), 1, 0.125),
                 (a, b, c, 64, 64, 3, 0, None, 1, 0.125), (a, b, c, 64, 64, 3, 3, C.byref(q), 1, 0.125), (a, b, c, 64, 64, 5, 0, C.byref(q), 1, 0.125),
                 (a, b, c, 64, 64, 3, 0, C.byref(q), 2, 0.125), (a, b, c, 64, 64, 3, 0, C.byref(q), 1, 0.0),
                 (a, b, c, 64, 64, 3, 2, C.byref(q), 1, 0.125)]:                         # level 2 is 16 x 16: no computable column
        refused(create(*args), -1)
    refused(create(a, b, c, 64, 64, 3, 0, C.byref(capi.sgbm_params(num_disparities=16, speckle_window_size=50)), 1, 0.125), -6)
    refused(create(a, b, c, 64, 64, 3, 0, C.byref(capi.sgbm_params(num_disparities=24)), 1, 0.125), -1)
    assert create(a, b, c, 64, 64, 3, 1, C.byref(q), 1, 0.125) == 0 and h              # 32 x 32 at level 1: 16 computable columns
    lib.ssba_image_pyramid_destroy(h)
    with pytest.raises(ValueError):
        ImagePyramid.create_stereo(t.left0, t.right0[:, :60], t.left1, 3)


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def test_raw_triple_in_pose_out():
    t = _triple(96, 128, 10, 10.0)
    params = dict(num_disparities=16, block_size=15)
    kw = dict(disparity_level=0, gradient_source=capi.GRADIENT_OF_TRACKED, gradient_scale=0.125, camera=t.pair.camera)
    o = capi.default_options(max_num_iterations=50, use_nonmonotonic_steps=1)
    # route one: the matcher on the device, the map downloaded once
    one = ImagePyramid.create_stereo(t.left0, t.right0, t.left1, 3, params=params, **kw)
    map1 = one.level(0).disparity
    pose1 = t.pair.pose_init.copy()
    rc1, sums1 = one.align(pose1, map1, coarsest_level=2, disparity_const=True, options=o)
    # route two: the reference's map through ssba_image_pyramid_create
    _, want = sr.sgbm(t.left0, t.right0, **params)
    assert _same_values(map1, want)
    map2 = want.copy()
    two = ImagePyramid(t.left0, t.left1, map2, 3, **kw)
    pose2 = t.pair.pose_init.copy()
    rc2, sums2 = two.align(pose2, map2, coarsest_level=2, disparity_const=True, options=o)
    dist = float(np.abs(pose1 - t.pair.pose_true).max())
    print(f"pose {dist:.3e} from the true one (numpy loop on the reference's map: {POSE_NUMPY:.3e}, bar {POSE_BAR:.3e}); levels: "
          + ", ".join(f"{x.initial_cost:.4f} -> {x.final_cost:.4f} ({x.num_iterations - 1})" for x in sums1))
    assert rc1 == rc2 == 0 and len(sums1) == len(sums2) == 3
    assert pose1.tobytes() == pose2.tobytes()
    for x, y in zip(sums1, sums2):
        for name in ("termination_type", "num_iterations", "num_successful_steps", "num_unsuccessful_steps", "initial_cost", "final_cost"):
            assert getattr(x, name) == getattr(y, name), name
    assert dist <= POSE_BAR


def test_sgbm_example_matches_the_python_result(tmp_path):
    """examples/dense_stereo_sgbm_gpu.cpp reads the raw triple the test writes: no disparity map.  Same library, same calls."""
    exe = build.build_examples("dense_stereo_sgbm_gpu")
    t = _triple(96, 128, 10, 10.0)
    q = capi.sgbm_params(num_disparities=16, block_size=15)
    raw = tmp_path / "triple.raw"
    with open(raw, "wb") as f:
        f.write(np.array([96, 128, 3, 0, ir.BILINEAR, 1, capi.GRADIENT_OF_TRACKED], np.int32).tobytes())
        f.write(np.array([0.125] + [t.pair.camera[k] for k in ("fu", "fv", "cu", "cv", "b")]).tobytes())
        f.write(t.pair.pose_init.tobytes())
        f.write(bytes(q))
        f.write(t.left0.tobytes() + t.right0.tobytes() + t.left1.tobytes())
    r = subprocess.run([exe, str(raw), "--coarse-to-fine", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    out = dict(ln.split(" ", 1) for ln in lines if not ln.startswith("level "))
    pyr = ImagePyramid.create_stereo(t.left0, t.right0, t.left1, 3, params=dict(num_disparities=16, block_size=15), disparity_level=0,
                                     gradient_source=capi.GRADIENT_OF_TRACKED, gradient_scale=0.125, camera=t.pair.camera)
    disp = pyr.level(0).disparity
    pose = t.pair.pose_init.copy()
    rc, sums = pyr.align(pose, disp, coarsest_level=2, interpolation=ir.BILINEAR, disparity_const=True)
    got = np.array([float(x) for x in out["pose"].split()])
    valid = int((np.isfinite(disp) & (disp > 0)).sum())
    print(f"example: valid {out['valid']} (python {valid}); {out['report']}; max |pose - python| = {np.abs(got - pose).max():.2e}")
    assert rc == 0 and int(out["valid"]) == valid == int(out["blocks"])
    assert [ln.split(" ", 2)[1] for ln in lines if ln.startswith("level ")] == ["2", "1", "0"]
    assert got.tobytes() == pose.tobytes()
