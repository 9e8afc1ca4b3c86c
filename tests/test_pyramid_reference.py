"""Pins tests/pyramid_reference.py, the numpy statement of the dense driver's pre-processing (include/ssba.h, "the driver's
pre-processing"), by known answers: OpenCV cannot run where the tests do.  The answers follow from the rules alone: the 5 x 5
kernel is the outer product of [1 4 6 4 1] (sum 256), so a constant and a linear ramp pass unchanged, and a single 255 spreads
as (255 w_i w_j + 128) >> 8.

The last test records the case the device tests use (tests/test_gpu_image_pyramid.py): at 96 x 128 with a motion of about 8 pixels
one level does not converge, three levels do."""
import numpy as np
import pytest

import image_reference as ir
import pyramid_reference as pr


def test_a_constant_image_halves_to_the_same_constant():
    for c in (0, 1, 127, 254, 255):
        out = pr.pyr_down(np.full((13, 18), c, np.uint8))
        assert out.shape == (6, 9) and (out == c).all()


def test_an_integer_ramp_halves_to_its_value_at_even_pixels_where_no_reflection_is_involved():
    rows, cols = 21, 30
    y, x = np.mgrid[0:rows, 0:cols]
    ramp = (3 * x + 5 * y + 7).astype(np.uint8)
    assert int((3 * x + 5 * y + 7).max()) <= 255
    out = pr.pyr_down(ramp)
    assert out.shape == (10, 15)
    # destination (y, x) reads source rows 2y-2 .. 2y+2 and columns 2x-2 .. 2x+2
    ys = [v for v in range(10) if 2 * v - 2 >= 0 and 2 * v + 2 <= rows - 1]
    xs = [u for u in range(15) if 2 * u - 2 >= 0 and 2 * u + 2 <= cols - 1]
    assert ys == list(range(1, 10)) and xs == list(range(1, 14))
    assert (out[np.ix_(ys, xs)] == ramp[::2, ::2][np.ix_(ys, xs)]).all()
    assert out[0, 0] != ramp[0, 0]          # the reflected corner is not the ramp


def _impulse(rows, cols, y, x):
    a = np.zeros((rows, cols), np.uint8)
    a[y, x] = 255
    return pr.pyr_down(a)


def test_a_single_255_at_an_interior_even_pixel():
    out = _impulse(20, 24, 8, 10)
    want = np.zeros_like(out)
    want[4, 5] = 36
    want[3, 5] = want[5, 5] = want[4, 4] = want[4, 6] = 6
    want[3, 4] = want[3, 6] = want[5, 4] = want[5, 6] = 1
    assert (out == want).all()


def test_a_single_255_at_an_interior_odd_column():
    out = _impulse(20, 24, 8, 11)
    assert out[4, 5] == 24 and out[4, 6] == 24
    assert out[3, 5] == 4 and out[5, 6] == 4          # (255 * 4 * 4 + 128) >> 8
    assert out.sum() == 2 * 24 + 4 * 4


def test_a_single_255_at_column_1_meets_the_reflected_border():
    out = _impulse(20, 24, 8, 1)
    assert out[4, 0] == 48          # weights 4 + 4 on source column 1 (once directly, once as the mirror of column -1), times 6
    assert out[4, 1] == 24          # destination column 1 reads source columns 0 .. 4: weight 4 on column 1, times 6
    out = _impulse(20, 24, 8, 22)   # the far side: destination column 11 reads 20 .. 24, column 24 is the mirror of column 22
    assert out[4, 11] == ((255 * (6 + 1) * 6 + 128) >> 8)
    out = _impulse(20, 25, 8, 23)   # odd width: destination column 11 reads 20 .. 24, all inside
    assert out[4, 11] == 24


def test_the_reflected_index():
    assert pr.reflect_101([-2, -1, 0, 5, 9, 10, 11], 10).tolist() == [2, 1, 0, 5, 9, 8, 7]


def test_conversion_is_one_multiplication():
    u8 = np.arange(256, dtype=np.uint8).reshape(16, 16)
    k = 1.0 / 255.0
    assert pr.convert(u8).tobytes() == (u8.astype(np.float64) * k).tobytes()
    assert (pr.convert(u8) != u8.astype(np.float64) / 255.0).any()      # ... which is not the division


@pytest.mark.parametrize("scale", [1.0, 0.125])
def test_sobel_of_a_ramp(scale):
    rows, cols = 9, 12
    y, x = np.mgrid[0:rows, 0:cols]
    a, b = 3.0, -2.0
    gx, gy = pr.sobel(a * x + b * y + 11.0, scale)
    assert (gx[:, 1:-1] == 8 * a * scale).all() and (gy[1:-1, :] == 8 * b * scale).all()
    assert (gx[:, 0] == 0).all() and (gx[:, -1] == 0).all() and (gy[0, :] == 0).all() and (gy[-1, :] == 0).all()


def test_sobel_is_synth_sobel():
    from ceres_slam_amd import synth
    rng = np.random.Generator(np.random.PCG64(0))
    img = rng.random((11, 14))
    for scale in (1.0, 0.125):
        gx, gy = pr.sobel(img, scale)
        sx, sy = synth.sobel(img, scale)
        assert gx.tobytes() == sx.tobytes() and gy.tobytes() == sy.tobytes()


def test_the_disparity_rule():
    d = np.arange(1, 36, dtype=np.float64).reshape(5, 7)
    d[0, 0], d[0, 2], d[2, 0], d[2, 2], d[2, 4] = np.nan, 0.0, -3.0, np.inf, -np.inf
    out = pr.disparity_down(d)
    assert out.shape == (2, 3)
    assert np.isnan(out[0, 0]) and out[0, 1] == 0.0 and out[0, 2] == d[0, 4] / 2
    assert out[1, 0] == -1.5 and out[1, 1] == np.inf and out[1, 2] == -np.inf
    usable = lambda m: np.isfinite(m) & (m > 0)
    assert (usable(out) == usable(d[0:4:2, 0:6:2])).all()


def test_the_level_camera():
    cam = dict(fu=700.0, fv=710.0, cu=301.5, cv=120.25, b=0.54)
    c2 = pr.level_camera(cam, 2)
    assert c2 == dict(fu=175.0, fv=177.5, cu=75.375, cv=30.0625, b=0.54)
    assert pr.level_camera(cam, 0) == cam


def test_build_halves_the_rounded_level_and_places_the_disparity():
    rng = np.random.Generator(np.random.PCG64(1))
    a, b = rng.integers(0, 256, (37, 50), dtype=np.uint8), rng.integers(0, 256, (37, 50), dtype=np.uint8)
    d1 = rng.random((18, 25)) + 0.5
    lv = pr.build(a, b, d1, 3, 1, pr.OF_REFERENCE, 1.0)
    assert [L["ref_u8"].shape for L in lv] == [(37, 50), (18, 25), (9, 12)]
    assert (lv[2]["track_u8"] == pr.pyr_down(pr.pyr_down(b))).all()
    assert lv[0]["disparity"] is None and lv[1]["disparity"].tobytes() == d1.tobytes() and (lv[2]["disparity"] == d1[0:18:2, 0:24:2] / 2).all()
    gx, _ = pr.sobel(pr.convert(lv[1]["ref_u8"]), 1.0)
    assert lv[1]["gradx"].tobytes() == gx.tobytes()
    lt = pr.build(a, b, d1, 3, 1, pr.OF_TRACKED, 1.0)
    assert lt[1]["gradx"].tobytes() == pr.sobel(pr.convert(lv[1]["track_u8"]), 1.0)[0].tobytes()


def test_one_level_does_not_converge_from_eight_pixels_and_three_levels_do():
    """96 x 128, seed=3, motion=10.0, min_wavelength_px=8.0, 8-bit images, BILINEAR, gradient of the tracked image at 0.125, constant
    disparities, 50 iterations per level, non-monotonic steps.  Measured: one level ends at cost 142.46 from 215.54, 1.8 from the
    true translation; levels 2 -> 1 -> 0 end at cost 0.2125, 6.4e-4 / 8.6e-5 from the true translation / rotation."""
    pair, _, _, levels = pr.case_96x128()
    T1, _, logs1 = pr.case_96x128_solved(0)
    T3, _, logs3 = pr.case_96x128_solved(2)
    cost1, cost3 = min(float(c) for c, _ in logs1[-1]), min(float(c) for c, _ in logs3[-1])
    dt1, dt3 = np.linalg.norm(T1[:3] - pair.pose_true[:3]), np.linalg.norm(T3[:3] - pair.pose_true[:3])
    dr3 = np.abs(T3[3:] - pair.pose_true[3:]).max()
    print(f"one level: cost {float(logs1[0][0][0]):.2f} -> {cost1:.2f}, {dt1:.2f} from the true translation; three levels: cost {cost3:.4f}, "
          f"{dt3:.1e} / {dr3:.1e} from the true translation / rotation")
    assert len(logs3) == 3
    assert cost1 > 10.0 and dt1 > 0.5
    assert dt3 <= 2e-3 and dr3 <= 2e-3 and np.abs(T3 - pair.pose_true).max() <= 2e-3
