"""Numpy statement of the dense driver's pre-processing (tests/dense_stereo_test.cpp:52-72 of the reference), the truth for
ceres_slam_amd/csrc/ssba_image_pyramid.hip.  Written from the rules include/ssba.h states, independently of the kernels: index
tables for the reflected border, integer sums for the halving, numpy's own left-to-right float64 arithmetic for the gradients.
OpenCV is not available where the tests run, so tests/test_pyramid_reference.py pins this file by known answers.

    halving     dst[y][x] = (sum_{i,j=-2..2} w_i w_j src[2y+i][2x+j] + 128) >> 8,  w = [1 4 6 4 1], BORDER_REFLECT_101,
                size floor(rows / 2) x floor(cols / 2), each level from the rounded 8-bit level above
    conversion  I = u8 * (1 / 255)
    gradients   3 x 3 Sobel, BORDER_REFLECT_101, times scale, summed as ceres_slam_amd.synth.sobel sums
    disparity   d_{l+1}[y][x] = d_l[2y][2x] / 2
    camera      fu, fv, cu, cv over 2^l; b unchanged

coarse_to_fine is the route a user has without the device pyramid: these functions, then tests/image_reference.py per level."""
import functools

import numpy as np

import image_reference as ir

OF_REFERENCE, OF_TRACKED = 0, 1
W = np.array([1, 4, 6, 4, 1], dtype=np.int64)


def reflect_101(i, n):
    """BORDER_REFLECT_101 index: -1 -> 1, -2 -> 2, n -> n - 2, n + 1 -> n - 3."""
    i = np.asarray(i, dtype=np.int64)
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * n - 2 - i, i)


def pyr_down(src):
    """cv::pyrDown(src, dst, Size(cols / 2, rows / 2)) on CV_8U."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 2
    rows, cols = src.shape
    s = src.astype(np.int64)
    ys = reflect_101(2 * np.arange(rows // 2)[:, None] + np.arange(-2, 3)[None, :], rows)        # (rows/2, 5)
    xs = reflect_101(2 * np.arange(cols // 2)[:, None] + np.arange(-2, 3)[None, :], cols)        # (cols/2, 5)
    horiz = (s[:, xs] * W).sum(axis=2)                   # (rows, cols/2)
    total = (horiz[ys, :] * W[None, :, None]).sum(axis=1)   # (rows/2, cols/2)
    return ((total + 128) >> 8).astype(np.uint8)


def convert(u8):
    """convertTo(CV_64F, 1. / 255.): one multiplication by the rounded constant."""
    return np.asarray(u8).astype(np.float64) * (1.0 / 255.0)


def sobel(img, scale):
    """cv::Sobel(img, out, -1, 1, 0) / (..., 0, 1) times scale; border BORDER_REFLECT_101; the summation order of synth.sobel."""
    img = np.asarray(img, dtype=np.float64)
    rows, cols = img.shape
    y, x = np.arange(rows), np.arange(cols)
    ym, yp, xm, xp = reflect_101(y - 1, rows), reflect_101(y + 1, rows), reflect_101(x - 1, cols), reflect_101(x + 1, cols)
    at = lambda yy, xx: img[yy[:, None], xx[None, :]]
    gx = (at(ym, xp) - at(ym, xm)) + 2.0 * (at(y, xp) - at(y, xm)) + (at(yp, xp) - at(yp, xm))
    gy = (at(yp, xm) - at(ym, xm)) + 2.0 * (at(yp, x) - at(ym, x)) + (at(yp, xp) - at(ym, xp))
    return scale * gx, scale * gy


def disparity_down(d):
    """d_{l+1}[y][x] = d_l[2y][2x] / 2 on floor(rows / 2) x floor(cols / 2); NaN, +-inf, 0 and negative entries stay invalid."""
    d = np.asarray(d, dtype=np.float64)
    rows, cols = d.shape
    return d[0:2 * (rows // 2):2, 0:2 * (cols // 2):2] / 2.0


def level_camera(cam, level):
    s = 0.5 ** level
    return dict(fu=cam["fu"] * s, fv=cam["fv"] * s, cu=cam["cu"] * s, cv=cam["cv"] * s, b=cam["b"])


def build(ref_u8, track_u8, disparity, levels, disparity_level, gradient_source, gradient_scale):
    """A list of dicts, one per level: ref_u8, track_u8, ref, track, gradx, grady, disparity (None below disparity_level)."""
    out = []
    u8 = [np.asarray(ref_u8), np.asarray(track_u8)]
    disp = None
    for l in range(levels):
        if l > 0:
            u8 = [pyr_down(a) for a in u8]
        if l == disparity_level:
            disp = np.array(disparity, dtype=np.float64)
            assert disp.shape == u8[0].shape
        elif l > disparity_level:
            disp = disparity_down(disp)
        ref, track = convert(u8[0]), convert(u8[1])
        gx, gy = sobel(track if gradient_source == OF_TRACKED else ref, gradient_scale)
        out.append(dict(ref_u8=u8[0], track_u8=u8[1], ref=ref, track=track, gradx=gx, grady=gy, disparity=None if disp is None else disp.copy()))
    return out


def quantise(img):
    """An image in [0, 1] as the 8-bit image a file holds: clipped and rounded."""
    return np.rint(np.clip(np.asarray(img, dtype=np.float64), 0.0, 1.0) * 255.0).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def case_96x128():
    """The coarse-to-fine case of the tests: 96 x 128, a motion of about 8 pixels, the pair clipped and rounded to 8 bit, the exact
    disparity map at level 0, three levels, gradient of the tracked image at 1/8.  (pair, ref_u8, track_u8, levels); shared and
    never written."""
    from ceres_slam_amd import synth
    pair = synth.make_image_pair(96, 128, seed=3, motion=10.0, min_wavelength_px=8.0)
    ref_u8, track_u8 = quantise(pair.ref), quantise(pair.track)
    levels = build(ref_u8, track_u8, pair.disparity, 3, 0, OF_TRACKED, 0.125)
    for a in [ref_u8, track_u8, pair.disparity, pair.pose_init, pair.pose_true] + [v for L in levels for v in L.values() if v is not None]:
        a.setflags(write=False)
    return pair, ref_u8, track_u8, levels


@functools.lru_cache(maxsize=None)
def case_96x128_solved(coarsest):
    """coarse_to_fine on the case from `coarsest` down to level 0, constant disparities, 50 iterations per level."""
    pair, _, _, levels = case_96x128()
    return coarse_to_fine(levels, pair.camera, pair.pose_init, coarsest, 0, max_iter=50)


def coarse_to_fine(levels, cam0, pose0, coarsest, base, interp=ir.BILINEAR, disp_const=True, max_iter=50):
    """The numpy route: image_reference's loop on levels coarsest ... base of `levels` (build's result), the pose carried down.
    Levels above `base` hold their disparities constant; the base level follows disp_const.  Returns (pose, base disparity,
    [log per level])."""
    T = np.asarray(pose0, dtype=np.float64).copy()
    logs, d = [], levels[base]["disparity"]
    for l in range(coarsest, base - 1, -1):
        L = levels[l]
        pr = ir.ImageProblem(level_camera(cam0, l), L["ref"], L["track"], L["gradx"], L["grady"], L["disparity"], interp,
                             disp_const=True if l > base else disp_const)
        T, d, log = pr.solve(T, L["disparity"], max_iter=max_iter)
        logs.append(log)
    return T, d, logs
