"""tests/sgbm_reference.py, the numpy statement of the semi-global matcher, pinned by known answers and structural checks (no GPU;
OpenCV is not available where the tests run, so bit parity with cv::StereoSGBM is unpinned).

The rendered plane (test 9): synth.make_stereo_triple(rows, cols, seed=3, min_wavelength_px=8), the matcher's default parameters
but for D and the block size, against the exact map of the render on the computable columns.  Measured with this file's
reference (seed 3), and the worst of seeds 10 ... 19:

    shape      D   block   valid of computable   within 1 px       within 0.25 px    median error
    24 x 80    16    5     0.9798 (0.9753)       0.9967 (0.9854)   0.9654 (0.9265)   0.064 px
    37 x 131   32   15     0.9760 (0.9741)       1.0000 (0.9967)   0.9874 (0.9599)   0.043 px
    96 x 128   16   15     0.9781 (0.9758)       1.0000 (0.9924)   0.9967 (0.9691)   0.044 px

Each bar is the measured share minus what the ten further seeds lose at worst, i.e. the worst seed's share, rounded down to four
digits.  The invalid 2 % are the first computable columns, whose match lies left of what the right image shows in common."""
import numpy as np
import pytest

import sgbm_reference as sr
from ceres_slam_amd import synth


def test_constant_pair_is_valid_at_the_first_disparity():
    img = np.full((9, 40), 77, np.uint8)
    for min_d in (0, 3):
        d16, d = sr.sgbm(img, img, min_disparity=min_d, num_disparities=16, block_size=3)
        maxD = min_d + 16
        assert d16.dtype == np.int16 and d.dtype == np.float64
        assert (d16[:, maxD:] == 16 * min_d).all() and (d[:, maxD:] == min_d).all()
        assert (d16[:, :maxD] == (min_d - 1) * 16).all() and np.isnan(d[:, :maxD]).all()


def test_integer_shift_is_found():
    rng = np.random.Generator(np.random.PCG64(1))
    k, D, bs = 5, 16, 5
    left = rng.integers(0, 256, (20, 80)).astype(np.uint8)
    right = np.roll(left, -k, axis=1)                 # right[x - k] = left[x]; the last k columns wrap around
    d16, _ = sr.sgbm(left, right, num_disparities=D, block_size=bs)
    m = bs // 2 + 2
    inner = d16[m:-m, D + m:80 - k - m].astype(np.int64)
    print("offsets from 16 k:", np.unique(inner - 16 * k))
    assert (inner >> 4 == k).all() and (np.abs(inner - 16 * k) <= 8).all()


def test_birchfield_tomasi_by_hand():
    A, B = np.array([[10, 20, 14]]), np.array([[40, 33, 30]])
    # a = 10 at column 0: a- = (10 + 10) / 2 = 10 (the neighbour clamped), a+ = (10 + 20) / 2 = 15: [10, 15]
    # b = 33 at column 1: b- = (33 + 40) / 2 = 36 and b+ = (33 + 30) / 2 = 31, both floored: [31, 36]
    # c0 = max(0, 10 - 36, 31 - 10) = 21, c1 = max(0, 33 - 15, 10 - 33) = 18
    lo, hi = sr.half_sample_range(A)
    assert lo.tolist() == [[10, 15, 14]] and hi.tolist() == [[15, 20, 17]]
    lo, hi = sr.half_sample_range(B)
    assert lo.tolist() == [[36, 31, 30]] and hi.tolist() == [[40, 36, 31]]
    assert sr.birchfield_tomasi(A, B, np.array([0]), np.array([1])).tolist() == [[18]]
    assert sr.birchfield_tomasi(B, A, np.array([1]), np.array([0])).tolist() == [[18]]      # symmetric
    assert sr.birchfield_tomasi(A, A, np.array([0, 1, 2]), np.array([0, 1, 2])).tolist() == [[0, 0, 0]]


def test_prefilter_by_hand():
    img = np.array([[0, 10, 50, 20], [5, 5, 5, 200], [9, 8, 7, 6]], np.uint8)
    # row 0 reflects to row 1 above: g[0][1] = (5 - 5) + 2 (50 - 0) + (5 - 5) = 100 -> capped at 15 -> 30
    # g[1][2] = (20 - 10) + 2 (200 - 5) + (6 - 8) -> 30;  g[2][1] = (5 - 5) + 2 (7 - 9) + (5 - 5) = -4 -> 11
    # g[2][2] = (200 - 5) + 2 (6 - 8) + (200 - 5) -> 30;  g[0][2] = (200 - 5) + 2 (20 - 10) + (200 - 5) -> 30
    P = sr.prefilter(img, 15)
    assert P[:, 0].tolist() == [15, 15, 15] and P[:, 3].tolist() == [15, 15, 15]
    assert P[:, 1:3].tolist() == [[30, 30], [15 + min(15, (50 - 0) + 2 * 0 + (7 - 9)), 30], [11, 30]]
    assert sr.prefilter(img, 63)[2, 1] == 63 - 4


def test_the_sub_pixel_division_truncates():
    assert sr.trunc_div(-7, 2) == -3 and -7 // 2 == -4
    assert sr.trunc_div(7, 2) == 3 and sr.trunc_div(-8, 2) == -4
    S = np.full((1, 1, 16), 1000)
    S[0, 0, 4:7] = [6, 5, 20]       # den = 6 + 20 - 10 = 16, numerator (6 - 20) 16 + 16 = -208, / 32 = -6.5 -> -6 (floor: -7)
    d16, d = sr.from_volume(S, 17, 0, 0, -1)
    assert d16[0, 16] == 16 * 5 - 6 and d[0, 16] == (16 * 5 - 6) / 16.0
    S[0, 0, 4:7] = [20, 5, 6]       # numerator (20 - 6) 16 + 16 = 240, / 32 = 7.5 -> 7
    assert sr.from_volume(S, 17, 0, 0, -1)[0][0, 16] == 16 * 5 + 7
    S[0, 0, :] = 1000
    S[0, 0, 0], S[0, 0, 1] = 5, 900     # the first disparity: no sub-pixel step
    assert sr.from_volume(S, 17, 0, 0, -1)[0][0, 16] == 0
    S[0, 0, :] = 1000
    S[0, 0, 15], S[0, 0, 14] = 5, 900   # the last one
    assert sr.from_volume(S, 17, 0, 0, -1)[0][0, 16] == 16 * 15


def _scalar_paths(C, P1, P2):
    """One Python loop per path and pixel, written from the recursion and not from the vectorised code."""
    rows, W, D = C.shape
    out = []
    for dx, dy in sr.PATHS:
        L = np.zeros((rows, W, D), dtype=np.int64)
        order = [(y, x) for y in range(rows) for x in (range(W) if dx <= 0 else range(W - 1, -1, -1))]
        for y, x in order:
            qx, qy = x + dx, y + dy
            for d in range(D):
                if qx < 0 or qx >= W or qy < 0:
                    L[y, x, d] = C[y, x, d]
                    continue
                q = L[qy, qx]
                m = int(q.min())
                cands = [int(q[d]), m + P2]
                if d > 0:
                    cands.append(int(q[d - 1]) + P1)
                if d < D - 1:
                    cands.append(int(q[d + 1]) + P1)
                L[y, x, d] = C[y, x, d] + min(cands) - m
        out.append(L)
    return out


def test_path_recursion_against_a_scalar_loop():
    rng = np.random.Generator(np.random.PCG64(2))
    C = rng.integers(0, 400, (6, 20, 16))
    for P1, P2 in ((2, 5), (40, 160)):
        got, want = sr.path_costs(C, P1, P2), _scalar_paths(C, P1, P2)
        for q in range(5):
            assert (got[q] == want[q]).all(), sr.PATHS[q]
    assert (got[2][1:, 0] == C[1:, 0]).all() and (got[4][1:, -1] == C[1:, -1]).all()       # diagonals that start on a side edge
    assert (got[2][0] == C[0]).all() and (got[3][0] == C[0]).all() and not (got[3][1] == C[1]).all()


def _claims(cost_16, cost_17):
    """One row, W = 4, D = 16, cols = 20: x = 16 wins at d = 2 and x = 17 at d = 3, both claim right column 14."""
    S = np.full((1, 4, 16), 100)
    S[0, 0, 2], S[0, 1, 3], S[0, 2, 0], S[0, 3, 0] = cost_16, cost_17, 10, 10
    return S


def test_left_right_rule():
    nan = np.isnan
    # equal cost: the scan runs right to left and replaces only on strictly smaller cost, so x = 17 keeps the column
    d16, d = sr.from_volume(_claims(10, 10), 20, 0, 0, 0)
    assert d16[0, 16:].tolist() == [-16, 48, 0, 0] and nan(d[0, 16]) and d[0, 17] == 3.0
    # x = 16 cheaper: it takes the column and x = 17 fails
    assert sr.from_volume(_claims(9, 10), 20, 0, 0, 0)[0][0, 16:].tolist() == [32, -16, 0, 0]
    # a difference of one passes at disp12_max_diff = 1; a negative value switches the check off
    assert sr.from_volume(_claims(10, 10), 20, 0, 0, 1)[0][0, 16:].tolist() == [32, 48, 0, 0]
    assert sr.from_volume(_claims(10, 10), 20, 0, 0, -1)[0][0, 16:].tolist() == [32, 48, 0, 0]
    # a winner that fails uniqueness claims nothing: x = 17 gets a rival, x = 16 then keeps column 14 and passes
    S = _claims(10, 10)
    S[0, 1, 9] = 10
    assert sr.from_volume(S, 20, 0, 10, 0)[0][0, 16:].tolist() == [32, -16, 0, 0]
    assert sr.from_volume(S, 20, 0, 0, 0)[0][0, 16:].tolist() == [-16, 48, 0, 0]        # ratio 0: an equal cost is no rival


def test_uniqueness():
    S = np.full((1, 1, 16), 1000)
    S[0, 0, 3], S[0, 0, 8] = 100, 105
    for uniq, valid in ((0, True), (4, True), (5, False), (10, False)):      # 105 (100 - u) < 100 * 100  <=>  u > 4.76
        d16, _ = sr.from_volume(S, 17, 0, uniq, -1)
        assert (d16[0, 16] == 48) == valid and (d16[0, 16] == -16) == (not valid), uniq
    S[0, 0, 8], S[0, 0, 4] = 1000, 100        # a neighbour of the winner is no rival (1000 * 50 >= 100 * 100 for the rest)
    assert sr.from_volume(S, 17, 0, 50, -1)[0][0, 16] >> 4 == 3
    S[0, 0, 5] = 100                          # two away is one
    assert sr.from_volume(S, 17, 0, 1, -1)[0][0, 16] == -16


@pytest.mark.parametrize("kw,exc", [
    (dict(min_disparity=-1), ValueError), (dict(num_disparities=0), ValueError), (dict(num_disparities=24), ValueError),
    (dict(num_disparities=272), ValueError), (dict(block_size=0), ValueError), (dict(block_size=4), ValueError), (dict(block_size=17), ValueError),
    (dict(uniqueness_ratio=-1), ValueError), (dict(uniqueness_ratio=101), ValueError), (dict(pre_filter_cap=128), ValueError),
    (dict(full_dp=1), ValueError), (dict(min_disparity=300), ValueError), (dict(block_size=15, p2=65535 - 20925 + 1), ValueError),
    (dict(block_size=15, pre_filter_cap=63, p2=23011), ValueError),      # (2 * 63 + 63) * 225 = 42525
    (dict(speckle_window_size=50), sr.Unsupported), (dict(speckle_range=1), sr.Unsupported)])
def test_every_refusal(kw, exc):
    img = np.zeros((8, 300), np.uint8)
    with pytest.raises(exc):
        sr.sgbm(img, img, **dict(dict(num_disparities=16, block_size=3), **kw))
    if exc is sr.Unsupported:
        assert issubclass(exc, ValueError)


def test_refusals_of_the_shape_and_what_is_just_allowed():
    img = np.zeros((8, 300), np.uint8)
    with pytest.raises(ValueError):
        sr.sgbm(img[:1], img[:1], num_disparities=16, block_size=3)            # one row cannot be reflected
    with pytest.raises(ValueError):
        sr.sgbm(img[:, :16], img[:, :16], num_disparities=16, block_size=3)      # no computable column
    with pytest.raises(ValueError):
        sr.sgbm(img, img.astype(np.int16), num_disparities=16)
    with pytest.raises(ValueError):
        sr.derive(8, 2100, min_disparity=2047 - 15, num_disparities=16)         # maxD = 2048
    with pytest.raises(sr.Unsupported):
        sr.derive(8, 5462, num_disparities=16)
    with pytest.raises(sr.Unsupported):
        sr.derive(4000, 5000, num_disparities=256)
    assert sr.derive(8, 5461, num_disparities=16)["W"] == 5461 - 16
    assert sr.derive(2, 17, num_disparities=16, block_size=15, p2=65535 - 20925)["P2"] == 44610
    k = sr.derive(8, 300)
    assert (k["D"], k["r"], k["cap"], k["P1"], k["P2"], k["uniq"], k["lr"]) == (64, 7, 15, 2, 5, 0, 0)
    assert sr.derive(8, 300, p1=7, p2=3, pre_filter_cap=32)["P2"] == 8 and sr.derive(8, 300, pre_filter_cap=32)["cap"] == 33
    assert sr.sgbm(img[:2, :17], img[:2, :17], num_disparities=16, block_size=3)[0].shape == (2, 17)


# valid of computable, within 1 px, within 0.25 px: the worst of seeds 10 ... 19 (the docstring's table)
PLANE = {(24, 80, 16, 5): (0.9753, 0.9854, 0.9265), (37, 131, 32, 15): (0.9741, 0.9967, 0.9599), (96, 128, 16, 15): (0.9758, 0.9924, 0.9691)}


@pytest.mark.parametrize("rows,cols,D,bs", list(PLANE))
def test_rendered_plane(rows, cols, D, bs):
    t = synth.make_stereo_triple(rows, cols, seed=3, min_wavelength_px=8.0)
    d16, d = sr.sgbm(t.left0, t.right0, num_disparities=D, block_size=bs)
    got, exact = d[:, D:], t.pair.disparity[:, D:]
    ok = np.isfinite(got)
    err = np.abs(got[ok] - exact[ok])
    shares = (ok.mean(), (err <= 1.0).mean(), (err <= 0.25).mean())
    print(f"{rows}x{cols} D {D} block {bs}: valid {shares[0]:.4f}, within 1 px {shares[1]:.4f}, within 0.25 px {shares[2]:.4f}, median {np.median(err):.3f} px; "
          f"bars {PLANE[rows, cols, D, bs]}")
    assert np.isnan(d[:, :D]).all() and (d16[:, :D] == -16).all()
    assert ((d16 == -16) == np.isnan(d)).all()
    for share, bar in zip(shares, PLANE[rows, cols, D, bs]):
        assert share >= bar


def test_the_triple_is_the_pair_quantised_and_the_right_view_is_shifted_by_the_disparity():
    t = synth.make_stereo_triple(24, 80, seed=3, motion=2.0, min_wavelength_px=8.0)
    pair = synth.make_image_pair(24, 80, seed=3, motion=2.0, min_wavelength_px=8.0)
    assert t.pair.ref.tobytes() == pair.ref.tobytes() and t.pair.track.tobytes() == pair.track.tobytes()
    assert t.pair.disparity.tobytes() == pair.disparity.tobytes() and t.pair.pose_true.tobytes() == pair.pose_true.tobytes()
    q = lambda a: np.rint(np.clip(a, 0.0, 1.0) * 255.0).astype(np.uint8)
    assert (t.left0 == q(pair.ref)).all() and (t.left1 == q(pair.track)).all() and t.right0.dtype == np.uint8
    # u_right = u - d: sampling the right image at u - d (linear interpolation) gives back the left image up to the rounding
    v, u = np.mgrid[0:24, 20:80]
    x = u - pair.disparity[v, u]
    x0 = np.floor(x).astype(int)
    w = x - x0
    back = (1 - w) * t.right0[v, x0] + w * t.right0[v, x0 + 1]
    assert np.abs(back - t.left0[v, u].astype(float)).max() <= 4.0
