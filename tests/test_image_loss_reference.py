"""CPU checks of the numpy statement of the ImageError blocks under ceres::HuberLoss (tests/image_loss_reference.py), the truth of
tests/test_gpu_image_loss.py: the corrected rows against central differences of sqrt(rho)-scaled residuals, rho and the
corrector at known values (|r| = a exactly), the step against the dense damped normal equations of the corrected Jacobian, the
float64 statement against numpy.longdouble, and what the loss is for: the pose error under an occluder."""
import functools

import numpy as np
import pytest

from ceres_slam_amd import synth

import image_reference as ir
import image_loss_reference as ilr

OCCLUDER_SEEDS = (0, 1, 10)
OCCLUDER_A, OCCLUDER_FRACTION = 0.02, 0.10


def _ramp_problem(a, rows=24, cols=32):
    """test_image_reference's ramp (bilinear sampling is exact on it) with a width that corrects about half of the rows."""
    gx, gy = 0.013, -0.021
    v, u = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing="ij")
    track = 0.2 + gx * u + gy * v
    rng = np.random.Generator(np.random.PCG64(3))
    ref = rng.random((rows, cols))
    cam = dict(fu=0.6 * cols, fv=0.55 * cols, cu=0.5 * (cols - 1), cv=0.5 * (rows - 1), b=0.54)
    disp = 1.0 + rng.random((rows, cols))
    T = synth.pose_pack(np.array([0.03, -0.02, 0.05]), synth.so3_exp(np.array([0.01, -0.02, 0.015])))
    pr = ilr.ImageLossProblem(cam, ref, track, np.full((rows, cols), gx), np.full((rows, cols), gy), disp, ir.BILINEAR, huber_a=a)
    return pr, T, disp


def test_corrected_rows_equal_central_differences_of_sqrt_rho_scaled_residuals():
    """Ceres' corrector with rho'' <= 0 leaves the Gauss-Newton model of f = sign(r) sqrt(rho(r^2)) up to the second-order term
    it drops: J~ = sqrt(rho') J while df/dx = rho' r / sqrt(rho) J.  Both are checked: J~ against sqrt(rho') times the central
    difference of the raw residual, and the gradient J~ r~ = rho' r J against the central difference of 1/2 rho, which is what
    the minimiser relies on."""
    a = 0.3
    pr, T, disp = _ramp_problem(a)
    raw_r, raw_Jp, raw_Jd, inb = pr.raw_rows(T, disp)
    r, Jp, Jd, inb2 = pr.rows(T, disp)
    assert (inb == inb2).all()
    big = raw_r * raw_r > a * a
    assert 0.25 < big[inb].mean() < 0.9 and pr.min_loss_margin > 1e-5        # both branches, none at the branch point
    h = 1e-6
    keep = inb.copy()
    num_p, num_rho_p = np.zeros_like(Jp), np.zeros_like(Jp)
    for c in range(6):
        e = np.zeros(6)
        e[c] = h
        Tp, Tm = ir.se3_plus(T, e, np.float64), ir.se3_plus(T, -e, np.float64)
        (rp, _), (rm, _) = pr.residuals(Tp, disp), pr.residuals(Tm, disp)
        keep &= pr.raw_rows(Tp, disp)[3] & pr.raw_rows(Tm, disp)[3]
        num_p[:, c] = (rp - rm) / (2 * h)
        num_rho_p[:, c] = (ilr.half_rho(rp, a, np.float64) - ilr.half_rho(rm, a, np.float64)) / (2 * h)
    (rp, _), (rm, _) = pr.residuals(T, disp + h), pr.residuals(T, disp - h)
    keep &= pr.raw_rows(T, disp + h)[3] & pr.raw_rows(T, disp - h)[3]
    num_d = (rp - rm) / (2 * h)
    num_rho_d = (ilr.half_rho(rp, a, np.float64) - ilr.half_rho(rm, a, np.float64)) / (2 * h)
    sc = ilr.corrector_scale(raw_r, a, np.float64)                              # sqrt(rho')
    assert keep.sum() > 0.5 * keep.size and (big & keep).sum() > 50 and (~big & keep).sum() > 50
    ep, ed = np.abs(Jp - sc[:, None] * num_p)[keep].max(), np.abs(Jd - sc * num_d)[keep].max()
    gp, gd = np.abs(Jp * r[:, None] - num_rho_p)[keep].max(), np.abs(Jd * r - num_rho_d)[keep].max()
    er = np.abs(r - sc * raw_r).max()
    print(f"ramp, a = {a}: |J~_pose - sqrt(rho') dr/dx| {ep:.3e}, |J~_disp - ..| {ed:.3e}, |J~^T r~ - d(rho/2)/dx| pose {gp:.3e} disp {gd:.3e}")
    assert ep <= 1e-6 and ed <= 1e-6 and gp <= 1e-6 and gd <= 1e-6 and er == 0.0
    # r~^2 = a |r| on corrected rows; out of bounds: exact zeros
    assert np.abs(r[big] ** 2 - a * np.abs(raw_r[big])).max() <= 1e-15
    assert not r[~inb].any() and not Jp[~inb].any() and not Jd[~inb].any()


def _dyadic(a):
    """ref = 0, track = 0.25 everywhere: every in-bounds residual is exactly 0.25; gradient images of ones."""
    rows, cols = 6, 8
    cam = dict(fu=4.0, fv=4.0, cu=3.5, cv=2.5, b=0.5)
    one = np.ones((rows, cols))
    pr = ilr.ImageLossProblem(cam, 0.0 * one, 0.25 * one, one, one, 2.0 * one, ir.BILINEAR, disp_const=True, huber_a=a)
    T = synth.pose_pack(np.zeros(3), np.eye(3))
    return pr, T, 2.0 * one


def test_rho_and_the_corrector_at_known_values():
    # |r| = a exactly: r^2 > a^2 is false, the block is uncorrected and costs 1/2 * 0.0625
    pr, T, disp = _dyadic(0.25)
    raw = pr.raw_rows(T, disp)
    r, Jp, Jd, inb = pr.rows(T, disp)
    n = int(inb.sum())
    assert n > 0 and (~inb).sum() > 0 and (raw[0][inb] == 0.25).all()
    assert r.tobytes() == raw[0].tobytes() and Jp.tobytes() == raw[1].tobytes() and Jd.tobytes() == raw[2].tobytes()
    assert pr.lm_step(T, disp, 1e4)["cost"] == n * 0.5 * 0.0625 and pr.residuals(T, disp)[1] == n * 0.5 * 0.0625
    assert pr.min_loss_margin == 0.0
    # one ulp below: the Huber formula applies
    a = np.nextafter(0.25, 0.0)
    pr, T, disp = _dyadic(a)
    r, Jp, Jd, inb = pr.rows(T, disp)
    sc = np.sqrt(a / 0.25)
    assert sc < 1.0 and (r[inb] == sc * 0.25).all() and (Jp[inb] == sc * raw[1][inb]).all() and not r[~inb].any()
    assert pr.lm_step(T, disp, 1e4)["cost"] == n * 0.5 * (2 * a * 0.25 - a * a)
    # plain values: a = 0.1
    for x, want_rho, want_sc in ((0.05, 0.0025, 1.0), (-0.1, 0.01, 1.0), (0.4, 2 * 0.1 * 0.4 - 0.01, 0.5), (-1.6, 2 * 0.1 * 1.6 - 0.01, 0.25)):
        assert abs(2 * ilr.half_rho(np.array([x]), 0.1, np.float64)[0] - want_rho) <= 1e-16
        assert abs(ilr.corrector_scale(np.array([x]), 0.1, np.float64)[0] - want_sc) <= 1e-16
    # a huge residual: sc^2 = a / |r| underflows to DBL_MIN, not to 0
    with np.errstate(over="ignore"):
        assert ilr.corrector_scale(np.array([1e308]), 1e-308, np.float64)[0] == np.sqrt(ilr.DBL_MIN)
    # a <= 0 is the NULL loss, bit for bit
    pair = synth.make_image_pair(12, 16, seed=1, invalid_fraction=0.1)
    args = (pair.camera, pair.ref, pair.track, pair.gradx, pair.grady, pair.disparity, ir.BILINEAR)
    s0, s1 = ir.ImageProblem(*args).lm_step(pair.pose_init, pair.disparity, 3.0), ilr.ImageLossProblem(*args, huber_a=0.0).lm_step(pair.pose_init, pair.disparity, 3.0)
    for k in ("cost", "r", "Jp", "Jd", "S", "rhs", "dp", "dd", "mcc"):
        assert np.asarray(s0[k]).tobytes() == np.asarray(s1[k]).tobytes(), k


@pytest.mark.parametrize("const", [False, True], ids=["free", "const"])
def test_the_step_equals_the_dense_normal_equations_of_the_corrected_jacobian(const):
    pair = synth.occlude_tracked(synth.make_image_pair(12, 16, seed=1, invalid_fraction=0.1), 0.10, 1)
    a = 0.02
    pr = ilr.ImageLossProblem(pair.camera, pair.ref, pair.track, pair.gradx, pair.grady, pair.disparity, ir.BILINEAR, disp_const=const, huber_a=a)
    st = pr.lm_step(pair.pose_init, pair.disparity, 3.0)
    raw_r, raw_Jp, raw_Jd, inb = pr.raw_rows(pair.pose_init, pair.disparity)
    big = raw_r * raw_r > a * a
    assert 0.05 < big.mean() < 0.95
    sc = np.where(big, np.sqrt(a / np.maximum(np.abs(raw_r), 1e-300)), 1.0)      # the corrector, restated
    n = pr.blk.shape[0]
    m = 6 if const else 6 + n
    J = np.zeros((n, m))
    J[:, :6] = raw_Jp * sc[:, None]
    if not const:
        J[np.arange(n), 6 + np.arange(n)] = raw_Jd * sc
    rt = raw_r * sc
    s = np.concatenate(st["scale"])[:m]
    D = np.clip((J * J).sum(0) * s * s, 1e-6, 1e32) / (3.0 * s * s)
    delta = np.linalg.solve(J.T @ J + np.diag(D), -J.T @ rt)
    assert np.abs(delta[:6] - st["dp"]).max() <= 1e-10 * np.abs(delta[:6]).max()
    if const:
        assert not st["dd"].any()
    else:
        assert np.abs(delta[6:] - st["dd"]).max() <= 1e-10 * np.abs(delta[6:]).max()
    Jd = J @ delta
    assert abs(-(Jd * (rt + Jd / 2)).sum() - st["mcc"]) <= 1e-10 * abs(st["mcc"])
    want_cost = np.where(big, (2 * a * np.abs(raw_r) - a * a) / 2, raw_r * raw_r / 2).sum()
    assert abs(st["cost"] - want_cost) <= 1e-14 * want_cost


def test_float64_statement_against_long_double():
    """The floor of what the device bars of tests/test_gpu_image_loss.py can show (DESIGN.md 4.2g holds the figures)."""
    pair = synth.occlude_tracked(synth.make_image_pair(64, 96, seed=0, invalid_fraction=0.05), 0.10, 0)
    out = {}
    for dt in (np.float64, np.longdouble):
        pr = ilr.ImageLossProblem(pair.camera, pair.ref, pair.track, pair.gradx, pair.grady, pair.disparity, ir.BILINEAR, dtype=dt, huber_a=0.02)
        out[dt] = pr.lm_step(pair.pose_init, pair.disparity, 1e4)
        assert pr.min_loss_margin >= 1e-9      # the two precisions take the same branch on every row
    a, b = out[np.float64], out[np.longdouble]
    eS = float(np.abs(a["S"] - b["S"]).max() / np.abs(b["S"]).max())
    ep = float(np.abs(a["dp"] - b["dp"]).max() / np.abs(b["dp"]).max())
    ed = float(np.abs(a["dd"] - b["dd"]).max() / np.abs(b["dd"]).max())
    ec = float(abs(a["cost"] - b["cost"]) / b["cost"])
    print(f"float64 against long double at 96 x 64, radius 1e4, a = 0.02: S {eS:.2e}, delta_pose {ep:.2e}, delta_disp {ed:.2e}, cost {ec:.2e}")
    assert eS <= 1e-11 and ep <= 1e-9 and ed <= 1e-9 and ec <= 1e-12      # a tenth of the device bars (1e-10, 1e-8)


@functools.lru_cache(maxsize=None)
def occluder_case(seed):
    """(pair, {a: (pose, iterations, loss margin)}) of the occluder cases, shared with tests/test_gpu_image_loss.py: 48 x 64,
    BILINEAR, constant disparities, 10 % of the tracked image repainted, the committed (non-monotonic) loop, at most 40
    iterations, with the NULL loss and with a = 0.02."""
    pair = synth.occlude_tracked(synth.make_image_pair(48, 64, seed=seed), OCCLUDER_FRACTION, seed)
    for x in (pair.ref, pair.track, pair.gradx, pair.grady, pair.disparity, pair.pose_init, pair.pose_true):
        x.setflags(write=False)
    out = {}
    for a in (0.0, OCCLUDER_A):
        pr = ilr.ImageLossProblem(pair.camera, pair.ref, pair.track, pair.gradx, pair.grady, pair.disparity, ir.BILINEAR, disp_const=True, huber_a=a)
        T, _, log = pr.solve(pair.pose_init, pair.disparity, max_iter=40)
        out[a] = (T, len(log) - 1, pr.min_loss_margin)
    return pair, out


@pytest.mark.parametrize("seed", OCCLUDER_SEEDS)
def test_the_loss_halves_the_pose_error_under_an_occluder(seed):
    """Largest absolute error of the 12 pose entries, with the loss <= 1/2 x without.  Ratios measured with this (committed,
    non-monotonic) loop are printed; DESIGN.md 4.2g records them."""
    pair, out = occluder_case(seed)
    e0, e1 = (float(np.abs(out[a][0] - pair.pose_true).max()) for a in (0.0, OCCLUDER_A))
    print(f"occluder seed {seed}: without loss {e0:.3e} ({out[0.0][1]} iterations), with Huber {e1:.3e} ({out[OCCLUDER_A][1]} iterations), "
          f"ratio {e1 / e0:.3f}, loss margin {out[OCCLUDER_A][2]:.2e}")
    assert e1 <= 0.5 * e0


def test_without_an_occluder_the_loss_changes_little():
    pair = synth.make_image_pair(48, 64, seed=0)
    T = []
    for a in (0.0, OCCLUDER_A):
        pr = ilr.ImageLossProblem(pair.camera, pair.ref, pair.track, pair.gradx, pair.grady, pair.disparity, ir.BILINEAR, disp_const=True, huber_a=a)
        T.append(pr.solve(pair.pose_init, pair.disparity, max_iter=40)[0])
    print(f"no occluder: max |pose(Huber) - pose(NULL)| = {np.abs(T[0] - T[1]).max():.2e}")
    assert np.abs(T[0] - T[1]).max() <= 1e-3


def test_occlude_tracked_is_what_it_says():
    pair = synth.make_image_pair(48, 64, seed=0)
    before = [x.copy() for x in (pair.ref, pair.track, pair.gradx, pair.grady, pair.disparity)]
    occ = synth.occlude_tracked(pair, 0.10, 5)
    for x, y in zip(before, (pair.ref, pair.track, pair.gradx, pair.grady, pair.disparity)):
        assert x.tobytes() == y.tobytes()                                        # the input is not written
    changed = occ.track != pair.track
    ys, xs = np.nonzero(changed)
    h, w = int(round(48 * np.sqrt(0.10))), int(round(64 * np.sqrt(0.10)))
    assert ys.min() >= 2 and xs.min() >= 2 and ys.max() <= 48 - 3 and xs.max() <= 64 - 3
    assert ys.max() - ys.min() + 1 <= h and xs.max() - xs.min() + 1 <= w and changed.sum() >= h * w - 4
    gx, gy = synth.sobel(occ.track)
    assert gx.tobytes() == occ.gradx.tobytes() and gy.tobytes() == occ.grady.tobytes()
    assert occ.ref is pair.ref and occ.disparity is pair.disparity
    assert synth.occlude_tracked(pair, 0.10, 5).track.tobytes() == occ.track.tobytes()
    assert synth.occlude_tracked(pair, 0.10, 6).track.tobytes() != occ.track.tobytes()
    u8 = synth.quantise_u8(pair.track)
    o8 = synth.occlude_tracked_u8(u8, 0.10, 5)
    assert o8.dtype == np.uint8 and ((o8 != u8) <= changed).all()
    assert (o8[changed] == synth.quantise_u8(occ.track)[changed]).all()


def test_coarse_to_fine_without_a_width_is_the_pyramid_reference_and_a_width_reaches_every_level():
    import pyramid_reference as pyr
    pair, _, _, levels = pyr.case_96x128()
    T0, d0, logs0 = pyr.coarse_to_fine(levels, pair.camera, pair.pose_init, 2, 0, max_iter=8)
    T1, d1, logs1, margin = ilr.coarse_to_fine(levels, pair.camera, pair.pose_init, 2, 0, max_iter=8, huber_a=0.0)
    assert T0.tobytes() == T1.tobytes() and logs0 == logs1 and margin == np.inf
    T2, _, logs2, margin = ilr.coarse_to_fine(levels, pair.camera, pair.pose_init, 2, 0, max_iter=8, huber_a=0.02)
    assert np.isfinite(margin) and len(logs2) == 3
    assert all(a[0][0] < b[0][0] for a, b in zip(logs2, logs0))         # rho <= r^2 on every level
