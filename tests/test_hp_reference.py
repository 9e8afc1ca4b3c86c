"""Pins the extended-precision reference of tests/hp_reference.py (CPU only): the refined solve against exact rational
solutions, the long-double rows and assembly in fp64 mode against np_reference, the Jacobians against complex step, and the
C oracle's reduced system and step against the same derived bounds the GPU tests hold the device to."""
from fractions import Fraction

import numpy as np
import pytest

import hp_reference as hp
import np_reference as npr
from ceres_slam_amd import synth
from oracle import oracle as orc


def _exact_solve(S, b):
    """Gaussian elimination over the rationals."""
    n = len(b)
    A = [[Fraction(float(S[i, j])) for j in range(n)] + [Fraction(float(b[i]))] for i in range(n)]
    for c in range(n):
        p = next(r for r in range(c, n) if A[r][c] != 0)
        A[c], A[p] = A[p], A[c]
        for r in range(c + 1, n):
            f = A[r][c] / A[c][c]
            if f:
                A[r] = [a - f * q for a, q in zip(A[r], A[c])]
    x = [Fraction(0)] * n
    for r in range(n - 1, -1, -1):
        x[r] = (A[r][n] - sum(A[r][j] * x[j] for j in range(r + 1, n))) / A[r][r]
    return x


def _ulps_from(x, exact):
    """Largest distance of x from the exact solution, in fp64 ulps of the exact entries."""
    worst = 0.0
    for xi, ei in zip(np.asarray(x, hp.LD), exact):
        e = float(ei)
        err = abs(Fraction(float(np.float64(xi))) + Fraction(float(np.float64(xi - hp.LD(np.float64(xi))))) - ei)
        worst = max(worst, float(err) / np.spacing(abs(e)))
    return worst


@pytest.mark.parametrize("case", ["random", "graded_1e12", "band"])
def test_refined_solve_hits_the_exact_solution(case):
    """Small SPD systems with fp64 entries, solved exactly over the rationals.  `graded_1e12` has kappa_2 ~ 1e12 through a
    diagonal grading (the ill-conditioning of a Jacobi-scaled LM system): the refined solution is within a few fp64 ulps of
    the exact one in every entry.  `band` goes through the banded factorisation."""
    rng = np.random.default_rng({"random": 1, "graded_1e12": 2, "band": 3}[case])
    n = 24
    A = rng.normal(size=(n, n))
    S = A @ A.T + n * np.eye(n)
    band = None
    if case == "graded_1e12":
        d = np.logspace(0, 6, n)
        S = d[:, None] * S * d[None, :]
    if case == "band":
        band = 5
        S = np.where(np.abs(np.subtract.outer(np.arange(n), np.arange(n))) <= band, S, 0.0)
        S += 2 * n * np.eye(n)
    b = rng.normal(size=n)
    exact = _exact_solve(S, b)
    x, kap = hp.refined_solve(S, b, band)
    if case == "graded_1e12":
        assert 1e11 < kap < 1e13
    assert _ulps_from(x, exact) <= 4.0
    assert kap == pytest.approx(np.linalg.cond(S), rel=1e-3)        # an estimate: eigvalsh of S itself


def test_refined_solve_band_kappa_uses_the_extreme_eigenvalues(monkeypatch):
    monkeypatch.setattr(hp, "DENSE_EIG_MAX", 10)
    rng = np.random.default_rng(4)
    n, bw = 60, 7
    A = rng.normal(size=(n, n))
    S = np.where(np.abs(np.subtract.outer(np.arange(n), np.arange(n))) <= bw, A + A.T, 0.0) + 40 * np.eye(n)
    b = rng.normal(size=n)
    x, kap = hp.refined_solve(S, b, bw)
    assert kap == pytest.approx(np.linalg.cond(S), rel=1e-8)
    assert hp.forward_error(x, np.linalg.solve(S.astype(hp.LD).astype(np.float64), b)) < 1e-13
    assert hp.backward_error(S, b, x) < 1e-18
    assert hp.backward_error_banded(S, b, x, bw) == pytest.approx(hp.backward_error(S, b, x), rel=1e-6)


@pytest.mark.parametrize("huber_a", [0.0, 1.345])
def test_rows_and_assembly_in_fp64_mode_match_numpy_ba(huber_a):
    prob = synth.make_problem(8, 60, track_len=5, seed=7)
    args = (prob.camera, prob.poses_init, prob.points_init, prob.obs_pose, prob.obs_point, prob.obs_uvd, prob.stiffness())
    ba = npr.NumpyBA(*args, huber_a=huber_a)
    cost, r, Jp, Jl = ba.residuals(prob.poses_init, prob.points_init, jac=True)
    rows = hp.stereo_rows(*args, huber_a=huber_a, dtype=np.float64)
    assert rows["cost"] == pytest.approx(cost, rel=1e-14)
    for a, b in ((rows["r"], r), (rows["Jp"], Jp), (rows["Jl"], Jl)):
        np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-12 * np.abs(b).max())
    # the sparse Jacobian of the rows is NumpyBA's
    J = ba.sparse_jacobian(rows["Jp"], rows["Jl"]).toarray()
    np.testing.assert_allclose(J, ba.sparse_jacobian(Jp, Jl).toarray(), rtol=1e-12, atol=1e-12 * np.abs(J).max())
    fidx = hp.free_index(prob.num_poses, prob.obs_pose, np.eye(1, prob.num_poses, 0, dtype=bool)[0])
    for radius in (1e4, 3.0):
        sy = hp.SchurSystem(hp.stereo_rows(*args, huber_a=huber_a), prob.obs_pose, prob.obs_point, fidx, prob.num_points, radius)
        x, kap = hp.refined_solve(sy.dense(), sy.rhs)
        dl = sy.back_substitute(x)
        mcc, _, _ = sy.model_cost_change(x, dl)
        dp2, dl2, mcc2, _, _ = ba.lm_step(prob.poses_init, prob.points_init, radius)
        assert hp.forward_error(dp2[1:].ravel(), x) < 1e-12
        assert hp.forward_error(dl2[sy.lm].ravel(), dl.ravel()) < 1e-12
        assert float(mcc) == pytest.approx(mcc2, rel=1e-12)


def test_long_double_jacobians_match_complex_step():
    prob = synth.make_problem(6, 40, track_len=4, seed=11)
    S = prob.stiffness()
    rows = hp.stereo_rows(prob.camera, prob.poses_init, prob.points_init, prob.obs_pose, prob.obs_point, prob.obs_uvd, S)
    for i in range(0, prob.num_obs, 7):
        k, j = int(prob.obs_pose[i]), int(prob.obs_point[i])
        Jp, Jl = npr.jacobians_complex_step(prob.camera, prob.poses_init[k], prob.points_init[j], prob.obs_uvd[i], S)
        np.testing.assert_allclose(np.asarray(rows["Jp"][i], np.float64), Jp, rtol=1e-13, atol=1e-13 * np.abs(Jp).max())
        np.testing.assert_allclose(np.asarray(rows["Jl"][i], np.float64), Jl, rtol=1e-13, atol=1e-13 * np.abs(Jl).max())


def _oracle_case(which):
    if which == "tiny":
        return synth.make_problem(8, 60, track_len=5, seed=7)
    return synth.make_config("C1")


@pytest.mark.parametrize("radius,huber", [(1e4, 0.0), (3.0, 0.0), (1e4, 1.345)])
@pytest.mark.parametrize("which", ["tiny", "c1"])
def test_oracle_system_and_step_satisfy_the_derived_bounds(which, radius, huber):
    """The fp64 oracle held to the bars of the device: S and rhs within E of the long-double assembly, its step within
    4096 u (backward) and min(4096 u kappa_2, 1e-8) (forward) of its own system, its model cost change within
    (m + c) u sum|terms| of the long-double one."""
    prob = _oracle_case(which)
    op = orc.OracleProblem.from_synth(prob, huber_a=huber)
    S2, rhs2, _ = op.reduced_system(radius)
    dp2, dl2, mcc2 = op.lm_step(radius)
    rows = hp.stereo_rows(prob.camera, prob.poses_init, prob.points_init, prob.obs_pose, prob.obs_point, prob.obs_uvd,
                          prob.stiffness(), huber)
    fidx = hp.free_index(prob.num_poses, prob.obs_pose, np.eye(1, prob.num_poses, 0, dtype=bool)[0])
    sy = hp.SchurSystem(rows, prob.obs_pose, prob.obs_point, fidx, prob.num_points, radius)
    ex_S, ex_rhs = sy.assembly_excess(S2, rhs2)
    assert ex_S <= 1.0 and ex_rhs <= 1.0
    x, kap = hp.refined_solve(S2, rhs2)
    eta_bar, fe_bar = hp.solve_bars(kap)
    assert hp.backward_error(S2, rhs2, dp2[1:].ravel()) <= eta_bar
    assert hp.forward_error(dp2[1:].ravel(), x) <= fe_bar
    mref, mag, nt = sy.model_cost_change(dp2[1:].ravel(), dl2[sy.lm])
    assert abs(mcc2 - float(mref)) <= (nt + hp.C_TERMS) * hp.U * mag


@pytest.mark.parametrize("radius", [1e4, 20.0, None])
def test_oracle_with_sun_and_prior_blocks_satisfies_the_derived_bounds(radius):
    """The _sun_problem of the covariance tests (no constant pose; the prior and the sun rows enter as fp64 blocks),
    damped and undamped; undamped also the covariance of three poses within the propagated bound.  Undamped, E and the
    propagated bound are loose enough to decide nothing where a landmark is nearly unobserved in depth (kappa(V_j) ~ 1e12:
    its terms in E exceed S); they are kept as what they are, bounds on the fp64 rounding."""
    from test_oracle_pose_factors import _sun_problem
    prob, factors = _sun_problem(P=8, L=480, seed=7)
    P = prob.num_poses
    none = np.zeros(P, bool)
    op = orc.OracleProblem(prob.camera, prob.poses_init, prob.points_init, prob.obs_pose, prob.obs_point, prob.obs_uvd,
                           prob.stiffness(), pose_const=none.astype(np.uint8), pose_factors=factors)
    S2, rhs2, _ = op.reduced_system(1e300 if radius is None else radius)
    fidx = hp.free_index(P, prob.obs_pose, none)
    H, g, Ha = hp.unary_pose_blocks(prob.poses_init, factors, fidx)
    rows = hp.stereo_rows(prob.camera, prob.poses_init, prob.points_init, prob.obs_pose, prob.obs_point, prob.obs_uvd, prob.stiffness())
    sy = hp.SchurSystem(rows, prob.obs_pose, prob.obs_point, fidx, prob.num_points, radius, H_unary=H, g_unary=g, Ha_unary=Ha)
    ex_S, ex_rhs = sy.assembly_excess(S2, rhs2)
    assert ex_S <= 1.0 and ex_rhs <= 1.0
    if radius is not None:
        dp2, dl2, mcc2 = op.lm_step(radius)
        x, kap = hp.refined_solve(S2, rhs2)
        assert hp.backward_error(S2, rhs2, dp2.ravel()) <= hp.solve_bars(kap)[0]
        assert hp.forward_error(dp2.ravel(), x) <= hp.solve_bars(kap)[1]
        return
    S_ld, E = sy.dense(), sy.dense_bound()
    inv2 = np.linalg.inv(S2)
    for k in (1, P // 2, P - 1):
        f = int(fidx[k])
        cov, kap = hp.covariance_truth(S_ld, f)
        cov = np.asarray(cov, np.float64)
        bound = hp.covariance_bound(np.asarray(S_ld, np.float64), E, f, kap, cov)
        assert np.all(np.abs(inv2[6 * f: 6 * f + 6, 6 * f: 6 * f + 6] - cov) <= bound)
