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


# ---- the device's intensity row (ssba_phong_device.h intensity_residual) in fp64 numpy, for the checks that the bars reject
# ---- a plausible kernel error
RSQ_EST = 2.0 ** -23      # modelled error of the f64 reciprocal(-square-root) estimates: the ISA gives them 2^29 ulp


def _rsqrt(a, newton):
    r = (1.0 / np.sqrt(a)) * (1 + RSQ_EST)          # the estimate at its worst
    for _ in range(newton):
        r = r * (1.5 - 0.5 * a * r * r)
    return r


def _rcp(a, newton):
    r = (1.0 / a) * (1 + RSQ_EST)
    for _ in range(newton):
        r = r + (1.0 - a * r) * r
    return r


def _dot3(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _neg_skew(g, a):
    return np.stack([-g[:, 1] * a[:, 2] + g[:, 2] * a[:, 1], g[:, 0] * a[:, 2] - g[:, 2] * a[:, 0], -g[:, 0] * a[:, 1] + g[:, 1] * a[:, 0]], 1)


def _device_intensity(light_type, T, p, n, phong, kd, light, colour, stiffness, newton=2, pow_alpha=None):
    """ssba_phong_device.h intensity_residual in fp64 numpy (one lane per row)."""
    T, p, n = (np.asarray(v, np.float64) for v in (T, p, n))
    N = T.shape[0]
    R = T[:, 3:].reshape(N, 3, 3)
    light = np.broadcast_to(np.asarray(light, np.float64), (N, 3))
    rs = lambda a: _rsqrt(a, newton)
    q = np.stack([R[:, i, 0] * p[:, 0] + R[:, i, 1] * p[:, 1] + R[:, i, 2] * p[:, 2] + T[:, i] for i in range(3)], 1)
    nc = np.stack([R[:, i, 0] * n[:, 0] + R[:, i, 1] * n[:, 1] + R[:, i, 2] * n[:, 2] for i in range(3)], 1)
    lc = np.stack([R[:, i, 0] * light[:, 0] + R[:, i, 1] * light[:, 1] + R[:, i, 2] * light[:, 2] + (T[:, i] if light_type == 0 else 0.0) for i in range(3)], 1)
    v = lc - q if light_type == 0 else lc
    rrho, rqn = rs(_dot3(v, v)), rs(_dot3(q, q))
    ell, cd = v * rrho[:, None], -q * rqn[:, None]
    kd, ks, alpha = np.asarray(kd, np.float64), phong[:, 1], phong[:, 2]
    g_ell, g_nc, g_cd, mat = np.zeros((N, 3)), np.zeros((N, 3)), np.zeros((N, 3)), np.zeros((N, 3))
    ldn = _dot3(ell, nc)
    lit = ldn > 0
    diffuse = np.where(lit, kd * ldn, 0.0)
    g_ell += np.where(lit[:, None], kd[:, None] * nc, 0.0)
    g_nc += np.where(lit[:, None], kd[:, None] * ell, 0.0)
    mat[:, 0] = np.where(lit, ldn, 0.0)
    mt = 2.0 * ldn[:, None] * nc - ell
    mu2 = _dot3(mt, mt)
    seen = mu2 > 0
    rmu = rs(np.where(seen, mu2, 1.0))
    m = mt * rmu[:, None]
    s = _dot3(m, cd)
    spec = seen & (s > 0)
    ss = np.where(spec, s, 1.0)
    ls = np.log(ss)
    sa = np.exp(alpha * ls) if pow_alpha is None else ss ** pow_alpha(alpha)
    specular = np.where(spec, ks * sa, 0.0)
    gs = ks * alpha * (sa * _rcp(ss, newton))
    w = (cd - m * ss[:, None]) * rmu[:, None]
    nw = _dot3(nc, w)
    sp = spec[:, None]
    g_ell += np.where(sp, gs[:, None] * (2.0 * nc * nw[:, None] - w), 0.0)
    g_nc += np.where(sp, gs[:, None] * 2.0 * (ldn[:, None] * w + ell * nw[:, None]), 0.0)
    g_cd += np.where(sp, gs[:, None] * m, 0.0)
    mat[:, 1] = np.where(spec, sa, 0.0)
    mat[:, 2] = np.where(spec, ks * sa * ls, 0.0)
    col = 1.0 * (0.0 + diffuse + specular)
    cl = (0.0 >= col) | (1.0 <= col)
    col = np.clip(col, 0.0, 1.0)
    for g in (g_ell, g_nc, g_cd, mat):
        g[cl] = 0.0
    r = stiffness * (col - colour)
    le, ce = _dot3(ell, g_ell), _dot3(cd, g_cd)
    gv = (g_ell - ell * le[:, None]) * rrho[:, None]
    gc = -(g_cd - cd * ce[:, None]) * rqn[:, None]
    g_q = gc - (gv if light_type == 0 else 0.0)
    J = np.zeros((N, 19))
    J[:, 0:3] = stiffness * (g_q + (gv if light_type == 0 else 0.0))
    J[:, 3:6] = stiffness * (_neg_skew(g_q, q) + _neg_skew(g_nc, nc) + _neg_skew(gv, lc))
    J[:, 6:9] = stiffness * np.einsum("ni,nij->nj", g_q, R)

    def unit_plus(g, x):
        inv = rs(_dot3(x, x))
        gx = _dot3(g, x) * inv * inv
        return (g - gx[:, None] * x) * inv[:, None]
    J[:, 9:12] = stiffness * unit_plus(np.einsum("ni,nij->nj", g_nc, R), n)
    J[:, 13], J[:, 14], J[:, 15] = stiffness * mat[:, 1], stiffness * mat[:, 2], stiffness * mat[:, 0]
    t3 = np.einsum("ni,nij->nj", gv, R)
    J[:, 16:19] = stiffness * (t3 if light_type == 0 else unit_plus(t3, light))
    return r, J


def _phong_batch(light_type, seed=7, P=8, L=60):
    prob, ph = synth.make_phong_problem(P, L, track_len=5, seed=seed, light_type=light_type)
    d = ph.as_oracle_dict("perturbed")
    k, j = prob.obs_pose.astype(np.int64), prob.obs_point.astype(np.int64)
    m = np.asarray(d["material_of_point"], np.int64)[j]
    args = (light_type, prob.poses_init[k], prob.points_init[j], d["normals"][j], d["phong"][m], d["texture"][m], d["light"],
            d["intensity"], d["int_stiffness"])
    return args, d["normal_obs"], d["normal_stiffness"]


def _row_excess(rows, r, J):
    """max |value - truth| / (C_ROW u mag) over the intensity residuals and over the Jacobian entries."""
    er = np.abs(np.asarray(np.asarray(r, hp.LD) - rows["r_int"], np.float64)) / np.maximum(hp.C_ROW * hp.U * rows["mag_r_int"], 1e-300)
    eJ = np.abs(np.asarray(np.asarray(J, hp.LD) - rows["J_int"], np.float64)) / np.maximum(hp.C_ROW * hp.U * rows["mag_J_int"], 1e-300)
    return float(er.max()), float(eJ.max())


@pytest.mark.parametrize("light_type", [0, 1])
def test_long_double_phong_rows_in_fp64_mode_match_complex_step_and_the_oracle(light_type):
    """phong_rows in fp64 mode is np_reference's complex step, vectorised: the same values to a few ulps of the row's
    magnitude; the long-double rows match the oracle's closed forms within the same row bar."""
    args, nobs, Sn = _phong_batch(light_type)
    r64 = hp.phong_rows(*args, nobs, Sn, dtype=np.float64, mags=False)
    ld = hp.phong_rows(*args, nobs, Sn)
    N = args[1].shape[0]
    for i in range(N):
        a = tuple(v[i] if np.ndim(v) and np.shape(v)[0] == N else v for v in args)
        r1 = npr.intensity_residual(*a).real
        J1 = npr.intensity_jacobian_complex_step(*a)
        assert abs(r64["r_int"][i] - r1) <= 4 * hp.U * ld["mag_r_int"][i]
        np.testing.assert_array_less(np.abs(r64["J_int"][i] - J1), 4 * hp.U * ld["mag_J_int"][i] + 1e-300)
        r2, J2 = orc.intensity_residual(*a, jac=True)
        rn, Jnp, Jnn = orc.normal_residual(a[1], a[3], nobs[i], Sn, jac=True)
        assert abs(r2 - float(ld["r_int"][i])) <= hp.C_ROW * hp.U * ld["mag_r_int"][i]
        np.testing.assert_array_less(np.abs(J2 - np.asarray(ld["J_int"][i], np.float64)), hp.C_ROW * hp.U * ld["mag_J_int"][i] + 1e-300)
        np.testing.assert_array_less(np.abs(rn - np.asarray(ld["r_nrm"][i], np.float64)), hp.C_ROW * hp.U * ld["mag_r_nrm"][i] + 1e-300)
        np.testing.assert_array_less(np.abs(Jnp - np.asarray(ld["J_np"][i], np.float64)), hp.C_ROW * hp.U * ld["mag_J_np"][i] + 1e-300)
        np.testing.assert_array_less(np.abs(Jnn - np.asarray(ld["J_nn"][i], np.float64)), hp.C_ROW * hp.U * ld["mag_J_nn"][i] + 1e-300)


def test_long_double_phong_rows_reproduce_the_light_test_answers():
    """The reference's light_test scene (test_oracle_phong): shade 0.27697118 (diffuse only) and 0.48917229."""
    from test_oracle_phong import ALPHA, KD, KS, LIGHT, V28, V245
    T = np.concatenate([np.zeros(3), np.eye(3).ravel()])[None].repeat(2, 0)
    p = np.stack([V28[0], V245[0]])
    n = np.stack([V28[1], V245[1]])
    rows = hp.phong_rows(0, T, p, n, np.array([[0.1, KS, ALPHA]] * 2), np.full(2, KD), LIGHT, np.zeros(2), 1.0,
                         np.zeros((2, 3)), np.eye(3), mags=False)
    np.testing.assert_allclose(np.asarray(rows["r_int"], np.float64), [0.27697118, 0.48917229], atol=5e-9)


@pytest.mark.parametrize("light_type", [0, 1])
@pytest.mark.parametrize("seed", [7, 3])
def test_device_arithmetic_meets_the_row_bar_and_plausible_errors_do_not(light_type, seed):
    """The device's intensity row, restated in fp64 numpy, is within C_ROW u mag of the long-double row; the same row with
    ONE Newton step on the hardware rsqrt / rcp estimates (modelled at their 2^-23 worst), or with the specular term
    computed as pow(s, float32(alpha)), is rejected by more than a factor 10.  With one Newton step the residual itself
    is off by only ~5x its bar: it meets the rsqrt error once, in the normalisation of ell and cd, where the Jacobian meets
    it two or three times over (ell and g_v, cd and g_c, the unit-vector projection) -- the Jacobian carries the check."""
    args, nobs, Sn = _phong_batch(light_type, seed)
    rows = hp.phong_rows(*args, nobs, Sn)
    er, eJ = _row_excess(rows, *_device_intensity(*args))
    assert er <= 1.0 and eJ <= 1.0, (er, eJ)
    er1, eJ1 = _row_excess(rows, *_device_intensity(*args, newton=1))
    assert eJ1 > 10 and er1 > 2, (er1, eJ1)
    erp, eJp = _row_excess(rows, *_device_intensity(*args, pow_alpha=lambda a: a.astype(np.float32).astype(np.float64)))
    assert erp > 10 and eJp > 10, (erp, eJp)


# ---- the long-double reduced system with 6-D landmarks and the border of free shared blocks -----------------------------
def _phong_system(light_type, shared_free, radius, huber=0.0, seed=7):
    prob, ph = synth.make_phong_problem(8, 60, track_len=5, seed=seed, light_type=light_type)
    d = ph.as_oracle_dict("perturbed" if shared_free else "truth")
    rows = hp.phong_observation_rows(prob.camera, prob.poses_init, prob.points_init, d["normals"], prob.obs_pose, prob.obs_point,
                                     prob.obs_uvd, prob.stiffness(), d, huber, shared_free)
    fidx = hp.free_index(prob.num_poses, prob.obs_pose, np.eye(1, prob.num_poses, 0, dtype=bool)[0])
    sy = hp.SchurSystem(rows, prob.obs_pose, prob.obs_point, fidx, prob.num_points, radius)
    return prob, d, sy, fidx


def _solve_bordered(sy):
    A, b = sy.bordered() if sy.nb else (sy.dense(), sy.rhs)
    x, _ = hp.refined_solve(A, b)
    return x[: sy.n], x[sy.n:]


@pytest.mark.parametrize("light_type", [0, 1])
@pytest.mark.parametrize("shared_free,nb", [(0, 0), (1, 3), (4, 4), (6, 16), (7, 19)])
def test_long_double_bordered_step_matches_the_sparse_phong_step(light_type, shared_free, nb):
    """The long-double reduced system, solved and back-substituted, is np_reference.phong_lm_step's direct sparse solve of
    the whole damped system (complex-step rows through Plus) to the fp64 level: pose, landmark and border steps and the
    model cost change."""
    for radius in (1e4, 3.0):
        prob, d, sy, fidx = _phong_system(light_type, shared_free, radius)
        assert sy.nb == nb and sy.d == 6
        x, db = _solve_bordered(sy)
        dl = sy.back_substitute(x, db)
        mcc, _, _ = sy.model_cost_change(x, dl, db)
        out = npr.phong_lm_step(prob.camera, prob.poses_init, prob.points_init, d["normals"], prob.obs_pose, prob.obs_point,
                                prob.obs_uvd, prob.stiffness(), d, radius, shared_free=shared_free)
        assert hp.forward_error(out[0][1:].ravel(), x) < 1e-10
        assert hp.forward_error(out[1][sy.lm].ravel(), dl.ravel()) < 1e-10
        assert float(mcc) == pytest.approx(out[2], rel=1e-10)
        if nb:
            assert hp.forward_error(out[4], db) < 1e-10


@pytest.mark.parametrize("light_type", [0, 1])
@pytest.mark.parametrize("shared_free", [0, 7])
def test_oracle_phong_reduced_system_is_within_the_assembly_bound(light_type, shared_free):
    prob, d, sy, fidx = _phong_system(light_type, shared_free, 5.0)
    op = orc.OracleProblem(prob.camera, prob.poses_init, prob.points_init, prob.obs_pose, prob.obs_point, prob.obs_uvd,
                           prob.stiffness(), lighting=d, shared_free=shared_free)
    A, b, _ = op.reduced_system(5.0)
    n = sy.n
    ex_S, ex_rhs = sy.assembly_excess(A[:n, :n], b[:n])
    assert ex_S <= 1.0 and ex_rhs <= 1.0, (ex_S, ex_rhs)
    if shared_free:
        assert max(sy.border_excess(A[:n, n:], A[n:, n:], b[n:])) <= 1.0


def test_assembly_and_border_bars_reject_plausible_kernel_errors():
    """One plausible kernel error at a time, on a copy of the long-double answer; each is rejected by more than 10x:
    one landmark's Schur term left out of S, one observation's texture column left out of S_pb, the light columns'
    gradient left out of rhs_b, and a delta_l whose normal rows are ignored."""
    prob, d, sy, fidx = _phong_system(0, 7, 5.0)
    n = sy.n
    S = np.asarray(sy.dense(), np.float64)
    # (1) S without the Schur term of the landmark with the most free observations
    so, fr = sy.slot_of_obs, sy._f >= 0
    obs0 = np.flatnonzero((so == np.bincount(so[fr]).argmax()) & fr)
    assert obs0.size >= 3
    X = np.einsum("nij,njk->nik", sy.W, sy.Vinv[so])
    S1 = np.asarray(sy.dense(), hp.LD)
    for a in obs0:
        for b in obs0:
            fa, fb = sy._f[a], sy._f[b]
            S1[6 * fa: 6 * fa + 6, 6 * fb: 6 * fb + 6] += X[a] @ sy.W[b].T
    assert sy.assembly_excess(np.asarray(S1, np.float64), np.asarray(sy.rhs, np.float64))[0] > 10
    assert sy.assembly_excess(S, np.asarray(sy.rhs, np.float64))[0] <= 1.0
    # (2) S_pb without observation i's texture column (the last M columns; the observation's material)
    i = int(np.flatnonzero(fr)[3])
    M = len(d["texture"])
    c = sy.nb - M + int(d["material_of_point"][prob.obs_point[i]])
    Spb = np.asarray(sy.S_pb, hp.LD).copy()
    Jp, Jb = sy.rows["Jp"][i], sy.rows["Jb"][i]
    Spb[6 * sy._f[i]: 6 * sy._f[i] + 6, c] -= Jp.T @ Jb[:, c]
    ok = sy.border_excess(np.asarray(sy.S_pb, np.float64), np.asarray(sy.S_bb, np.float64), np.asarray(sy.rhs_b, np.float64))
    assert max(ok) <= 1.0
    assert sy.border_excess(np.asarray(Spb, np.float64), sy.S_bb, sy.rhs_b)[0] > 10
    # (3) rhs_b without the light columns' gradient
    g_light = np.einsum("na,na->", sy.rows["Jb"][:, :, 0], sy.rows["r"])
    rb = np.asarray(sy.rhs_b, hp.LD).copy()
    rb[:3] += np.einsum("nab,na->b", sy.rows["Jb"][:, :, :3], sy.rows["r"])
    assert g_light != 0 and sy.border_excess(sy.S_pb, sy.S_bb, np.asarray(rb, np.float64))[2] > 10
    # (4) delta_l from a system whose landmark blocks ignore the normal rows
    x, db = _solve_bordered(sy)
    dl = sy.back_substitute(x, db)
    rows2 = dict(sy.rows)
    for k in ("Jl", "Jla"):
        rows2[k] = sy.rows[k].copy()
        rows2[k][:, 4:] = 0
    sy2 = hp.SchurSystem(rows2, prob.obs_pose, prob.obs_point, fidx, prob.num_points, 5.0)
    dl_bad = sy2.back_substitute(x, db)
    err = np.abs(np.asarray(dl_bad - dl, np.float64)).max(1)
    bound = (np.bincount(so, minlength=sy.lm.shape[0]) + hp.C_TERMS) * hp.U * sy.kappa_V * np.abs(np.asarray(dl, np.float64)).max(1)
    assert (err / bound).max() > 10


# ---------------------------------------------------------------------------------------------------------------- dogleg
def _first_numpy_dogleg(ba, mu=1e-8):
    """The first linearisation of np_reference.dogleg_solve (its own dogleg_linearize), with the sums in unscaled terms."""
    keep = np.concatenate([np.ones(6 * ba.nf, bool), np.repeat(ba.active, 3)])
    st = npr.dogleg_linearize(ba, ba.poses, ba.points, keep, None, mu)
    grad, gn, D, Js = st["grad"], st["gn"], st["D"], st["Js"]
    Jg, Jn = Js @ (grad / D), Js @ (gn / D)
    return dict(state=st, sums=[grad @ grad, gn @ gn, grad @ gn, Jg @ Jg, Jn @ Jn, Jg @ Jn], alpha=st["alpha"],
                gn_unscaled=gn / D * st["scale"], v=st["scale"] * grad / D)


def _tiny_reference(mu=1e-8, huber=0.0):
    prob = synth.make_problem(8, 60, track_len=5, seed=7)
    const = np.zeros(8, bool)
    const[0] = True
    rows = hp.stereo_rows(prob.camera, prob.poses_init, prob.points_init, prob.obs_pose, prob.obs_point, prob.obs_uvd,
                          prob.stiffness(), huber)
    fidx = hp.free_index(8, prob.obs_pose, const)
    return prob, hp.DoglegReference(rows, prob.obs_pose, prob.obs_point, fidx, prob.num_points, mu), fidx


def _ref_sums(ref, v, gn):
    return list(ref.param_sums(v, gn)[0]) + [ref.row_sums(x, y)[0] for x, y in ((v, v), (gn, gn), (v, gn))]


def test_dogleg_reference_reproduces_the_numpy_first_step():
    """TRADITIONAL_DOGLEG's first step of np_reference.dogleg_solve (sparse fp64 solve, scaled coordinates): the six sums,
    alpha, v, the Gauss-Newton step and beta / gamma in all three branches, to fp64 accuracy."""
    prob, ref, fidx = _tiny_reference()
    ba = npr.NumpyBA(prob.camera, prob.poses_init, prob.points_init, prob.obs_pose, prob.obs_point, prob.obs_uvd, prob.stiffness(),
                     pose_const=fidx < 0)
    npf = _first_numpy_dogleg(ba)
    gn, kap = ref.gauss_newton()
    sums = _ref_sums(ref, ref.v, gn)
    for a, b in zip(sums, npf["sums"]):
        assert abs(float(a) - b) <= 1e-9 * abs(b), (float(a), b)
    assert np.allclose(np.asarray(gn, np.float64), npf["gn_unscaled"], rtol=0, atol=1e-9 * np.abs(npf["gn_unscaled"]).max())
    assert np.allclose(np.asarray(ref.v, np.float64), npf["v"], rtol=0, atol=1e-9 * np.abs(npf["v"]).max())
    A, Bn = float(sums[0]), float(sums[1])
    cauchy = float(sums[0] / sums[3]) * np.sqrt(A)
    grad, gnD = npf["state"]["grad"], npf["state"]["gn"]
    for r, branch in ((2 * np.sqrt(Bn), "gn"), (0.5 * cauchy, "cauchy"), (np.sqrt(cauchy * np.sqrt(Bn)), "dogleg")):
        sc = hp.dogleg_scalars(sums, r, 0)
        assert sc["branch"] == branch
        assert abs(float(sc["alpha"]) - npf["alpha"]) <= 1e-10 * npf["alpha"]
        # np_reference's own step (dogleg_traditional_step, D-scaled) against beta gn + gamma gradient_
        step, _, mcc_np = npr.dogleg_traditional_step(npf["state"], r)
        mine = float(sc["beta"]) * gnD + float(sc["gamma"]) * grad
        assert np.allclose(mine, step, rtol=0, atol=1e-9 * np.abs(step).max()), branch
        assert abs(float(sc["mcc"]) - mcc_np) <= 1e-9 * abs(mcc_np), (branch, float(sc["mcc"]), mcc_np)
        # mcc from the sums equals the true model cost change of the step, row by row
        delta = sc["beta"] * gn + sc["gamma"] * ref.v
        m, mag = ref.model_cost_change(delta)
        assert abs(m - sc["mcc"]) <= 1e-15 * mag


def _oracle_problem(which):
    from test_oracle_pose_factors import _sun_problem
    factors = None
    if which == "tiny":
        prob = synth.make_problem(8, 60, track_len=5, seed=7)
    elif which == "c1":
        prob = synth.make_config("C1")
    else:
        prob, factors = _sun_problem()
    const = np.zeros(prob.num_poses, bool)
    if factors is None:
        const[0] = True
    return prob, factors, const


@pytest.mark.parametrize("radius", ["gn", "boundary"])
@pytest.mark.parametrize("dogleg_type", [0, 1])
@pytest.mark.parametrize("which", ["tiny", "c1", "sun"])
def test_dogleg_reference_reproduces_the_oracles_first_iteration(which, dogleg_type, radius):
    """The C oracle's first DOGLEG iteration (mu 1e-8; initial radius 1e4 -- the Gauss-Newton step inside -- or the geometric
    mean of the Cauchy and Gauss-Newton step lengths -- on the dogleg / the subspace boundary): its model cost change,
    recovered as cost_change / relative_decrease of iteration 1, against the reference's true model cost change of the step at
    the same radius -- within the bars of the device (sums' bars propagated, plus the row bar of the model cost change)."""
    prob, factors, const = _oracle_problem(which)
    rows = hp.stereo_rows(prob.camera, prob.poses_init, prob.points_init, prob.obs_pose, prob.obs_point, prob.obs_uvd,
                          prob.stiffness())
    fidx = hp.free_index(prob.num_poses, prob.obs_pose, const)
    un = hp.unary_rows(prob.poses_init, factors) if factors else None
    ref = hp.DoglegReference(rows, prob.obs_pose, prob.obs_point, fidx, prob.num_points, 1e-8, unary=un)
    gn, _ = ref.gauss_newton()
    (a, b, c), (ea, eb, ec) = ref.param_sums(ref.v, gn)
    rs = [ref.row_sums(x, y) for x, y in ((ref.v, ref.v), (gn, gn), (ref.v, gn))]
    sums, bars = [a, b, c] + [t[0] for t in rs], [ea, eb, ec] + [t[1] for t in rs]
    r = 1e4 if radius == "gn" else float(np.sqrt(float(a / sums[3]) * float(np.sqrt(a)) * float(np.sqrt(b))))
    sc = hp.dogleg_scalars(sums, r, dogleg_type)
    assert sc["branch"] == ("gn" if radius == "gn" else ("dogleg", "boundary")[dogleg_type])
    op = orc.OracleProblem(prob.camera, prob.poses_init.copy(), prob.points_init.copy(), prob.obs_pose, prob.obs_point, prob.obs_uvd,
                           prob.stiffness(), pose_const=const.astype(np.uint8), pose_factors=factors)
    o = orc.default_options(trust_region_strategy_type=1, dogleg_type=dogleg_type, max_num_iterations=1, initial_trust_region_radius=r)
    _, log = op.solve(o)
    assert log["cost"].shape[0] >= 2 and log["relative_decrease"][1] != 0
    mcc_orc = log["cost_change"][1] / log["relative_decrease"][1]
    m, mag = ref.model_cost_change(sc["beta"] * gn + sc["gamma"] * ref.v)
    prop = hp.propagate(lambda s: {"mcc": hp.dogleg_scalars(s, r, dogleg_type)["mcc"]}, sums, bars)["mcc"]
    bar = (ref.c_sum() + 2 * hp.C_DL_ROW) * hp.U * mag + prop + 16 * hp.U * abs(float(m))
    print(which, dogleg_type, sc["branch"], float(m), mcc_orc, abs(mcc_orc - float(m)) / bar)
    assert abs(mcc_orc - float(m)) <= bar, (which, dogleg_type, mcc_orc, float(m), bar)


def _closed_form_problem(J, r):
    """A linear least-squares problem with its J entered directly, as row groups of a DoglegReference-like object."""
    class P:
        pass
    J, r = np.asarray(J, hp.LD), np.asarray(r, hp.LD)
    p = P()
    p.g, p.h = J.T @ r, (J * J).sum(0)
    p.s = 1 / (1 + np.sqrt(p.h))
    p.D2 = np.clip(p.s * p.s * p.h, hp.LD(1e-6), hp.LD(1e32))
    p.J, p.r = J, r
    return p


@pytest.mark.parametrize("J,r", [([[2.0, 0.0], [0.0, 0.5], [1.0, 1.0]], [1.0, -3.0, 0.5]),
                                 ([[3.0, 1.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 0.1], [1.0, 0.0, 1.0]], [0.2, 1.0, -2.0, 0.3])])
def test_dogleg_scalars_match_the_closed_form(J, r):
    """alpha = |gradient_|^2 / |J_s gradient_ / D|^2, the dogleg beta from |a + beta (b - a)| = radius, and the subspace boundary
    minimum from the 2x2 eigenproblem of the model, by hand in long double -- every branch, to a few long-double ulps."""
    p = _closed_form_problem(J, r)
    Js = p.J * p.s
    D = np.sqrt(p.D2)
    grad = Js.T @ p.r / D
    Jv = Js @ (grad / D)
    gn = -D * _ld_solve(Js.T @ Js + hp.LD(1e-8) * np.diag(p.D2), Js.T @ p.r)
    Jg = Js @ (gn / D)
    sums = [grad @ grad, gn @ gn, grad @ gn, Jv @ Jv, Jg @ Jg, Jv @ Jg]
    alpha = sums[0] / sums[3]
    eps = 64 * np.finfo(hp.LD).eps
    a = -alpha * grad
    gnorm, nnorm = np.sqrt(sums[0]), np.sqrt(sums[1])
    radius_dl = np.sqrt(alpha * gnorm * nnorm)
    for rad, branch in ((2 * nnorm, "gn"), (0.5 * alpha * gnorm, "cauchy"), (radius_dl, "dogleg")):
        sc = hp.dogleg_scalars(sums, rad, 0)
        assert sc["branch"] == branch
        assert abs(sc["alpha"] - alpha) <= eps * alpha
        step = sc["beta"] * gn + sc["gamma"] * grad          # D-scaled space: v maps to gradient_
        if branch == "gn":
            assert sc["beta"] == 1 and sc["gamma"] == 0
        elif branch == "cauchy":
            assert np.all(np.abs(step + rad / gnorm * grad) <= eps * rad)
        else:   # on the segment a -> gn, at the boundary
            t = sc["beta"]
            assert abs(np.sqrt(((a + t * (gn - a)) ** 2).sum()) - rad) <= eps * rad
            assert np.all(np.abs(step - (a + t * (gn - a))) <= eps * rad)
        m_true = -(step / D * p.s) @ p.g - hp.LD(0.5) * ((p.J @ (step / D * p.s)) ** 2).sum()
        assert abs(sc["mcc"] - m_true) <= eps * abs(m_true)
    # SUBSPACE at the dogleg radius: minimise over the circle of the orthonormal basis by the 2x2 secular equation
    sc = hp.dogleg_scalars(sums, radius_dl, 1)
    assert sc["branch"] == "boundary"
    Q = np.stack([grad / gnorm, gn - (gn @ grad) / sums[0] * grad])
    Q[1] /= np.sqrt(Q[1] @ Q[1])
    g2 = Q @ grad
    B2 = (Js @ (Q / D).T).T @ (Js @ (Q / D).T)
    best = _secular_minimum(g2, B2, radius_dl)
    step = sc["beta"] * gn + sc["gamma"] * grad
    y = Q @ step
    model = lambda y: g2 @ y + hp.LD(0.5) * y @ B2 @ y
    assert abs(model(y) - model(best)) <= eps * abs(model(best))
    assert np.all(np.abs(y - best) <= 1e-9 * radius_dl)


def test_dogleg_scalars_one_dimensional_subspace():
    """J = c I: gradient_ and the Gauss-Newton step are collinear, the subspace is one-dimensional and the step is the
    scaled steepest descent to the boundary."""
    p = _closed_form_problem(np.eye(3) * 2.0, [1.0, -2.0, 0.5])
    Js = p.J * p.s
    D = np.sqrt(p.D2)
    grad = Js.T @ p.r / D
    Jv = Js @ (grad / D)
    gn = -D * _ld_solve(Js.T @ Js + hp.LD(1e-8) * np.diag(p.D2), Js.T @ p.r)
    Jg = Js @ (gn / D)
    sums = [grad @ grad, gn @ gn, grad @ gn, Jv @ Jv, Jg @ Jg, Jv @ Jg]
    rad = 0.5 * np.sqrt(sums[1])
    sc = hp.dogleg_scalars(sums, rad, 1)
    assert sc["one_dim"] and sc["branch"] == "one_dim"
    assert sc["beta"] == 0 and abs(sc["gamma"] + rad / np.sqrt(sums[0])) <= 4 * np.finfo(hp.LD).eps * abs(sc["gamma"])


def _ld_solve(A, b):
    A, b = np.asarray(A, hp.LD).copy(), np.asarray(b, hp.LD).copy()
    n = len(b)
    for c in range(n):
        for rr in range(c + 1, n):
            f = A[rr, c] / A[c, c]
            A[rr] -= f * A[c]
            b[rr] -= f * b[c]
    x = np.zeros(n, hp.LD)
    for rr in range(n - 1, -1, -1):
        x[rr] = (b[rr] - A[rr, rr + 1:] @ x[rr + 1:]) / A[rr, rr]
    return x


def _secular_minimum(g, B, r):
    """min of g.y + y^T B y / 2 on |y| = r: y = -(B + l I)^-1 g with |y| = r, l >= -lambda_min, by bisection in long double
    in the eigenbasis of B (the hard case does not occur for these problems)."""
    B64 = np.asarray(B, np.float64)
    w, V = np.linalg.eigh(B64)
    V = np.asarray(V, hp.LD)
    w = np.asarray(w, hp.LD)
    c = V.T @ np.asarray(g, hp.LD)
    norm = lambda l: np.sqrt(((c / (w + l)) ** 2).sum())
    lo, hi = -w[0] + hp.LD(1e-30), -w[0] + np.sqrt((c * c).sum()) / r + 1
    for _ in range(200):
        mid = (lo + hi) / 2
        lo, hi = (mid, hi) if norm(mid) > r else (lo, mid)
    y = V @ (-c / (w + (lo + hi) / 2))
    return y * (r / np.sqrt(y @ y))


def test_boundary_minimum_matches_the_quartic_roots():
    """The theta-grid + Newton minimiser against the quartic of Ceres' FindMinimumOnTrustRegionBoundary solved by numpy.roots
    on random well-separated 2-D models: same minimum value, same minimiser."""
    rng = np.random.default_rng(5)
    for _ in range(200):
        A = rng.normal(size=(2, 2))
        B = A @ A.T + 0.1 * np.eye(2)
        g = rng.normal(size=2) * 3
        r = float(np.exp(rng.uniform(-2, 1)))
        if np.linalg.norm(np.linalg.solve(B, g)) <= 1.2 * r:
            continue                   # the Gauss-Newton step lies inside: no boundary minimum is asked for
        detB, trB = np.linalg.det(B), np.trace(B)
        adj = np.array([[B[1, 1], -B[0, 1]], [-B[0, 1], B[0, 0]]])
        ag = adj @ g
        r2 = r * r
        poly = [r2, 2 * r2 * trB, r2 * (trB ** 2 + 2 * detB) - g @ g, -2 * (g @ ag - r2 * detB * trB), r2 * detB ** 2 - ag @ ag]
        cands = []
        for lam in np.roots(poly):
            if abs(lam.imag) > 1e-8 * max(1, abs(lam)):
                continue
            y = -np.linalg.solve(B + lam.real * np.eye(2), g)
            y *= r / np.linalg.norm(y)
            cands.append((g @ y + 0.5 * y @ B @ y, y))
        fq, yq = min(cands, key=lambda t: t[0])
        y = np.asarray(hp.boundary_minimum(g, B, r), np.float64)
        f = g @ y + 0.5 * y @ B @ y
        assert abs(f - fq) <= 1e-12 * max(1.0, abs(fq)), (f, fq)
        assert np.allclose(y, yq, atol=1e-6 * r), (y, yq)


def _device_dogleg(ref, rows, gn, radius, dogleg_type, mut=""):
    """float64 restatement of the device's dogleg arithmetic (k_dogleg_vec, k_dogleg_gn / k_ph_dogleg_gn, k_dogleg_interp) on the
    reference's rows: v = s^2 g / D^2 in unscaled coordinates, the row-space sums from the one-pass identity
        x^T J^T J y = sum_l [x_l^T H_ll y_l + x_l . (tt_y - g_l) + y_l . (tt_x - g_l)] + sum_rows e_x e_y,   e = J_p x_p + J_b x_b
    (H_ll over all rows of the landmark, constant poses included), the unary rows of each pose with the relative-pose cross
    term counted once, and the model cost change from the six sums.  `mut` applies one plausible kernel error."""
    f64 = lambda a: np.asarray(a, np.float64)
    g, h = f64(ref.g), f64(ref.h)
    s = 1.0 / (1.0 + np.sqrt(h))
    D2 = s * s * h if mut == "unclamped" else np.clip(s * s * h, 1e-6, 1e32)
    v = (g / D2) if mut == "no_s2" else s * s * g / D2
    gn = f64(gn)
    A = float((s * s * g * g / D2).sum()) if mut != "no_s2" else float((g * g / D2).sum())
    sums = [A, float((D2 * gn * gn / (s * s)).sum()), float((g * gn).sum())]
    sy = ref.sy
    free = sy._f >= 0
    so = sy.slot_of_obs
    Jp, Jl, r = f64(rows["Jp"]), f64(rows["Jl"]), f64(rows["r"])
    Jb = f64(rows["Jb"]) if ref.nb else None
    gl = np.zeros((ref.Lp, ref.d))
    np.add.at(gl, so, np.einsum("nai,na->ni", Jl, r))
    Hrows = free if mut == "drop_const" else np.ones_like(free)
    H = np.zeros((ref.Lp, ref.d, ref.d))
    np.add.at(H, so[Hrows], np.einsum("nai,naj->nij", Jl[Hrows], Jl[Hrows]))

    def parts(x):
        xp, xl, xb = (f64(t) for t in ref.split(x))
        e = np.zeros(r.shape)
        e[free] = np.einsum("nai,ni->na", Jp[free], xp[sy._f[free]])
        if ref.nb and mut != "no_border":
            e += np.einsum("nab,b->na", Jb, xb)
        t = np.zeros((ref.Lp, ref.d))
        np.add.at(t, so, np.einsum("nai,na->ni", Jl, e))
        return xl, e, (gl if mut == "cross_gl" else t)

    def q(x, y):
        xl, ex, tx = parts(x)
        yl, ey, ty = parts(y)
        val = (np.einsum("li,lij,lj->", xl, H, yl) + (xl * ty).sum() + (yl * tx).sum() + (ex * ey).sum())
        xe, ye = np.concatenate([f64(x), [0.0]]), np.concatenate([f64(y), [0.0]])
        for G in ref.groups[1:]:
            a = [f64(J[0]) @ xe[col[0]] for J, _, col in G["blocks"]]
            b = [f64(J[0]) @ ye[col[0]] for J, _, col in G["blocks"]]
            val += sum(ai @ bi for ai, bi in zip(a, b))
            if len(a) == 2:
                val += (2.0 if mut == "cross_twice" else 1.0) * (a[0] @ b[1] + a[1] @ b[0])
        return float(val)

    sums += [q(v, v), q(gn, gn), q(v, gn)]
    if mut == "g2_in_mcc":
        chain_sums = [float((g * g).sum())] + sums[1:]
    else:
        chain_sums = sums
    sc = hp.dogleg_scalars(sums, radius, dogleg_type)
    beta, gamma = float(sc["beta"]), float(sc["gamma"])
    if mut == "subspace_largest":
        y = hp.boundary_minimum(-sc["sub_g"], -sc["sub_B"], radius)
        gamma, beta = float(y @ sc["sub_e"][:, 0]), float(y @ sc["sub_e"][:, 1])
    A_, Bn, C, Jv2, Jg2, Jvg = chain_sums
    mcc = -(beta * C + gamma * A_) - 0.5 * (beta * beta * Jg2 + 2 * beta * gamma * Jvg + gamma * gamma * Jv2)
    return v, sums, mcc, beta, gamma


def _mutation_ratios(ref, rows, radius, dogleg_type, mut):
    gn, _ = ref.gauss_newton()
    v, sums, mcc, beta, gamma = _device_dogleg(ref, rows, gn, radius, dogleg_type, mut)
    vr = float((np.abs(np.asarray(np.asarray(v, hp.LD) - ref.v, np.float64)) / np.maximum(ref.v_bar(), 1e-300)).max())
    (a, b, c), (ea, eb, ec) = ref.param_sums(ref.v, gn)
    rs = [ref.row_sums(x, y) for x, y in ((ref.v, ref.v), (gn, gn), (ref.v, gn))]
    ref_sums, bars = [a, b, c] + [t[0] for t in rs], [ea, eb, ec] + [t[1] for t in rs]
    sr = max(float(abs(hp.LD(x) - y)) / e for x, y, e in zip(sums, ref_sums, bars))
    keys = ("mcc",)
    prop = hp.propagate(lambda s: {k: hp.dogleg_scalars(s, radius, dogleg_type)[k] for k in keys}, ref_sums, bars)
    truth = hp.dogleg_scalars(ref_sums, radius, dogleg_type)
    delta = truth["beta"] * gn + truth["gamma"] * ref.v
    mref, mag = ref.model_cost_change(delta)
    mbar = (ref.c_sum() + 2 * hp.C_DL_ROW) * hp.U * mag + prop["mcc"] + 16 * hp.U * abs(float(mref))
    mr = float(abs(hp.LD(mcc) - mref)) / mbar
    return max(vr, sr, mr)


def _mutation_problem():
    """Constant poses at the start and inside the chain, Huber with outliers, a far landmark under the diagonal clamp,
    odometry and a loop closure (relative-pose rows) -- every term the mutations below touch."""
    from test_oracle_pose_factors import _odometry_factors
    prob = synth.make_problem(8, 60, track_len=5, seed=7, outlier_fraction=0.15)
    pts = prob.points_init.copy()
    T0 = prob.poses_init[prob.obs_pose[prob.obs_point == 5][0]]
    cam = -T0[3:].reshape(3, 3).T @ T0[:3]
    pts[5] = cam + (pts[5] - cam) * 1e5
    const = np.zeros(8, bool)
    const[[0, 4]] = True
    factors = [f for f in _odometry_factors(prob) if f["type"] == 2 and not const[f["pose"]] and not const[f["pose2"]]]
    rows = hp.stereo_rows(prob.camera, prob.poses_init, pts, prob.obs_pose, prob.obs_point, prob.obs_uvd, prob.stiffness(), 1.345)
    fidx = hp.free_index(8, prob.obs_pose, const)
    un = hp.unary_rows(prob.poses_init, factors)
    ref = hp.DoglegReference(rows, prob.obs_pose, prob.obs_point, fidx, prob.num_points, 1e-8, unary=un)
    assert np.any(ref.clamped) and np.any(np.asarray(hp.huber_weight((np.asarray(rows["r"], np.float64) ** 2).sum(1), 1.345)) < 1)
    rows_nh = hp.stereo_rows(prob.camera, prob.poses_init, pts, prob.obs_pose, prob.obs_point, prob.obs_uvd, prob.stiffness(), 0.0)
    return ref, rows, rows_nh


def _dogleg_radius(ref):
    gn, _ = ref.gauss_newton()
    (A, Bn, _), _ = ref.param_sums(ref.v, gn)
    jv2 = ref.row_sums(ref.v, ref.v)[0]
    return float(np.sqrt(float(A / jv2) * float(np.sqrt(A)) * float(np.sqrt(Bn))))


@pytest.mark.parametrize("mut,dogleg_type", [("", 0), ("", 1), ("cross_gl", 0), ("drop_const", 0), ("unclamped", 0), ("no_s2", 0),
                                             ("g2_in_mcc", 0), ("no_huber", 0), ("cross_twice", 0), ("subspace_largest", 1)])
def test_dogleg_bars_hold_the_device_arithmetic_and_reject_plausible_errors(mut, dogleg_type):
    """The device's formulas restated in float64 sit within the bars of test_gpu_hp_dogleg.py (max ratio <= 0.5); each plausible
    kernel error exceeds them by more than 10x."""
    ref, rows, rows_nh = _mutation_problem()
    ratio = _mutation_ratios(ref, rows_nh if mut == "no_huber" else rows, _dogleg_radius(ref), dogleg_type, mut)
    print("mutation", mut or "none", dogleg_type, ratio)
    if mut:
        assert ratio > 10.0, (mut, ratio)
    else:
        assert ratio <= 0.5, ratio


@pytest.mark.parametrize("mut", ["", "no_border"])
def test_dogleg_bars_reject_a_missing_border_term(mut):
    """Lighting terms with all shared blocks free: the border step in e_g of k_ph_dogleg_gn."""
    prob, ph = synth.make_phong_problem(8, 60, num_materials=4, seed=4)
    d = ph.as_oracle_dict("truth")
    rows = hp.phong_observation_rows(prob.camera, prob.poses_init, prob.points_init, d["normals"], prob.obs_pose, prob.obs_point,
                                     prob.obs_uvd, prob.stiffness(), d, 0.0, 7)
    const = np.zeros(prob.num_poses, bool)
    const[0] = True
    fidx = hp.free_index(prob.num_poses, prob.obs_pose, const)
    ref = hp.DoglegReference(rows, prob.obs_pose, prob.obs_point, fidx, prob.num_points, 1e-3)
    assert ref.nb == 19
    ratio = _mutation_ratios(ref, rows, _dogleg_radius(ref), 0, mut)
    print("mutation", mut or "none", ratio)
    if mut:
        assert ratio > 10.0, (mut, ratio)
    else:
        assert ratio <= 0.5, ratio


# ------------------------------------------------------------------------ the second half of a trust-region iteration
def _rand_pose(rng, scale=50.0):
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    Q = Q * np.sign(np.linalg.det(Q))
    return np.concatenate([rng.normal(size=3) * scale, Q.ravel()])


def test_se3_plus_closed_forms():
    """Rotation about one axis in closed form, the composition Plus(Plus(T, a e), b e) = Plus(T, (a + b) e) about a fixed
    axis, and the first-order branch at |eps_r| <= DBL_EPSILON."""
    LD = hp.LD
    rng = np.random.default_rng(0)
    T = _rand_pose(rng)
    t, R = np.asarray(T[:3], LD), np.asarray(T[3:], LD).reshape(3, 3)
    for th in (0.3, -2.5, 1e-9, 1e4):
        out, _ = hp.se3_plus(T, [0.25, -1.0, 2.0, 0, 0, th])
        c, s = np.cos(LD(th)), np.sin(LD(th))
        E = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], LD)
        ref = np.concatenate([E @ t + np.array([0.25, -1.0, 2.0], LD), (E @ R).ravel()])
        assert np.abs(out[0] - ref).max() <= 2.0 ** -60 * (1 + np.abs(T).max())
    e = rng.normal(size=3)
    e /= np.linalg.norm(e)
    a, b = 0.7, -0.2
    ax = lambda s: np.concatenate([np.zeros(3), np.asarray(e, LD) * LD(s)])
    one, _ = hp.se3_plus(hp.se3_plus(T, ax(a))[0][0], ax(b))
    both, _ = hp.se3_plus(T, ax(LD(a) + LD(b)))
    assert np.abs(one - both).max() <= 2.0 ** -58 * (1 + np.abs(T).max())
    # first-order branch: E = I + eps_r^ exactly up to DBL_EPSILON (beyond it Rodrigues gives the same to 2^-104), no 0 / 0 at 0
    for ang in (2.0 ** -52, 1e-20, 2.0 ** -52 * (1 + 2.0 ** -50)):
        out, bar = hp.se3_plus(T, np.array([0, 0, 0, ang, 0, 0]))
        E1 = np.eye(3, dtype=LD) + np.array([[0, 0, 0], [0, 0, -ang], [0, ang, 0]], LD)
        exact = np.concatenate([E1 @ t, (E1 @ R).ravel()])
        assert np.abs(out[0] - exact).max() <= (0 if ang <= 2.0 ** -52 else 2.0 ** -100) and np.all(np.isfinite(bar))
    out, _ = hp.se3_plus(T, np.zeros(6))
    assert np.all(out[0] == np.asarray(T, LD))


def test_se3_plus_and_unit_plus_bars_hold_for_the_oracle():
    """The C oracle's fp64 Plus operators within the derived bars, small steps to angles far beyond pi."""
    rng = np.random.default_rng(1)
    worst = 0.0
    for scale in (1e-12, 1e-6, 1e-2, 1.0, 30.0, 1e4):
        for _ in range(50):
            T, eps = _rand_pose(rng), rng.normal(size=6) * scale
            ref, bar = hp.se3_plus(T, eps)
            worst = max(worst, float((np.abs(np.asarray(orc.se3_plus(T, eps), hp.LD) - ref[0]) / bar[0].clip(1e-300)).max()))
    assert worst <= 1.0, worst
    worst_u = 0.0
    for scale in (1e-12, 1e-3, 1.0, 100.0):
        for _ in range(50):
            x, d = rng.normal(size=3), rng.normal(size=3) * scale
            x /= np.linalg.norm(x)
            ref, bar = hp.unit_plus(x, d)
            worst_u = max(worst_u, float((np.abs(np.asarray(orc.unit_vector_plus(x, d), hp.LD) - ref[0]) / bar[0]).max()))
    assert worst_u <= 1.0, worst_u
    print("PLUSREF se3", worst, "unit", worst_u)


def test_unit_plus_closed_forms():
    LD = hp.LD
    out, _ = hp.unit_plus([0, 0, 1.0], [0.5, 0, 0.25])          # the component along x is projected out
    assert np.abs(out[0] - np.array([0.5, 0, 1], LD) / np.sqrt(LD(1.25))).max() <= 2.0 ** -62
    out, _ = hp.unit_plus([0, 3.0, 4.0], [0, 0.375, 0.5])        # parallel step: x / |x|
    assert np.abs(out[0] - np.array([0, 3, 4], LD) / 5).max() <= 2.0 ** -62 and abs(float((out[0] ** 2).sum()) - 1) < 1e-18


def test_projected_plus_clamps_after_the_add():
    (l, ph, tx), _ = hp.projected_plus(0, [1.0, 2, 3], [[0.5, 0.875, 2.0]], [0.125], [1, 1, 1, 0.25, 0.25, -5.0, -0.5], 7,
                                       bounds=([0, 0, 1, 0], [1, 1, np.inf, 1]))
    assert np.all(l == [2, 3, 4]) and np.all(ph == np.array([[0.75, 1.0, 1.0]], hp.LD)) and tx[0] == 0
    (l, ph, tx), _ = hp.projected_plus(1, [0, 0, 1.0], [[0.5, 0.9, 2.0]], [0.1], [0.5, 0, 0.25], 1)
    assert np.abs(l - np.array([0.5, 0, 1], hp.LD) / np.sqrt(hp.LD(1.25))).max() <= 2.0 ** -62 and ph[0, 0] == 0.5


def _tiny_problem(huber):
    return synth.make_problem(8, 60, track_len=5, seed=7, outlier_fraction=0.1 if huber else 0.0)


@pytest.mark.parametrize("case", ["stereo", "huber", "phong0", "phong1", "sun", "odometry_huber"])
def test_cost_at_against_the_oracle(case):
    """OracleProblem.cost (fp64) within the derived bar of the long-double cost."""
    factors, lighting, huber, const = None, None, 0.0, None
    if case in ("stereo", "huber"):
        huber = 1.345 if case == "huber" else 0.0
        prob = _tiny_problem(huber)
    elif case.startswith("phong"):
        prob, ph = synth.make_phong_problem(8, 60, track_len=5, seed=7, light_type=int(case[-1]), num_materials=4)
        lighting = ph.as_oracle_dict("perturbed")
    elif case == "sun":
        from test_oracle_pose_factors import _sun_problem
        prob, factors = _sun_problem(huber=0.5)
        const = np.zeros(prob.num_poses, np.uint8)
    else:
        from test_oracle_pose_factors import _odometry_factors
        prob = synth.make_problem(7, 100, track_len=4, seed=6)
        factors = _odometry_factors(prob, huber=0.05)
        const = np.zeros(prob.num_poses, np.uint8)
    args = (prob.camera, prob.poses_init, prob.points_init, prob.obs_pose, prob.obs_point, prob.obs_uvd, prob.stiffness())
    op = orc.OracleProblem(*args, pose_const=const, huber_a=huber, lighting=lighting, pose_factors=factors)
    c = hp.cost_at(*args, huber_a=huber, factors=factors, lighting=lighting)
    err = abs(float(hp.LD(op.cost()) - c["cost"]))
    print("COSTREF", case, "cost", float(c["cost"]), "err/bar", err / c["bar"], "bar/cost", c["bar"] / float(c["cost"]))
    assert err <= c["bar"], (err, c["bar"])
    assert c["bar"] <= 1e-9 * float(c["cost"])              # the bar is a bar: far below the oracle-parity tolerance


def _tiny_oracle(prob, huber):
    return orc.OracleProblem.from_synth(prob, huber_a=huber)


def _dl_norm(prob, huber, x_poses, x_points, radius, mu, dogleg_type):
    """|delta|_D of the dogleg step at this point from the long-double reference."""
    rows = hp.stereo_rows(prob.camera, x_poses, x_points, prob.obs_pose, prob.obs_point, prob.obs_uvd, prob.stiffness(), huber)
    const = np.zeros(prob.num_poses, bool)
    const[0] = True
    fidx = hp.free_index(prob.num_poses, prob.obs_pose, const)
    ref = hp.DoglegReference(rows, prob.obs_pose, prob.obs_point, fidx, prob.num_points, mu)
    gn, _ = ref.gauss_newton()
    sums = list(ref.param_sums(ref.v, gn)[0]) + [ref.row_sums(x, y)[0] for x, y in ((ref.v, ref.v), (gn, gn), (ref.v, gn))]
    return hp.dogleg_scalars(sums, radius, dogleg_type)["step_norm"]


def _iterate(prob, huber, o_kw, k):
    """The oracle's point after k iterations (the lowest-cost iterate: the current one while accepted costs decrease)."""
    op = _tiny_oracle(prob, huber)
    kw = dict(o_kw)
    kw["max_num_iterations"] = k
    op.solve(orc.default_options(**kw))
    return op.poses.copy(), op.points.copy()


def _x_norm(prob, poses, points):
    const = np.zeros(prob.num_poses, bool)
    const[0] = True
    fidx = hp.free_index(prob.num_poses, prob.obs_pose, const)
    present = np.unique(prob.obs_point)
    return hp.block_norms(fidx, present, poses, points), fidx, present


REPLAYS = [(s, dt, h, nm, r0) for h in (0.0, 1.345) for s, dt in ((0, 0), (1, 0), (1, 1)) for nm in (0, 1)
           for r0 in ((1.0, 1e4) if s == 0 else (1e4,))]


@pytest.mark.parametrize("strategy,dogleg_type,huber,nonmono,r0", REPLAYS)
def test_trust_region_decision_replays_the_oracle_log(strategy, dogleg_type, huber, nonmono, r0):
    """Whole oracle solves replayed by trust_region_decision from the logged costs and norms: every accept flag, every
    radius, the termination iteration and type.  Not in the log and taken from elsewhere: x_norm (the start's, with the
    steps taken so far as its bar -- the parameter tolerance stays beyond it), the model cost change (inverted from the
    logged rho by the evaluator's own formulas, which the replay carries), |delta|_D of a dogleg step with rho > 0.75 (from
    the long-double dogleg at the oracle's iterate; with outliers the Gauss-Newton step at mu = 1e-8 sends landmarks 1e6 away,
    its norm is not determined to a per cent in fp64, and the logged radius itself is taken where it grew) and the last, unlogged iteration that meets a tolerance (LM: the
    oracle's step at the final point, this file's Plus and the oracle's cost; DOGLEG runs end on max_num_iterations)."""
    LD = hp.LD
    prob = _tiny_problem(huber)
    o_kw = dict(trust_region_strategy_type=strategy, dogleg_type=dogleg_type, use_nonmonotonic_steps=nonmono,
                initial_trust_region_radius=r0, max_num_iterations=200 if strategy == 0 else (8 if huber else 3))
    op = _tiny_oracle(prob, huber)
    s, log = op.solve(orc.default_options(**o_kw))
    n = log["cost"].shape[0]
    opts = hp.trust_region_options(trust_region_strategy_type=strategy, use_nonmonotonic_steps=nonmono,
                                   max_num_iterations=o_kw["max_num_iterations"])
    st = hp.trust_region_state(log["cost"][0], r0, opts)
    (xn0, _), fidx, present = _x_norm(prob, prob.poses_init, prob.points_init)
    x_cost, iteration, moved, accepted_costs = LD(log["cost"][0]), 0, 0.0, [log["cost"][0]]
    flags, monotone = [], True
    for i in range(1, n):
        assert hp.can_continue(iteration, log["gradient_max_norm"][i - 1], st["radius"], opts) is None
        iteration += 1
        invalid = log["relative_decrease"][i] == 0 and log["step_norm"][i] == 0
        assert not invalid          # these problems produce none
        cc, rho_log = LD(log["cost_change"][i]), LD(log["relative_decrease"][i])
        cand = x_cost - cc
        mcc = (st["se_current"] - cand) / rho_log
        if (st["se_reference"] - cand) / (st["se_acc_ref"] + mcc) > rho_log * (1 + 1e-12):       # rho_1 was the larger quotient
            mcc = (st["se_reference"] - cand) / rho_log - st["se_acc_ref"]
        dl = None
        if strategy == 1 and rho_log > 0.75:
            if huber:       # (see the docstring: mu = 1e-8 and outliers)
                dl = max(LD(log["trust_region_radius"][i]), st["radius"]) / 3
            else:
                assert monotone
                xp, xl = _iterate(prob, huber, o_kw, iteration - 1)
                dl = _dl_norm(prob, huber, xp, xl, st["radius"], float(st["mu"]), dogleg_type)
        bars = dict(x_cost=4 * hp.U * float(x_cost), candidate_cost=4 * hp.U * float(x_cost), mcc=8 * hp.U * abs(float(mcc)),
                    x_norm=moved)
        d = hp.trust_region_decision(x_cost, cand, mcc, log["step_norm"][i], xn0, st, opts, dl_norm=dl, bars=bars)
        assert d["valid"] and d["termination"] is None, (i, d["termination"], d["margins"])
        assert d["margins"]["parameter"] > 1 and d["margins"]["accept"] > 1, (i, d["margins"])
        assert abs(float(d["rho"] - rho_log)) <= 1e-12 * abs(float(rho_log)), (i, d["rho"], rho_log)
        assert int(d["accepted"]) == log["step_is_successful"][i], (i, d["rho"])
        rbar = d["radius_bar"] + (1e-8 if strategy == 1 else 1e-13) * float(d["radius"])
        assert abs(float(d["radius"]) - log["trust_region_radius"][i]) <= rbar, (i, d["radius"], log["trust_region_radius"][i], rbar)
        st = d["state"]
        flags.append(int(d["accepted"]))
        if d["accepted"]:
            x_cost = LD(log["cost"][i])
            moved += log["step_norm"][i]
            monotone = monotone and log["cost"][i] < accepted_costs[-1]     # then the written-back lowest-cost iterate is the current one
            accepted_costs.append(log["cost"][i])
        else:
            assert abs(float(cand) - log["cost"][i]) <= 8 * hp.U * float(x_cost)      # a rejected row logs the candidate's cost
    assert 0 in flags or r0 == 1e4 or huber == 0.0 or nonmono       # the monotonic radius-1 outlier run rejects a step
    end = hp.can_continue(iteration, log["gradient_max_norm"][n - 1], st["radius"], opts)
    if end is not None:
        assert (end, s.termination_type) in (("no_convergence", 1), ("gradient", 0), ("radius", 0)) and s.num_iterations == n
        return
    if not monotone:        # a non-monotonic run that accepted an increase: the oracle hands back its best point, not the last
        assert nonmono and s.termination_type == 0
        return
    # the last iteration met a tolerance and was not logged: LM only (DOGLEG runs are cut by max_num_iterations above)
    assert strategy == 0 and s.termination_type == 0
    op2 = orc.OracleProblem(prob.camera, op.poses, op.points, prob.obs_pose, prob.obs_point, prob.obs_uvd, prob.stiffness(),
                            huber_a=huber)
    assert op2.cost() == accepted_costs[-1] or abs(op2.cost() - accepted_costs[-1]) <= 1e-12 * accepted_costs[-1]
    dp, dlm, mcc = op2.lm_step(float(st["radius"]))
    cp, _ = hp.se3_plus(op.poses, dp)
    cp = np.where((fidx >= 0)[:, None], np.asarray(cp, np.float64), op.poses)
    cl = op.points + dlm
    cand = orc.OracleProblem(prob.camera, cp, cl, prob.obs_pose, prob.obs_point, prob.obs_uvd, prob.stiffness(), huber_a=huber).cost()
    sn, _ = hp.block_norms(fidx, present, op.poses, op.points, cp, cl)
    xn, _ = hp.block_norms(fidx, present, op.poses, op.points)
    d = hp.trust_region_decision(x_cost, cand, mcc, sn, xn, st, opts)
    assert d["termination"] in ("function", "parameter"), d
    assert min(d["margins"][k] for k in ("parameter", "function") if k in d["margins"]) > 0
    assert iteration + 1 == n           # the terminating iteration is the one after the last logged row


def test_the_outlier_problem_rejects_its_third_lm_step_from_radius_one():
    prob = _tiny_problem(1.345)
    s, log = _tiny_oracle(prob, 1.345).solve(orc.default_options(initial_trust_region_radius=1.0))
    assert log["step_is_successful"][3] == 0 and -0.2 < log["relative_decrease"][3] < 0, log["relative_decrease"][:5]


def test_gradient_max_norm_and_step_norm_against_the_oracle_log():
    """Row 0's gradient max norm and row 1's step norm of an oracle solve within the derived bars of the references."""
    for huber in (0.0, 1.345):
        prob = _tiny_problem(huber)
        op = _tiny_oracle(prob, huber)
        s, log = op.solve(orc.default_options(max_num_iterations=1, initial_trust_region_radius=1e4))
        rows = hp.stereo_rows(prob.camera, prob.poses_init, prob.points_init, prob.obs_pose, prob.obs_point, prob.obs_uvd,
                              prob.stiffness(), huber)
        (xn, _), fidx, present = _x_norm(prob, prob.poses_init, prob.points_init)
        ref = hp.DoglegReference(rows, prob.obs_pose, prob.obs_point, fidx, prob.num_points, 1e-8)
        g, bar = hp.gradient_max_norm(ref, fidx, prob.poses_init)
        assert abs(float(hp.LD(log["gradient_max_norm"][0]) - g)) <= bar and bar <= 1e-9 * float(g), (g, bar)
        assert log["step_is_successful"][1] == 1
        sn, sbar = hp.block_norms(fidx, present, prob.poses_init, prob.points_init, op.poses, op.points)
        assert abs(float(hp.LD(log["step_norm"][1]) - sn)) <= sbar and sbar <= 1e-12 * float(sn), (sn, sbar)


def test_trust_region_decision_margins_and_invalid_steps():
    """The margins measure the distance to each threshold in units of the propagated bars; an invalid step takes the LM /
    DOGLEG StepIsInvalid path and the fifth in a row fails."""
    o = hp.trust_region_options()
    st = hp.trust_region_state(100.0, 10.0, o)
    d = hp.trust_region_decision(100.0, 99.0, 2.0, 1.0, 50.0, st, o, bars=dict(x_cost=0.1, candidate_cost=0.1, mcc=0.0))
    assert d["accepted"] and float(d["rho"]) == 0.5 and abs(d["rho_bar"] - 0.1) < 1e-6
    assert abs(d["margins"]["accept"] - (0.5 - 1e-3) / 0.1) < 1e-4 and float(d["radius"]) == 10.0
    d = hp.trust_region_decision(100.0, 99.0, 1.0, 1.0, 50.0, st, o)                    # rho = 1: radius * 3
    assert float(d["radius"]) == 30.0 and d["margins"]["accept"] == float("inf")
    d = hp.trust_region_decision(100.0, 100.5, 1.0, 1.0, 50.0, st, o)                   # rejected: radius / 2, then / 4
    assert not d["accepted"] and float(d["radius"]) == 5.0 and float(d["state"]["decrease_factor"]) == 4.0
    d2 = hp.trust_region_decision(100.0, 100.5, 1.0, 1.0, 50.0, d["state"], o)
    assert float(d2["radius"]) == 1.25
    assert hp.trust_region_decision(100.0, 100.0 - 5e-5, 1.0, 1.0, 50.0, st, o)["termination"] == "function"
    assert hp.trust_region_decision(100.0, 99.0, 1.0, 5e-7, 50.0, st, o)["termination"] == "parameter"
    s = st
    for k in range(5):
        d = hp.trust_region_decision(100.0, 99.0, -1.0, 1.0, 50.0, s, o)
        assert not d["valid"] and d["termination"] == ("failure" if k == 4 else None)
        s = d["state"]
    assert float(s["radius"]) == 10.0 / (2 * 4 * 8 * 16 * 32)
    od = hp.trust_region_options(trust_region_strategy_type=1)
    d = hp.trust_region_decision(100.0, 99.0, -1.0, 1.0, 50.0, hp.trust_region_state(100.0, 10.0, od), od)
    assert float(d["state"]["mu"]) == float(hp.LD(1e-8) * 10) and float(d["radius"]) == 10.0
    d = hp.trust_region_decision(100.0, 99.0, 1.1, 1.0, 50.0, hp.trust_region_state(100.0, 10.0, od), od, dl_norm=4.0)
    assert float(d["radius"]) == 12.0 and d["accepted"]
    d = hp.trust_region_decision(100.0, 99.9, 1.0, 1.0, 50.0, hp.trust_region_state(100.0, 10.0, od), od, dl_norm=4.0)
    assert float(d["radius"]) == 5.0 and d["accepted"]
    # non-monotonic: a cost increase within the allowance is accepted against the reference cost
    on = hp.trust_region_options(use_nonmonotonic_steps=1)
    s = hp.trust_region_decision(100.0, 90.0, 10.0, 1.0, 50.0, hp.trust_region_state(100.0, 10.0, on), on)["state"]
    assert float(s["se_reference"]) == 100.0 and float(s["se_current"]) == 90.0 and float(s["se_acc_ref"]) == 10.0
    d = hp.trust_region_decision(90.0, 91.0, 1.0, 1.0, 50.0, s, on)
    assert float(d["rho0"]) == -1.0 and abs(float(d["rho1"]) - 9.0 / 11.0) < 1e-15 and d["accepted"]


# ------------------------------------------------------------------------------------------------------- pose-factor rows
import pose_factor_edges as pfe

PF_BATCHES = ["prior", "sun", "relative_a", "relative_b", "relative_huber"]


def _pf_ratios(rows, got):
    """Worst |got - truth| / (C_ROW u mag) over the residuals and over the Jacobians; `got`: (r, [J per pose]) per factor."""
    wr = wj = 0.0
    for a, (r, Js) in zip(rows, got):
        assert len(Js) == len(a["blocks"])
        dr = np.abs(np.asarray(np.asarray(r, hp.LD) - a["r"], np.float64))
        bar = hp.C_ROW * hp.U * a["mag_r"]
        if dr.any():
            wr = max(wr, float((dr / np.maximum(bar, 1e-300)).max()))
        for J, (_, Jt), (_, m) in zip(Js, a["blocks"], a["mag_blocks"]):
            dj = np.abs(np.asarray(np.asarray(J, hp.LD) - Jt, np.float64))
            if dj.any():
                wj = max(wj, float((dj / np.maximum(hp.C_ROW * hp.U * m, 1e-300)).max()))
    return wr, wj


@pytest.mark.parametrize("name", PF_BATCHES)
def test_fp64_pose_factor_rows_meet_the_row_bar_on_every_edge_batch(name):
    """The proof that C_ROW u mag is a bar the reference's own formulas meet in fp64: np_reference in complex128 against the
    long-double rows, on every row of every edge batch (none left out), after the batch has shown that it holds its edges."""
    poses, factors = pfe.batches()[name]
    rows = pfe.truth(name)
    pfe.assert_edges(name, poses, factors, rows)
    r64 = hp.pose_factor_rows(poses, factors, dtype=np.float64, mags=False)
    assert len(r64) == len(rows) == len(factors)
    assert [a["outlier"] for a in r64] == [a["outlier"] for a in rows]
    wr, wj = _pf_ratios(rows, [(a["r"], [J for _, J in a["blocks"]]) for a in r64])
    print("HPREF pose-factor rows fp64", name, f"rows={len(rows)} r_over_bar={wr:.3g} J_over_bar={wj:.3g}")
    assert wr <= 1.0 and wj <= 1.0, (name, wr, wj)


def _dev_so3_log(R):
    axis = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = 0.5 * np.sqrt(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2])
    c = 0.5 * (R[0, 0] + R[1, 1] + R[2, 2] - 1.0)
    angle = np.arctan2(s, c)
    if abs(angle) <= 2.0 ** -52:
        return 0.5 * axis
    return 0.5 * angle * axis / s


def _dev_inv_right_jacobian(phi, mut=""):
    th2 = phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2]
    th = np.sqrt(th2)
    W = npr.wedge(phi)
    if mut == "series_everywhere":
        c = 1.0 / 12.0 + th2 / 720.0
    else:
        c = 1.0 / 12.0 + th2 / 720.0 if th < 1e-5 else 1.0 / th2 - (1.0 + np.cos(th)) / (2.0 * th * np.sin(th))
    return np.eye(3) + 0.5 * W + c * (W @ W)


def _device_pose_factor(f, poses, mut=""):
    """The arithmetic of pf_prior / pf_sun / pf_rel and the corrector of pf_evaluate in fp64 (closed-form Jacobians), written
    out on the host; `mut`: a plausible kernel error."""
    S = np.asarray(f["stiffness"], np.float64)
    d = np.asarray(f["data"], np.float64)
    T = poses[f["pose"]]
    if f["type"] == 1:
        S = S.reshape(2, 2)
        oc, eg = d[:3] / np.sqrt(d[:3] @ d[:3]), d[3:6] / np.sqrt(d[3:6] @ d[3:6])
        sc = T[3:].reshape(3, 3) @ eg
        raz, rzen = np.arctan2(sc[0], sc[2]) - np.arctan2(oc[0], oc[2]), np.arccos(-sc[1]) - np.arccos(-oc[1])
        if raz > np.pi:
            raz -= 2 * np.pi
        elif raz < -np.pi:
            raz += 2 * np.pi
        kaz, kzen = not abs(raz) > d[6], not abs(rzen) > d[7]
        raz, rzen = raz * kaz, rzen * kzen
        r = S @ np.array([raz, rzen])
        x, y, z = sc
        d2 = x * x + z * z
        gaz, gzen = np.array([z / d2, 0.0, -x / d2]), np.array([0.0, 1.0 / np.sqrt(1.0 - y * y), 0.0])
        jaz, jzen = -np.cross(gaz, sc) * kaz, -np.cross(gzen, sc) * (kzen or mut == "threshold_keeps_gradient")
        Js = [np.concatenate([np.zeros((2, 3)), S @ np.stack([jaz, jzen])], 1)]
    elif f["type"] == 0:
        S = S.reshape(6, 6)
        Rres = d[3:12].reshape(3, 3) @ T[3:].reshape(3, 3).T
        e = np.concatenate([d[:3] - Rres @ T[:3], _dev_so3_log(Rres)])
        r = S @ e
        Jr = _dev_inv_right_jacobian(e[3:], mut)
        Js = [-S @ np.block([[Rres, np.zeros((3, 3))], [np.zeros((3, 3)), Jr]])]
    else:
        S = S.reshape(6, 6)
        T2, Rr = poses[f["pose2"]], d[3:12].reshape(3, 3)
        R12 = T[3:].reshape(3, 3) @ T2[3:].reshape(3, 3).T
        v = T[:3] - R12 @ T2[:3]
        Rres = Rr @ R12
        e = np.concatenate([Rr @ v + d[:3], _dev_so3_log(Rres)])
        r = S @ e
        Jr = _dev_inv_right_jacobian(e[3:], mut)
        Z = np.zeros((3, 3))
        Js = [S @ np.block([[Rr, -Rr @ npr.wedge(v)], [Z, (Jr if mut == "left_is_right" else Jr.T) @ Rr]]), -S @ np.block([[Rres, Z], [Z, Jr]])]
    sq, a = r @ r, f.get("huber", 0.0)
    if a > 0 and sq > a * a:
        w = np.sqrt(a / np.sqrt(sq))
        r = r * w
        Js = [J * (1.0 if (mut == "huber_on_first_only" and i == 1) else w) for i, J in enumerate(Js)]
    return r, Js


@pytest.mark.parametrize("name", PF_BATCHES)
def test_device_closed_forms_meet_the_pose_factor_row_bar_and_plausible_errors_do_not(name):
    """The kernels' closed forms (inverse right Jacobian with its series branch, the angle gradients of the sun block) on the
    host in fp64, against the long-double complex-step rows at the same bar -- and four plausible errors that must not pass
    it: the series coefficient used beyond its branch, Jr^-1 in place of Jl^-1 for the first pose of a relative block, the
    Huber scale on J_1 but not on J_2, a zeroed zenith residual that keeps its gradient."""
    poses, factors = pfe.batches()[name]
    rows = pfe.truth(name)
    wr, wj = _pf_ratios(rows, [_device_pose_factor(f, poses) for f in factors])
    print("HPREF pose-factor rows closed-form", name, f"r_over_bar={wr:.3g} J_over_bar={wj:.3g}")
    assert wr <= 1.0 and wj <= 1.0, (name, wr, wj)
    muts = {"prior": ["series_everywhere"], "sun": ["threshold_keeps_gradient"], "relative_a": [], "relative_b": ["series_everywhere", "left_is_right"],
            "relative_huber": ["huber_on_first_only", "left_is_right"]}[name]
    for mut in muts:
        _, mj = _pf_ratios(rows, [_device_pose_factor(f, poses, mut) for f in factors])
        assert mj > 1e3, (name, mut, mj)


def test_long_double_pose_factor_jacobians_match_central_differences():
    """On the generic rows (angles 1e-3 and 1, no Huber, nothing zeroed) the complex-step Jacobians against a long-double
    central difference of the long-double residual through hp.se3_plus: step 2^-20, so the truncation is ~2^-40 |J| and the
    rounding 2^-64 2^20 mag."""
    h = hp.LD(2.0) ** -20
    for name in ("prior", "sun", "relative_b"):
        poses, factors = pfe.batches()[name]
        pick = [i for i, f in enumerate(factors) if f["edge"] and (f["edge"][0] == "generic" or f["edge"][:2] in (("angle", "1e-3"), ("angle", "1")))]
        assert len(pick) >= 4
        fs = [dict(factors[i], huber=0.0) for i in pick]
        rows = hp.pose_factor_rows(poses, fs, mags=False)
        for which in range(2 if name == "relative_b" else 1):
            touched = sorted({f["pose2" if which else "pose"] for f in fs})
            for c in range(6):
                res = []
                for sgn in (1, -1):
                    eps = np.zeros((len(touched), 6), hp.LD)
                    eps[:, c] = sgn * h
                    P = np.asarray(poses, hp.LD).copy()
                    P[touched] = hp.se3_plus(poses[touched], eps)[0]
                    res.append([a["r"] for a in _pf_rows_ld(P, fs)])
                for a, rp, rm in zip(rows, *res):
                    J = a["blocks"][which][1]
                    fd = (rp - rm) / (2 * h)
                    assert float(np.abs(fd - J[:, c]).max()) <= 1e-9 * max(float(np.abs(J).max()), 1e-300)


def _pf_rows_ld(P, fs):
    """pose_factor_rows at long-double poses (the central difference moves them off the fp64 grid)."""
    out = []
    for f in fs:
        d = np.asarray(f["data"], hp.LD)
        m = 2 if f["type"] == 1 else 6
        S = np.asarray(f["stiffness"], hp.LD).reshape(m, m)
        c = lambda v: np.asarray(v, np.clongdouble)[None]
        if f["type"] == 0:
            r = npr.pose_prior_residual(c(P[f["pose"]]), c(d[:12]), c(S))
        elif f["type"] == 1:
            r = npr.sun_sensor_residual(c(P[f["pose"]]), c(d[:3]), c(d[3:6]), c(S), c(d[6])[0], c(d[7])[0])
        else:
            r = npr.relative_pose_residual(c(P[f["pose"]]), c(P[f["pose2"]]), c(d[:12]), c(S))
        out.append(dict(r=r[0].real))
    return out


def test_huber_corrector_and_zeroed_sun_rows_behave_as_documented():
    for name in ("prior", "sun", "relative_huber"):
        poses, factors = pfe.batches()[name]
        rows = pfe.truth(name)
        raw = hp.pose_factor_rows(poses, [dict(f, huber=0.0) for f in factors], mags=False)
        n_out = 0
        for f, a, b in zip(factors, rows, raw):
            a_h = hp.LD(f.get("huber", 0.0))
            assert a["sq"] == b["sq"] and np.array_equal(b["r"] * b["r"], b["r"] ** 2) and not b["outlier"]
            assert a["outlier"] == bool(a_h > 0 and a["sq"] > a_h * a_h)
            w = np.sqrt(a_h / np.sqrt(a["sq"])) if a["outlier"] else hp.LD(1)
            tol = hp.LD(2.0) ** -60
            assert np.all(np.abs(a["r"] - w * b["r"]) <= tol * np.abs(b["r"]))
            for (_, Ja), (_, Jb) in zip(a["blocks"], b["blocks"]):
                assert np.all(np.abs(Ja - w * Jb) <= tol * np.abs(Jb))
            rho = 2 * a_h * np.sqrt(a["sq"]) - a_h * a_h if a["outlier"] else a["sq"]
            assert abs(a["cost"] - rho / 2) <= tol * rho
            if f["edge"] and f["edge"][0] == "huber":       # the corrected row is continuous across the switch
                assert abs(float(w) - 1) <= f["edge"][1]
            n_out += a["outlier"]
        assert n_out >= 4
    poses, factors = pfe.batches()["sun"]
    for f, a in zip(factors, pfe.truth("sun")):
        if not (f["edge"] and f["edge"][0] == "threshold"):
            continue
        S = np.asarray(f["stiffness"], hp.LD).reshape(2, 2)
        J = a["blocks"][0][1]
        zero_az, zero_zen = f["edge"][1], f["edge"][2]
        if zero_az and zero_zen:     # both angles zeroed: the row, its Jacobian and their bars are exact zeros
            assert not a["r"].any() and not J.any() and not a["mag_r"].any() and not a["mag_blocks"][0][1].any()
        elif zero_az or zero_zen:    # one angle left: r and every column of J are multiples of that angle's column of S
            col = S[:, 1 if zero_az else 0]
            assert a["r"].any() and J[:, 3:].any() and not J[:, :3].any()
            for v in [a["r"]] + [J[:, c] for c in range(3, 6)]:
                assert abs(v[0] * col[1] - v[1] * col[0]) <= hp.LD(2.0) ** -60 * abs(v[0] * col[1])
        else:
            assert abs(np.linalg.det(np.asarray(J[:, 3:] @ J[:, 3:].T, np.float64))) > 0


def test_fp64_pose_factor_rows_agree_with_unary_rows():
    """unary_rows (the fp64 rows the dogleg and candidate references were built on) and pose_factor_rows at np.float64 are two
    fp64 evaluations of the same formulas: both within the row bar of the long-double rows."""
    from test_oracle_pose_factors import _odometry_factors, _sun_problem
    prob, factors = _sun_problem(huber=0.5)
    factors = factors + _odometry_factors(prob, huber=0.05)[1:]
    rows = hp.pose_factor_rows(prob.poses_init, factors)
    for got in (hp.unary_rows(prob.poses_init, factors), hp.pose_factor_rows(prob.poses_init, factors, dtype=np.float64, mags=False)):
        wr, wj = _pf_ratios(rows, [(a["r"], [J for _, J in a["blocks"]]) for a in got])
        assert wr <= 1.0 and wj <= 1.0, (wr, wj)


@pytest.mark.parametrize("huber", [0.0, 0.05])
def test_oracle_system_with_odometry_blocks_is_within_the_assembly_bound_and_plausible_errors_are_not(huber):
    """SchurSystem with the long-double factor blocks (PoseFactorSums) on a chain whose last states are free through odometry
    alone: the oracle's fp64 system and step meet E; a cross block stored transposed, or one whose Huber scale reached J_1 but
    not J_2, does not."""
    import dataclasses
    from test_oracle_pose_factors import _odometry_factors
    prob = synth.make_problem(9, 300, track_len=5, seed=6)
    keep = prob.obs_pose <= 4
    prob = dataclasses.replace(prob, obs_pose=prob.obs_pose[keep], obs_point=prob.obs_point[keep], obs_uvd=prob.obs_uvd[keep])
    const = np.zeros(9, np.uint8)
    factors = _odometry_factors(prob, loop=False, huber=huber)
    rows = hp.stereo_rows(prob.camera, prob.poses_init, prob.points_init, prob.obs_pose, prob.obs_point, prob.obs_uvd, prob.stiffness())
    assert (hp.free_index(9, prob.obs_pose, const) >= 0).sum() == 5
    fidx = hp.free_index(9, prob.obs_pose, const, hp.factor_poses(factors))
    assert np.array_equal(fidx, np.arange(9))
    pr = hp.pose_factor_rows(prob.poses_init, factors)
    assert huber == 0 or sum(a["outlier"] for a in pr) >= 1
    sy = hp.SchurSystem(rows, prob.obs_pose, prob.obs_point, fidx, prob.num_points, 20.0, factor_sums=hp.PoseFactorSums(9, factors, pr))
    op = orc.OracleProblem(prob.camera, prob.poses_init, prob.points_init, prob.obs_pose, prob.obs_point, prob.obs_uvd, prob.stiffness(),
                           pose_const=const, pose_factors=factors)
    S, rhs, _ = op.reduced_system(20.0)
    dp, dl, mcc = op.lm_step(20.0)
    ex = sy.assembly_excess(S, rhs)
    assert max(ex) <= 1.0, ex
    mref, mag, nt = sy.model_cost_change(dp.ravel(), dl[sy.lm])
    assert abs(mcc - float(mref)) <= (nt + hp.C_TERMS) * hp.U * mag
    blk = lambda a, b: (slice(6 * a, 6 * a + 6), slice(6 * b, 6 * b + 6))
    bad = S.copy()
    bad[blk(6, 7)] = S[blk(6, 7)].T
    assert sy.assembly_excess(bad, rhs)[0] > 1e3
    out = [i for i, a in enumerate(pr) if a["outlier"] and factors[i]["type"] == 2]
    if out:
        i = out[-1]
        (k1, J1), (k2, J2) = pr[i]["blocks"]
        w = float(np.sqrt(hp.LD(huber) / np.sqrt(pr[i]["sq"])))
        bad = S.copy()
        bad[blk(k1, k2)] += np.asarray(J1.T @ J2, np.float64) * (1 / w - 1)
        assert sy.assembly_excess(bad, rhs)[0] > 1e3


# ------------------------------------------------------------------------------------------------- se3_minus and the recovered step
def test_se3_minus_inverts_se3_plus_within_its_bar():
    """se3_minus(se3_plus(T, eps), T) == eps for steps from 1e-9 to 1 and on the first-order branch of se3_plus (|eps_r| <=
    DBL_EPSILON, zero included) -- with the candidate kept in long double, and rounded to fp64 as a device writes it back, which
    is the error the bar is made for: an fp64 entry of Plus is within its se3_plus bar of the truth."""
    rng = np.random.default_rng(11)
    scales = [1e-9, 1e-7, 1e-5, 1e-3, 1e-2, 0.1, 0.5, 1.0, 1e-17, 0.0]
    T = np.stack([_rand_pose(rng) for _ in range(8 * len(scales))])
    eps = rng.standard_normal((T.shape[0], 6)) * np.repeat(scales, 8)[:, None]
    eps[-16:, :3] = rng.standard_normal((16, 3)) * 1e-3                    # first-order rotations with an ordinary translation
    ang = np.sqrt((eps[:, 3:] ** 2).sum(1))
    assert (ang <= hp.DBL_EPSILON).sum() == 16 and ang.max() > 0.5
    Tn, pb = hp.se3_plus(T, eps)
    for cand in (Tn, np.asarray(Tn, np.float64)):
        back, bar = hp.se3_minus(cand, T)
        err = np.abs(np.asarray(back - np.asarray(eps, hp.LD), np.float64))
        assert np.all(err <= bar), float((err / bar).max())
    # the rounded candidate does use the bar (the check is not vacuous), and a rotation entry off by 1e-10 leaves it
    assert (err / bar).max() > 1e-3
    bad = np.asarray(Tn, np.float64)
    bad[:, 4] += 1e-10
    back, bar = hp.se3_minus(bad, T)
    assert np.all((np.abs(np.asarray(back - np.asarray(eps, hp.LD), np.float64)) / bar).max(1) > 1)


@pytest.mark.parametrize("huber,strategy,dogleg_type,radius", [(0.0, 0, 0, 1e4), (1.345, 0, 0, 30.0), (0.0, 1, 0, 3.0)])
def test_recovered_step_comparison_holds_with_the_oracle_as_the_ranks(huber, strategy, dogleg_type, radius):
    """The whole comparison of tests/test_gpu_hp_sharded.py with one iteration of the CPU oracle in place of the ranks: the
    precondition, the recovery of the step from the written-back point, every bar."""
    import test_gpu_hp_sharded as sh
    T = sh.truth((61, 2400, 8), huber, strategy, dogleg_type, radius)
    out = sh.compare(f"oracle {T['tag']}", T, [sh.oracle_as_rank(T)])
    assert out["fe"] < 1e-11 and out["r_fe"] < 1e-2                       # the recovery costs nothing against the bar


# ------------------------------------------------------------------------------------------- the projected line search
def _oracle_armijo_steps(phi, dphi, capacity=24):
    """The C oracle's state machine (orc_armijo_trace) fed by evaluating phi at what it asks for: the hook replays a recorded
    sequence, so it is called with the evaluations so far plus a dummy that is never accepted."""
    import ctypes as C
    lib = orc.lib()
    dp = C.POINTER(C.c_double)
    lib.orc_armijo_trace.argtypes = [dp, dp, C.c_int, C.c_double, C.c_double, C.c_double, dp, dp]
    steps = []
    while len(steps) < capacity:
        vals = np.array([phi(x) for x in steps] + [1e300])
        grads = np.array([dphi(x) for x in steps] + [0.0])
        out, optimal = np.zeros(capacity + 2), C.c_double()
        n = lib.orc_armijo_trace(vals.ctypes.data_as(dp), grads.ctypes.data_as(dp), len(steps) + 1, phi(0.0), dphi(0.0), 1.0,
                                 out.ctypes.data_as(dp), C.byref(optimal))
        if n == len(steps):
            return steps, optimal.value
        steps.append(float(out[len(steps)]))
    return steps, -1.0


def _elimination_ratios(steps, phi, dphi):
    """|alpha_fp64 - alpha_mpmath| / (u kappa_inf(A) |alpha|) of every interior step of an fp64 search: the 50-digit minimiser
    of the fp64 side's OWN samples (exact inputs), so only its elimination and root finding differ."""
    init, out = (0.0, phi(0.0), dphi(0.0)), []
    for k in range(1, len(steps)):
        cur = (steps[k - 1], phi(steps[k - 1]), dphi(steps[k - 1]))
        smp = [init, cur] + ([(steps[k - 2], phi(steps[k - 2]), dphi(steps[k - 2]))] if k >= 2 else [])
        m = hp.interpolation_minimum(smp, hp.ARMIJO["max_step_contraction"] * cur[0], hp.ARMIJO["min_step_contraction"] * cur[0])
        if m["interior"]:
            out.append(abs(steps[k] - m["x"]) / (hp.U * m["kappa"] * abs(m["x"])))
        else:
            assert steps[k] == pytest.approx(m["x"], rel=1e-15), (steps, m)
    return out


def test_armijo_search_matches_the_fp64_restatements_and_fixes_the_elimination_constant():
    """hp.armijo_search on the 40 synthetic searches of tests/test_oracle_bounds.py against the numpy restatement and the C
    oracle: the same number of steps, the same accepted step, every step within 1e-6 (what those two are held to among
    themselves).  Then the constant of the elimination term: the worst |alpha_fp64 - alpha_50 digits| / (u kappa_inf(A) |alpha|)
    over all interior steps of both fp64 sides (each against the 50-digit minimiser of its own samples) is what ARMIJO_C
    quadruples."""
    from test_oracle_bounds import _np_armijo, _search_cases
    worst, interior, searched = 0.0, 0, 0
    for phi, dphi in _search_cases(40):
        s = hp.armijo_search(phi, dphi)
        steps, opt = _np_armijo(phi, dphi)
        osteps, oopt = _oracle_armijo_steps(phi, dphi)
        assert s["count"] == len(steps) == len(osteps), (s["alphas"], steps, osteps)
        np.testing.assert_allclose(s["alphas"], steps, rtol=1e-6)
        np.testing.assert_allclose(s["alphas"], osteps, rtol=1e-6)
        assert s["success"] == (opt > 0) == (oopt > 0) and (not s["success"] or s["optimal"] == pytest.approx(opt, rel=1e-6))
        assert s["kinds"][0] is None and len(s["kinds"]) == s["count"]
        for side in (steps, osteps):
            r = _elimination_ratios(side, phi, dphi)
            interior += len(r)
            worst = max([worst] + r)
        searched += s["count"] >= 3
    print(f"\nLSREF elimination constant: worst ratio {worst:.3g} over {interior} interior steps, ARMIJO_C = {hp.ARMIJO_C}")
    assert searched >= 10 and interior >= 40
    assert worst * 4 <= hp.ARMIJO_C and worst * 16 >= hp.ARMIJO_C, (worst, hp.ARMIJO_C)


def test_interpolation_minimum_closed_forms():
    """A cubic through two samples whose minimiser is known, a clamp on each side, and a sample that beats the polynomial."""
    p = lambda a: (a - 0.25) ** 2 * (a + 1.0) + 3.0            # minimum at a = 0.25 (the other stationary point is a = -0.5)
    dp = lambda a: 2 * (a - 0.25) * (a + 1.0) + (a - 0.25) ** 2
    smp = [(0.0, p(0.0), dp(0.0)), (1.0, p(1.0), dp(1.0))]
    m = hp.interpolation_minimum(smp, 1e-3, 0.6, [(1e-16, 1e-16)] * 2)
    assert m["kind"] == "root" and m["interior"] and abs(m["x"] - 0.25) < 1e-15 and m["x_bar"] < 1e-14 and m["edge_margin"] > 1e10
    assert hp.interpolation_minimum(smp, 0.3, 0.6)["kind"] == "lo" and hp.interpolation_minimum(smp, 1e-3, 0.2)["kind"] == "hi"
    # a root within its bar of the upper end: the edge margin says so
    m = hp.interpolation_minimum(smp, 1e-3, 0.25 + 1e-12, [(1e-9, 1e-9)] * 2)
    assert m["edge_margin"] < 1


def _ls_case(name="lm 2"):
    import test_gpu_hp_linesearch as ls
    case = ls.build_case(name)
    return ls, case, ls.reference_search(case)


def test_line_search_derivative_against_a_central_difference_of_the_cost():
    """phi'*(a) = delta . g* is the derivative of the cost along delta IN THE TANGENT SPACE OF THE TRIAL POINT x_a = Plus(x, a
    delta), with delta in full for entries on a bound -- so it is held against the central difference of eps -> cost(Plus(x_a,
    eps delta)) in long double with the projection switched off, at steps a where no entry's projection state changes within
    a (1 +- 1e-3).  It is NOT d/da cost(Plus(x, a delta)) for a > 0: SE3Perturbation adds delta_t to E t, so the tangent of the
    path at x_a has the translation delta_t + delta_r x (E t) while the trial point's own tangent space gives delta_t + delta_r x
    (E t + a delta_t) (second order in the step: 4e-7 of phi' at a = 0.05 here), and an entry held on its bound does not move
    at all.  Both differences are shown to be visible, so a reference that took the path derivative would fail this test."""
    ls, case, rs = _ls_case()
    spec, x = case["spec"], case["x"]
    free = ls.Spec(case["prob"], lighting=case["d"], shared_free=7, use_bounds=False)
    ref, rows = spec.reference(x, 1e-8)
    delta = ls._reference_step(spec, x, ref, rows, *case["strategy"], case["radius"])[0]
    M = len(x["texture"])
    lo = np.concatenate([np.tile(spec.bounds[0][:3], M), np.full(M, spec.bounds[0][3])])
    hi = np.concatenate([np.tile(spec.bounds[1][:3], M), np.full(M, spec.bounds[1][3])])
    x_sh = np.concatenate([np.asarray(x["phong"], hp.LD).ravel(), np.asarray(x["texture"], hp.LD).ravel()])
    db = ref.split(delta)[2][3:]
    state = lambda a: np.asarray((x_sh + hp.LD(a) * db < lo) | (x_sh + hp.LD(a) * db > hi))
    used, with_projection, path_differs = 0, 0, 0
    for a in (1e-3, 0.05, 0.25, 0.6, 1.0):
        if not (np.array_equal(state(a), state(a * (1 - 1e-3))) and np.array_equal(state(a), state(a * (1 + 1e-3)))):
            continue
        f = hp.line_search_function(spec, x, ref, delta, a)
        h = 2.0 ** -13

        def central(hh, along_path=False):
            if along_path:
                up, dn = (spec.cost(spec.plus(x, ref, hp.LD(a * (1 + s * hh)) * delta)[0]) for s in (1, -1))
                return (up["cost"] - dn["cost"]) / (2 * hp.LD(a) * hp.LD(hh))
            up, dn = (free.cost(free.plus(f["trial"], ref, hp.LD(s * hh) * delta)[0]) for s in (1, -1))
            return (up["cost"] - dn["cost"]) / (2 * hp.LD(hh))
        cd, cd2 = central(h), central(2 * h)
        # the truncation (third derivative times h^2 / 6) is a third of |cd(2 h) - cd(h)| (Richardson); the long-double rounding
        # of the two costs is their fp64 bar times 2^-11, over h
        tol = abs(float(cd2 - cd)) + f["phi_bar"] * 2.0 ** -11 / h
        assert abs(float(f["dphi"] - cd)) <= tol, (a, float(f["dphi"]), float(cd), tol)
        assert tol < 1e-6 * abs(float(f["dphi"])), (a, tol)          # the comparison resolves six digits at least
        used += 1
        proj = state(a)
        on_bound = (f["grad"].g[f["grad"].o_b + 3:][proj] * db[proj]).sum()
        with_projection += bool(proj.any() and abs(float(on_bound)) > 1e3 * tol)
        path_differs += bool(abs(float(f["dphi"] - on_bound - central(h, along_path=True))) > 10 * tol)
    assert used >= 3 and with_projection >= 1 and path_differs >= 1, (used, with_projection, path_differs)


def test_line_search_bars_reject_a_scaled_step_where_the_full_one_belongs():
    """Two plausible restatements: phi' formed with alpha delta (an alpha applied twice), and rho formed with the model cost
    change of alpha delta instead of delta.  Both leave their bars by orders of magnitude at the accepted step of the case."""
    ls, case, rs = _ls_case()
    spec, x = case["spec"], case["x"]
    ref, rows = spec.reference(x, 1e-8)
    delta, mcc, mag, dl_norm = ls._reference_step(spec, x, ref, rows, *case["strategy"], case["radius"])
    a = rs["alpha"]
    assert 0 < a < 0.6
    f = hp.line_search_function(spec, x, ref, delta, a)
    wrong = hp.line_search_function(spec, x, ref, hp.LD(a) * delta, 1.0, trial=f["trial"])
    assert abs(float(wrong["dphi"] - hp.LD(a) * f["dphi"])) <= 1e-15 * abs(float(f["dphi"]))
    assert abs(float(wrong["dphi"] - f["dphi"])) > 1e6 * f["dphi_bar"], (float(wrong["dphi"]), float(f["dphi"]), f["dphi_bar"])
    dec = rs["decision"]
    mcc_scaled = ref.model_cost_change(hp.LD(a) * delta)[0]
    rho_wrong = dec["cost_change"] / mcc_scaled
    assert abs(float(rho_wrong - dec["rho"])) > 1e6 * dec["rho_bar"], (float(rho_wrong), float(dec["rho"]), dec["rho_bar"])


LS_CPU_CASES = ["lm 2", "lm 3", "traditional 2", "traditional 3", "subspace 2", "subspace 3", "two panels 2", "lm long", "traditional long"]


@pytest.mark.parametrize("name", LS_CPU_CASES)
def test_line_search_references_hold_with_the_oracle_in_the_devices_place(name):
    """The cases of tests/test_gpu_hp_linesearch.py without a GPU: the reference alone clears its 4-bar conditions, counts the
    evaluations the oracle counted in that iteration, and the oracle's cost of the iteration (accepted: at its own written-back
    point) is within the cost bar of the long-double cost there."""
    ls, case, rs = _ls_case(name)
    s = rs["search"]
    print(f"\nLSREF cpu {name}: count {s['count']} oracle {case['oracle_count']} alphas {s['alphas']} margin {s['margin']:.3g} "
          f"decision margin {rs['decision_margin']:.3g} seconds {rs['cpu_seconds']:.1f}")
    assert rs["kept"], (s["armijo_margins"], s["choice_margins"], rs["decision"]["margins"])
    assert s["count"] == case["oracle_count"] == case["evals"]
    log, k = case["oracle_log"], case["k"]
    assert bool(log["step_is_successful"][k]) == rs["decision"]["accepted"]
    assert s["success"] or s["count"] >= 10          # the searches that fail are the long ones: the candidate is the full step again
    if rs["decision"]["accepted"]:
        c = case["spec"].cost(case["oracle_after"])
        assert abs(float(hp.LD(log["cost"][k]) - c["cost"])) <= c["bar"]


@pytest.mark.parametrize("name,margin", [("refused traditional a", 2.25), ("refused lm", 1.99), ("refused traditional b", 0.997)])
def test_line_search_candidates_that_are_refused(name, margin):
    """Candidates the 4-bar rule refuses: long searches that FAIL, whose last Armijo comparison (at alpha ~ 1e-9,
    where phi(alpha) - phi(0) is a few cost bars) is within 4 bars of its threshold.  Kept here so that the refusal is a result
    of the reference and not a choice: the count is still the oracle's."""
    ls, case, rs = _ls_case(name)
    s = rs["search"]
    assert not rs["kept"] and not s["success"] and s["count"] == case["oracle_count"] and 10 <= s["count"] <= 13
    assert s["margin"] == s["armijo_margins"][-1] == pytest.approx(margin, rel=0.05), s["armijo_margins"]
