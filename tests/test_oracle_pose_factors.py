"""Row N4: unary pose residual blocks of the sun-aided driver (tests/dataset_vo_sun.cpp:80-124) --
PoseErrorAutomatic (pose prior, pose_error.hpp:22-55) and SunSensorErrorAutomatic (sun_sensor_error.hpp:35-104).
The oracle's closed-form Jacobians against complex-step / finite differences of the reference formulas through
SE3Perturbation, and the LM step of a prior-anchored problem against a dense numpy solve.  CPU only."""
import ctypes as C

import numpy as np
import pytest

import np_reference as npr
from ceres_slam_amd import synth
from oracle import oracle as orc

_dp = C.POINTER(C.c_double)
# the reference formulas of the unary pose rows live in np_reference (shared with hp_reference)
_so3_log, _prior_res, _sun_res, _cs_jac = npr.so3_log, npr.pose_prior_residual, npr.sun_sensor_residual, npr.se3_complex_step_jacobian


def _c(a):
    return np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(_dp)


def _rand_pose(rng, scale=0.3):
    return npr.se3_plus(np.array([0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1.0]), np.concatenate([rng.normal(size=3), scale * rng.normal(size=3)]))


def test_pose_prior_residual_and_jacobian():
    L = orc.lib()
    L.orc_pose_prior_residual.argtypes = [_dp] * 5
    rng = np.random.default_rng(0)
    for it in range(100):
        T_ref = _rand_pose(rng, 1.0)
        T = npr.se3_plus(T_ref, np.concatenate([0.5 * rng.normal(size=3), (0.3 if it % 2 else 1e-9) * rng.normal(size=3)]))
        A = rng.normal(size=(6, 6))
        S = np.linalg.inv(np.linalg.cholesky(A @ A.T + np.eye(6)))
        r, J = np.zeros(6), np.zeros(36)
        L.orc_pose_prior_residual(_c(T), _c(T_ref), _c(S), r.ctypes.data_as(_dp), J.ctypes.data_as(_dp))
        np.testing.assert_allclose(r, _prior_res(T, T_ref, S), rtol=1e-11, atol=1e-12)
        np.testing.assert_allclose(J.reshape(6, 6), _cs_jac(lambda X: _prior_res(X, T_ref, S), T), rtol=1e-7, atol=1e-8)


def test_sun_sensor_residual_and_jacobian():
    L = orc.lib()
    L.orc_sun_residual.argtypes = [_dp, _dp, _dp, _dp, C.c_double, C.c_double, _dp, _dp]
    rng = np.random.default_rng(1)
    for it in range(200):
        T = _rand_pose(rng, 1.0)
        eg = rng.normal(size=3)
        oc = T[3:].reshape(3, 3) @ (eg / np.linalg.norm(eg)) + 0.05 * rng.normal(size=3)
        A = rng.normal(size=(2, 2))
        S = np.linalg.inv(np.linalg.cholesky(A @ A.T + np.eye(2)))
        taz, tzen = (1000.0, 1000.0) if it % 3 else (0.03, 0.03)       # dataset_vo_sun.cpp:28-29 defaults / tight
        r, J = np.zeros(2), np.zeros(12)
        L.orc_sun_residual(_c(T), _c(oc), _c(eg), _c(S), taz, tzen, r.ctypes.data_as(_dp), J.ctypes.data_as(_dp))
        np.testing.assert_allclose(r, _sun_res(T, oc, eg, S, taz, tzen), rtol=1e-11, atol=1e-13)
        np.testing.assert_allclose(J.reshape(2, 6), _cs_jac(lambda X: _sun_res(X, oc, eg, S, taz, tzen), T), rtol=1e-7, atol=1e-9)
    # wrap-around of the azimuth difference
    T = np.array([0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1.0])
    r = np.zeros(2)
    L.orc_sun_residual(_c(T), _c([0.02, -0.5, -1.0]), _c([-0.02, -0.5, -1.0]), _c(np.eye(2)), 1000.0, 1000.0, r.ctypes.data_as(_dp), None)
    assert abs(r[0]) < 0.1


def _sun_problem(P=8, L=120, seed=2, huber=0.0):
    prob = synth.make_problem(P, L, track_len=5, seed=seed)
    rng = np.random.default_rng(seed)
    sun_g = np.array([0.3, -0.8, 0.5])
    factors = [dict(pose=0, type=0, data=prob.poses_init[0], stiffness=np.eye(6) * 1e2)]          # prior on the first pose (:107-124)
    for k in range(P):
        if k % 4 == 3:
            continue                                                                               # state_has_sun_obs
        obs = prob.poses_gt[k][3:].reshape(3, 3) @ sun_g + 0.01 * rng.normal(size=3)
        factors.append(dict(pose=k, type=1, data=np.concatenate([obs, sun_g, [1000.0, 1000.0]]), stiffness=np.eye(2).ravel() * 50.0,
                            huber=huber))
    return prob, factors


def _rel_res(T1, T2, T_ref, S):
    """RelativePoseErrorAutomatic (relative_pose_error.hpp:22-40) on complex inputs: S log(T_ref T1 T2^-1)."""
    R1, R2, Rr = T1[3:].reshape(3, 3), T2[3:].reshape(3, 3), T_ref[3:].reshape(3, 3)
    R12 = R1 @ R2.T
    t = Rr @ (T1[:3] - R12 @ T2[:3]) + T_ref[:3]
    return S @ np.concatenate([t, _so3_log(Rr @ R12)])


def _check_lm_step_against_dense(prob, factors, radius=50.0):
    """The oracle's LM step against a dense restatement: complex-step Jacobians of every residual block, Jacobi
    scaling, clamped LM diagonal, one dense solve."""
    none_const = np.zeros(prob.num_poses, dtype=np.uint8)                                          # no constant pose: the prior anchors
    op = orc.OracleProblem(prob.camera, prob.poses_init, prob.points_init, prob.obs_pose, prob.obs_point, prob.obs_uvd, prob.stiffness(),
                           pose_const=none_const, pose_factors=factors)
    dp, dl, mcc = op.lm_step(radius)
    P, Lm = prob.num_poses, prob.num_points
    rows, r = [], []
    S = prob.stiffness()
    for i in range(prob.num_obs):
        k, j = int(prob.obs_pose[i]), int(prob.obs_point[i])
        Jp, Jl = npr.jacobians_complex_step(prob.camera, prob.poses_init[k], prob.points_init[j], prob.obs_uvd[i], S)
        ri = npr.residual_global(prob.camera, prob.poses_init[k], prob.points_init[j], prob.obs_uvd[i], S)
        for m in range(3):
            row = np.zeros(6 * P + 3 * Lm)
            row[6 * k: 6 * k + 6] = Jp[m]
            row[6 * P + 3 * j: 6 * P + 3 * j + 3] = Jl[m]
            rows.append(row); r.append(ri[m])
    cost = 0.5 * float(np.dot(r, r)) if not getattr(prob, "_huber", 0) else None
    for f in factors:
        k, T = f["pose"], prob.poses_init[f["pose"]]
        blocks = {}
        if f["type"] == 0:
            fun = lambda X: _prior_res(X, np.asarray(f["data"]), np.asarray(f["stiffness"]).reshape(6, 6))
            rf, blocks[k] = fun(T).real, _cs_jac(fun, T)
        elif f["type"] == 1:
            d = np.asarray(f["data"])
            fun = lambda X: _sun_res(X, d[:3], d[3:6], np.asarray(f["stiffness"]).reshape(2, 2), d[6], d[7])
            rf, blocks[k] = fun(T).real, _cs_jac(fun, T)
        else:       # relative pose block on (pose, pose2)
            k2, T2 = f["pose2"], prob.poses_init[f["pose2"]]
            Tr, Sf = np.asarray(f["data"], dtype=float), np.asarray(f["stiffness"]).reshape(6, 6)
            rf = _rel_res(T, T2, Tr, Sf).real
            blocks[k] = _cs_jac(lambda X: _rel_res(X, T2.astype(complex), Tr, Sf), T)
            blocks[k2] = _cs_jac(lambda X: _rel_res(T.astype(complex), X, Tr, Sf), T2)
        a = f.get("huber", 0.0)
        sq = rf @ rf
        sc = np.sqrt(a / np.sqrt(sq)) if a > 0 and sq > a * a else 1.0
        for m in range(len(rf)):
            row = np.zeros(6 * P + 3 * Lm)
            for kk, Jf in blocks.items():
                row[6 * kk: 6 * kk + 6] = Jf[m] * sc
            rows.append(row); r.append(rf[m] * sc)
    J, r = np.array(rows), np.array(r)
    active = np.concatenate([np.ones(6 * P, bool), np.repeat(np.bincount(prob.obs_point, minlength=Lm) > 0, 3)])
    J = J[:, active]
    scale = 1.0 / (1.0 + np.sqrt((J * J).sum(0)))
    Js = J * scale
    D = np.clip((Js * Js).sum(0), 1e-6, 1e32) / radius
    y = np.linalg.solve(Js.T @ Js + np.diag(D), Js.T @ r)
    delta = np.zeros(6 * P + 3 * Lm)
    delta[active] = -y * scale
    np.testing.assert_allclose(dp.ravel(), delta[:6 * P], rtol=1e-7, atol=1e-10)
    np.testing.assert_allclose(dl.ravel(), delta[6 * P:], rtol=1e-7, atol=1e-9)
    Jd = J @ delta[active]
    assert mcc == pytest.approx(-Jd @ (r + 0.5 * Jd), rel=1e-8)
    if all(f.get("huber", 0.0) == 0.0 for f in factors):
        assert op.cost() == pytest.approx(0.5 * float(r @ r), rel=1e-12)
    return op


@pytest.mark.parametrize("huber", [0.0, 0.5])
def test_lm_step_with_pose_factors_matches_dense_numpy_solve(huber):
    prob, factors = _sun_problem(huber=huber)
    _check_lm_step_against_dense(prob, factors)


def _odometry_factors(prob, seed=0, loop=True, huber=0.0):
    """RelativePoseErrorAutomatic blocks (tests/blowup_test.cpp:55-76): noisy T_2_1 between consecutive states, one
    between the first and the last state, and the prior that holds the gauge."""
    rng = np.random.default_rng(seed)
    P = prob.num_poses
    pairs = [(k, k + 1) for k in range(P - 1)] + ([(0, P - 1)] if loop else [])
    factors = [dict(pose=0, type=0, data=prob.poses_init[0], stiffness=np.eye(6) * 1e2)]
    for k1, k2 in pairs:
        T1, T2 = prob.poses_gt[k1], prob.poses_gt[k2]
        R1, R2 = T1[3:].reshape(3, 3), T2[3:].reshape(3, 3)
        T21 = np.concatenate([T2[:3] - R2 @ R1.T @ T1[:3], (R2 @ R1.T).ravel()])
        A = rng.normal(size=(6, 6)) * 0.3
        factors.append(dict(pose=k1, pose2=k2, type=2, data=npr.se3_plus(T21, 0.01 * rng.normal(size=6)),
                            stiffness=(A @ A.T + np.diag([30.0] * 3 + [100.0] * 3)).ravel(), huber=huber))
    return factors


@pytest.mark.parametrize("huber", [0.0, 0.05])
def test_lm_step_with_relative_pose_blocks_matches_dense_numpy_solve(huber):
    prob = synth.make_problem(7, 100, track_len=4, seed=6)
    _check_lm_step_against_dense(prob, _odometry_factors(prob, huber=huber))


def test_pose_graph_solve_pulls_the_trajectory_together():
    """Stereo blocks + odometry + one loop factor: converges, and the odometry blocks shrink the pose error."""
    prob = synth.make_problem(12, 240, track_len=4, seed=9, pose_sigma=(0.2, 0.03))
    none_const = np.zeros(prob.num_poses, dtype=np.uint8)
    args = (prob.camera, prob.poses_init, prob.points_init, prob.obs_pose, prob.obs_point, prob.obs_uvd, prob.stiffness())
    op = orc.OracleProblem(*args, pose_const=none_const, pose_factors=_odometry_factors(prob))
    s, _ = op.solve(orc.driver_options(num_threads=2))
    assert s.termination_type == 0 and s.final_cost < s.initial_cost
    assert np.abs(op.poses[:, :3] - prob.poses_gt[:, :3]).max() < np.abs(prob.poses_init[:, :3] - prob.poses_gt[:, :3]).max()


def test_sun_aided_solve_reduces_heading_drift():
    prob, factors = _sun_problem(P=12, L=300, seed=5)
    none_const = np.zeros(prob.num_poses, dtype=np.uint8)
    kw = dict(pose_const=none_const)
    op = orc.OracleProblem(prob.camera, prob.poses_init, prob.points_init, prob.obs_pose, prob.obs_point, prob.obs_uvd, prob.stiffness(),
                           pose_factors=factors, **kw)
    s, log = op.solve(orc.driver_options(num_threads=2, trust_region_strategy_type=1, dogleg_type=1))      # :141-143
    assert s.termination_type == 0 and s.final_cost < 0.2 * s.initial_cost
    assert np.abs(op.poses[0] - prob.poses_init[0]).max() < 0.02              # the prior holds the first pose in place


def test_per_block_stereo_stiffness():
    """tests/dataset_vo_sun.cpp:56-65 gives every stereo block the stiffness of its map point: with the same matrix
    everywhere the oracle reproduces the shared-stiffness problem bit for bit, and the cost follows the definition."""
    prob = synth.make_problem(8, 200, track_len=5, seed=2)
    same = np.broadcast_to(prob.stiffness(), (prob.num_obs, 3, 3)).copy()
    a = orc.OracleProblem.from_synth(prob)
    b = orc.OracleProblem(prob.camera, prob.poses_init, prob.points_init, prob.obs_pose, prob.obs_point, prob.obs_uvd, same)
    assert a.cost() == b.cost()
    sa, _ = a.solve(orc.driver_options(num_threads=1))
    sb, _ = b.solve(orc.driver_options(num_threads=1))
    assert sa.final_cost == sb.final_cost and np.array_equal(a.poses, b.poses)
    rng = np.random.default_rng(0)
    S = same * rng.uniform(0.5, 2.0, size=(prob.num_obs, 1, 1))
    c = orc.OracleProblem(prob.camera, prob.poses_init, prob.points_init, prob.obs_pose, prob.obs_point, prob.obs_uvd, S)
    q = np.einsum("nij,nj->ni", prob.poses_init[prob.obs_pose, 3:].reshape(-1, 3, 3), prob.points_init[prob.obs_point]) + prob.poses_init[prob.obs_pose, :3]
    e = synth.project(prob.camera, q) - prob.obs_uvd
    r = np.einsum("nij,nj->ni", S, e)
    assert c.cost() == pytest.approx(0.5 * (r * r).sum(), rel=1e-12)


def test_relative_pose_residual_and_jacobians_match_complex_step():
    rng = np.random.default_rng(3)
    L = orc.lib()
    L.orc_relative_pose_residual.argtypes = [_dp] * 7
    L.orc_relative_pose_residual.restype = None
    p = lambda a: a.ctypes.data_as(_dp)
    for _ in range(5):
        T1, T2 = _rand_pose(rng), _rand_pose(rng)
        # a measurement near the true relative pose T_2_1 = T2 T1^-1, so that the residual is a small tangent vector
        R1, R2 = T1[3:].reshape(3, 3), T2[3:].reshape(3, 3)
        T21 = np.concatenate([T2[:3] - R2 @ R1.T @ T1[:3], (R2 @ R1.T).ravel()])
        T_ref = npr.se3_plus(T21, 0.1 * rng.normal(size=6))
        A = rng.normal(size=(6, 6))
        S = np.ascontiguousarray(A @ A.T + 6 * np.eye(6))
        r, J1, J2 = np.zeros(6), np.zeros((6, 6)), np.zeros((6, 6))
        L.orc_relative_pose_residual(p(T1), p(T2), p(T_ref), p(S), p(r), p(J1), p(J2))
        np.testing.assert_allclose(r, _rel_res(T1, T2, T_ref, S).real, rtol=1e-12, atol=1e-13)
        assert np.abs(r).max() < 5.0
        np.testing.assert_allclose(J1, _cs_jac(lambda X: _rel_res(X, T2.astype(complex), T_ref, S), T1), rtol=1e-7, atol=1e-8)
        np.testing.assert_allclose(J2, _cs_jac(lambda X: _rel_res(T1.astype(complex), X, T_ref, S), T2), rtol=1e-7, atol=1e-8)


def test_sun_window_matches_golden():
    """tests/golden/sun_window.json (oracle output, made by tests/golden/make_golden.py): a regression pin."""
    import json, os
    gold = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "sun_window.json")))
    prob, factors = _sun_problem(P=8, L=400, seed=4, huber=0.5)
    op = orc.OracleProblem(prob.camera, prob.poses_init, prob.points_init, prob.obs_pose, prob.obs_point, prob.obs_uvd, prob.stiffness(),
                           pose_const=np.zeros(prob.num_poses, np.uint8), pose_factors=factors)
    assert op.cost() == pytest.approx(gold["initial_cost"], rel=1e-12)
    s, log = op.solve(orc.driver_options(num_threads=2, trust_region_strategy_type=1, dogleg_type=1))
    assert s.num_iterations == gold["num_iterations"] and log["step_is_successful"].tolist() == gold["step_is_successful"]
    np.testing.assert_allclose(log["cost"], gold["cost"], rtol=1e-9)
    np.testing.assert_allclose(op.poses, gold["poses"], atol=1e-8)
