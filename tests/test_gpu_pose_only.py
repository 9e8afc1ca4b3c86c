"""The pose-only layout (every observed point block constant, ssba_stats.general_structure == 3): one 6 x 6 system per free
pose, k_po_step . k_po_eval . k_decide . k_best per Levenberg-Marquardt iteration.

Reference: the C oracle with positions_const=True (pinned against the numpy reference by tests/test_const_points_reference.py).
Bars: same accept / reject sequence and iteration count, cost log 1e-9, final cost and poses 1e-6; against
the windowed route of the same library (SSBA_NO_POSE_ONLY=1) the bars of test_closure_border_equals_general_path: equal decisions,
cost log 1e-9, poses 1e-7.  Both sides are cut at the same iteration count K.

The shapes are chosen to break the kernel: a work-group has 128 lanes with five observations in flight each, so 127 / 128 / 129
observations sit around one lane row and 640 / 641 around one trip of the loop; 700 observations take two trips; 257 free poses
need more than one XCD group of work-groups; a pose with one or two observations has a rank-deficient block that only the
damping makes solvable."""
import dataclasses
import functools
import os

import numpy as np
import pytest

import np_reference as npr
from ceres_slam_amd import capi, synth
from ceres_slam_amd.solver import StereoBA
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

K = 10
CAM = dict(fu=400.0, fv=400.0, cu=320.0, cv=240.0, b=0.24)


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300))


def _make(P, L, counts, seed=0, sigma=0.5, outliers=0.0):
    """P cameras near the origin looking down +z, L points in a box in front of them; pose k observes the first counts[k]
    points of a permutation of its own (every point is visible from every camera, so any count up to L can be had)."""
    rng = np.random.default_rng(seed)
    t = rng.normal(scale=0.3, size=(P, 3))
    R = np.array([synth.so3_exp(rng.normal(scale=0.05, size=3)) for _ in range(P)])
    poses_gt = synth.pose_pack(t, R)
    pts = np.stack([rng.uniform(-4, 4, L), rng.uniform(-3, 3, L), rng.uniform(6, 30, L)], 1)
    ti = t + rng.normal(scale=0.05, size=(P, 3))
    Ri = np.array([R[k] @ synth.so3_exp(rng.normal(scale=0.01, size=3)) for k in range(P)])
    ok, oj, uvd = [], [], []
    for k in range(P):
        js = rng.permutation(L)[:counts[k]]
        q = pts[js] @ R[k].T + t[k]
        z = synth.project(CAM, q) + rng.normal(scale=sigma, size=(len(js), 3))
        ok += [k] * len(js)
        oj += js.tolist()
        uvd.append(z)
    uvd = np.concatenate(uvd) if uvd else np.zeros((0, 3))
    mask = None
    if outliers > 0:
        mask = rng.random(len(ok)) < outliers
        uvd[mask, :2] += rng.normal(scale=40.0, size=(int(mask.sum()), 2))
    return synth.StereoBAProblem(camera=CAM, poses_gt=poses_gt, poses_init=synth.pose_pack(ti, Ri), points_gt=pts,
                                 points_init=pts + rng.normal(scale=0.02, size=pts.shape), obs_pose=np.array(ok, np.uint32),
                                 obs_point=np.array(oj, np.uint32), obs_uvd=uvd, stereo_obs_var=np.full(3, sigma * sigma), outlier_mask=mask)


@functools.lru_cache(maxsize=None)
def _shape(name):
    """-> (problem, pose_const)."""
    none = lambda P: np.zeros(P, np.uint8)
    if name == "1x30":
        return _make(1, 30, [30], 1), none(1)
    if name == "8x60":
        p = synth.make_problem(8, 60, track_len=5, seed=7)
        c = none(8)
        c[0] = 1
        return p, c
    if name == "3x700":
        return _make(3, 700, [700] * 3, 2), none(3)
    if name == "edges":          # one lane row more or less, one trip of the loop more or less
        return _make(5, 700, [127, 128, 129, 640, 641], 3), none(5)
    if name == "40x300":
        return _make(40, 300, [300] * 40, 4), none(40)
    if name == "257x6":
        return _make(257, 600, [6] * 257, 5), none(257)
    if name == "few_obs":        # poses with 1 and 2 observations: rank-deficient undamped, fine under LM
        return _make(6, 80, [1, 2, 40, 3, 60, 80], 6), none(6)
    if name == "const_between":  # constant poses in between: their residual blocks only add to the cost
        c = none(7)
        c[[0, 3, 5]] = 1
        return _make(7, 120, [50, 60, 70, 80, 90, 100, 120], 7), c
    if name == "repeated":       # two residual blocks on one (pose, point) pair
        p = _make(4, 90, [90, 60, 30, 45], 8)
        extra = np.array([0, 5, len(p.obs_pose) - 1])
        return dataclasses.replace(p, obs_pose=np.concatenate([p.obs_pose, p.obs_pose[extra]]), obs_point=np.concatenate([p.obs_point, p.obs_point[extra]]),
                                   obs_uvd=np.concatenate([p.obs_uvd, p.obs_uvd[extra] + 0.3])), none(4)
    if name == "outliers":
        return _make(6, 200, [150] * 6, 9, outliers=0.3), none(6)
    raise KeyError(name)


SHAPES = ["1x30", "8x60", "3x700", "edges", "40x300", "257x6", "few_obs", "const_between", "repeated"]


def _args(prob):
    return (prob.camera, prob.poses_init, prob.points_init, prob.obs_pose, prob.obs_point, prob.obs_uvd)


def _pair(prob, const, stiffness=None, huber_a=0.0, pose_factors=None):
    S = prob.stiffness() if stiffness is None else stiffness
    a = _args(prob)
    ba = StereoBA(a[0], a[1].copy(), a[2].copy(), *a[3:], S, pose_const=const, huber_a=huber_a, points_const=True, pose_factors=pose_factors)
    op = orc.OracleProblem(*a, S, pose_const=const, huber_a=huber_a, positions_const=True, pose_factors=pose_factors)
    return ba, op


def _check_against_oracle(tag, ba, op, prob, **opts):
    assert ba.stats().general_structure == 3
    kw = dict(max_num_iterations=K, use_nonmonotonic_steps=1, **opts)
    s, log = ba.solve(capi.default_options(**kw))
    s2, log2 = op.solve(orc.driver_options(num_threads=2, **kw))
    print(tag, "iterations", s.num_iterations, s2.num_iterations, "cost log", _rel(log["cost"][:len(log2["cost"])], log2["cost"][:len(log["cost"])]),
          "poses", np.abs(ba.poses - op.poses).max())
    assert s.num_iterations == s2.num_iterations
    assert log["step_is_successful"].tolist() == log2["step_is_successful"].tolist()
    np.testing.assert_allclose(log["cost"], log2["cost"], rtol=1e-9)
    assert s.final_cost == pytest.approx(s2.final_cost, rel=1e-6)
    assert np.abs(ba.poses - op.poses).max() <= 1e-6
    assert ba.points.tobytes() == prob.points_init.tobytes()          # bit-unchanged
    assert ba.stats().general_structure == 3
    return s, log


@pytest.mark.parametrize("huber_a", [0.0, 1.345])
@pytest.mark.parametrize("name", SHAPES)
def test_lm_solve_matches_the_oracle(name, huber_a):
    prob, const = _shape(name)
    ba, op = _pair(prob, const, huber_a=huber_a)
    s, log = _check_against_oracle(f"{name} huber {huber_a}", ba, op, prob)
    assert s.final_cost < s.initial_cost


def test_huber_with_outliers_matches_the_oracle():
    prob, const = _shape("outliers")
    ba, op = _pair(prob, const, huber_a=1.345)
    _check_against_oracle("outliers", ba, op, prob)


def test_per_observation_stiffness():
    prob, const = _shape("const_between")
    rng = np.random.default_rng(3)
    S = np.array([np.diag(1.0 / rng.uniform(0.3, 1.5, 3)) + 0.05 * np.triu(rng.normal(size=(3, 3)), 1) for _ in range(prob.num_obs)])
    ba, op = _pair(prob, const, stiffness=S)
    _check_against_oracle("per-observation stiffness", ba, op, prob)


def test_prior_and_sun_blocks_without_a_constant_pose():
    from test_gpu_const_points import _sun_prior_factors
    prob = synth.make_problem(20, 700, track_len=6, seed=11, pose_sigma=(0.1, 0.02))
    const = np.zeros(prob.num_poses, np.uint8)
    ba, op = _pair(prob, const, pose_factors=_sun_prior_factors(prob))
    _check_against_oracle("prior + sun", ba, op, prob)


def test_relative_pose_block_with_one_constant_pose_and_between_free_poses():
    """A relative-pose block whose other pose is constant is a unary block: pose-only.  One between two free poses couples
    them: the windowed layout with constant points."""
    from test_oracle_pose_factors import _odometry_factors
    prob = synth.make_problem(9, 300, track_len=5, seed=6)
    chain = [f for f in _odometry_factors(prob, loop=False, huber=0.0) if f["type"] == 2]
    const = np.zeros(prob.num_poses, np.uint8)
    const[0] = 1
    first = [f for f in chain if {int(f["pose"]), int(f["pose2"])} == {0, 1}]
    assert len(first) == 1
    ba, op = _pair(prob, const, pose_factors=first)
    _check_against_oracle("relative pose, one constant pose", ba, op, prob)
    ba2, _ = _pair(prob, const, pose_factors=[f for f in chain if 0 not in (int(f["pose"]), int(f["pose2"]))])
    assert ba2.stats().general_structure == 0


@pytest.mark.parametrize("name", ["8x60", "const_between"])
def test_windowed_route_of_the_same_library_agrees(monkeypatch, name):
    """SSBA_NO_POSE_ONLY=1 at ssba_finalize: the windowed layout with every point flagged constant."""
    prob, const = _shape("8x60") if name == "8x60" else (synth.make_problem(30, 900, track_len=8, seed=5), None)
    if const is None:
        const = np.zeros(prob.num_poses, np.uint8)
        const[[0, 11, 12]] = 1
    out = []
    for env in ("0", "1"):
        monkeypatch.setenv("SSBA_NO_POSE_ONLY", env)
        ba, _ = _pair(prob, const, huber_a=1.345)
        assert ba.stats().general_structure == (3 if env == "0" else 0)
        s, log = ba.solve(capi.default_options(max_num_iterations=K, use_nonmonotonic_steps=1))
        out.append((s, log, ba.poses.copy()))
    (s0, l0, p0), (s1, l1, p1) = out
    assert s0.num_iterations == s1.num_iterations and s0.termination_type == s1.termination_type
    assert l0["step_is_successful"].tolist() == l1["step_is_successful"].tolist()
    np.testing.assert_allclose(l0["cost"], l1["cost"], rtol=1e-9)
    np.testing.assert_allclose(l0["gradient_max_norm"], l1["gradient_max_norm"], rtol=1e-6)
    assert np.abs(p0 - p1).max() <= 1e-7


@pytest.mark.parametrize("dogleg_type", [0, 1])
def test_dogleg_hands_over_to_the_windowed_layout(dogleg_type):
    prob, const = _shape("8x60")
    ba, op = _pair(prob, const)
    assert ba.stats().general_structure == 3
    kw = dict(max_num_iterations=K, use_nonmonotonic_steps=1, trust_region_strategy_type=1, dogleg_type=dogleg_type)
    s, log = ba.solve(capi.default_options(**kw))
    assert ba.stats().general_structure == 0
    s2, log2 = op.solve(orc.driver_options(num_threads=2, **kw))
    assert s.num_iterations == s2.num_iterations
    assert log["step_is_successful"].tolist() == log2["step_is_successful"].tolist()
    np.testing.assert_allclose(log["cost"], log2["cost"], rtol=1e-9)
    assert np.abs(ba.poses - op.poses).max() <= 1e-6
    assert ba.points.tobytes() == prob.points_init.tobytes()


def test_hand_over_is_refused_where_the_windowed_layout_does_not_fit_and_after_a_solve_began():
    prob, const = _shape("40x300")          # tracks of 40
    ba, _ = _pair(prob, const)
    with pytest.raises(capi.SsbaError) as e:
        ba.solve(capi.default_options(max_num_iterations=3, trust_region_strategy_type=1))
    assert e.value.status == -6 and "pose-only" in str(e.value)
    assert ba.stats().general_structure == 3                        # the handle kept its layout ...
    s, _ = ba.solve(capi.default_options(max_num_iterations=K))      # ... and still solves
    assert s.final_cost < s.initial_cost
    prob, const = _shape("8x60")
    ba, _ = _pair(prob, const)
    ba.solve_begin(capi.default_options(max_num_iterations=K))
    ba.step(2)
    assert ba.lib.ssba_evaluate(ba.h, None, None, None, None, None) == -7
    ba.solve_end()


def _reference_blocks(prob, const, poses, points):
    """J_p^T J_p of every pose from the numpy residual rows at (poses, points)."""
    ref = npr.NumpyBA(prob.camera, poses, points, prob.obs_pose, prob.obs_point, prob.obs_uvd, prob.stiffness(), pose_const=const.astype(bool))
    _, r, Jp, _ = ref.residuals(poses, points, jac=True)
    H = np.zeros((prob.num_poses, 6, 6))
    np.add.at(H, prob.obs_pose.astype(np.int64), np.einsum("nij,nik->njk", Jp, Jp))
    return H


@pytest.mark.parametrize("name", ["8x60", "const_between", "edges"])
def test_covariance_blocks(name):
    prob, const = _shape(name)
    ba, _ = _pair(prob, const)
    ba.solve(capi.default_options(max_num_iterations=30, use_nonmonotonic_steps=1))
    P = prob.num_poses
    H = _reference_blocks(prob, const, ba.poses, ba.points)
    free = [k for k in range(P) if not const[k]]
    pairs = [(("pose", k), ("pose", k)) for k in range(P)] + [(("pose", free[0]), ("pose", free[-1])), (("point", 3), ("point", 3)),
                                                               (("pose", free[0]), ("point", 3)), (("point", 5), ("pose", free[-1]))]
    out = ba.covariance_blocks(pairs)
    assert ba.stats().general_structure == 3
    for k in range(P):
        if const[k]:
            assert not out[k].any()
        else:
            assert _rel(out[k], np.linalg.inv(H[k])) <= 1e-9, (k, _rel(out[k], np.linalg.inv(H[k])))
    for blk in out[P:]:
        assert not blk.any()
    assert _rel(ba.pose_covariance(free[1]), np.linalg.inv(H[free[1]])) <= 1e-9
    assert ba.points.tobytes() == prob.points_init.tobytes()


def test_covariance_of_a_pose_with_one_observation_is_a_numerical_failure():
    prob, const = _shape("few_obs")
    ba, _ = _pair(prob, const)
    with pytest.raises(capi.SsbaError) as e:
        ba.pose_covariance(0)
    assert e.value.status == -3
    assert _rel(ba.pose_covariance(2), np.linalg.inv(_reference_blocks(prob, const, ba.poses, ba.points)[2])) <= 1e-9


def test_two_runs_are_bit_equal_and_a_second_solve_on_the_handle_repeats_the_first():
    prob, const = _shape("edges")
    runs = []
    for _ in range(2):
        ba, _ = _pair(prob, const, huber_a=1.345)
        s, log = ba.solve(capi.default_options(max_num_iterations=K, use_nonmonotonic_steps=1))
        runs.append((log["cost"].tobytes(), ba.poses.tobytes()))
    assert runs[0] == runs[1]
    ba.poses[:] = prob.poses_init            # move the poses back: the same handle, the same solve
    s, log = ba.solve(capi.default_options(max_num_iterations=K, use_nonmonotonic_steps=1))
    assert (log["cost"].tobytes(), ba.poses.tobytes()) == runs[0]
    s, log = ba.solve(capi.default_options(max_num_iterations=K, use_nonmonotonic_steps=1))      # from the solution: converged at once
    assert s.termination_type == 0 and s.num_iterations <= 3


def test_stepwise_api_with_graph_replays_matches_the_blocking_solve():
    prob, const = _shape("40x300")
    ba, _ = _pair(prob, const)
    o = capi.default_options(max_num_iterations=1000, use_nonmonotonic_steps=1)
    s, log = ba.solve(o)
    ref = ba.poses.copy()
    ba.poses[:] = prob.poses_init
    ba.solve_begin(o)
    ba.step(40)                 # eager iterations, the single-iteration graph and batches of ten
    s2 = ba.solve_end()
    assert s2.num_iterations == s.num_iterations and s2.final_cost == s.final_cost
    assert ba.poses.tobytes() == ref.tobytes()


def test_python_mirror_with_every_point_block_constant():
    from ceres_slam_amd import ceres_api as ceres
    prob, const = _shape("8x60")
    poses, points = prob.poses_init.copy(), prob.points_init.copy()
    problem = ceres.Problem()
    problem.AddStereoResidualBlocks(ceres.StereoCamera(**prob.camera), prob.stiffness(), None, poses, points, prob.obs_pose, prob.obs_point, prob.obs_uvd)
    for k in range(prob.num_poses):
        problem.SetParameterization(poses[k], ceres.SE3Perturbation())
    problem.SetParameterBlockConstant(poses[0])
    for j in range(prob.num_points):
        problem.SetParameterBlockConstant(points[j])
    options, summary = ceres.SolverOptions(), ceres.SolverSummary()
    options.max_num_iterations = 1000
    options.use_nonmonotonic_steps = 1
    ceres.Solve(options, problem, summary)
    assert summary.termination_type == ceres.CONVERGENCE
    ba, _ = _pair(prob, const)
    s, _ = ba.solve(capi.default_options(max_num_iterations=1000, use_nonmonotonic_steps=1))
    assert ba.stats().general_structure == 3
    assert summary.final_cost == s.final_cost and poses.tobytes() == ba.poses.tobytes()
    assert points.tobytes() == prob.points_init.tobytes()
