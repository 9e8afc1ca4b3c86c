"""Relative-pose blocks between neighbouring free poses (odometry) on the windowed layout: the rule of ssba_finalize, the cross
block J_1^T J_2 that the linearisation launch leaves for k_assemble_reduced, and everything that reads the assembled D / L
blocks (LM step, dogleg, solves, covariance) against the oracle, the general layout (SSBA_FORCE_DENSE=1) and the long-double
reference.

"Cut at k": every landmark with an observation in a state <= k and one in a state > k is removed and the rest re-indexed, so
that nothing but the odometry block couples the states k and k + 1.  With 27 free poses the super-block boundaries are 11|12
(coupling block L[1], stored transposed) and 23|24 (L[2], stored plain); the cut at 23 leaves the states 24-26 without any
observation, held by odometry alone."""
import dataclasses
import functools

import numpy as np
import pytest

from ceres_slam_amd import capi, synth
from ceres_slam_amd.solver import StereoBA
from oracle import oracle as orc
from test_gpu_edge_cases import assert_fixed_count_parity
import hp_reference as hp
from test_gpu_hp_reference import _check_against_truth, _factor_reference, _step_case
from test_gpu_pose_factors import _rel
from test_oracle_pose_factors import _odometry_factors

pytestmark = pytest.mark.gpu


def _cut(prob, k):
    lo = np.full(prob.num_points, prob.num_poses, np.int64)
    hi = np.full(prob.num_points, -1, np.int64)
    np.minimum.at(lo, prob.obs_point, prob.obs_pose)
    np.maximum.at(hi, prob.obs_point, prob.obs_pose)
    keep = ~((lo <= k) & (hi > k))
    new = np.cumsum(keep) - 1
    ok = keep[prob.obs_point]
    return dataclasses.replace(prob, points_gt=prob.points_gt[keep], points_init=prob.points_init[keep], obs_pose=prob.obs_pose[ok],
                               obs_point=new[prob.obs_point[ok]].astype(np.uint32), obs_uvd=prob.obs_uvd[ok])


@functools.lru_cache(maxsize=None)
def _problem(name):
    """-> (problem, constant poses).  p1 / p2 / p3 as the module docstring's sizes, c<k>: cut at k, k12: state 12 constant."""
    base = {"p1": lambda: synth.make_problem(27, 810, track_len=4, seed=3, pose_sigma=(0.1, 0.02)),
            "p2": lambda: synth.make_problem(20, 700, track_len=6, seed=11, pose_sigma=(0.1, 0.02)),
            "p3": lambda: synth.make_problem(9, 300, track_len=5, seed=6)}[name[:2]]()
    const = np.zeros(base.num_poses, np.uint8)
    for part in name.split("_")[1:]:
        if part[0] == "c":
            base = _cut(base, int(part[1:]))
        else:
            const[int(part[1:])] = 1
    cnt = np.bincount(base.obs_pose, minlength=base.num_poses)
    assert min(c for c in cnt if c) >= 30
    return base, const


P1_VARIANTS = ["p1", "p1_c11", "p1_c12", "p1_c23", "p1_c11_k12"]
ALL = P1_VARIANTS + ["p2", "p2_c9", "p3_c4"]


def _handle(name, huber=0.0, factors="chain"):
    prob, const = _problem(name)
    f = None if factors is None else _odometry_factors(prob, loop=factors == "loop", huber=huber)
    return StereoBA(prob.camera, prob.poses_init.copy(), prob.points_init.copy(), prob.obs_pose, prob.obs_point, prob.obs_uvd, prob.stiffness(),
                    pose_const=const, pose_factors=f)


def _oracle(name, huber=0.0):
    prob, const = _problem(name)
    return orc.OracleProblem(prob.camera, prob.poses_init, prob.points_init, prob.obs_pose, prob.obs_point, prob.obs_uvd, prob.stiffness(),
                             pose_const=const, pose_factors=_odometry_factors(prob, loop=False, huber=huber))


# ------------------------------------------------------------------------------------------------------------------ 1. layout
@pytest.mark.parametrize("name", ALL)
def test_chain_keeps_the_windowed_layout(name):
    prob, const = _problem(name)
    st = _handle(name).stats()
    assert st.general_structure == 0
    assert st.pose_bandwidth >= 1
    seen = np.bincount(prob.obs_pose, minlength=prob.num_poses) > 0
    plain = _handle(name, factors=None).stats()
    assert plain.general_structure == 0
    if seen.all():
        assert st.num_superblocks == plain.num_superblocks
    else:
        # (p1_c23, p3_c4) the states without observations are free only through their odometry blocks: the handle without
        # factors has fewer free poses, so its super-block count is that of the observed states alone
        assert st.num_free_poses == prob.num_poses - int(const.sum()) and st.num_superblocks == -(-st.num_free_poses // 12)
        assert plain.num_free_poses == int((seen & (const == 0)).sum()) and plain.num_superblocks == -(-plain.num_free_poses // 12)


def test_loop_block_and_pose_graph_take_the_general_layout():
    assert _handle("p1", factors="loop").stats().general_structure == 1
    prob, _ = _problem("p1")
    none = (np.zeros((0, 3)), np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros((0, 3)), np.eye(3))
    ba = StereoBA(prob.camera, prob.poses_init.copy(), *none, pose_const=np.zeros(prob.num_poses, np.uint8),
                  pose_factors=_odometry_factors(prob, loop=False))
    assert ba.stats().general_structure == 1


# --------------------------------------------------------------------------------------------------- 2. one step against the oracle
def _blk(S, a, b):
    return S[6 * a: 6 * a + 6, 6 * b: 6 * b + 6]


@pytest.mark.parametrize("huber", [0.0, 0.05])
@pytest.mark.parametrize("radius", [1e4, 20.0])
@pytest.mark.parametrize("name", P1_VARIANTS + ["p3_c4"])
def test_lm_step_with_odometry_chain_matches_oracle(name, radius, huber):
    ba, op = _handle(name, huber), _oracle(name, huber)
    assert ba.stats().general_structure == 0
    S, rhs, dp, dl, mcc = ba.lm_step(radius)
    S2, rhs2, _ = op.reduced_system(radius)
    dp2, dl2, mcc2 = op.lm_step(radius)
    print("ODOM step", name, radius, huber, "S", _rel(S, S2), "rhs", _rel(rhs, rhs2), "dp", _rel(dp, dp2), "dl", _rel(dl, dl2),
          "mcc", abs(mcc - mcc2) / abs(mcc2))
    assert _rel(S, S2) < 1e-9 and _rel(rhs, rhs2) < 1e-9
    assert _rel(dp, dp2) < 1e-7 and _rel(dl, dl2) < 1e-7
    assert mcc == pytest.approx(mcc2, rel=1e-8)
    assert ba.evaluate()[0] == pytest.approx(op.cost(), rel=1e-12)
    # the block across a super-block boundary that the odometry block alone fills
    for nm, (a, b) in (("p1_c11", (11, 12)), ("p1_c23", (23, 24))):
        if name == nm:
            assert np.abs(_blk(S2, a, b)).max() > 0 and np.abs(_blk(S, a, b)).max() > 0
            assert _rel(_blk(S, a, b), _blk(S2, a, b)) < 1e-9
            assert _rel(_blk(S, b, a), _blk(S2, b, a)) < 1e-9
    if name == "p1_c11_k12":        # free index 12 is state 13: two unary halves, nothing across the boundary
        assert not _blk(S2, 11, 12).any() and not _blk(S, 11, 12).any() and not _blk(S, 12, 11).any()


# ----------------------------------------------------------------------------------------------------------- 3. the two layouts agree
@pytest.mark.parametrize("huber", [0.0, 0.05])
@pytest.mark.parametrize("radius", [1e4, 20.0])
@pytest.mark.parametrize("name", P1_VARIANTS + ["p3_c4"])
def test_windowed_and_general_layout_agree(monkeypatch, name, radius, huber):
    ba = _handle(name, huber)
    assert ba.stats().general_structure == 0
    S, rhs, dp, dl, mcc = ba.lm_step(radius)
    monkeypatch.setenv("SSBA_FORCE_DENSE", "1")
    bd = _handle(name, huber)
    assert bd.stats().general_structure == 1
    Sd, rhsd, dpd, dld, mccd = bd.lm_step(radius)
    print("ODOM layouts", name, radius, huber, "S", _rel(S, Sd), "rhs", _rel(rhs, rhsd), "dp", _rel(dp, dpd), "dl", _rel(dl, dld))
    assert _rel(S, Sd) < 2e-9 and _rel(rhs, rhsd) < 2e-9       # each within 1e-9 of the oracle
    assert _rel(dp, dpd) < 2e-7 and _rel(dl, dld) < 2e-7


# ------------------------------------------------------------------------------------------------------------------ 4. long double
@pytest.mark.parametrize("radius", [1e4, 20.0, 3.0])
@pytest.mark.parametrize("huber", [0.0, 0.05])
@pytest.mark.parametrize("name", ["p1_c11", "p1", "p1_c12", "p1_c23", "p3_c4"])
def test_step_with_odometry_chain_is_fp64_accurate(name, huber, radius):
    """The windowed assembly and solve at the derived bars of test_gpu_hp_reference (eta <= 4096 u, forward error <= min(4096 u
    kappa_2, 1e-8) against the refined solve of the device's own system).  The states 24-26 of p1_c23 and 5-8 of p3_c4 are free
    through odometry alone."""
    prob, const = _problem(name)
    ba = _handle(name, huber)
    assert ba.stats().general_structure == 0 and ba.stats().num_superblocks == (1 if name == "p3_c4" else 3)
    _step_case(f"odometry_chain {name} h={huber} r={radius}", ba, prob, radius, pose_const=const.astype(bool),
               factor_poses=hp.factor_poses(_odometry_factors(prob, loop=False)))


@pytest.mark.parametrize("radius", [1e4, 3.0])
@pytest.mark.parametrize("huber", [0.0, 0.05])
@pytest.mark.parametrize("name,factors", [("p1_c11", "chain"), ("p1_c12", "chain"), ("p1_c23", "chain"), ("p3_c4", "chain"), ("p1", "loop")])
def test_assembled_system_with_odometry_blocks_against_the_truth(name, factors, huber, radius):
    """S (every entry: the cross blocks J_1^T J_2 of pf_cross in both orientations and the blocks that landmarks and odometry
    fill together), rhs, delta_l and the model cost change against the long-double system with the long-double factor blocks.
    Windowed: pf_rel_wave and k_assemble_reduced, the cut at 11 and at 23 leaving the block across a super-block boundary to the
    odometry block alone, p1_c23 and p3_c4 with states free through odometry alone; p1 with the loop block: pf_evaluate in the
    general kernels."""
    prob, const = _problem(name)
    ba = _handle(name, huber, factors)
    assert ba.stats().general_structure == int(factors == "loop")
    S, rhs, dp, dl, mcc = ba.lm_step(radius)
    fl = _odometry_factors(prob, loop=factors == "loop", huber=huber)
    sy, fidx = _factor_reference((name, factors, huber), prob, fl, const, radius)
    assert sy.n == S.shape[0]
    _check_against_truth(f"odometry {name} {factors} h={huber} r={radius}", sy, S, rhs, dp, dl, mcc, fidx, prob.points_init)


# ----------------------------------------------------------------------------------------------------------------------- 5. solves
@pytest.mark.parametrize("strategy", [(0, 0), (1, 0), (1, 1)])
@pytest.mark.parametrize("huber", [0.0, 0.05])
@pytest.mark.parametrize("name", ["p2", "p2_c9"])
def test_solve_with_odometry_chain_matches_oracle(name, strategy, huber):
    kw = dict(max_num_iterations=1000, use_nonmonotonic_steps=1, trust_region_strategy_type=strategy[0], dogleg_type=strategy[1])
    ba, op = _handle(name, huber), _oracle(name, huber)
    s2, log2 = op.solve(orc.driver_options(num_threads=4, **kw))
    assert s2.termination_type == 0         # the oracle converges from here (shown first: the bars below need it)
    assert ba.stats().general_structure == 0
    s, log = ba.solve(capi.default_options(**kw))
    assert s.termination_type == 0
    n = min(len(log["cost"]), len(log2["cost"]), 12)
    assert log["step_is_successful"][:n].tolist() == log2["step_is_successful"][:n].tolist()
    ok = np.asarray(log2["step_is_successful"][:n], dtype=bool)
    ok[0] = True
    np.testing.assert_allclose(log["cost"][:n][ok], log2["cost"][:n][ok], rtol=1e-7)
    assert_fixed_count_parity(_handle(name, huber), _oracle(name, huber), 12, **{k: v for k, v in kw.items() if k != "max_num_iterations"})
    assert np.abs(ba.poses - op.poses).max() < 1e-4
    assert ba.stats().general_structure == 0


@pytest.mark.parametrize("strategy", [(0, 0), (1, 1)])
@pytest.mark.parametrize("name", ["p1_c23", "p3_c4"])
def test_solve_with_odometry_only_states_matches_oracle(name, strategy):
    kw = dict(max_num_iterations=1000, use_nonmonotonic_steps=1, trust_region_strategy_type=strategy[0], dogleg_type=strategy[1])
    ba, op = _handle(name, 0.05), _oracle(name, 0.05)
    s2, _ = op.solve(orc.driver_options(num_threads=4, **kw))
    assert s2.termination_type == 0
    s, _ = ba.solve(capi.default_options(**kw))
    assert s.termination_type == 0 and s.num_iterations == s2.num_iterations
    assert s.final_cost == pytest.approx(s2.final_cost, rel=1e-6)


# ------------------------------------------------------------------------------------------------------------------- 6. covariance
def test_covariance_with_odometry_chain_matches_dense_inverse():
    """Bars and reasoning of test_pose_covariance_block_matches_dense_inverse: 1e-6 against the inverse of the device's own
    undamped system, 1e-3 against the oracle's (the gauge is held by the prior alone)."""
    name = "p1_c11"
    ba, op = _handle(name), _oracle(name)
    ba.solve(capi.default_options(max_num_iterations=1000, use_nonmonotonic_steps=1))
    op.poses[:], op.points[:] = ba.poses, ba.points
    S, _, free_idx = op.reduced_system(1e300)
    Sinv = np.linalg.inv(S)
    Sginv = np.linalg.inv(ba.lm_step(1e300)[0])
    for k in (1, 11, 12, 26):
        f = int(free_idx[k])
        cov = ba.pose_covariance(k)
        assert _rel(cov, _blk(Sginv, f, f)) < 1e-6
        assert _rel(cov, _blk(Sinv, f, f)) < 1e-3
        assert np.all(np.linalg.eigvalsh(0.5 * (cov + cov.T)) > 0)
    c01, c10 = ba.covariance_blocks([(("pose", 11), ("pose", 12)), (("pose", 12), ("pose", 11))])
    for cov, (a, b) in ((c01, (11, 12)), (c10, (12, 11))):
        fa, fb = int(free_idx[a]), int(free_idx[b])
        assert _rel(cov, _blk(Sginv, fa, fb)) < 1e-6
        assert _rel(cov, _blk(Sinv, fa, fb)) < 1e-3
    assert ba.stats().general_structure == 0


# ------------------------------------------------------------------------------------------------------- 7. the Python Ceres mirror
def test_odometry_chain_through_the_python_api_mirror():
    from ceres_slam_amd import ceres_api as ceres
    prob, _ = _problem("p2")
    factors = _odometry_factors(prob, loop=False, huber=0.05)
    poses, points = prob.poses_init.copy(), prob.points_init.copy()
    problem = ceres.Problem()
    problem.AddStereoResidualBlocks(ceres.StereoCamera(**prob.camera), prob.stiffness(), None, poses, points, prob.obs_pose, prob.obs_point, prob.obs_uvd)
    for f in factors:
        S = np.asarray(f["stiffness"]).reshape(6, 6)
        if f["type"] == 0:
            problem.AddResidualBlock(ceres.PoseErrorAutomatic.Create(f["data"], S), None, poses[f["pose"]])
        else:
            problem.AddResidualBlock(ceres.RelativePoseErrorAutomatic.Create(f["data"], S), ceres.HuberLoss(0.05), poses[f["pose"]], poses[f["pose2"]])
    for k in range(prob.num_poses):
        problem.SetParameterization(poses[k], ceres.SE3Perturbation.Create())
    lowered = ceres._lower(problem)
    assert lowered.stats().general_structure == 0
    lowered.close()
    options = ceres.SolverOptions()
    options.max_num_iterations, options.use_nonmonotonic_steps = 1000, 1
    summary = ceres.SolverSummary()
    ceres.Solve(options, problem, summary)
    ba = _handle("p2", 0.05)
    s, log = ba.solve(options.as_c())
    assert summary.termination_type == s.termination_type == ceres.CONVERGENCE
    np.testing.assert_allclose([it["cost"] for it in summary.iterations], log["cost"], rtol=1e-13)
    assert [it["step_is_successful"] for it in summary.iterations] == [bool(x) for x in log["step_is_successful"]]
    np.testing.assert_allclose(poses, ba.poses, rtol=0, atol=1e-12)
    np.testing.assert_allclose(points, ba.points, rtol=0, atol=1e-10)
