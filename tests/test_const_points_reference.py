"""The CPU reference for constant point blocks (tests/const_points_reference.py) against the C oracle where the oracle has
a switch: every point constant (positions_const=True on a stereo-only problem).  Same accept / reject sequence, cost log to
1e-9.  This pins the numpy reference that the GPU tests use for SUBSETS of the points, where the oracle has no switch.

The oracle takes positions_const with Levenberg-Marquardt and with both dogleg types (it zeroes the position columns of every
Jacobian row, whatever the strategy).  np_reference has a TRADITIONAL dogleg loop only; the SUBSPACE loop lives in
const_points_reference and is pinned here as well."""
import numpy as np
import pytest

import const_points_reference as cpr
import np_reference as npr
from ceres_slam_amd import synth
from oracle import oracle as orc

SHAPES = {"8x60": (8, 60, 5), "20x200": (20, 200, 8)}
K = 12      # both loops cut at the same iteration count, before any flat tail


def _problem(shape, huber_a):
    P, L, T = SHAPES[shape]
    return synth.make_problem(P, L, track_len=T, seed=7, outlier_fraction=0.3 if huber_a > 0 else 0.0)


def _oracle_all_const(prob, huber_a):
    return orc.OracleProblem(prob.camera, prob.poses_init, prob.points_init, prob.obs_pose, prob.obs_point, prob.obs_uvd,
                             prob.stiffness(), huber_a=huber_a, positions_const=True)


@pytest.mark.parametrize("huber_a", [0.0, 1.345])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_lm_with_every_point_constant_matches_the_oracle(shape, huber_a):
    prob = _problem(shape, huber_a)
    op = _oracle_all_const(prob, huber_a)
    s, log = op.solve(orc.driver_options(num_threads=2, max_num_iterations=K))
    ref = cpr.ConstPointsBA.from_synth(prob, point_const=np.ones(prob.num_points, bool), huber_a=huber_a)
    assert not ref.active.any()
    x_p, x_l, rlog = ref.solve(max_iter=K)
    n = min(len(log["cost"]), len(rlog))
    assert n >= 3
    assert log["step_is_successful"][:n].tolist() == [int(ok) for _, ok in rlog][:n]
    np.testing.assert_allclose(log["cost"][:n], [c for c, _ in rlog][:n], rtol=1e-9)
    assert np.array_equal(x_l, prob.points_init) and np.array_equal(op.points, prob.points_init)
    if len(rlog) == len(log["cost"]):
        np.testing.assert_allclose(op.poses, x_p, atol=1e-7)


@pytest.mark.parametrize("dogleg_type", [0, 1])
@pytest.mark.parametrize("huber_a", [0.0, 1.345])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_dogleg_with_every_point_constant_matches_the_oracle(shape, huber_a, dogleg_type):
    """TRADITIONAL_DOGLEG through np_reference's loop, SUBSPACE_DOGLEG through the loop of const_points_reference."""
    prob = _problem(shape, huber_a)
    op = _oracle_all_const(prob, huber_a)
    s, log = op.solve(orc.driver_options(num_threads=2, max_num_iterations=K, trust_region_strategy_type=1, dogleg_type=dogleg_type))
    ref = cpr.ConstPointsBA.from_synth(prob, point_const=np.ones(prob.num_points, bool), huber_a=huber_a)
    x_p, x_l, rlog = cpr.dogleg_solve(ref, dogleg_type, max_iter=K)
    n = min(len(log["cost"]), len(rlog))
    assert n >= 3
    assert log["step_is_successful"][:n].tolist() == [int(ok) for _, ok in rlog][:n]
    np.testing.assert_allclose(log["cost"][:n], [c for c, _ in rlog][:n], rtol=1e-9)
    assert np.array_equal(x_l, prob.points_init) and np.array_equal(op.points, prob.points_init)


@pytest.mark.parametrize("dogleg_type", [0, 1])
def test_dogleg_loops_match_the_oracle_with_every_point_free(dogleg_type):
    """The same two loops on the unmodified problem (no constant point), where the oracle needs no switch: the subspace loop
    written here is pinned on a problem with landmark columns too."""
    prob = synth.make_problem(8, 60, track_len=5, seed=7)
    op = orc.OracleProblem.from_synth(prob)
    s, log = op.solve(orc.driver_options(num_threads=2, max_num_iterations=K, trust_region_strategy_type=1, dogleg_type=dogleg_type))
    ref = cpr.ConstPointsBA.from_synth(prob)
    x_p, x_l, rlog = cpr.dogleg_solve(ref, dogleg_type, max_iter=K)
    n = min(len(log["cost"]), len(rlog))
    assert n >= 3
    assert log["step_is_successful"][:n].tolist() == [int(ok) for _, ok in rlog][:n]
    np.testing.assert_allclose(log["cost"][:n], [c for c, _ in rlog][:n], rtol=1e-8)


def test_dense_reduced_system_reproduces_the_sparse_lm_step():
    """dense_reduced_system (Schur complement over the free landmarks) and NumpyBA.lm_step (sparse solve of the full damped
    normal equations) are two routes to the same step, for a subset of constant points."""
    prob = synth.make_problem(8, 60, track_len=5, seed=7)
    mask = np.arange(prob.num_points) % 3 == 0
    ref = cpr.ConstPointsBA.from_synth(prob, point_const=mask)
    for radius in (1e4, 3.0):
        S, rhs, dp, dl, _ = cpr.dense_reduced_system(ref, ref.poses, ref.points, radius)
        dp2, dl2, _, _, _ = ref.lm_step(ref.poses, ref.points, radius)
        assert np.abs(dp - dp2).max() <= 1e-9 * np.abs(dp2).max()
        assert np.abs(dl - dl2).max() <= 1e-9 * np.abs(dl2).max()
        assert not dl[mask].any() and not dl2[mask].any()
        assert np.allclose(S, S.T, rtol=0, atol=1e-9 * np.abs(S).max())
