"""Covariance blocks on a wide handle (tracks of 13..24 observations, 144-row super-blocks) AFTER its solve: the columns of
Sigma come from a right-hand-side panel through the handle's own parallel cyclic reduction (ssba_wide_covariance.hip), the
handle stays on the wide layout, and a later solve is unchanged.  A covariance request before the first solve still hands
the handle over to the blocked Cholesky (tests/test_gpu_general_structure.py, tests/test_gpu_covariance_blocks.py).

Shapes: the smallest at which the panel reduction takes another path -- one super-block (no reduction step), two (one step, the
second block nearly all padding), three (two steps, not a power of two), five (three steps, chain ends lose neighbours at
different strides).  Truth never comes from the device (tests/test_gpu_covariance_blocks.py: long double).
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import hp_reference as hp
from ceres_slam_amd import capi, synth
from ceres_slam_amd.solver import StereoBA
from test_gpu_covariance_blocks import Truth, _check_against_schur_truth, _pose_const, _rel
from test_gpu_general_structure import _no_wide

pytestmark = pytest.mark.gpu
LD = np.longdouble

CASES = [(14, 300, 13), (30, 900, 24), (60, 1500, 16), (110, 2200, 20)]
SEED = 3


@functools.lru_cache(maxsize=None)
def _solved_wide(case):
    """One solved wide handle per shape, shared by the tests (they only read it: covariance calls leave the parameters alone)."""
    P, L, T = case
    prob = synth.make_problem(P, L, track_len=T, seed=SEED)
    ba = StereoBA.from_synth(prob, device=0)
    st = ba.stats()
    assert st.wide_superblocks == (st.num_free_poses + 23) // 24, (st.wide_superblocks, st.num_free_poses)
    assert st.num_free_poses == P - 1
    ba.solve(capi.default_options(max_num_iterations=50, use_nonmonotonic_steps=1))
    return prob, ba


def _fresh_cholesky(prob, ba):
    """The route that served this need before: a fresh handle at the solved parameters on the blocked Cholesky."""
    with _no_wide():
        ba2 = StereoBA(prob.camera, ba.poses.copy(), ba.points.copy(), prob.obs_pose, prob.obs_point, prob.obs_uvd, prob.stiffness(), device=0)
    assert ba2.stats().wide_superblocks == 0 and ba2.stats().general_structure == 1
    return ba2


def _route_distance(ba):
    """Worst relative distance of the handle's diagonal pose blocks from the long-double inverse of its own undamped S."""
    S = np.asarray(ba.lm_step(1e300)[0], LD)
    Sinv = hp.refined_solve(S, np.eye(S.shape[0]))[0]
    blocks = ba.pose_marginals()
    free = [k for k in range(blocks.shape[0]) if blocks[k].any()]
    assert len(free) == S.shape[0] // 6
    return max(_rel(blocks[k], Sinv[6 * f:6 * f + 6, 6 * f:6 * f + 6]) for f, k in enumerate(free))


@functools.lru_cache(maxsize=None)
def _distances(case):
    prob, ba = _solved_wide(case)
    return _route_distance(ba), _route_distance(_fresh_cholesky(prob, ba))


# ------------------------------------------------------------------------------------------------ (1) after-solve calls work
@pytest.mark.parametrize("case", CASES)
def test_pose_covariance_after_the_solve_stays_on_the_wide_layout(case):
    prob, ba = _solved_wide(case)
    n_sb = ba.stats().wide_superblocks
    nf = ba.stats().num_free_poses
    free_idx = sorted({0, nf - 1} | ({23, 24} if nf > 24 else set()))
    for f in free_idx:
        cov = ba.pose_covariance(f + 1)          # pose 0 is constant: free index f is pose f + 1
        assert np.isfinite(cov).all()
        assert _rel(cov, cov.T) < 1e-9, (case, f, _rel(cov, cov.T))
        assert np.all(np.linalg.eigvalsh(0.5 * (cov + cov.T)) > 0), (case, f)
    st = ba.stats()
    assert st.wide_superblocks == n_sb and st.wide_superblocks > 0


# ------------------------------------------------------------------------------------------------ (2) against the truth
@pytest.mark.parametrize("case", CASES)
def test_wide_route_against_the_truth(case):
    """The bars of _check_against_schur_truth as they stand (1e-8 against the device's own S inverted in long double,
    max(1e-8, 20 e_route) against the row-level truth), on the solved wide handle and on a blocked-Cholesky handle at the same
    parameters.  Measured on an MI355X (worst diagonal pose block against the long-double inverse of the handle's own S,
    wide route / blocked Cholesky): 4.8e-15 / 4.2e-15, 5.7e-15 / 6.3e-15, 4.6e-14 / 1.5e-14, 1.5e-13 / 3.4e-14 for the four
    shapes -- the 1e-8 bar holds with five orders to spare, so the 4 x clause below has not been needed.
    Nearly all of this test's time is the long-double truth on the host (twice per shape: 13 s at 60 poses, 67 s at 110)."""
    P, L, T = case
    prob, ba = _solved_wide(case)
    n_sb = ba.stats().wide_superblocks
    _check_against_schur_truth(f"wide after solve {case}", ba, prob, prob.stiffness(), _pose_const(P))
    assert ba.stats().wide_superblocks == n_sb
    ba2 = _fresh_cholesky(prob, ba)
    _check_against_schur_truth(f"blocked Cholesky {case}", ba2, prob, prob.stiffness(), _pose_const(P))
    d_wide, d_chol = _distances(case)
    print(f"route distance {case}: wide {d_wide:.3e}  blocked Cholesky {d_chol:.3e}  ratio {d_wide / max(d_chol, 1e-300):.2f}")
    # the reduction adds ceil(log2 n) <= 3 factor levels to the one of the blocked Cholesky: beyond 1e-8 no more than 4 x its distance
    assert d_wide <= max(1e-8, 4.0 * d_chol), (case, d_wide, d_chol)


# ------------------------------------------------------------------------------------------------ (3) the two routes agree
def test_wide_route_equals_the_fresh_handle_route():
    case = (30, 900, 24)
    prob, ba = _solved_wide(case)
    tol = max(_distances(case))
    a = ba.pose_covariance(7)
    b = _fresh_cholesky(prob, ba).pose_covariance(7)
    print("pose 7: wide against fresh blocked Cholesky", _rel(a, b), "tolerance", tol)
    assert _rel(a, b) <= tol, (_rel(a, b), tol)


# ------------------------------------------------------------------------------------------------ (4) prior, sun blocks, DOGLEG
def test_prior_and_sun_blocks_with_dogleg():
    """The sun-aided window (tests/dataset_vo_sun.cpp:80-124) on tracks of 16: no constant pose, the prior on pose 0 anchors, sun
    blocks on three states out of four -- all unary blocks on the diagonal of the wide system, so in the covariance."""
    from oracle import oracle as orc
    P, L = 30, 900
    prob = synth.make_problem(P, L, track_len=16, seed=7)
    rng = np.random.default_rng(7)
    sun_g = np.array([0.3, -0.8, 0.5])
    factors = [dict(pose=0, type=0, data=prob.poses_init[0], stiffness=np.eye(6) * 1e2)]
    for k in range(P):
        if k % 4 == 3:
            continue
        obs = prob.poses_gt[k][3:].reshape(3, 3) @ sun_g + 0.01 * rng.normal(size=3)
        factors.append(dict(pose=k, type=1, data=np.concatenate([obs, sun_g, [1000.0, 1000.0]]), stiffness=np.eye(2).ravel() * 50.0, huber=0.0))
    none_const = np.zeros(P, dtype=np.uint8)
    ba = StereoBA(prob.camera, prob.poses_init.copy(), prob.points_init.copy(), prob.obs_pose, prob.obs_point, prob.obs_uvd, prob.stiffness(),
                  pose_const=none_const, pose_factors=factors, device=0)
    assert ba.stats().wide_superblocks == (P + 23) // 24
    ba.solve(capi.default_options(max_num_iterations=1000, use_nonmonotonic_steps=1, trust_region_strategy_type=1, dogleg_type=1))
    covs = {k: ba.pose_covariance(k) for k in (1, P // 2, P - 1)}
    assert ba.stats().wide_superblocks == (P + 23) // 24
    op = orc.OracleProblem(prob.camera, prob.poses_init, prob.points_init, prob.obs_pose, prob.obs_point, prob.obs_uvd, prob.stiffness(),
                           pose_const=none_const, pose_factors=factors)
    op.poses[:], op.points[:] = ba.poses, ba.points
    S, _, free_idx = op.reduced_system(1e300)
    Sinv = np.linalg.inv(S)
    Sginv = np.linalg.inv(ba.lm_step(1e300)[0])
    for k, cov in covs.items():
        f = int(free_idx[k])
        print("pose", k, "device S", _rel(cov, Sginv[6 * f:6 * f + 6, 6 * f:6 * f + 6]), "oracle S", _rel(cov, Sinv[6 * f:6 * f + 6, 6 * f:6 * f + 6]))
        # the gauge is held by the prior alone, cond(S) ~ 1e9: the bars of test_pose_covariance_block_matches_dense_inverse
        assert _rel(cov, Sginv[6 * f:6 * f + 6, 6 * f:6 * f + 6]) < 1e-6
        assert _rel(cov, Sinv[6 * f:6 * f + 6, 6 * f:6 * f + 6]) < 1e-3
        assert np.all(np.linalg.eigvalsh(0.5 * (cov + cov.T)) > 0)


# ------------------------------------------------------------------------------------------------ (5) a later solve is unchanged
def test_a_later_solve_is_unchanged():
    P, L, T = 60, 1500, 16
    runs = []
    for ask in (False, True):
        prob = synth.make_problem(P, L, track_len=T, seed=6)
        ba = StereoBA.from_synth(prob, device=0)
        n_sb = ba.stats().wide_superblocks
        assert n_sb == 3
        ba.solve(capi.default_options(max_num_iterations=3, use_nonmonotonic_steps=1))
        if ask:
            pm, lm = ba.pose_marginals(), ba.point_marginals()
            assert pm[1:].any() and np.isfinite(pm).all() and np.isfinite(lm).all()
        s, log = ba.solve(capi.default_options(max_num_iterations=50, use_nonmonotonic_steps=1))
        assert ba.stats().wide_superblocks == n_sb
        runs.append((s.num_iterations, s.final_cost, {k: np.asarray(v).copy() for k, v in log.items()}, ba.poses.copy(), ba.points.copy()))
    a, b = runs
    assert a[0] == b[0] and a[1] == b[1]
    for k in a[2]:
        assert np.array_equal(a[2][k], b[2][k]), k
    assert np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])


# ------------------------------------------------------------------------------------------------ (6) bit reproducible
def test_bit_reproducible():
    prob, ba = _solved_wide((60, 1500, 16))
    pairs = [(("pose", k), ("pose", k)) for k in range(60)] + [(("pose", 2), ("pose", 57)), (("pose", 30), ("point", 700))]
    pairs += [(("point", l), ("point", l)) for l in range(0, 1500, 7)]
    a, b = ba.covariance_blocks(pairs), ba.covariance_blocks(pairs)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert any(x.any() for x in a)


# ------------------------------------------------------------------------------------------------ (7) semantics
def test_semantics_on_the_solved_wide_handle():
    prob, ba = _solved_wide((30, 900, 24))
    out = ba.covariance_blocks([(("pose", 0), ("pose", 3)), (("pose", 0), ("point", 5)), (("point", 5), ("pose", 0)),
                                (("pose", 2), ("pose", 29)), (("pose", 29), ("pose", 2)), (("pose", 4), ("pose", 7)),
                                (("pose", 7), ("pose", 4)), (("pose", 9), ("point", 280)), (("point", 280), ("pose", 9))])
    assert out[0].shape == (6, 6) and not out[0].any()
    assert out[1].shape == (6, 3) and not out[1].any() and out[2].shape == (3, 6) and not out[2].any()
    assert np.array_equal(out[3], out[4].T) and out[3].any()
    assert np.array_equal(out[5], out[6].T) and out[5].any()
    assert np.array_equal(out[7], out[8].T) and out[7].any()
    with pytest.raises(capi.SsbaError) as e:
        ba.pose_covariance(0)                    # a constant pose has no block of its own (ssba_pose_covariance)
    assert e.value.status == -1
    P, L = 30, 900
    for pairs, status in [([(("pose", P), ("pose", 0))], -1), ([(("point", L), ("point", L))], -1), ([(("point", 1), ("point", 2))], -6)]:
        with pytest.raises(capi.SsbaError) as e:
            ba.covariance_blocks(pairs)
        assert e.value.status == status
    assert ba.stats().wide_superblocks == 2


def test_gauge_free_wide_problem_fails_or_reports_enormous_variances():
    P = 20
    prob = synth.make_problem(P, 400, track_len=16, seed=3)
    ba = StereoBA.from_synth(prob, device=0, pose_const=np.zeros(P, dtype=np.uint8))
    assert ba.stats().wide_superblocks == 1
    ba.solve(capi.default_options(max_num_iterations=5, use_nonmonotonic_steps=1))
    try:
        c = ba.pose_covariance(1)
        assert np.abs(c).max() > 1e6
    except capi.SsbaError as e:
        assert e.status == -3
    assert ba.stats().wide_superblocks == 1


def test_sharded_wide_handle_is_still_unsupported():
    prob = synth.make_problem(20, 400, track_len=16, seed=1)
    ba = StereoBA.from_synth(prob, world_size=2, rank=0)
    assert ba.stats().wide_superblocks == 1
    with pytest.raises(capi.SsbaError) as e:
        ba.covariance_blocks([(("pose", 1), ("pose", 1))])
    assert e.value.status == -6
    with pytest.raises(capi.SsbaError) as e:
        ba.pose_covariance(1)
    assert e.value.status == -6


# ------------------------------------------------------------------------------------------------ (8) through the shims
def test_python_shim_on_a_window_of_long_tracks():
    """Solve, then Covariance.Compute on a window of 16 states with tracks of 16 and a prior (the Python mirror lowers the problem
    to a fresh handle per call, so its Compute takes the hand-over of an unsolved wide handle)."""
    from ceres_slam_amd import ceres_api as ceres
    P, L = 16, 400
    prob = synth.make_problem(P, L, track_len=16, seed=4)
    poses, points = prob.poses_init.copy(), prob.points_init.copy()
    camera = ceres.StereoCamera(**prob.camera)
    problem = ceres.Problem()
    S = prob.stiffness()
    for i in range(prob.num_obs):
        cost = ceres.StereoReprojectionErrorAutomatic.Create(camera, prob.obs_uvd[i], S)
        problem.AddResidualBlock(cost, None, poses[int(prob.obs_pose[i])], points[int(prob.obs_point[i])])
    problem.AddResidualBlock(ceres.PoseErrorAutomatic.Create(prob.poses_init[0].copy(), np.eye(6) * 1e2), None, poses[0])
    for k in range(P):
        problem.SetParameterization(poses[k], ceres.SE3Perturbation.Create())
    options = ceres.SolverOptions()
    options.max_num_iterations, options.use_nonmonotonic_steps = 1000, 1
    options.trust_region_strategy_type, options.dogleg_type = 1, 1
    summary = ceres.SolverSummary()
    ceres.Solve(options, problem, summary)
    assert summary.termination_type == ceres.CONVERGENCE
    covariance = ceres.Covariance()
    assert covariance.Compute([(poses[1], poses[1])], problem), covariance.message
    cov = np.zeros((6, 6))
    assert covariance.GetCovarianceBlockInTangentSpace(poses[1], poses[1], cov)
    assert np.all(np.linalg.eigvalsh(0.5 * (cov + cov.T)) > 0)


def test_cpp_shim_serves_the_request_from_the_solved_wide_handle():
    """examples/covariance_blocks_gpu with tracks of 16 observations: the C++ shim's Covariance::Compute runs on the handle its
    Solve used (ceres_shim.hpp: shim_prepare), a wide one here, after the solve.  Reference: the C ABI on a fresh handle at the
    printed solution (which, not solved yet, hands over to the blocked Cholesky), at the bar of
    test_cpp_example_blocks_match_the_c_abi."""
    from ceres_slam_amd import build
    exe = build.build_examples("covariance_blocks_gpu")
    r = subprocess.run([exe, "30", "400", "4.0"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    lines = [ln.split() for ln in r.stdout.decode().splitlines()]
    P, L, N = (int(x) for x in lines[0][1:])
    poses, points, ok, oj, uvd, cp, cpt, cpp = np.zeros((P, 12)), np.zeros((L, 3)), [], [], [], {}, {}, {}
    for w in lines[1:]:
        v = [float(x) for x in w[2:]]
        if w[0] == "pose":
            poses[int(w[1])] = v
        elif w[0] == "point":
            points[int(w[1])] = v
        elif w[0] == "obs":
            ok.append(int(w[1])); oj.append(int(w[2])); uvd.append(v[1:])
        elif w[0] == "cov_pose":
            cp[int(w[1])] = np.array(v).reshape(6, 6)
        elif w[0] == "cov_point":
            cpt[int(w[1])] = np.array(v).reshape(3, 3)
        elif w[0] == "cov_pose_point":
            cpp[(int(w[1]), int(w[2]))] = np.array(v[1:]).reshape(6, 3)
    assert len(ok) == N and len(cp) == P and cpt and cpp
    assert 13 <= np.bincount(oj).max() <= 24
    const = np.zeros(P, dtype=np.uint8); const[0] = 1
    cam = dict(fu=400.0, fv=400.0, cu=320.0, cv=240.0, b=0.24)
    ba = StereoBA(cam, poses, points, np.array(ok), np.array(oj), np.array(uvd), np.eye(3), pose_const=const, device=0)
    assert ba.stats().wide_superblocks == 2          # the layout the shim's handle of the same problem is on
    (j,) = cpt.keys()
    ((k, j2),) = cpp.keys()
    ref = ba.covariance_blocks([(("pose", q), ("pose", q)) for q in range(P)] + [(("point", j), ("point", j)), (("pose", k), ("point", j2))])
    assert not cp[0].any()
    for q in range(1, P):
        assert _rel(cp[q], ref[q]) <= 1e-9, q
    assert _rel(cpt[j], ref[P]) <= 1e-9
    assert _rel(cpp[(k, j2)], ref[P + 1]) <= 1e-9


def test_sun_driver_on_a_window_of_fourteen_states(tmp_path):
    """examples/dataset_vo_sun_gpu with tracks that span its window: every window's ceres::Covariance succeeds and the block it
    hands to the next window's prior is that window's own (SSBA_DRIVER_COVARS=1 prints it).  The driver gives every stereo
    block its point's own stiffness, which keeps its windows on the blocked Cholesky (ssba_layout.cpp: per-block stiffness
    lives in the general layout only): this pins the driver's chain of priors, not the wide route."""
    from ceres_slam_amd import build
    exe = build.build_examples("dataset_vo_sun_gpu")
    window = 14
    prob = synth.make_problem(17, 500, track_len=16, seed=4, obs_var=(0.04, 0.04, 0.04))
    sun = synth.make_sun_data(prob, seed=1)
    track, ref, obs = synth.write_reference_sun_csv(prob, sun, str(tmp_path / "sim.csv"))
    r = subprocess.run([exe, track, ref, obs, "--window", str(window), "--sun-only"], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, SSBA_DRIVER_COVARS="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Covariance computation failed" not in r.stdout and "WARNING" not in r.stdout
    n_windows = prob.num_poses - window + 1
    reports = [l for l in r.stdout.splitlines() if l.startswith("Ceres Solver Report")]
    assert len(reports) == n_windows and all("CONVERGENCE" in l for l in reports)
    covs = [np.array([float(x) for x in l.split(":")[1].split()]).reshape(6, 6) for l in r.stderr.splitlines() if l.startswith("pose covariance ")]
    assert len(covs) == n_windows
    for c in covs:
        assert np.all(np.linalg.eigvalsh(0.5 * (c + c.T)) > 0)
    for a, b in zip(covs, covs[1:]):
        assert not np.array_equal(a, b)
