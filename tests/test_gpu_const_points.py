"""Constant point blocks on stereo problems (ssba_set_point_constant), windowed layout, some or all points constant.

As in Ceres a constant point is not part of x: no Jacobian columns, no Jacobi scale, no damping, no share in the norms; its
residual blocks stay in the cost.  The reference is tests/const_points_reference.py (np_reference.NumpyBA with the constant
points cleared from its `active` mask; pinned against the C oracle by tests/test_const_points_reference.py), the bars are the
project's: reduced system 1e-10, step 1e-8, cost log 1e-9, end point 1e-6.

The masks are chosen in DEVICE order (landmarks sorted by first pose, last pose, index; windows grown greedily over pose sets of
at most 12), which this file re-derives, so that "one 64-landmark group", "one window" and "63, 64, 65" (the last lane of one
wavefront and the first two of the next) mean what the kernels see."""
import functools

import numpy as np
import pytest

import const_points_reference as cpr
from ceres_slam_amd import capi, synth
from ceres_slam_amd.solver import StereoBA
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

SIZES = {"small": (8, 60, 5), "big": (40, 1600, 6)}
MASKS = ["third", "group", "window", "l63_65", "const_pose_only", "all_but_one"]
K = 8       # whole solves are cut at the same iteration count on both sides


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300))


@functools.lru_cache(maxsize=None)
def _prob(size, outliers=False):
    P, L, T = SIZES[size]
    return synth.make_problem(P, L, track_len=T, seed=7, outlier_fraction=0.3 if outliers else 0.0)


def _device_order(prob):
    """Observed landmarks in device order, and the first landmark of every window."""
    L, P = prob.num_points, prob.num_poses
    lo, hi = np.full(L, P, np.int64), np.full(L, -1, np.int64)
    np.minimum.at(lo, prob.obs_point, prob.obs_pose)
    np.maximum.at(hi, prob.obs_point, prob.obs_pose)
    seen = np.flatnonzero(hi >= 0)
    order = seen[np.lexsort((seen, hi[seen], lo[seen]))]
    sets = [set(prob.obs_pose[prob.obs_point == j].tolist()) for j in order]
    begins, cur = [0], set()
    for i, s in enumerate(sets):
        if len(cur | s) > 12:
            begins.append(i)
            cur = set(s)
        else:
            cur |= s
    return order, begins + [len(order)]


@functools.lru_cache(maxsize=None)
def _case(size, mask):
    """-> (point_const mask over the caller's points, pose_const)."""
    prob = _prob(size)
    L, P = prob.num_points, prob.num_poses
    order, wb = _device_order(prob)
    m = np.zeros(L, bool)
    pose_const = np.zeros(P, bool)
    pose_const[0] = True
    if mask == "third":
        m[::3] = True
    elif mask == "group":           # the second 64-landmark group where there is one, else the only (partial) group
        m[order[64:128] if len(order) >= 128 else order[:64]] = True
    elif mask == "window":          # every landmark of one window (= one or more whole Schur items)
        w = min(1, len(wb) - 2)
        m[order[wb[w]:wb[w + 1]]] = True
    elif mask == "l63_65":
        m[order[[i for i in (63, 64, 65) if i < len(order)]]] = True
        if len(order) < 66:         # (60 landmarks: the last three lanes of the only wavefront instead)
            m[order[-3:]] = True
    elif mask == "const_pose_only":  # a constant point all of whose observing poses are constant too: cost only
        j = int(order[len(order) // 2])
        m[j] = True
        pose_const[np.unique(prob.obs_pose[prob.obs_point == j])] = True
        m[::5] = True
    elif mask == "all_but_one":
        m[:] = True
        m[int(order[len(order) // 2])] = False
    else:
        assert mask == "none"
    return m, pose_const


def _structure(size, mask):
    """3 (pose-only layout) when the mask covers every observed point, else 0 (windowed)."""
    m, _ = _case(size, mask)
    prob = _prob(size)
    return 3 if m[np.unique(prob.obs_point)].all() else 0


def _handle(size, mask, huber_a=0.0, outliers=False, **kw):
    prob = _prob(size, outliers)
    m, pc = _case(size, mask)
    return StereoBA.from_synth(prob, pose_const=pc, point_const=m, huber_a=huber_a, **kw)


def _reference(size, mask, huber_a=0.0, outliers=False):
    prob = _prob(size, outliers)
    m, pc = _case(size, mask)
    return cpr.ConstPointsBA.from_synth(prob, point_const=m, pose_const=pc, huber_a=huber_a)


@functools.lru_cache(maxsize=None)
def _reference_solve(size, mask, strategy, dogleg_type, huber_a, outliers=False):
    ref = _reference(size, mask, huber_a, outliers)
    x_p, x_l, log = ref.solve(max_iter=K) if strategy == 0 else cpr.dogleg_solve(ref, dogleg_type, max_iter=K)
    # the iterate the solver hands back is the lowest-cost one it accepted (the first of equals): with non-monotonic steps that
    # need not be the last, so the loop is run again up to that iteration
    accepted = [(c, i) for i, (c, ok) in enumerate(log) if ok or i == 0]
    best = min(accepted)[1]
    if best != accepted[-1][1]:
        x_p, x_l, _ = ref.solve(max_iter=best) if strategy == 0 else cpr.dogleg_solve(ref, dogleg_type, max_iter=best)
    for a in (x_p, x_l):
        a.setflags(write=False)
    return x_p, x_l, tuple(log)


# ------------------------------------------------------------------------------------------------------ one step
@pytest.mark.parametrize("radius", [1e4, 3.0])
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("size", list(SIZES))
def test_reduced_system_and_step_match_the_dense_reference(size, mask, radius):
    ba = _handle(size, mask)
    assert ba.stats().general_structure == _structure(size, mask)
    m, _ = _case(size, mask)
    S, rhs, dp, dl, mcc = ba.lm_step(radius)
    assert ba.stats().general_structure == 0       # (a pose-only handle hands over to the windowed layout for the hook)
    ref = _reference(size, mask)
    S2, rhs2, dp2, dl2, _ = cpr.dense_reduced_system(ref, ref.poses, ref.points, radius)
    _, _, mcc2, _, _ = ref.lm_step(ref.poses, ref.points, radius)
    print(size, mask, radius, "S", _rel(S, S2), "rhs", _rel(rhs, rhs2), "dp", _rel(dp, dp2), "dl", _rel(dl, dl2))
    assert _rel(S, S2) <= 1e-10 and _rel(rhs, rhs2) <= 1e-10
    assert _rel(dp, dp2) <= 1e-8 and _rel(dl, dl2) <= 1e-8
    assert mcc == pytest.approx(mcc2, rel=1e-9)
    assert not dl[m].any()                      # exact zeros
    assert np.array_equal(ba.points, _prob(size).points_init)


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("size", list(SIZES))
def test_evaluate_reports_zero_blocks_for_constant_points(size, mask):
    ba = _handle(size, mask)
    m, _ = _case(size, mask)
    cost, g_p, g_l, H_pp, H_ll = ba.evaluate()
    ref = _reference(size, mask)
    c2, _ = ref.residuals(ref.poses, ref.points)
    assert cost == pytest.approx(c2, rel=1e-12)          # every residual block counts, constant ones too
    assert not g_l[m].any() and not H_ll[m].any()
    full = StereoBA.from_synth(_prob(size), pose_const=_case(size, mask)[1])
    _, g_p0, g_l0, H_pp0, H_ll0 = full.evaluate()
    assert np.array_equal(g_l[~m], g_l0[~m]) and np.array_equal(H_ll[~m], H_ll0[~m])
    assert np.array_equal(g_p, g_p0) and np.array_equal(H_pp, H_pp0)     # J_p^T J_p of the constant points stays


@pytest.mark.parametrize("dogleg_type", [0, 1])
@pytest.mark.parametrize("mask", ["third", "all_but_one"])
def test_dogleg_step_has_no_entries_for_constant_points(mask, dogleg_type):
    ba = _handle("small", mask)
    m, _ = _case("small", mask)
    st = ba.dogleg_step(1e4, 1e-8, capi.default_options(dogleg_type=dogleg_type))
    assert not st.gn_l[m].any() and not st.v_l[m].any()
    ref = _reference("small", mask)
    import np_reference as npr
    keep = np.concatenate([np.ones(6 * ref.nf, bool), np.repeat(ref.active, 3)])
    s = npr.dogleg_linearize(ref, ref.poses, ref.points, keep, None, 1e-8)
    Jg = s["Js"] @ (s["grad"] / s["D"])
    Jn = s["Js"] @ (s["gn"] / s["D"])
    sums = np.array([s["grad"] @ s["grad"], s["gn"] @ s["gn"], s["grad"] @ s["gn"], Jg @ Jg, Jn @ Jn, Jg @ Jn])
    print(mask, dogleg_type, st.sums / sums - 1)
    np.testing.assert_allclose(st.sums, sums, rtol=1e-8)


# ------------------------------------------------------------------------------------------------------ whole solves
@pytest.mark.parametrize("huber_a", [0.0, 1.345])
@pytest.mark.parametrize("strategy,dogleg_type", [(0, 0), (1, 0), (1, 1)])
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("size", list(SIZES))
def test_solve_matches_the_numpy_reference(size, mask, strategy, dogleg_type, huber_a):
    """The two problems as synth.make_problem gives them (no gross outliers; at the 2-pixel noise of the generator a good share
    of the residual blocks still sits in the linear part of the Huber loss at 1.345).  Same accept / reject sequence and
    iteration count, cost log 1e-9, final cost and poses 1e-6, constant points bit-equal to the input."""
    ba = _handle(size, mask, huber_a)
    m, _ = _case(size, mask)
    s, log = ba.solve(capi.default_options(max_num_iterations=K, use_nonmonotonic_steps=1, trust_region_strategy_type=strategy,
                                           dogleg_type=dogleg_type))
    x_p, x_l, rlog = _reference_solve(size, mask, strategy, dogleg_type, huber_a)
    assert ba.stats().general_structure == (_structure(size, mask) if strategy == 0 else 0)      # DOGLEG hands a pose-only handle over
    n = min(len(log["cost"]), len(rlog))
    print(size, mask, strategy, dogleg_type, huber_a, "iterations", len(log["cost"]), len(rlog),
          "cost log", _rel(log["cost"][:n], np.array([c for c, _ in rlog][:n])))
    assert len(log["cost"]) == len(rlog)
    assert log["step_is_successful"].tolist() == [int(ok) for _, ok in rlog]
    np.testing.assert_allclose(log["cost"], [c for c, _ in rlog], rtol=1e-9)
    accepted = [c for i, (c, ok) in enumerate(rlog) if ok or i == 0]
    assert s.final_cost == pytest.approx(min(accepted), rel=1e-6)
    assert np.abs(ba.poses - x_p).max() <= 1e-6           # (x_p, x_l: the reference's lowest-cost iterate)
    if not m.all():
        assert (np.abs(ba.points[~m] - x_l[~m]) / np.maximum(1.0, np.abs(x_l[~m]))).max() <= 1e-6
    init = _prob(size).points_init
    assert ba.points[m].tobytes() == init[m].tobytes()          # bit-equal to the input


@pytest.mark.parametrize("strategy", [0, 1])
@pytest.mark.parametrize("mask", ["none", "third", "all_but_one"])
@pytest.mark.parametrize("size", list(SIZES))
def test_huber_solve_with_gross_outliers(size, mask, strategy):
    """Beyond the cases above: 30 % gross outliers under the Huber loss.  Badly observed landmarks travel 1e5 m and the cost
    traces of two correct fp64 implementations part at the 1e-9 level whether or not a point is constant (mask "none" is the
    plain handle, printed next to the others), so this configuration keeps the bar it has elsewhere in the suite
    (test_gpu_parity.test_huber_outlier_solve_matches_oracle): cost log 1e-8, final cost 1e-6; the accept / reject sequence
    is the same."""
    ba = _handle(size, mask, 1.345, outliers=True)
    m, _ = _case(size, mask)
    s, log = ba.solve(capi.default_options(max_num_iterations=K, use_nonmonotonic_steps=1, trust_region_strategy_type=strategy))
    x_p, x_l, rlog = _reference_solve(size, mask, strategy, 0, 1.345, True)
    rc = np.array([c for c, _ in rlog])
    n = min(len(log["cost"]), len(rlog))
    print(size, mask, strategy, "outliers: iterations", len(log["cost"]), len(rlog), "cost log", _rel(log["cost"][:n], rc[:n]),
          "poses", np.abs(ba.poses - x_p).max())
    assert len(log["cost"]) == len(rlog)
    assert log["step_is_successful"].tolist() == [int(ok) for _, ok in rlog]
    np.testing.assert_allclose(log["cost"], rc, rtol=1e-8)
    accepted = [c for i, (c, ok) in enumerate(rlog) if ok or i == 0]
    assert s.final_cost == pytest.approx(min(accepted), rel=1e-6)
    assert ba.points[m].tobytes() == _prob(size, True).points_init[m].tobytes()


@pytest.mark.parametrize("strategy", [0, 1])
def test_two_solves_are_bit_equal(strategy):
    out = []
    for _ in range(2):
        ba = _handle("big", "third")
        s, log = ba.solve(capi.default_options(max_num_iterations=K, use_nonmonotonic_steps=1, trust_region_strategy_type=strategy))
        out.append((log["cost"].tobytes(), ba.poses.tobytes(), ba.points.tobytes()))
    assert out[0] == out[1]


def test_a_handle_without_constant_points_is_unchanged_by_an_empty_mask():
    """point_const all False goes through ssba_set_point_constant with an empty list: same bits as the handle that never
    heard of it."""
    prob = _prob("big")
    out = []
    for pc in (None, np.zeros(prob.num_points, bool)):
        ba = StereoBA.from_synth(prob, point_const=pc)
        s, log = ba.solve(capi.default_options(max_num_iterations=K, use_nonmonotonic_steps=1))
        out.append((log["cost"].tobytes(), ba.poses.tobytes(), ba.points.tobytes()))
    assert out[0] == out[1]


def test_every_point_constant_through_both_calls_matches_the_oracle():
    """ssba_set_point_blocks_constant(1) on a stereo handle = every point through ssba_set_point_constant; both against the C
    oracle's positions_const, which exists for exactly this mask."""
    prob = _prob("big")
    op = orc.OracleProblem(prob.camera, prob.poses_init, prob.points_init, prob.obs_pose, prob.obs_point, prob.obs_uvd, prob.stiffness(),
                           positions_const=True)
    s2, log2 = op.solve(orc.driver_options(num_threads=2, max_num_iterations=K))
    logs = []
    for kw in (dict(points_const=True), dict(point_const=np.ones(prob.num_points, bool))):
        ba = StereoBA.from_synth(prob, **kw)
        assert ba.stats().general_structure == 3
        s, log = ba.solve(capi.default_options(max_num_iterations=K, use_nonmonotonic_steps=1))
        assert s.num_iterations == s2.num_iterations
        assert log["step_is_successful"].tolist() == log2["step_is_successful"].tolist()
        np.testing.assert_allclose(log["cost"], log2["cost"], rtol=1e-9)
        assert s.final_cost == pytest.approx(s2.final_cost, rel=1e-6)
        assert np.abs(ba.poses - op.poses).max() <= 1e-6
        assert ba.points.tobytes() == prob.points_init.tobytes()
        logs.append(log["cost"].tobytes())
    assert logs[0] == logs[1]


# ------------------------------------------------------------------------------------------------------ pose factors
def _sun_prior_factors(prob):
    """The factor set of test_gpu_wide_covariance.test_prior_and_sun_blocks_with_dogleg."""
    rng = np.random.default_rng(7)
    sun_g = np.array([0.3, -0.8, 0.5])
    factors = [dict(pose=0, type=0, data=prob.poses_init[0], stiffness=np.eye(6) * 1e2)]
    for k in range(prob.num_poses):
        if k % 4 == 3:
            continue
        obs = prob.poses_gt[k][3:].reshape(3, 3) @ sun_g + 0.01 * rng.normal(size=3)
        factors.append(dict(pose=k, type=1, data=np.concatenate([obs, sun_g, [1000.0, 1000.0]]), stiffness=np.eye(2).ravel() * 50.0, huber=0.0))
    return factors


@pytest.mark.parametrize("which", ["odometry", "prior_sun"])
def test_pose_factors_with_constant_points_match_the_oracle(which):
    """Odometry chain (the factor set of test_gpu_odometry_chain) / prior + sun blocks with no constant pose: blocks that touch
    no landmark ride along unchanged.  The oracle has a switch for "every point" only, so that is the mask; the windowed kernels
    that run are those of the subset masks above."""
    from test_oracle_pose_factors import _odometry_factors
    prob = synth.make_problem(20, 700, track_len=6, seed=11, pose_sigma=(0.1, 0.02))
    if which == "odometry":
        const = np.zeros(prob.num_poses, np.uint8)       # (the chain's prior on pose 0 holds the gauge)
        factors = _odometry_factors(prob, loop=False, huber=0.0)
    else:
        const = np.zeros(prob.num_poses, np.uint8)
        factors = _sun_prior_factors(prob)
    ba = StereoBA(prob.camera, prob.poses_init.copy(), prob.points_init.copy(), prob.obs_pose, prob.obs_point, prob.obs_uvd, prob.stiffness(),
                  pose_const=const, pose_factors=factors, point_const=np.ones(prob.num_points, bool))
    assert ba.stats().general_structure == (0 if which == "odometry" else 3)      # a chain couples free poses: windowed
    op = orc.OracleProblem(prob.camera, prob.poses_init, prob.points_init, prob.obs_pose, prob.obs_point, prob.obs_uvd, prob.stiffness(),
                           pose_const=const, pose_factors=factors, positions_const=True)
    s, log = ba.solve(capi.default_options(max_num_iterations=K, use_nonmonotonic_steps=1))
    s2, log2 = op.solve(orc.driver_options(num_threads=2, max_num_iterations=K))
    assert s.num_iterations == s2.num_iterations
    assert log["step_is_successful"].tolist() == log2["step_is_successful"].tolist()
    np.testing.assert_allclose(log["cost"], log2["cost"], rtol=1e-9)
    assert s.final_cost == pytest.approx(s2.final_cost, rel=1e-6)
    assert np.abs(ba.poses - op.poses).max() <= 1e-6
    assert ba.points.tobytes() == prob.points_init.tobytes()


@pytest.mark.parametrize("radius", [1e4, 3.0])
@pytest.mark.parametrize("which", ["odometry", "prior_sun"])
def test_pose_factors_with_a_subset_of_constant_points(which, radius):
    """The same factor sets with every third point constant: nonzero Schur products next to chain blocks and unary blocks.
    The oracle has no per-point switch, so it supplies what it can -- the contribution of the pose-only blocks to the reduced
    system, as the difference of its systems with and without them (they touch no landmark column; their damping is linear in
    diag(J^T J) away from the clamps) -- and the reference removes the constant columns from the stereo part:
    S = S_reference(stereo, subset) + (S_oracle(with blocks) - S_oracle(without)), the right-hand side alike.  Bars of the step
    test above: S and rhs 1e-10, step 1e-8, exact zeros for the constant points."""
    from test_oracle_pose_factors import _odometry_factors
    prob = synth.make_problem(20, 700, track_len=6, seed=11, pose_sigma=(0.1, 0.02))
    const = np.zeros(prob.num_poses, np.uint8)
    factors = _odometry_factors(prob, loop=False, huber=0.0) if which == "odometry" else _sun_prior_factors(prob)
    m = np.arange(prob.num_points) % 3 == 0
    args = (prob.camera, prob.poses_init, prob.points_init, prob.obs_pose, prob.obs_point, prob.obs_uvd, prob.stiffness())
    ba = StereoBA(prob.camera, prob.poses_init.copy(), prob.points_init.copy(), *args[3:], pose_const=const, pose_factors=factors, point_const=m)
    assert ba.stats().general_structure == 0
    S, rhs, dp, dl, _ = ba.lm_step(radius)
    Sa, ra, fa = orc.OracleProblem(*args, pose_const=const, pose_factors=factors).reduced_system(radius)
    Sb, rb, fb = orc.OracleProblem(*args, pose_const=const).reduced_system(radius)
    assert np.array_equal(fa, fb) and (fa >= 0).all()
    ref = cpr.ConstPointsBA(*args, pose_const=const.astype(bool), point_const=m)
    S2, rhs2, dp2, dl2, _ = cpr.dense_reduced_system(ref, ref.poses, ref.points, radius, extra_S=Sa - Sb, extra_rhs=ra - rb)
    print(which, radius, "S", _rel(S, S2), "rhs", _rel(rhs, rhs2), "dp", _rel(dp, dp2), "dl", _rel(dl, dl2))
    assert _rel(S, S2) <= 1e-10 and _rel(rhs, rhs2) <= 1e-10
    assert _rel(dp, dp2) <= 1e-8 and _rel(dl, dl2) <= 1e-8
    assert not dl[m].any() and dl[~m].any()


# ------------------------------------------------------------------------------------------------------ covariance
@pytest.mark.parametrize("mask", ["third", "window", "all_but_one"])
def test_covariance_blocks(mask):
    size = "big"
    ba = _handle(size, mask)
    m, pc = _case(size, mask)
    ba.solve(capi.default_options(max_num_iterations=30, use_nonmonotonic_steps=1))
    P, L = ba.poses.shape[0], ba.points.shape[0]
    cst, fre = np.flatnonzero(m), np.flatnonzero(~m)
    pairs = [(("pose", k), ("pose", k)) for k in range(P)] + [(("pose", 1), ("pose", P - 1)), (("pose", 3), ("pose", 4))]
    n_pose = len(pairs)
    pairs += [(("point", int(j)), ("point", int(j))) for j in cst[:5]]
    pairs += [(("pose", 2), ("point", int(cst[0]))), (("point", int(cst[-1])), ("pose", P - 2))]
    pairs += [(("point", int(fre[0])), ("point", int(fre[0])))]
    out = ba.covariance_blocks(pairs)
    for blk in out[n_pose:-1]:
        assert not blk.any()                         # every block that touches a constant point
    assert out[-1].any()
    ref = cpr.ConstPointsBA(_prob(size).camera, ba.poses, ba.points, _prob(size).obs_pose, _prob(size).obs_point, _prob(size).obs_uvd,
                            _prob(size).stiffness(), pose_const=pc, point_const=m)
    Sinv = np.linalg.inv(cpr.undamped_reduced_system(ref, ref.poses, ref.points))
    worst = 0.0
    for ((_, a), (_, b)), blk in zip(pairs[:n_pose], out[:n_pose]):
        fa, fb = ref.free_idx[a], ref.free_idx[b]
        if fa < 0 or fb < 0:
            assert not blk.any()
            continue
        worst = max(worst, _rel(blk, Sinv[6 * fa:6 * fa + 6, 6 * fb:6 * fb + 6]))
    print(mask, "pose blocks against the inverse of the reference S", worst)
    assert worst <= 1e-8
    assert ba.points[m].tobytes() == _prob(size).points_init[m].tobytes()


# ------------------------------------------------------------------------------------------------------ not in this layout
def test_unsupported_combinations_say_so():
    prob = _prob("big")
    L = prob.num_points
    some = np.arange(L) % 3 == 0

    def refused(make):
        with pytest.raises(capi.SsbaError) as e:
            make()
        assert e.value.status == -6, e.value
        return str(e.value)

    pprob, ph = synth.make_phong_problem(40, 1600, num_materials=3, seed=4)
    assert "lighting" in refused(lambda: StereoBA.from_synth(pprob, lighting=ph.as_oracle_dict("truth"), point_const=some))
    assert "sharding" in refused(lambda: StereoBA.from_synth(prob, world_size=2, rank=0, point_const=some))
    loop = synth.add_loop_closure(synth.make_problem(60, 2400, track_len=6, seed=5))
    assert StereoBA.from_synth(loop).stats().general_structure == 2
    assert "closure border" in refused(lambda: StereoBA.from_synth(loop, point_const=np.arange(loop.num_points) % 3 == 0))
    long = synth.make_problem(30, 900, track_len=20, seed=7)
    one_free = np.ones(long.num_points, bool)
    one_free[17] = False
    assert "layout" in refused(lambda: StereoBA.from_synth(long, point_const=one_free))
    # an index out of range, and a call after ssba_finalize
    ba = StereoBA.from_synth(prob, finalize=False)
    bad = np.array([L], dtype=np.uint32)
    assert ba.lib.ssba_set_point_constant(ba.h, bad.ctypes.data_as(capi._u32p), 1, 1) == -1
    ba.finalize()
    ok = np.array([0], dtype=np.uint32)
    assert ba.lib.ssba_set_point_constant(ba.h, ok.ctypes.data_as(capi._u32p), 1, 1) == -7


# ------------------------------------------------------------------------------------------------------ the shims
def test_python_mirror_holds_point_blocks_constant():
    from ceres_slam_amd import ceres_api as ceres
    prob = _prob("small")
    m, _ = _case("small", "third")
    poses, points = prob.poses_init.copy(), prob.points_init.copy()
    problem = ceres.Problem()
    cam = ceres.StereoCamera(**prob.camera)
    problem.AddStereoResidualBlocks(cam, prob.stiffness(), None, poses, points, prob.obs_pose, prob.obs_point, prob.obs_uvd)
    for k in range(prob.num_poses):
        problem.SetParameterization(poses[k], ceres.SE3Perturbation())
    problem.SetParameterBlockConstant(poses[0])
    for j in np.flatnonzero(m):
        problem.SetParameterBlockConstant(points[j])
    problem.SetParameterBlockConstant(points[1])
    problem.SetParameterBlockVariable(points[1])
    options, summary = ceres.SolverOptions(), ceres.SolverSummary()
    options.max_num_iterations = K
    options.use_nonmonotonic_steps = True
    ceres.Solve(options, problem, summary)
    x_p, x_l, rlog = _reference_solve("small", "third", 0, 0, 0.0)
    np.testing.assert_allclose([it["cost"] for it in summary.iterations], [c for c, _ in rlog], rtol=1e-9)
    assert points[m].tobytes() == prob.points_init[m].tobytes()
    assert np.abs(points[~m] - prob.points_init[~m]).max() > 0


@pytest.mark.parametrize("which", ["all", "third"])
def test_cpp_example_through_the_shim_matches_the_c_abi(which):
    """examples/const_points_gpu.cpp: SetParameterBlockConstant on point blocks through ceres_shim.hpp (all of them ->
    ssba_set_point_blocks_constant, a subset -> ssba_set_point_constant); the same problem through the C ABI gives the same poses."""
    import subprocess
    from ceres_slam_amd import build
    exe = build.build_examples("const_points_gpu")
    r = subprocess.run([exe, which, "16", "200"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    lines = [ln.split() for ln in r.stdout.decode().splitlines()]
    P, L, N = (int(x) for x in lines[0][1:])
    p0, x0, p1, x1 = np.zeros((P, 12)), np.zeros((L, 3)), np.zeros((P, 12)), np.zeros((L, 3))
    m = np.zeros(L, bool)
    ok, oj, uvd = [], [], []
    for w in lines[1:]:
        if w[0] in ("pose0", "pose"):
            (p0 if w[0] == "pose0" else p1)[int(w[1])] = [float(x) for x in w[2:]]
        elif w[0] in ("point0", "point"):
            (x0 if w[0] == "point0" else x1)[int(w[1])] = [float(x) for x in w[2:]]
        elif w[0] == "const":
            m[int(w[1])] = True
        elif w[0] == "obs":
            ok.append(int(w[1])); oj.append(int(w[2])); uvd.append([float(x) for x in w[3:]])
    assert len(ok) == N and m.sum() == (L if which == "all" else (L + 2) // 3)
    assert "Termination: CONVERGENCE" in r.stdout.decode()
    cam = dict(fu=400.0, fv=400.0, cu=320.0, cv=240.0, b=0.24)
    const = np.zeros(P, dtype=np.uint8)
    const[0] = 1
    ba = StereoBA(cam, p0.copy(), x0.copy(), np.array(ok), np.array(oj), np.array(uvd), np.eye(3), pose_const=const, point_const=m, device=0)
    assert ba.stats().general_structure == (3 if which == "all" else 0)
    s, _ = ba.solve(capi.default_options(max_num_iterations=100))
    assert s.termination_type == 0
    assert np.abs(p1 - ba.poses).max() <= 1e-9 and np.abs(p1 - p0).max() > 1e-3
    assert x1[m].tobytes() == x0[m].tobytes()
    if which == "third":
        assert np.abs(x1[~m] - ba.points[~m]).max() <= 1e-9 and np.abs(x1[~m] - x0[~m]).max() > 1e-4
