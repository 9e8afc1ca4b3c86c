"""The HIP solve paths against the extended-precision reference of tests/hp_reference.py, with bars derived from conditioning
instead of from the oracle's own fp64 answer.

(A) every solve path on the system the device itself factorises (ssba_lm_step copies it out before the solve):
    eta <= 4096 u and |delta_p - x*| / |x*| <= min(4096 u kappa_2, 1e-8), x* from the refined solve.  A PCR sub-step that
    drops a Gram term of relative size 1e-10 moves the step by ~1e-10 relative: outside these bars for every kappa_2 below 2e8.
(B) the device's S and rhs against the long-double assembly within the entrywise bound E, the device's delta_l against the
    long-double back-substitution of its own delta_p, the model cost change against the long-double -J d.(r + J d / 2).
(C) the pose covariance against six refined solves of the long-double undamped S, within |S^-1| E |S^-1| + solve term, and
    no farther from that truth than the oracle's inverse or the fp64 solve bar 4096 u kappa_2, whichever is larger.  Where
    the solution holds a landmark nearly unobserved in depth (|p| ~ 1e6, kappa(V_j) ~ 1e12-1e13, eliminated undamped), the
    undamped E and the propagated bound exceed S and the covariance themselves and decide nothing; the distances do.
(D) one C2 step (84 super-blocks, k_bcr_factor_mf<3,2>): (A) on the band of its S, (B) on the whole block tridiagonal.

Every case asserts through ssba_stats that the intended path ran.  Run with -s to see the measured eta / error / kappa."""
import numpy as np
import pytest

import hp_reference as hp
from ceres_slam_amd import capi, synth
from ceres_slam_amd.solver import StereoBA
from oracle import oracle as orc

pytestmark = pytest.mark.gpu


def _report(tag, **kv):
    print("HPREF", tag, " ".join(f"{k}={v:.3g}" if isinstance(v, float) else f"{k}={v}" for k, v in kv.items()))


def _check_solve(tag, S, rhs, x_dev, band=None):
    """(A) on one system; returns (eta, forward error, kappa_2)."""
    x_ref, kap = hp.refined_solve(S, rhs, band)
    eta = hp.backward_error_banded(S, rhs, x_dev, band) if band is not None else hp.backward_error(S, rhs, x_dev)
    fe = hp.forward_error(x_dev, x_ref)
    eta_bar, fe_bar = hp.solve_bars(kap)
    _report(tag, n=S.shape[0], eta=eta, fe=fe, kappa=kap, eta_ratio=eta / eta_bar, fe_ratio=fe / fe_bar)
    assert eta <= eta_bar, (tag, eta, eta_bar)
    assert fe <= fe_bar, (tag, fe, fe_bar, kap)
    return eta, fe, kap


def _free_mask(prob, pose_const):
    return hp.free_index(prob.num_poses, prob.obs_pose, pose_const) >= 0


def _default_const(P):
    c = np.zeros(P, bool)
    c[0] = True
    return c


def _step_case(tag, ba, prob, radius, pose_const=None, factor_poses=None):
    S, rhs, dp, dl, mcc = ba.lm_step(radius)
    const = _default_const(prob.num_poses) if pose_const is None else np.asarray(pose_const, bool)
    free = hp.free_index(prob.num_poses, prob.obs_pose, const, factor_poses) >= 0
    assert 6 * int(free.sum()) == S.shape[0]
    return _check_solve(tag, S, rhs, dp[free].ravel())


RADII = [(1e4, 0.0), (3.0, 0.0), (1e4, 1.345)]


# ---------------------------------------------------------------------------------------------------- (A) the windowed chain
@pytest.mark.parametrize("radius,huber", RADII)
@pytest.mark.parametrize("last", ["padded", "full"])
@pytest.mark.parametrize("blocks", [1, 2, 3, 4, 5, 8, 9, 16, 17])
def test_fused_pcr_step_is_fp64_accurate(blocks, last, radius, huber):
    """Default plan (one launch per PCR step), k super-blocks: 12 (k - 1) + 1 free poses (the last block holds one pose and
    eleven identity rows) or 12 k (the last block full)."""
    P = 12 * (blocks - 1) + 2 if last == "padded" else 12 * blocks + 1
    prob = synth.make_problem(P, 40 * P, track_len=12, seed=P)
    ba = StereoBA.from_synth(prob, huber_a=huber)
    st = ba.stats()
    assert st.general_structure == 0 and st.num_superblocks == blocks
    if blocks > 1:
        assert st.pcr_blocks == blocks and st.pcr_fused == 1
    _step_case(f"fused_pcr k={blocks} {last} r={radius} h={huber}", ba, prob, radius)


@pytest.mark.parametrize("radius,huber", RADII)
@pytest.mark.parametrize("P,blocks", [(14, 2), (26, 3), (300, 25)])
def test_two_launch_pcr_step_is_fp64_accurate(monkeypatch, P, blocks, radius, huber):
    monkeypatch.setenv("SSBA_NO_PCR_FUSED", "1")
    prob = synth.make_problem(P, 30 * P, track_len=12, seed=3)
    ba = StereoBA.from_synth(prob, huber_a=huber)
    st = ba.stats()
    assert st.general_structure == 0 and st.num_superblocks == blocks and st.pcr_blocks == blocks
    _step_case(f"two_launch_pcr k={blocks} r={radius} h={huber}", ba, prob, radius)


@pytest.mark.parametrize("radius,huber", RADII)
def test_classic_bcr_step_is_fp64_accurate(monkeypatch, radius, huber):
    monkeypatch.setenv("SSBA_NO_PCR", "1")
    prob = synth.make_problem(300, 9000, track_len=12, seed=3)
    ba = StereoBA.from_synth(prob, huber_a=huber)
    st = ba.stats()
    assert st.general_structure == 0 and st.num_superblocks == 25 and st.pcr_blocks == 0
    _step_case(f"classic_bcr k=25 r={radius} h={huber}", ba, prob, radius)


@pytest.mark.parametrize("radius,huber", RADII)
@pytest.mark.parametrize("P,blocks", [(100, 9), (300, 25)])
def test_plain_levels_under_a_pcr_top_are_fp64_accurate(monkeypatch, P, blocks, radius, huber):
    """SSBA_PCR_MAX_BLOCKS=4: plain cyclic-reduction levels (two for 9 blocks, three for 25) below a parallel top."""
    monkeypatch.setenv("SSBA_PCR_MAX_BLOCKS", "4")
    prob = synth.make_problem(P, 30 * P, track_len=12, seed=3)
    ba = StereoBA.from_synth(prob, huber_a=huber)
    st = ba.stats()
    assert st.general_structure == 0 and st.num_superblocks == blocks and 0 < st.pcr_blocks <= 4
    _step_case(f"plain_levels k={blocks} top={st.pcr_blocks} r={radius} h={huber}", ba, prob, radius)


@pytest.mark.parametrize("radius,huber", RADII)
def test_constant_poses_inside_the_chain(radius, huber):
    """Gaps in the free index: constant poses in the middle of the chain (one of them at a super-block edge)."""
    prob = synth.make_problem(40, 1600, track_len=12, seed=8)
    const = np.zeros(40, bool)
    const[[0, 12, 13, 25]] = True
    ba = StereoBA(prob.camera, prob.poses_init.copy(), prob.points_init.copy(), prob.obs_pose, prob.obs_point, prob.obs_uvd,
                  prob.stiffness(), pose_const=const, huber_a=huber)
    st = ba.stats()
    assert st.general_structure == 0 and st.num_free_poses == 36 and st.num_superblocks == 3
    _step_case(f"const_gaps r={radius} h={huber}", ba, prob, radius, pose_const=const)


@pytest.mark.parametrize("radius,huber", RADII)
@pytest.mark.parametrize("L", [63, 64, 65])
def test_landmark_group_edges(L, radius, huber):
    """One window: all landmarks in one group of LMG = 64 lanes -- one short of, exactly, and one over a full group."""
    prob = synth.make_problem(8, L, track_len=5, seed=L)
    ba = StereoBA.from_synth(prob, huber_a=huber)
    assert ba.stats().general_structure == 0 and ba.stats().num_superblocks == 1
    _step_case(f"lmg L={L} r={radius} h={huber}", ba, prob, radius)


# ------------------------------------------------------------------------------------ (A) the general layout and the borders
@pytest.mark.parametrize("radius,huber", RADII)
@pytest.mark.parametrize("size,wide", [((14, 300, 13), 1), ((30, 900, 24), 2), ((75, 1800, 20), 4), ((200, 3000, 17), 9)])
def test_wide_superblock_step_is_fp64_accurate(size, wide, radius, huber):
    prob = synth.make_problem(size[0], size[1], track_len=size[2], seed=3)
    ba = StereoBA.from_synth(prob, huber_a=huber)
    st = ba.stats()
    assert st.general_structure == 1 and st.wide_superblocks == wide
    _step_case(f"wide k={wide} r={radius} h={huber}", ba, prob, radius)


@pytest.mark.parametrize("radius,huber", RADII)
@pytest.mark.parametrize("valu", [False, True])
@pytest.mark.parametrize("size,n", [((5, 120, 4), 24), ((11, 300, 8), 60), ((15, 400, 8), 84), ((30, 900, 12), 174)])
def test_blocked_cholesky_step_is_fp64_accurate(monkeypatch, size, n, valu, radius, huber):
    """SSBA_FORCE_DENSE=1: n below one 64-column panel, just across it (84) and over two.  Matrix-core panels, or with
    SSBA_DENSE_VALU=1 the VALU partner -- ssba_stats has no flag for the latter (both time under one kernel class), so
    what is asserted is the general layout without wide super-blocks; the variable is read by every dense solve."""
    monkeypatch.setenv("SSBA_FORCE_DENSE", "1")
    if valu:
        monkeypatch.setenv("SSBA_DENSE_VALU", "1")
    prob = synth.make_problem(size[0], size[1], track_len=size[2], seed=3)
    ba = StereoBA.from_synth(prob, huber_a=huber)
    st = ba.stats()
    assert st.general_structure == 1 and st.wide_superblocks == 0 and 6 * st.num_free_poses == n
    _step_case(f"dense{'_valu' if valu else ''} n={n} r={radius} h={huber}", ba, prob, radius)


@pytest.mark.parametrize("radius,huber", RADII)
def test_blocked_cholesky_of_long_tracks_without_wide_blocks(monkeypatch, radius, huber):
    monkeypatch.setenv("SSBA_NO_WIDE", "1")
    prob = synth.make_problem(30, 900, track_len=24, seed=3)
    ba = StereoBA.from_synth(prob, huber_a=huber)
    st = ba.stats()
    assert st.general_structure == 1 and st.wide_superblocks == 0
    _step_case(f"no_wide n={6 * st.num_free_poses} r={radius} h={huber}", ba, prob, radius)


@pytest.mark.parametrize("radius,huber", RADII)
@pytest.mark.parametrize("materials,nb", [(4, 19), (7, 31)])
def test_free_shared_border_step_is_fp64_accurate(materials, nb, radius, huber):
    """Lighting terms with the light, Phong parameters and textures free: [S S_pb; S_pb^T S_bb] at C1 size, 19 border
    columns and 31 (seven materials, one short of the 32-column cap)."""
    prob, ph = synth.make_phong_problem(50, 2000, num_materials=materials, seed=4)
    ba = StereoBA.from_synth(prob, lighting=ph.as_oracle_dict("truth"), shared_free=7, huber_a=huber)
    assert ba.stats().general_structure == 0
    S, rhs, dp, dl, mcc = ba.lm_step(radius)
    S_pb, S_bb, rhs_b, db = ba.border_system()
    assert S_pb.shape[1] == nb
    A = np.block([[S, S_pb], [S_pb.T, S_bb]])
    _check_solve(f"phong_border nb={nb} r={radius} h={huber}", A, np.concatenate([rhs, rhs_b]), np.concatenate([dp[1:].ravel(), db]))


# ------------------------------------------------------------------------------------------------- (A) unary and relative pose blocks
def _pose_factor_pair(prob, factors):
    none_const = np.zeros(prob.num_poses, dtype=np.uint8)
    return StereoBA(prob.camera, prob.poses_init.copy(), prob.points_init.copy(), prob.obs_pose, prob.obs_point, prob.obs_uvd,
                    prob.stiffness(), pose_const=none_const, pose_factors=factors)


@pytest.mark.parametrize("radius", [1e4, 20.0, 3.0])
@pytest.mark.parametrize("huber", [0.0, 0.5])
def test_step_with_sun_and_prior_blocks_is_fp64_accurate(huber, radius):
    from test_oracle_pose_factors import _sun_problem
    prob, factors = _sun_problem(huber=huber)
    ba = _pose_factor_pair(prob, factors)
    _step_case(f"sun_prior h={huber} r={radius}", ba, prob, radius, pose_const=np.zeros(prob.num_poses, bool))


@pytest.mark.parametrize("radius", [1e4, 20.0, 3.0])
@pytest.mark.parametrize("huber", [0.0, 0.05])
def test_step_with_relative_pose_blocks_is_fp64_accurate(huber, radius):
    from test_oracle_pose_factors import _odometry_factors
    prob = synth.make_problem(7, 100, track_len=4, seed=6)
    ba = _pose_factor_pair(prob, _odometry_factors(prob, huber=huber))
    _step_case(f"odometry h={huber} r={radius}", ba, prob, radius, pose_const=np.zeros(prob.num_poses, bool))


# ------------------------------------------------------------------------------------------------------ (B) against the truth
def _reference(prob, radius, huber=0.0, pose_const=None, stiffness=None):
    const = _default_const(prob.num_poses) if pose_const is None else pose_const
    rows = hp.stereo_rows(prob.camera, prob.poses_init, prob.points_init, prob.obs_pose, prob.obs_point, prob.obs_uvd,
                          prob.stiffness() if stiffness is None else stiffness, huber)
    fidx = hp.free_index(prob.num_poses, prob.obs_pose, const)
    return hp.SchurSystem(rows, prob.obs_pose, prob.obs_point, fidx, prob.num_points, radius), fidx


def _check_against_truth(tag, sy, S, rhs, dp, dl, mcc, fidx, prob_points):
    ex_S, ex_rhs = sy.assembly_excess(S, rhs)
    _report(tag + " assembly", S_over_E=ex_S, rhs_over_E=ex_rhs)
    assert ex_S <= 1.0 and ex_rhs <= 1.0, (tag, ex_S, ex_rhs)
    _check_back_substitution(tag, sy, dp, dl, mcc, fidx, prob_points)


def _back_substitution_bound(sy, x, dl_ref, prob_points, db=None):
    """Per landmark present: (t_j + c) u kappa(V_j) |V^-1| (|J_l|^T |r| + |J_l|^T |J_p| |delta_p|) + 2 u (|p_j| + |delta_l,j|)."""
    rows, fr, so = sy.rows, sy._f >= 0, sy.slot_of_obs
    gla = np.zeros((sy.lm.shape[0], sy.d))
    np.add.at(gla, so, np.einsum("nai,na->ni", rows["Jla"], rows["rabs"]))
    jdp = np.einsum("naj,nj->na", rows["Jpa"][fr], np.abs(x.reshape(-1, 6))[sy._f[fr]])
    np.add.at(gla, so[fr], np.einsum("nai,na->ni", rows["Jla"][fr], jdp))
    if sy.nb:       # the border step enters as J_l^T (J_b delta_b)
        np.add.at(gla, so, np.einsum("nai,na->ni", rows["Jla"], np.einsum("nab,b->na", rows["Jba"], np.abs(db))))
    mag = np.einsum("nij,nj->ni", np.abs(np.asarray(sy.Vinv, np.float64)), gla).max(1)
    t = np.bincount(sy.slot_of_obs, minlength=sy.lm.shape[0])
    pts = np.abs(prob_points[sy.lm]).max(1)
    return (t + hp.C_TERMS) * hp.U * sy.kappa_V * mag + 2 * hp.U * (pts + np.abs(np.asarray(dl_ref, np.float64)).max(1))


def _check_back_substitution(tag, sy, dp, dl, mcc, fidx, prob_points, db=None):
    x = dp[fidx >= 0].ravel()
    # delta_l from the device's own delta_p, per landmark within (t_j + c) u kappa(V_j) |V^-1| (|J_l|^T |r| + |J_l|^T |J_p| |delta_p|)
    # -- the device forms W^T delta_p as J_l^T (J_p delta_p) from re-linearised rows (k_backsub_eval), so the magnitudes are those
    # of the rows (Jla, Jpa, rabs: hp_reference.stereo_rows), not of |W| -- plus 2 u (|p_j| + |delta_l,j|): the hook reports
    # delta_l as fl(p + delta_l) - p (candidate minus current point)
    dl_ref = sy.back_substitute(x, db)
    bound = _back_substitution_bound(sy, x, dl_ref, prob_points, db)
    err = np.abs(np.asarray(np.asarray(dl[sy.lm], hp.LD) - dl_ref, np.float64)).max(1)
    _report(tag + " back-substitution", worst_over_bound=float((err / bound).max()))
    assert np.all(err <= bound), (tag, float((err / bound).max()))
    mref, mag_m, nt = sy.model_cost_change(x, dl[sy.lm], db)
    mb = (nt + hp.C_TERMS) * hp.U * mag_m
    _report(tag + " model cost change", err=abs(mcc - float(mref)), bound=mb)
    assert abs(mcc - float(mref)) <= mb


@pytest.mark.parametrize("radius,huber", RADII)
@pytest.mark.parametrize("which", ["tiny", "c1", "wide", "dense"])
def test_assembly_back_substitution_and_model_cost_against_the_truth(monkeypatch, which, radius, huber):
    if which == "tiny":
        prob = synth.make_problem(8, 60, track_len=5, seed=7)
    elif which == "c1":
        prob = synth.make_config("C1")
    elif which == "wide":
        prob = synth.make_problem(75, 1800, track_len=20, seed=3)
    else:
        monkeypatch.setenv("SSBA_FORCE_DENSE", "1")
        prob = synth.make_problem(30, 900, track_len=12, seed=3)
    ba = StereoBA.from_synth(prob, huber_a=huber)
    st = ba.stats()
    assert st.general_structure == (0 if which in ("tiny", "c1") else 1)
    assert (st.wide_superblocks > 0) == (which == "wide")
    S, rhs, dp, dl, mcc = ba.lm_step(radius)
    sy, fidx = _reference(prob, radius, huber)
    _check_against_truth(f"{which} r={radius} h={huber}", sy, S, rhs, dp, dl, mcc, fidx, prob.points_init)


_FACTOR_ROWS = {}


def _factor_reference(key, prob, factors, const, radius):
    """The long-double system of a problem with pose-only residual blocks (no loss on the stereo blocks): the stereo rows and
    the factor rows are computed once per `key` and shared by the radii."""
    if key not in _FACTOR_ROWS:
        rows = hp.stereo_rows(prob.camera, prob.poses_init, prob.points_init, prob.obs_pose, prob.obs_point, prob.obs_uvd, prob.stiffness())
        fidx = hp.free_index(prob.num_poses, prob.obs_pose, np.asarray(const, bool), hp.factor_poses(factors))
        sums = hp.PoseFactorSums(prob.num_poses, factors, hp.pose_factor_rows(prob.poses_init, factors), np.flatnonzero(fidx >= 0))
        _FACTOR_ROWS[key] = rows, fidx, sums
    rows, fidx, sums = _FACTOR_ROWS[key]
    return hp.SchurSystem(rows, prob.obs_pose, prob.obs_point, fidx, prob.num_points, radius, factor_sums=sums), fidx


@pytest.mark.parametrize("radius", [1e4, 3.0])
@pytest.mark.parametrize("huber", [0.0, 0.05])
@pytest.mark.parametrize("layout", ["windowed", "general"])
def test_assembly_with_sun_and_prior_blocks_against_the_truth(monkeypatch, layout, huber, radius):
    """S, rhs, delta_l and the model cost change of the sun-and-prior problem entrywise against the long-double system with the
    long-double factor blocks, on both layouts (the unary lanes of lin_pose_body; SSBA_FORCE_DENSE=1: pf_evaluate in the general
    kernels)."""
    from test_oracle_pose_factors import _sun_problem
    if layout == "general":
        monkeypatch.setenv("SSBA_FORCE_DENSE", "1")
    prob, factors = _sun_problem(huber=huber)
    ba = _pose_factor_pair(prob, factors)
    assert ba.stats().general_structure == int(layout == "general")
    S, rhs, dp, dl, mcc = ba.lm_step(radius)
    sy, fidx = _factor_reference(("sun", huber), prob, factors, np.zeros(prob.num_poses, bool), radius)
    _check_against_truth(f"sun_prior {layout} h={huber} r={radius}", sy, S, rhs, dp, dl, mcc, fidx, prob.points_init)


# ------------------------------------------------------------------------------------------------------- (C) the covariance
def _covariance_case(tag, ba, prob, factors, stiffness):
    P = prob.num_poses
    none_const = np.zeros(P, bool)
    fidx = hp.free_index(P, prob.obs_pose, none_const)
    H, g, Ha = hp.unary_pose_blocks(ba.poses, factors, fidx)
    rows = hp.stereo_rows(prob.camera, ba.poses, ba.points, prob.obs_pose, prob.obs_point, prob.obs_uvd, stiffness)
    sy = hp.SchurSystem(rows, prob.obs_pose, prob.obs_point, fidx, prob.num_points, None, H_unary=H, g_unary=g, Ha_unary=Ha)
    S_ld, E = sy.dense(), sy.dense_bound()
    S64 = np.asarray(S_ld, np.float64)
    Sg = ba.lm_step(1e300)[0]
    ex = sy.assembly_excess(Sg, np.zeros(sy.n))[0]
    op = orc.OracleProblem(prob.camera, ba.poses, ba.points, prob.obs_pose, prob.obs_point, prob.obs_uvd, stiffness,
                           pose_const=none_const.astype(np.uint8), pose_factors=factors)
    S2 = op.reduced_system(1e300)[0]
    ex2 = sy.assembly_excess(S2, np.zeros(sy.n))[0]
    # undamped, E bounds the cancellation only (see the module docstring): reported with what makes it so
    far = np.abs(ba.points[sy.lm]).max(1)
    _report(tag + " undamped S", device_over_E=ex, oracle_over_E=ex2, max_kappa_V=float(sy.kappa_V.max()),
            max_abs_point=float(far.max()), E_over_S=float((E / np.maximum(np.abs(S64), 1e-300)).max()))
    assert ex <= 1.0, (tag, ex)
    S2inv = np.linalg.inv(S2)
    out = []
    for k in (1, P // 2, P - 1):
        f = int(fidx[k])
        cov_true, kap = hp.covariance_truth(S_ld, f)
        cov_true = np.asarray(cov_true, np.float64)
        bound = hp.covariance_bound(S64, E, f, kap, cov_true)
        cov = ba.pose_covariance(k)
        cov_o = S2inv[6 * f: 6 * f + 6, 6 * f: 6 * f + 6]
        scale = np.abs(cov_true).max()
        d_hip, d_orc = np.abs(cov - cov_true).max() / scale, np.abs(cov_o - cov_true).max() / scale
        ratio = float((np.abs(cov - cov_true) / bound).max())
        solve_bar = hp.SOLVE_C * hp.U * kap
        _report(f"{tag} k={k}", kappa=kap, hip_to_truth=d_hip, oracle_to_truth=d_orc, solve_bar=solve_bar,
                bound_rel=float(bound.max() / scale), hip_over_bound=ratio)
        msg = (f"{tag} pose {k}: HIP to truth {d_hip:.3g}, oracle to truth {d_orc:.3g}, solve bar {solve_bar:.3g}, "
               f"propagated bound {bound.max() / scale:.3g}")
        assert ratio <= 1.0, msg
        # both are fp64 answers: where the oracle is within the solve bar this asks no more of the device than that bar;
        # where the oracle is far outside it (a landmark near infinity), the device must not be farther
        assert d_hip <= max(d_orc, solve_bar), msg


@pytest.mark.parametrize("P", [6, 30])
def test_pose_covariance_on_the_general_path_against_the_truth(P):
    """test_pose_covariance_on_the_general_path's problems (per-point stiffness, SUBSPACE_DOGLEG solve).  At P = 30 the
    solution holds a landmark nearly unobserved in depth (|p| ~ 1e6, kappa(V_j) 8e12, eliminated undamped): the oracle's inverse is
    ~1e-2 off the long-double truth, the device's ~1e-5, so the 6e-2 bar of that test measures the oracle there.  The
    reference carries the same error mechanism at 2^-64, ~2^-11 of the oracle's distance: it ranks the two sides, it does not
    certify the device's 1e-5.  At P = 6 both sides are at fp64 rounding level (~1e-11)."""
    from test_gpu_general_structure import _per_point_stiffness
    from test_oracle_pose_factors import _sun_problem
    prob, factors = _sun_problem(P=P, L=60 * P, seed=7)
    S = _per_point_stiffness(prob, seed=3)
    ba = StereoBA(prob.camera, prob.poses_init.copy(), prob.points_init.copy(), prob.obs_pose, prob.obs_point, prob.obs_uvd, S,
                  pose_const=np.zeros(P, dtype=np.uint8), pose_factors=factors)
    assert ba.stats().general_structure == 1
    ba.solve(capi.default_options(max_num_iterations=1000, use_nonmonotonic_steps=1, trust_region_strategy_type=1, dogleg_type=1))
    _covariance_case(f"cov_general P={P}", ba, prob, factors, S)


@pytest.mark.parametrize("P", [8, 30])
def test_pose_covariance_block_against_the_truth(P):
    """test_pose_covariance_block_matches_dense_inverse's problems (shared stiffness, windowed layout, LM solve).  At P = 8 a
    landmark nearly unobserved in depth (kappa(V_j) 3.7e12) again puts the oracle ~5e-4 off the truth and the device ~3e-7 (within the
    reference's own ~2^-11 of the oracle's distance); at P = 30 both are at fp64 rounding level (~1e-10)."""
    from test_oracle_pose_factors import _sun_problem
    prob, factors = _sun_problem(P=P, L=60 * P, seed=7)
    ba = _pose_factor_pair(prob, factors)
    ba.solve(capi.default_options(max_num_iterations=1000, use_nonmonotonic_steps=1))
    _covariance_case(f"cov_window P={P}", ba, prob, factors, prob.stiffness())


# --------------------------------------------------------------------------------------------------------- (D) full size, C2
def test_c2_step_against_the_truth():
    """One C2 step at the initial point: 1 000 poses, 84 super-blocks, seven k_bcr_factor_mf<3,2> launches.  (A) on the band of
    the device's S (lower bandwidth < 144); (B) on the whole block tridiagonal: S, rhs (and zeros outside the co-visible
    blocks), delta_l and the model cost change."""
    prob = synth.make_config("C2")
    ba = StereoBA.from_synth(prob)
    st = ba.stats()
    assert st.general_structure == 0 and st.num_superblocks == 84 and st.pcr_blocks == 84 and st.pcr_fused == 1
    S, rhs, dp, dl, mcc = ba.lm_step(1e4)
    bw = hp.bandwidth(S)
    assert bw < 2 * 72
    x_dev = dp[1:].ravel()
    _check_solve("c2 r=1e4", S, rhs, x_dev, band=bw)
    sy, fidx = _reference(prob, 1e4)
    _check_against_truth("c2", sy, S, rhs, dp, dl, mcc, fidx, prob.points_init)
