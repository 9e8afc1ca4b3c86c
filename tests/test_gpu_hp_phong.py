"""The lighting rows and the closure border against the extended-precision reference of tests/hp_reference.py.

(R) capi.phong_evaluate (the rows of ssba_phong_device.h: ph_rsqrt / ph_rcp, exp(alpha log s), the guards and the clamp) on
    batches built to sit on the edges: every residual and Jacobian entry within C_ROW u mag of the long-double row
    (hp_reference.phong_rows).  Each batch asserts that it holds the edge it was built for, on both sides of the guard.
(B) the lighting path's reduced system (inv6_spd, k_ph_schur_windows, the border sums k_ph_hpb / k_ph_spb_assemble /
    k_ph_border_landmarks / k_ph_border_schur, k_ph_backsub_eval) against the long-double SchurSystem with 6-D landmarks and
    the border: S, rhs, S_pb, S_bb, rhs_b within E (zeros outside the co-visible blocks), delta_l against the long-double
    back-substitution of the device's own (delta_p, delta_b), the model cost change, and the bordered solve through
    _check_solve.  Not included: a C3-sized step.  Its long-double rows need about 60 complex-step evaluations per row for
    the rounding magnitudes (some 20 s per 10^4 observations on one core here), which at C3 size alone exceeds the time
    this file may take; the windowed kernels it would add are the ones the C1 cases already span over several super-blocks.
(E) the closure border (general_structure == 2, ssba_border.hip): the device's delta_p against the refined solve x* of the
    long-double reduced system over all free poses in user order,
        |delta_p - x*|_inf <= || |S^-1| (E |x*| + E_rhs) ||_inf + 4096 u kappa_2 |x*|_inf,
    and delta_l and the model cost change against the long-double back-substitution of the device's own delta_p.

Run with -s to see the HPREF lines: the worst ratio to each bar."""
import os

import numpy as np
import pytest

import hp_reference as hp
from ceres_slam_amd import capi, synth
from ceres_slam_amd.solver import StereoBA
from test_gpu_hp_reference import _check_back_substitution, _check_solve, _reference, _report

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------- (R) rows
def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _rotation(rng):
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return Q * np.sign(np.linalg.det(Q))


def _edge_batch(kind, light_type, rng, N=64):
    """Rows whose camera-frame quantities are chosen, then carried to the world frame through one pose (R, t)."""
    R, t = _rotation(rng), rng.normal(size=3)
    T = np.tile(np.concatenate([t, R.ravel()]), (N, 1))
    q = _unit(rng.normal(size=(N, 3)) * [1, 1, 0.3] + [0, 0, 1]) * rng.uniform(2, 8, (N, 1))
    q[:, 2] = np.abs(q[:, 2]) + 0.5
    cd = -_unit(q)
    lc = np.array([0.5, -3.0, 1.0]) if light_type == 0 else _unit(np.array([0.3, -0.8, 0.5]))
    if kind == "near_light":
        lc = q[0] + np.array([1e-6, -2e-6, 0.5e-6])          # a point light 2.4e-6 from the first point
        q = q[0] + rng.normal(size=(N, 3)) * 1e-5
        cd = -_unit(q)
    ell = _unit(lc - q) if light_type == 0 else np.tile(lc, (N, 1))
    kd = rng.uniform(0.2, 0.9, N)
    phong = np.stack([np.zeros(N), rng.uniform(0.05, 0.5, N), rng.uniform(1, 20, N)], 1)
    colour = rng.uniform(0, 1, N)
    if kind == "ldn":                          # ell . nc within 1e-12 of 0, both sides, down to 3e-15 (not within fp64
        # rounding of the guard: there either branch is a correct fp64 answer and the perturbation magnitude measures the jump)
        eps = np.tile([1e-12, -1e-12, 1e-13, -1e-13, 3e-15, -3e-15, 1e-14, -1e-14], N // 8)
        perp = _unit(np.cross(ell, rng.normal(size=(N, 3))))
        nc = _unit(perp + eps[:, None] * ell)
    elif kind == "s_small":                    # s = m . cd just above 0, alpha 1 and 20
        sig = np.tile([1e-3, 1e-6, 1e-8, 1e-10], N // 4)
        perp = _unit(np.cross(cd, rng.normal(size=(N, 3))))
        m = _unit(perp + sig[:, None] * cd)
        nc = _unit(ell + m)
        phong[:, 2] = np.tile([1.0, 20.0], N // 2)
        kd[:] = 0.0
    else:
        nc = _unit(ell + _unit(rng.normal(size=(N, 3))) * 0.7)
    ldn = (ell * nc).sum(1)
    if kind == "clamp":                        # col = kd ldn (ks = 0): beyond 1, 1e-14 inside 1, 1e-14 above 0, at or below 0
        nc = _unit(ell + _unit(rng.normal(size=(N, 3))) * 0.3)
        ldn = (ell * nc).sum(1)
        target = np.tile([1 + 1e-10, 1 - 1e-14, 1 - 1e-13, 1e-14, 1e-13, 0.5, 2.0, -0.3], N // 8)
        kd = target / ldn
        phong[:, 1] = 0.0
    n = nc @ R                                   # world normal: R^T nc
    if kind == "norm":                           # |n| = 1 +- 1e-15
        n *= (1 + np.tile([1e-15, -1e-15, 2e-15, -2e-15], N // 4))[:, None]
    p = (q - t) @ R
    light = R.T @ (lc - t) if light_type == 0 else R.T @ lc
    if kind == "dir_scaled":
        light = light * 3.7
    nobs = nc + rng.normal(size=(N, 3)) * 1e-2
    Sn = np.diag([100.0, 80.0, 120.0]) + 5.0
    return (light_type, T, p, n, phong, kd, light, colour, 100.0, nobs, Sn), dict(ldn=ldn)


def _branch_counts(kind, rows):
    ldn, s, col = (np.asarray(rows[k], np.float64) for k in ("ldn", "s", "col"))
    return dict(ldn_pos=int((ldn > 0).sum()), ldn_nonpos=int((ldn <= 0).sum()), s_pos=int((s > 0).sum()),
                s_small=int(((s > 0) & (s < 1e-5)).sum()), clamp_hi=int((col >= 1).sum()), clamp_lo=int((col <= 0).sum()),
                inside_hi=int(((col < 1) & (col > 1 - 1e-12)).sum()), inside_lo=int(((col > 0) & (col < 1e-12)).sum()))


ROW_CASES = [("ldn", 0), ("ldn", 1), ("s_small", 0), ("s_small", 1), ("clamp", 0), ("clamp", 1), ("norm", 0), ("norm", 1),
             ("near_light", 0), ("dir_scaled", 1), ("generic", 0), ("generic", 1)]


@pytest.mark.parametrize("kind,light_type", ROW_CASES)
def test_phong_rows_on_the_edges_against_the_truth(kind, light_type):
    rng = np.random.default_rng(17 + 7 * ROW_CASES.index((kind, light_type)))
    args, _ = _edge_batch(kind, light_type, rng)
    rows = hp.phong_rows(*args)
    c = _branch_counts(kind, rows)
    if kind == "ldn":
        assert c["ldn_pos"] >= 20 and c["ldn_nonpos"] >= 20, c
        assert np.abs(np.asarray(rows["ldn"], np.float64)).max() < 2e-12
        # and no row's bar is a guard crossing measured by the perturbation (that would be ~1e15 |J|)
        assert rows["mag_J_int"].max() <= 1e4 * float(np.abs(np.asarray(rows["J_int"], np.float64)).max())
    if kind == "s_small":
        assert c["s_small"] >= 32 and c["s_pos"] == 64, c
    if kind == "clamp":
        assert c["clamp_hi"] >= 16 and c["clamp_lo"] >= 8 and c["inside_hi"] >= 16 and c["inside_lo"] >= 16, c
    if kind == "norm":
        nn = np.linalg.norm(args[3], axis=1)
        assert (nn > 1).sum() >= 16 and (nn < 1).sum() >= 16
    light_type, T, p, n, phong, kd, light, colour, st, nobs, Sn = args
    r_int, J_int, r_nrm, J_np, J_nn = capi.phong_evaluate(light_type, T, p, n, phong, kd, light, colour, st, nobs, Sn)
    worst = {}
    for name, dev in (("r_int", r_int), ("J_int", J_int), ("r_nrm", r_nrm), ("J_np", J_np), ("J_nn", J_nn)):
        err = np.abs(np.asarray(np.asarray(dev, hp.LD) - rows[name], np.float64))
        bar = hp.C_ROW * hp.U * rows["mag_" + name]
        worst[name] = float((err / np.maximum(bar, 1e-300)).max())
        bad = np.argwhere(err > bar)
        assert bad.size == 0, (kind, light_type, name, bad[:5].tolist(), err[tuple(bad[0])], bar[tuple(bad[0])])
    _report(f"rows {kind} light={light_type}", **worst, **c)


# ------------------------------------------------------------------------------------- (B) the lighting reduced system
_PHONG = {}


def _phong_case(which, light_type, materials):
    key = (which, light_type, materials)
    if key not in _PHONG:
        if which == "tiny":
            prob, ph = synth.make_phong_problem(8, 60, track_len=5, seed=7, light_type=light_type, num_materials=materials)
        elif which == "c1":
            prob, ph = synth.make_phong_problem(50, 2000, seed=4, light_type=light_type, num_materials=materials)
        else:           # the ragged keep[::7] problem of test_phong_ragged_tracks_and_long_window
            prob, ph = synth.make_phong_problem(30, 3000, seed=11, light_type=light_type, num_materials=materials)
        d = ph.as_oracle_dict("perturbed")
        obs = (prob.obs_pose, prob.obs_point, prob.obs_uvd)
        if which == "ragged":
            keep = np.ones(prob.num_obs, dtype=bool)
            keep[::7] = False
            d["intensity"], d["normal_obs"] = d["intensity"][keep], d["normal_obs"][keep]
            obs = tuple(a[keep] for a in obs)
        rows = {}
        _PHONG[key] = (prob, d, obs, rows)
    return _PHONG[key]


PHONG_CASES = ([("tiny", lt, 4, sf, r, 0.0) for lt in (0, 1) for sf in (0, 1, 4, 6, 7) for r in (1e4, 3.0)]
               + [("tiny", 0, 7, 7, 1e4, 0.0), ("tiny", 1, 4, 7, 1e4, 1.345), ("tiny", 0, 4, 0, 3.0, 1.345)]
               + [("c1", lt, 4, sf, 1e4, 0.0) for lt in (0, 1) for sf in (0, 7)]
               + [("c1", 0, 4, 7, 3.0, 0.0), ("c1", 1, 4, 7, 1e4, 1.345), ("ragged", 0, 4, 7, 3.0, 0.0)])


@pytest.mark.parametrize("which,light_type,materials,shared_free,radius,huber", PHONG_CASES)
def test_phong_assembly_border_and_step_against_the_truth(which, light_type, materials, shared_free, radius, huber):
    prob, d, (op, oj, ouvd), cache = _phong_case(which, light_type, materials)
    ba = StereoBA(prob.camera, prob.poses_init.copy(), prob.points_init.copy(), op, oj, ouvd, prob.stiffness(), lighting=d,
                  shared_free=shared_free, huber_a=huber)
    st = ba.stats()
    blocks = {"tiny": 1, "c1": 5, "ragged": 3}[which]
    assert st.general_structure == 0 and st.num_superblocks == blocks, (st.general_structure, st.num_superblocks)
    S, rhs, dp, dl, mcc = ba.lm_step(radius)
    S_pb, S_bb, rhs_b, db = ba.border_system()
    M = len(d["texture"])
    nb = (3 if shared_free & 1 else 0) + (3 * M if shared_free & 2 else 0) + (M if shared_free & 4 else 0)
    assert S_pb.shape[1] == nb
    if (shared_free, huber) not in cache:
        cache[(shared_free, huber)] = hp.phong_observation_rows(prob.camera, prob.poses_init, prob.points_init, d["normals"], op, oj,
                                                                ouvd, prob.stiffness(), d, huber, shared_free,
                                                                phong=cache.get("phong"))
        cache["phong"] = cache[(shared_free, huber)]["phong"]
    rows = cache[(shared_free, huber)]
    fidx = hp.free_index(prob.num_poses, op, np.eye(1, prob.num_poses, 0, dtype=bool)[0])
    sy = hp.SchurSystem(rows, op, oj, fidx, prob.num_points, radius)
    assert sy.nb == nb
    tag = f"phong {which} light={light_type} M={materials} sf={shared_free} r={radius} h={huber}"
    ex_S, ex_rhs = sy.assembly_excess(S, rhs)
    kv = dict(S_over_E=ex_S, rhs_over_E=ex_rhs, max_kappa_V=float(sy.kappa_V.max()))
    if nb:
        kv.update(zip(("S_pb_over_E", "S_bb_over_E", "rhs_b_over_E"), sy.border_excess(S_pb, S_bb, rhs_b)))
    _report(tag + " assembly", **kv)
    assert max(v for k, v in kv.items() if k.endswith("_E")) <= 1.0, (tag, kv)
    _check_back_substitution(tag, sy, dp, dl, mcc, fidx, prob.points_init, db if nb else None)
    if nb:
        A = np.block([[S, S_pb], [S_pb.T, S_bb]])
        _check_solve(tag + " bordered solve", A, np.concatenate([rhs, rhs_b]), np.concatenate([dp[fidx >= 0].ravel(), db]))
    else:
        _check_solve(tag + " solve", S, rhs, dp[fidx >= 0].ravel())


# ----------------------------------------------------------------------------------------------------- (E) closure border
_CLOSURE = {}


def _closure_problem(size):
    if size not in _CLOSURE:
        prob = synth.make_problem(size[0], size[1], track_len=size[2], seed=5, pose_sigma=(0.004, 0.001))
        _CLOSURE[size] = synth.add_loop_closure(prob, num_states=3, num_landmarks=80, max_track=12)
    return _CLOSURE[size]


@pytest.mark.parametrize("radius,huber", [(1e4, 0.0), (3.0, 0.0), (1e4, 1.345), (3.0, 1.345)])
@pytest.mark.parametrize("size,pcr_max", [((100, 3000, 8), None), ((100, 3000, 8), "4"), ((300, 6000, 9), None)])
def test_closure_border_step_against_the_truth(monkeypatch, size, pcr_max, radius, huber):
    """The chains of test_closure_border_chain_lengths (9 and 25 super-blocks; plain levels under a PCR top of 4).  The
    propagated bound is asserted but, at radius 1e4, kappa(V_j) E makes it exceed |x*| by 1e5 and it decides nothing; what
    decides is the solve bar |delta_p - x*|_inf <= 4096 u kappa_2 |x*|_inf (1e-6 |x*| at kappa_2 = 2e6), which a zero, a
    sign-flipped or a mis-ordered delta_p exceeds by orders of magnitude."""
    if pcr_max:
        monkeypatch.setenv("SSBA_PCR_MAX_BLOCKS", pcr_max)
    q = _closure_problem(size)
    ba = StereoBA.from_synth(q, huber_a=huber)
    st = ba.stats()
    assert st.general_structure == 2 and st.num_superblocks == {100: 9, 300: 25}[size[0]], (st.general_structure, st.num_superblocks)
    # the border columns follow a parallel plan only when it is parallel from level 0 (ssba_api.hip, the PCR plan): with
    # SSBA_PCR_MAX_BLOCKS=4 below the chain's 9 blocks the closure handle takes plain cyclic-reduction levels throughout
    assert st.pcr_blocks == (0 if pcr_max else st.num_superblocks), (pcr_max, st.pcr_blocks)
    _, _, dp, dl, mcc = ba.lm_step(radius)
    sy, fidx = _reference(q, radius, huber)
    S = sy.dense()
    x_ref, kap = hp.refined_solve(S, sy.rhs)
    x_ref = np.asarray(x_ref, np.float64)
    Si = np.abs(np.linalg.inv(np.asarray(S, np.float64)))
    bound = float((Si @ (sy.dense_bound() @ np.abs(x_ref) + sy.E_rhs)).max()) + hp.SOLVE_C * hp.U * kap * np.abs(x_ref).max()
    err = float(np.abs(dp[fidx >= 0].ravel() - x_ref).max())
    tag = f"closure P={size[0]} pcr_max={pcr_max} r={radius} h={huber}"
    solve_bar = hp.SOLVE_C * hp.U * kap * float(np.abs(x_ref).max())
    _report(tag + " delta_p", err=err, x_max=float(np.abs(x_ref).max()), kappa=kap, dp_over_solve_bar=err / solve_bar,
            dp_over_bound=err / bound)
    assert err <= bound, (tag, err, bound)
    assert err <= solve_bar, (tag, err, solve_bar)
    _check_back_substitution(tag, sy, dp, dl, mcc, fidx, q.points_init)
