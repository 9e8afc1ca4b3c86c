"""One dogleg step of the device (ssba_dogleg_step: the kernels of a solve iteration, in its order) against the long-double
dogleg of tests/hp_reference.py, which is written as Ceres writes it -- Jacobi-scaled coordinates, every J x formed row by row,
the subspace boundary minimum from a theta grid and Newton instead of the quartic.  For every case:

* v (entrywise, hp_reference.DoglegReference.v_bar), delta_gn (poses: the fp64 solve bar min(4096 u kappa_2, 1e-8) against the
  refined solve; landmarks: the long-double back-substitution of the device's own pose and border step, as the LM test);
* the six sums against the long-double sums of the device's own vectors, within their derived bars (row_sums / param_sums);
* alpha, beta, gamma, |delta|_D and the model cost change recomputed from those sums (the subspace minimum by
  hp_reference.boundary_minimum), with the sums' bars propagated by central differences, and the same branch;
* dl_mcc against the true -delta.g - |J delta|^2 / 2 of delta = beta gn + gamma v, row by row;
* SUBSPACE: the exported basis and model (sub_e, sub_g, sub_B) against the reference's from the same sums, and the boundary
  minimiser y where the model separates it from the other local minimum on the circle by more than the bar.

Radii are chosen from the reference's own norms and asserted to lie away from every branch boundary (radius / |gn| and
radius / (alpha |gradient_|) outside [0.9, 1.1]).  SUBSPACE_DOGLEG's one-dimensional case (gradient_ and the Gauss-Newton step
collinear to 2 eps) is not reached here: it needs J_s^T J_s + mu D^2 to map gradient_ onto itself, which no bundle-adjustment
problem these builders make does (a diagonal J with equal scaled entries would -- not a problem the API can express with
poses and landmarks); tests/test_hp_reference.py pins the reference's one_dim branch in closed form.

Every case asserts through ssba_stats that the intended layout ran.  Run with -s to see the ratios (lines DLREF)."""
import numpy as np
import pytest

import hp_reference as hp
from ceres_slam_amd import capi, synth
from ceres_slam_amd.solver import StereoBA

pytestmark = pytest.mark.gpu

U = hp.U
LD = hp.LD
NAMES = ("grad2", "gn2", "g_gn", "jv2", "jg2", "jvg")


def _report(tag, **kv):
    print("DLREF", tag, " ".join(f"{k}={v:.3g}" if isinstance(v, float) else f"{k}={v}" for k, v in kv.items()))


def _pack(ref, fidx, p6, l, b):
    return ref.pack(np.asarray(p6)[fidx >= 0], np.asarray(l)[ref.sy.lm], b)


def _radius(ref, gn, dogleg_type, branch):
    """A radius well inside the intended branch, from the reference's own norms."""
    (A, Bn, _), _ = ref.param_sums(ref.v, gn)
    jv2 = ref.row_sums(ref.v, ref.v)[0]
    gnorm, gn_norm = float(np.sqrt(A)), float(np.sqrt(Bn))
    cauchy = float(A / jv2) * gnorm
    if branch == "gn":
        return 2.0 * gn_norm
    if branch == "cauchy":
        return 0.5 * cauchy
    assert cauchy < 0.9 * gn_norm, (cauchy, gn_norm)       # the dogleg / boundary branch exists
    return float(np.sqrt(cauchy * gn_norm))


def dogleg_case(tag, ba, ref, fidx, mu, dogleg_type, branch, points_init, rhs_rounding=None, band=None):
    gn_ref, kap = ref.gauss_newton(band)
    radius = _radius(ref, gn_ref, dogleg_type, branch)
    o = capi.default_options(trust_region_strategy_type=1, dogleg_type=dogleg_type)
    st = ba.dogleg_step(radius, mu, o)
    gn = _pack(ref, fidx, st.gn_p, st.gn_l, st.gn_b)
    v = _pack(ref, fidx, st.v_p, st.v_l, st.v_b)
    out = {}
    # v, entrywise
    vb = ref.v_bar()
    out["v"] = float((np.abs(np.asarray(np.asarray(v, LD) - ref.v, np.float64)) / np.maximum(vb, 1e-300)).max())
    # delta_gn: poses (and border) against the refined solve, landmarks against the back-substitution of the device's own step
    n = ref.o_l
    xp_ref = np.concatenate([gn_ref[:n], gn_ref[ref.o_b:]])
    xp_dev = np.concatenate([gn[:n], gn[ref.o_b:]])
    fe = hp.forward_error(xp_dev, xp_ref)
    if kap > 0:
        fe_bar = hp.solve_bars(kap)[1]
        if rhs_rounding is not None:
            fe_bar += rhs_rounding(xp_ref)
        out["gn_p"] = fe / fe_bar
    else:
        # fp64 eigvalsh finds a non-positive eigenvalue: kappa_2 is beyond 1 / u (the bordered lighting system at mu = 1e-8,
        # whose unit-vector blocks have rank 2 and only the damping mu D^2 in the third direction) and no forward-error bar
        # exists; a backward-stable solve still has eta <= 4096 u against the long-double system
        A, b = ref.sy.bordered() if ref.nb else (ref.sy.dense() + ref.unary_offdiag, ref.sy.rhs)
        if ref.nb:
            A[: ref.sy.n, : ref.sy.n] += ref.unary_offdiag
        out["gn_p_eta"] = hp.backward_error(A, b, xp_dev) / hp.solve_bars(1.0)[0]
        _report(tag + " singular", fe=fe)
    dpf, dlp, dbb = ref.split(gn)
    dl_ref = ref.sy.back_substitute(dpf.ravel(), dbb if ref.nb else None)
    out["gn_l"] = _back_substitution_ratio(ref, dpf, dbb, dlp, dl_ref, points_init)
    # the six sums of the device's vectors
    (a, b, c), (ea, eb, ec) = ref.param_sums(v, gn)
    jv2, e3 = ref.row_sums(v, v)
    jg2, e4 = ref.row_sums(gn, gn)
    jvg, e5 = ref.row_sums(v, gn)
    sums, bars = [a, b, c, jv2, jg2, jvg], [ea, eb, ec, e3, e4, e5]
    for i, nm in enumerate(NAMES):
        out[nm] = float(abs(LD(st.sums[i]) - sums[i])) / bars[i]
    # the scalar chain from those sums
    sc = hp.dogleg_scalars(sums, radius, dogleg_type)
    truth = hp.dogleg_scalars(list(ref.param_sums(ref.v, gn_ref)[0]) + [ref.row_sums(x, y)[0] for x, y in
                                                                    ((ref.v, ref.v), (gn_ref, gn_ref), (ref.v, gn_ref))],
                              radius, dogleg_type)
    assert sc["branch"] == truth["branch"] == branch or (branch == "dogleg" and dogleg_type == 1 and truth["branch"] == "boundary"), \
        (tag, sc["branch"], truth["branch"], branch)
    (tA2, tB2, _), _ = ref.param_sums(ref.v, gn_ref)
    edges = (float(truth["alpha"] * np.sqrt(tA2)), float(np.sqrt(tB2)))     # |alpha gradient_|, |gn|: where the branch changes
    for edge in edges:
        assert not 0.9 <= radius / edge <= 1.1, (tag, radius, edges)
    keys = ("alpha", "beta", "gamma", "step_norm", "mcc")
    prop = hp.propagate(lambda s: {k: hp.dogleg_scalars(s, radius, dogleg_type)[k] for k in keys}, sums, bars)
    dev = dict(alpha=st.alpha, beta=st.beta, gamma=st.gamma, step_norm=st.step_norm, mcc=st.mcc)
    for k in keys:
        bar = prop[k] + 16 * U * abs(float(sc[k]))
        err = abs(float(LD(dev[k]) - sc[k]))
        out[k] = err / bar if bar > 0 else (0.0 if err == 0 else np.inf)
    if dogleg_type == 1:
        out.update(_subspace_ratios(st, sc, sums, bars, radius))
    # device branch
    if branch == "gn":
        assert st.beta == 1.0 and st.gamma == 0.0, tag
    elif branch == "cauchy":
        assert st.beta == 0.0 and st.gamma < 0.0, tag
    else:
        assert 0.0 < st.beta < 1.0 or dogleg_type == 1, (tag, st.beta)
        assert abs(st.step_norm - radius) <= 1e-12 * radius, tag
    # mcc against the true model cost change of the step actually taken
    delta = LD(st.beta) * np.asarray(gn, LD) + LD(st.gamma) * np.asarray(v, LD)
    mref, mag = ref.model_cost_change(delta)
    mbar = (ref.c_sum() + 2 * hp.C_DL_ROW) * U * mag + prop["mcc"]
    out["mcc_true"] = float(abs(LD(st.mcc) - mref)) / mbar
    assert np.sign(st.mcc) == np.sign(float(mref)), (tag, st.mcc, float(mref))
    _report(tag, radius=radius, branch=sc["branch"], kappa=kap, **out)
    for k, r in out.items():
        assert r <= 1.0, (tag, k, r, out)
    return st, out, radius


SUB_KEYS = ("e00", "e01", "e10", "e11", "g0", "g1", "B00", "B01", "B11")


def _sub_flat(sc):
    e, g, B = sc["sub_e"], sc["sub_g"], sc["sub_B"]
    return dict(e00=e[0, 0], e01=e[0, 1], e10=e[1, 0], e11=e[1, 1], g0=g[0], g1=g[1], B00=B[0, 0], B01=B[0, 1], B11=B[1, 1])


def _subspace_ratios(st, sc, sums, bars, radius):
    """The exported subspace basis and model against the reference's from the same sums (bars: the sums' bars propagated plus
    16 u of the value), and the boundary minimiser y: its model value through mcc (above), y itself where the model's other
    local minimum on the circle lies more than twice the model bar above the global one -- there |theta_dev - theta*| <=
    sqrt(2 bar / f''(theta*))."""
    out = {}
    ref_flat = _sub_flat(sc)
    prop = hp.propagate(lambda s: _sub_flat(hp.dogleg_scalars(s, radius, 1)), sums, bars)
    dev = dict(zip(SUB_KEYS, [*st.sub_e.ravel(), *st.sub_g, st.sub_B[0], st.sub_B[1], st.sub_B[2]]))
    # rounding of the device's own evaluation, 16 u of the magnitude of its terms: g_i = e_i0 |gradient_|^2 + e_i1 gradient_.gn
    # (g_1 is zero in exact arithmetic, so a bar relative to the value would be none), B_ij = sum e e jj over the three sums
    e = np.abs(np.asarray(sc["sub_e"], np.float64))
    A, Bn, C, Jv2, Jg2, Jvg = (abs(float(x)) for x in sums)
    mag = dict(e00=e[0, 0], e01=e[0, 1], e10=e[1, 0], e11=e[1, 1], g0=e[0, 0] * A + e[0, 1] * C, g1=e[1, 0] * A + e[1, 1] * C)
    for k, (i, j) in (("B00", (0, 0)), ("B01", (0, 1)), ("B11", (1, 1))):
        mag[k] = e[i, 0] * e[j, 0] * Jv2 + (e[i, 0] * e[j, 1] + e[i, 1] * e[j, 0]) * Jvg + e[i, 1] * e[j, 1] * Jg2
    out["sub_model"] = max(float(abs(LD(dev[k]) - ref_flat[k])) / (prop[k] + 16 * U * mag[k] + 1e-300) for k in SUB_KEYS)
    if sc["branch"] != "boundary":
        return out
    g, B, r = (np.asarray(x, np.float64) for x in (sc["sub_g"], sc["sub_B"], radius))
    f = lambda t: r * (g[0] * np.cos(t) + g[1] * np.sin(t)) + 0.5 * r * r * (
        B[0, 0] * np.cos(t) ** 2 + 2 * B[0, 1] * np.cos(t) * np.sin(t) + B[1, 1] * np.sin(t) ** 2)
    th = np.linspace(0, 2 * np.pi, 8192, endpoint=False)
    fv = f(th)
    loc = np.flatnonzero((fv < np.roll(fv, 1)) & (fv <= np.roll(fv, -1)))
    vals = np.sort(fv[loc])
    fbar = float(hp.propagate(lambda s: {"mcc": hp.dogleg_scalars(s, radius, 1)["mcc"]}, sums, bars)["mcc"]) + 16 * U * abs(vals[0])
    if vals.size > 1 and vals[1] - vals[0] <= 2 * fbar:
        return out          # two minima within the bar: the model does not determine y to better than the bar
    y_ref = np.asarray(sc["y"], np.float64)
    e = np.asarray(sc["sub_e"], np.float64)
    A, Bn, C = (float(x) for x in sums[:3])
    dD = np.array([st.gamma * A + st.beta * C, st.gamma * C + st.beta * Bn])       # gradient_ . delta_D, gn . delta_D
    y_dev = e @ dD
    t_ref, t_dev = np.arctan2(y_ref[1], y_ref[0]), np.arctan2(y_dev[1], y_dev[0])
    t = float(t_ref)
    f2 = -r * (g[0] * np.cos(t) + g[1] * np.sin(t)) + r * r * ((B[1, 1] - B[0, 0]) * np.cos(2 * t) - 2 * B[0, 1] * np.sin(2 * t))
    dth = abs((t_dev - t_ref + np.pi) % (2 * np.pi) - np.pi)
    out["y"] = dth / (np.sqrt(2 * fbar / f2) + 16 * U)
    return out


def _back_substitution_ratio(ref, dpf, dbb, dlp, dl_ref, points_init):
    """delta_l within (t_j + c) u kappa(V_j) |V^-1| (|J_l|^T |r| + |J_l|^T |J_p| |delta_p| + |J_l|^T |J_b| |delta_b|) (the LM
    test's bar: k_dogleg_gn forms tt = g_l + sum J_l^T J_p delta_p from re-linearised rows)."""
    sy = ref.sy
    rows, fr, so = sy.rows, sy._f >= 0, sy.slot_of_obs
    gla = np.zeros((sy.lm.shape[0], sy.d))
    np.add.at(gla, so, np.einsum("nai,na->ni", rows["Jla"], rows["rabs"]))
    x = np.abs(np.asarray(dpf, np.float64))
    jdp = np.einsum("naj,nj->na", rows["Jpa"][fr], x[sy._f[fr]])
    np.add.at(gla, so[fr], np.einsum("nai,na->ni", rows["Jla"][fr], jdp))
    if sy.nb:
        np.add.at(gla, so, np.einsum("nai,na->ni", rows["Jla"], np.einsum("nab,b->na", rows["Jba"], np.abs(np.asarray(dbb, np.float64)))))
    mag = np.einsum("nij,nj->ni", np.abs(np.asarray(sy.Vinv, np.float64)), gla).max(1)
    t = np.bincount(so, minlength=sy.lm.shape[0])
    bound = (t + hp.C_TERMS) * U * sy.kappa_V * mag + 2 * U * np.abs(np.asarray(dl_ref, np.float64)).max(1)
    err = np.abs(np.asarray(np.asarray(dlp, LD) - dl_ref, np.float64)).max(1)
    return float((err / bound).max())


def _stereo(prob, pose_const=None, huber=0.0, factors=None, mu=1e-8):
    const = np.zeros(prob.num_poses, bool) if pose_const is None else np.asarray(pose_const, bool)
    if pose_const is None and factors is None:
        const[0] = True
    ba = StereoBA(prob.camera, prob.poses_init.copy(), prob.points_init.copy(), prob.obs_pose, prob.obs_point, prob.obs_uvd,
                  prob.stiffness(), pose_const=const, huber_a=huber, pose_factors=factors)
    rows = hp.stereo_rows(prob.camera, prob.poses_init, prob.points_init, prob.obs_pose, prob.obs_point, prob.obs_uvd,
                          prob.stiffness(), huber)
    fidx = hp.free_index(prob.num_poses, prob.obs_pose, const)
    un = hp.unary_rows(prob.poses_init, factors) if factors else None
    ref = hp.DoglegReference(rows, prob.obs_pose, prob.obs_point, fidx, prob.num_points, mu, unary=un)
    return ba, ref, fidx


BRANCHES = [(0, "gn"), (0, "cauchy"), (0, "dogleg"), (1, "gn"), (1, "dogleg")]


# -------------------------------------------------------------------------------------------- windowed layout, k_dogleg_gn<false>
@pytest.mark.parametrize("mu,dogleg_type,branch", [(m, t, b) for m in (1e-8, 1e-3) for t, b in BRANCHES]
                         + [(1.0, 0, "gn"), (1.0, 0, "cauchy"), (1.0, 1, "gn")])
@pytest.mark.parametrize("huber", [0.0, 1.345])
def test_windowed_tiny(huber, mu, dogleg_type, branch):
    """(At mu = 1 the damped Gauss-Newton step is shorter than the Cauchy step of this problem: no dogleg branch exists.)"""
    prob = synth.make_problem(8, 60, track_len=5, seed=7, outlier_fraction=0.1 if huber else 0.0)
    ba, ref, fidx = _stereo(prob, huber=huber, mu=mu)
    assert ba.stats().general_structure == 0
    dogleg_case(f"tiny h={huber} mu={mu} {dogleg_type}/{branch}", ba, ref, fidx, mu, dogleg_type, branch, prob.points_init)


@pytest.mark.parametrize("dogleg_type,branch", BRANCHES)
def test_windowed_c1(dogleg_type, branch):
    prob = synth.make_config("C1")
    ba, ref, fidx = _stereo(prob)
    assert ba.stats().general_structure == 0
    dogleg_case(f"c1 {dogleg_type}/{branch}", ba, ref, fidx, 1e-8, dogleg_type, branch, prob.points_init)


@pytest.mark.parametrize("L", [63, 64, 65])
def test_landmark_group_edges(L):
    prob = synth.make_problem(8, L, track_len=5, seed=L)
    ba, ref, fidx = _stereo(prob)
    assert ba.stats().general_structure == 0 and ba.stats().num_superblocks == 1
    dogleg_case(f"lmg L={L}", ba, ref, fidx, 1e-8, 0, "dogleg", prob.points_init)


def test_constant_poses_inside_the_chain():
    prob = synth.make_problem(40, 1600, track_len=12, seed=8)
    const = np.zeros(40, bool)
    const[[0, 12, 13, 25]] = True
    ba, ref, fidx = _stereo(prob, pose_const=const, huber=1.345, mu=1e-3)
    st = ba.stats()
    assert st.general_structure == 0 and st.num_free_poses == 36
    for t, b in ((0, "dogleg"), (1, "dogleg")):
        dogleg_case(f"const_gaps {t}/{b}", ba, ref, fidx, 1e-3, t, b, prob.points_init)


# ---------------------------------------------------------------------------------------------- general layout, k_dogleg_gn<true>
@pytest.mark.parametrize("size,wide", [((30, 900, 16), 2), ((30, 900, 24), 2)])
def test_wide_superblocks(size, wide):
    prob = synth.make_problem(size[0], size[1], track_len=size[2], seed=3)
    ba, ref, fidx = _stereo(prob)
    st = ba.stats()
    assert st.general_structure == 1 and st.wide_superblocks == wide
    for t, b in ((0, "dogleg"), (1, "dogleg")):
        dogleg_case(f"wide T={size[2]} {t}/{b}", ba, ref, fidx, 1e-8, t, b, prob.points_init)


def test_dense_general(monkeypatch):
    monkeypatch.setenv("SSBA_FORCE_DENSE", "1")
    prob = synth.make_problem(15, 400, track_len=8, seed=3)
    ba, ref, fidx = _stereo(prob, huber=1.345, mu=1e-3)
    st = ba.stats()
    assert st.general_structure == 1 and st.wide_superblocks == 0
    for t, b in BRANCHES:
        dogleg_case(f"dense {t}/{b}", ba, ref, fidx, 1e-3, t, b, prob.points_init)


# ----------------------------------------------------------------------------------------------------------- unary pose rows
@pytest.mark.parametrize("huber", [0.0, 0.5])
def test_sun_and_prior_rows(huber):
    from test_oracle_pose_factors import _sun_problem
    prob, factors = _sun_problem(huber=huber)
    ba, ref, fidx = _stereo(prob, factors=factors, pose_const=np.zeros(prob.num_poses, bool))
    for t, b in BRANCHES:
        dogleg_case(f"sun_prior h={huber} {t}/{b}", ba, ref, fidx, 1e-8, t, b, prob.points_init)


@pytest.mark.parametrize("huber", [0.0, 0.05])
def test_relative_pose_rows_with_a_loop(huber):
    """Odometry and a loop closure between the first and last state, both halves free: the relative-pose cross term of
    k_dogleg_vec, on the general layout."""
    from test_oracle_pose_factors import _odometry_factors
    prob = synth.make_problem(7, 100, track_len=4, seed=6)
    factors = _odometry_factors(prob, huber=huber)
    ba, ref, fidx = _stereo(prob, factors=factors, pose_const=np.zeros(prob.num_poses, bool))
    assert ba.stats().general_structure == 1
    for t, b in BRANCHES:
        dogleg_case(f"odometry h={huber} {t}/{b}", ba, ref, fidx, 1e-8, t, b, prob.points_init)


def test_relative_pose_next_to_a_constant_pose():
    from test_oracle_pose_factors import _odometry_factors
    prob = synth.make_problem(7, 100, track_len=4, seed=6)
    factors = [f for f in _odometry_factors(prob) if f["type"] == 2]
    const = np.zeros(prob.num_poses, bool)
    const[3] = True
    ba, ref, fidx = _stereo(prob, factors=factors, pose_const=const)
    assert ba.stats().general_structure == 1
    dogleg_case("odometry const=3", ba, ref, fidx, 1e-8, 0, "dogleg", prob.points_init)


# ---------------------------------------------------------------------------------------------------------- lighting terms
@pytest.mark.parametrize("light_type,shared_free", [(0, 0), (1, 0), (0, 7), (1, 7)])
def test_lighting_terms(light_type, shared_free):
    from test_gpu_hp_phong import _phong_case
    prob, d, (op, oj, ouvd), _ = _phong_case("tiny", light_type, 4)
    ba = StereoBA(prob.camera, prob.poses_init.copy(), prob.points_init.copy(), op, oj, ouvd, prob.stiffness(), lighting=d,
                  shared_free=shared_free)
    assert ba.stats().general_structure == 0
    rows = hp.phong_observation_rows(prob.camera, prob.poses_init, prob.points_init, d["normals"], op, oj, ouvd, prob.stiffness(),
                                     d, 0.0, shared_free)
    const = np.zeros(prob.num_poses, bool)
    const[0] = True
    fidx = hp.free_index(prob.num_poses, op, const)
    for mu in (1e-8, 1e-3):
        ref = hp.DoglegReference(rows, op, oj, fidx, prob.num_points, mu)
        assert ref.nb == (0 if shared_free == 0 else 3 + 4 * 4)
        for t, b in BRANCHES:
            dogleg_case(f"phong lt={light_type} sf={shared_free} mu={mu} {t}/{b}", ba, ref, fidx, mu, t, b, prob.points_init)


# ------------------------------------------------------------------------------------------------------------ clamp, far landmark
def test_far_landmark_hits_the_diagonal_clamp():
    """A landmark pushed far out along its ray: its depth column of J^T J falls under min_lm_diagonal after scaling."""
    prob = synth.make_problem(8, 60, track_len=5, seed=7)
    pts = prob.points_init.copy()
    T0 = prob.poses_init[prob.obs_pose[prob.obs_point == 5][0]]
    c = -T0[3:].reshape(3, 3).T @ T0[:3]
    pts[5] = c + (pts[5] - c) * 1e5
    prob.points_init = pts
    ba, ref, fidx = _stereo(prob)
    assert np.any(ref.clamped[ref.o_l: ref.o_b]), "the clamp is not active"
    for t, b in ((0, "gn"), (0, "dogleg"), (1, "dogleg")):
        dogleg_case(f"far landmark {t}/{b}", ba, ref, fidx, 1e-8, t, b, pts)


# ------------------------------------------------------------------------------------------------------------ near convergence
def _measured_assembly_rounding(ba, ref, mu):
    """For a step whose right-hand side -g is far below the magnitude of its terms (a converged point): the first-order effect
    on the pose step of the rounding the device's assembly actually made, S_ld^-1 (drhs - dS x) / |x|, with dS, drhs the
    device's reduced system (ssba_lm_step at radius 1 / mu: the same kernels and damping values as the dogleg's Gauss-Newton
    solve) minus the long-double one -- after asserting that the device's system is within its entrywise bound E.  The
    second-order remainder is covered by the factor (1 + e) / (1 - e), e = kappa_2 |dS|_2 / |S|_2."""
    S_dev, rhs_dev, _, _, _ = ba.lm_step(1.0 / mu)
    ex_S, ex_rhs = ref.sy.assembly_excess(S_dev, rhs_dev)
    assert ex_S <= 1.0 and ex_rhs <= 1.0, (ex_S, ex_rhs)
    S_ld = ref.sy.dense()
    dS = np.asarray(S_dev, LD) - S_ld
    drhs = np.asarray(rhs_dev, LD) - ref.sy.rhs
    S64, dS64 = np.asarray(S_ld, np.float64), np.asarray(dS, np.float64)
    kap = float(np.linalg.cond(S64))
    e = kap * np.linalg.norm(dS64, 2) / np.linalg.norm(S64, 2)
    assert e < 0.5, e

    def term(x):
        y, _ = hp.refined_solve(S_ld, drhs - dS @ np.asarray(x, LD))
        return float(np.sqrt((np.asarray(y, np.float64) ** 2).sum() / (np.asarray(x, np.float64) ** 2).sum())) * (1 + e) / (1 - e)
    return term, ex_S, ex_rhs


def test_near_convergence():
    """LM run to convergence on the device, then one dogleg step from there: mcc is a tiny fraction of the cost.  The pose
    Gauss-Newton step here is held to the solve bar plus the effect of the device's measured assembly rounding: rhs = -g has
    cancelled to ~1e-13 of its terms, so even the correctly rounded right-hand side moves the step by more than 4096 u kappa_2
    (12.6x that bar alone on this point)."""
    prob = synth.make_problem(8, 60, track_len=5, seed=7)
    const = np.zeros(prob.num_poses, bool)
    const[0] = True
    ba = StereoBA(prob.camera, prob.poses_init.copy(), prob.points_init.copy(), prob.obs_pose, prob.obs_point, prob.obs_uvd,
                  prob.stiffness(), pose_const=const)
    ba.solve(capi.default_options(max_num_iterations=200, function_tolerance=1e-14, parameter_tolerance=1e-14))
    rows = hp.stereo_rows(prob.camera, ba.poses, ba.points, prob.obs_pose, prob.obs_point, prob.obs_uvd, prob.stiffness())
    fidx = hp.free_index(prob.num_poses, prob.obs_pose, const)
    ref = hp.DoglegReference(rows, prob.obs_pose, prob.obs_point, fidx, prob.num_points, 1e-8)
    term, ex_S, ex_rhs = _measured_assembly_rounding(ba, ref, 1e-8)
    cost = float(rows["cost"])
    gn_ref, kap = ref.gauss_newton()
    _report("converged assembly", S_over_E=ex_S, rhs_over_E=ex_rhs, measured_term=term(gn_ref[: ref.o_l]),
            solve_bar=hp.solve_bars(kap)[1])
    for t, b in ((0, "gn"), (0, "dogleg"), (1, "dogleg")):
        st, out, _ = dogleg_case(f"converged {t}/{b}", ba, ref, fidx, 1e-8, t, b, ba.points, rhs_rounding=term)
        _report(f"converged {t}/{b}", cost=cost, mcc=st.mcc, mcc_over_cost=st.mcc / cost)


# ------------------------------------------------------------------------------------------------------------------- scale
def test_c2_traditional_step():
    """One C2 step at mu = 1e-8, TRADITIONAL on the dogleg: the six sums and mcc against the row-by-row long-double pass
    (1.2 million rows), delta_gn against the banded refined solve of the long-double system."""
    prob = synth.make_config("C2")
    ba, ref, fidx = _stereo(prob)
    st = ba.stats()
    assert st.general_structure == 0 and st.num_superblocks == 84
    band = hp.bandwidth(np.asarray(ref.sy.dense(), np.float64))
    assert band < 2 * 72
    dogleg_case("c2 0/dogleg", ba, ref, fidx, 1e-8, 0, "dogleg", prob.points_init, band=band)


# ------------------------------------------------------------------------------------------------------------ hook against solve
@pytest.mark.parametrize("which", ["tiny", "c1", "phong"])
@pytest.mark.parametrize("dogleg_type", [0, 1])
def test_hook_matches_the_first_solve_iteration(which, dogleg_type):
    """The hook's dl_mcc at (r, mu = 1e-8) is the model cost change of the first iteration of a solve begun at radius r
    (cost_change / relative_decrease of its log, 4 ulps), and an accepted step writes back Plus(x, beta gn + gamma v)."""
    import np_reference as npr
    if which == "phong":
        from test_gpu_hp_phong import _phong_case
        prob, d, (op, oj, ouvd), _ = _phong_case("tiny", 0, 4)
        mk = lambda: StereoBA(prob.camera, prob.poses_init.copy(), prob.points_init.copy(), op, oj, ouvd, prob.stiffness(),
                              lighting=d, shared_free=7)
    else:
        prob = synth.make_problem(8, 60, track_len=5, seed=7) if which == "tiny" else synth.make_config("C1")
        mk = lambda: StereoBA.from_synth(prob)
    ba = mk()
    o = capi.default_options(trust_region_strategy_type=1, dogleg_type=dogleg_type)
    st = ba.dogleg_step(1e4, 1e-8, o)
    r = 0.5 * st.step_norm if st.beta == 1.0 else 1e4       # a radius on the boundary branch when the first step is GN
    st = ba.dogleg_step(r, 1e-8, o)
    ba2 = mk()
    ba2.solve_begin(capi.default_options(trust_region_strategy_type=1, dogleg_type=dogleg_type, initial_trust_region_radius=r,
                                         max_num_iterations=1))
    ba2.step(2)         # (an accepted step is logged by the check of the next iteration, which then stops: max_num_iterations = 1)
    ba2.solve_end()
    log = ba2.iteration_log()
    mcc_solve = log["cost_change"][1] / log["relative_decrease"][1]
    _report(f"hook-vs-solve {which} {dogleg_type}", mcc_hook=st.mcc, mcc_solve=mcc_solve, accepted=int(log["step_is_successful"][1]))
    assert abs(mcc_solve - st.mcc) <= 4 * np.spacing(abs(st.mcc)), \
        (mcc_solve, st.mcc)
    if log["step_is_successful"][1]:
        free = np.zeros(prob.num_poses, bool)
        free[np.unique(prob.obs_pose if which != "phong" else op)] = True
        free[0] = False
        for k in np.flatnonzero(free):
            Tk = npr.se3_plus(prob.poses_init[k], st.beta * st.gn_p[k] + st.gamma * st.v_p[k])
            assert np.allclose(ba2.poses[k], Tk, rtol=0, atol=64 * U * (1 + np.abs(Tk).max())), (k, ba2.poses[k] - Tk)
