"""Borders of free shared lighting blocks wider than 32 columns: 8 to 15 materials with every kind free (nb = 3 + 4M, up to
63 columns), kept as two panels of 32 columns (csrc/ssba_types.h: Dev::np), through the C ABI.

(1) a border of 35 columns finalizes and ssba_border_system returns every column;
(2) the bordered LM step [S S_pb; S_pb^T S_bb] against the long-double refined solve, at nb = 35, 33 (the first column of the
    second panel) and 63, and the assembly of S_pb, S_bb, rhs_b against the long-double SchurSystem;
(3) ssba_dogleg_step at M = 15 against the long-double dogleg reference;
(4)-(7) whole solves against the CPU oracle: LM and the Phong driver's configuration at C1 size, the general layout, the C++
    driver on a ten-material dataset, and the driver's configuration at full size (1 000 poses / 100 000 landmarks);
(8) what stays refused: landmark sharding with a border wider than 32 columns, and 16 materials."""
import numpy as np
import pytest

import hp_reference as hp
from ceres_slam_amd import capi, synth
from ceres_slam_amd.solver import StereoBA
from oracle import oracle as orc
from test_gpu_hp_dogleg import BRANCHES, dogleg_case
from test_gpu_hp_reference import _check_solve, _report

pytestmark = pytest.mark.gpu


def _nb(materials, shared_free):
    return (3 if shared_free & 1 else 0) + (3 * materials if shared_free & 2 else 0) + (materials if shared_free & 4 else 0)


def _oracle(prob, d, **kw):
    return orc.OracleProblem(prob.camera, prob.poses_init, prob.points_init, prob.obs_pose, prob.obs_point, prob.obs_uvd,
                             prob.stiffness(), lighting=d, **kw)


# ------------------------------------------------------------------------------------------------------------ (1) finalize
def test_border_of_35_columns_finalizes_and_returns_every_column():
    prob, ph = synth.make_phong_problem(50, 2000, num_materials=8)
    ba = StereoBA.from_synth(prob, lighting=ph.as_oracle_dict("perturbed"), shared_free=7)
    ba.lm_step(1e4)
    S_pb, S_bb, rhs_b, db = ba.border_system()
    assert S_pb.shape == (6 * (prob.num_poses - 1), 35) and S_bb.shape == (35, 35) and rhs_b.shape == db.shape == (35,)
    assert np.all(np.isfinite(S_pb)) and np.all(np.isfinite(db))
    # every column of the second panel is filled: the texture columns 27..34 see the landmarks of their material
    assert np.all(np.abs(S_pb[:, 32:]).max(axis=0) > 0) and np.all(np.diag(S_bb) > 0)


# ------------------------------------------------------------------------------------------------- (2) step and assembly
STEP_CASES = [(8, 7, 35), (11, 2, 33), (15, 7, 63)]
RADII = [(1e4, 0.0), (3.0, 0.0), (1e4, 1.345), (3.0, 1.345)]


@pytest.mark.parametrize("radius,huber", RADII)
@pytest.mark.parametrize("materials,shared_free,nb", STEP_CASES)
def test_wide_border_step_is_fp64_accurate(materials, shared_free, nb, radius, huber):
    """As test_free_shared_border_step_is_fp64_accurate (C1 size), with borders of two panels."""
    prob, ph = synth.make_phong_problem(50, 2000, num_materials=materials, seed=4)
    ba = StereoBA.from_synth(prob, lighting=ph.as_oracle_dict("truth"), shared_free=shared_free, huber_a=huber)
    assert ba.stats().general_structure == 0
    S, rhs, dp, dl, mcc = ba.lm_step(radius)
    S_pb, S_bb, rhs_b, db = ba.border_system()
    assert S_pb.shape[1] == nb == _nb(materials, shared_free)
    A = np.block([[S, S_pb], [S_pb.T, S_bb]])
    _check_solve(f"wide_border nb={nb} r={radius} h={huber}", A, np.concatenate([rhs, rhs_b]), np.concatenate([dp[1:].ravel(), db]))


_SMALL = {}


def _small_case(materials):
    """12 poses, 300 landmarks: every material has landmarks, and the long-double rows take seconds."""
    if materials not in _SMALL:
        prob, ph = synth.make_phong_problem(12, 300, track_len=6, seed=21, num_materials=materials)
        d = ph.as_oracle_dict("perturbed")
        assert len(np.unique(d["material_of_point"])) == materials
        _SMALL[materials] = (prob, d)
    return _SMALL[materials]


@pytest.mark.parametrize("radius,huber", [(1e4, 0.0), (3.0, 1.345)])
@pytest.mark.parametrize("materials,shared_free,nb", STEP_CASES)
def test_wide_border_assembly_against_the_truth(materials, shared_free, nb, radius, huber):
    """S_pb, S_bb, rhs_b within the rounding bars of the long-double SchurSystem (as
    test_phong_assembly_border_and_step_against_the_truth), and the bordered solve."""
    prob, d = _small_case(materials)
    op, oj, ouvd = prob.obs_pose, prob.obs_point, prob.obs_uvd
    ba = StereoBA(prob.camera, prob.poses_init.copy(), prob.points_init.copy(), op, oj, ouvd, prob.stiffness(), lighting=d,
                  shared_free=shared_free, huber_a=huber)
    assert ba.stats().general_structure == 0
    S, rhs, dp, dl, mcc = ba.lm_step(radius)
    S_pb, S_bb, rhs_b, db = ba.border_system()
    assert S_pb.shape[1] == nb
    rows = hp.phong_observation_rows(prob.camera, prob.poses_init, prob.points_init, d["normals"], op, oj, ouvd, prob.stiffness(),
                                     d, huber, shared_free)
    fidx = hp.free_index(prob.num_poses, op, np.eye(1, prob.num_poses, 0, dtype=bool)[0])
    sy = hp.SchurSystem(rows, op, oj, fidx, prob.num_points, radius)
    assert sy.nb == nb
    tag = f"wide_border M={materials} sf={shared_free} r={radius} h={huber}"
    kv = dict(zip(("S_pb_over_E", "S_bb_over_E", "rhs_b_over_E"), sy.border_excess(S_pb, S_bb, rhs_b)))
    _report(tag + " assembly", **kv)
    assert max(kv.values()) <= 1.0, (tag, kv)
    A = np.block([[S, S_pb], [S_pb.T, S_bb]])
    _check_solve(tag + " bordered solve", A, np.concatenate([rhs, rhs_b]), np.concatenate([dp[fidx >= 0].ravel(), db]))


# ------------------------------------------------------------------------------------------------------------ (3) dogleg
def test_dogleg_step_with_fifteen_materials():
    """ssba_dogleg_step (gn_b, v_b over all 63 columns) against hp.DoglegReference, TRADITIONAL and SUBSPACE, as
    test_lighting_terms does for four materials."""
    prob, d = _small_case(15)
    op, oj, ouvd = prob.obs_pose, prob.obs_point, prob.obs_uvd
    ba = StereoBA(prob.camera, prob.poses_init.copy(), prob.points_init.copy(), op, oj, ouvd, prob.stiffness(), lighting=d,
                  shared_free=7)
    assert ba.stats().general_structure == 0
    rows = hp.phong_observation_rows(prob.camera, prob.poses_init, prob.points_init, d["normals"], op, oj, ouvd, prob.stiffness(),
                                     d, 0.0, 7)
    const = np.zeros(prob.num_poses, bool)
    const[0] = True
    fidx = hp.free_index(prob.num_poses, op, const)
    for mu in (1e-8, 1e-3):
        ref = hp.DoglegReference(rows, op, oj, fidx, prob.num_points, mu)
        assert ref.nb == 63
        for t, b in BRANCHES:
            dogleg_case(f"wide_border M=15 mu={mu} {t}/{b}", ba, ref, fidx, mu, t, b, prob.points_init)


# ------------------------------------------------------------------------------------------------ (4) solves at C1 size
@pytest.mark.parametrize("materials", [8, 15])
def test_lm_solve_with_every_kind_free_matches_oracle(materials):
    """The bars of test_twelve_materials_with_free_light_and_textures, with the Phong parameters free as well."""
    prob, ph = synth.make_phong_problem(50, 2000, num_materials=materials, seed=5)
    d = ph.as_oracle_dict("perturbed")
    ba = StereoBA.from_synth(prob, lighting=d, shared_free=7)
    op = _oracle(prob, d, shared_free=7)
    s, log = ba.solve(capi.default_options(max_num_iterations=25, use_nonmonotonic_steps=1))
    s2, log2 = op.solve(orc.driver_options(num_threads=4, max_num_iterations=25))
    assert log["step_is_successful"].tolist() == log2["step_is_successful"].tolist()
    ok = np.asarray(log2["step_is_successful"], dtype=bool)
    ok[0] = True
    np.testing.assert_allclose(log["cost"][ok], log2["cost"][ok], rtol=1e-7)
    assert s.final_cost == pytest.approx(s2.final_cost, rel=1e-6)
    assert np.abs(ba.poses - op.poses).max() < 1e-6
    assert np.abs(ba.texture - op.texture).max() < 1e-6 and np.abs(ba.light - op.light).max() < 1e-5


@pytest.mark.parametrize("materials", [8, 15])
def test_driver_configuration_matches_oracle(materials):
    """SUBSPACE_DOGLEG, non-monotonic steps, bounds (projected Armijo line search), the reference's initial values: K = 15
    iterations step for step with the oracle (as test_bounded_solve_matches_oracle compares the first twelve), then a solve
    to convergence.  Over a whole solve of 50 - 100 iterations the two drift apart on these problems, whose bordered systems
    reach kappa ~ 1e17 (the HPREF lines above): at M = 7 on one panel, the parent's route, the same seed gives 61 / 55
    iterations with costs 1e-4 apart by iteration 40.  Measured here: M = 15 takes 32 / 32 iterations, final costs 6e-9 apart;
    M = 8 ends in different minima even between two runs of the oracle itself with four threads (1.01483e5 after 83
    iterations, 9.99336e4 after 103; the device: 1.01483e5 after 103), so there the whole solve is held to 2e-2, the
    oracle's own spread, and its iteration count is asserted at M = 15 only.  The cost bar of the first 15 iterations is 1e-5: at M = 8 the two part at 5e-6 there
    (M = 4: 1e-6)."""
    prob, ph = synth.make_phong_problem(50, 2000, num_materials=materials, seed=6)
    d = ph.as_oracle_dict("reference")
    kw = dict(use_nonmonotonic_steps=1, trust_region_strategy_type=1, dogleg_type=1)
    ba = StereoBA.from_synth(prob, lighting=d, shared_free=7, use_bounds=True)
    op = _oracle(prob, d, shared_free=7, use_bounds=True)
    s, log = ba.solve(capi.default_options(max_num_iterations=15, **kw))
    s2, log2 = op.solve(orc.driver_options(num_threads=4, max_num_iterations=15, **kw))
    assert s.num_iterations == s2.num_iterations
    assert s.num_line_search_steps == s2.num_line_search_steps
    assert log["step_is_successful"].tolist() == log2["step_is_successful"].tolist()
    ok = np.asarray(log2["step_is_successful"], dtype=bool)
    ok[0] = True
    np.testing.assert_allclose(log["cost"][ok], log2["cost"][ok], rtol=1e-5)
    ba = StereoBA.from_synth(prob, lighting=d, shared_free=7, use_bounds=True)
    op = _oracle(prob, d, shared_free=7, use_bounds=True)
    s, log = ba.solve(capi.default_options(max_num_iterations=1000, **kw))
    s2, log2 = op.solve(orc.driver_options(num_threads=4, max_num_iterations=1000, **kw))
    print(f"wide_border driver M={materials}: {s.num_iterations} / {s2.num_iterations} iterations, final cost {s.final_cost:.12e} / "
          f"{s2.final_cost:.12e}")
    assert s.termination_type == s2.termination_type == 0
    if materials == 15:
        assert s.num_iterations == s2.num_iterations
        assert s.final_cost == pytest.approx(s2.final_cost, rel=1e-6)
    else:
        assert s.final_cost == pytest.approx(s2.final_cost, rel=2e-2)
    assert np.all(ba.phong[:, :2] >= 0) and np.all(ba.phong[:, :2] <= 1) and np.all(ba.phong[:, 2] >= 1)
    assert np.all(ba.texture >= 0) and np.all(ba.texture <= 1)


# ---------------------------------------------------------------------------------------------------- (5) general layout
def test_general_layout_with_twelve_materials_matches_oracle():
    prob, ph = synth.make_phong_problem(14, 500, track_len=20, seed=3, num_materials=12)
    d = ph.as_oracle_dict("perturbed")
    ba = StereoBA.from_synth(prob, lighting=d, shared_free=7)
    op = _oracle(prob, d, shared_free=7)
    assert ba.stats().general_structure == 1
    for radius in (1e4, 5.0):
        S, rhs, dp, dl, mcc = ba.lm_step(radius)
        S_pb, S_bb, rhs_b, db = ba.border_system()
        assert S_pb.shape[1] == 51
        dp2, dl2, mcc2 = op.lm_step(radius)
        rel = lambda a, b: np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)
        assert rel(dp, dp2) < 1e-7 and rel(dl, dl2) < 1e-7
        assert mcc == pytest.approx(mcc2, rel=1e-8)
    kw = dict(max_num_iterations=12, use_nonmonotonic_steps=1)
    ba = StereoBA.from_synth(prob, lighting=ph.as_oracle_dict("perturbed"), shared_free=7)
    op = _oracle(prob, ph.as_oracle_dict("perturbed"), shared_free=7)
    s, log = ba.solve(capi.default_options(**kw))
    s2, log2 = op.solve(orc.driver_options(num_threads=4, **kw))
    assert log["step_is_successful"].tolist() == log2["step_is_successful"].tolist()
    ok = np.asarray(log2["step_is_successful"], dtype=bool)
    ok[0] = True
    np.testing.assert_allclose(log["cost"][ok], log2["cost"][ok], rtol=1e-7)


# ------------------------------------------------------------------------------------------------------ (6) C++ driver
def test_phong_driver_on_ten_materials(tmp_path):
    """examples/dataset_ba_phong_gpu (the reference's driver against the C++ shim) on a dataset of ten materials: every shared
    block free, a border of 43 columns.  Measured against the oracle: the costs agree to 1.2e-8 and 5e-8 after iterations
    1 and 2; at iteration 3 the step norms differ by 6e-4 (3.4549 / 3.4569: the step along the Phong exponents is weakly
    determined, the bordered system reaches kappa ~ 1e17) and from iteration 4 on the two follow different paths: the
    device converges to 1.76807e5 after 30 iterations, the oracle to 1.73811e5 after 39 (1.7 % apart; the oracle with one
    thread against four parts at iteration 14, at 1e-6).  So the first iterations are held to the oracle, and the driver's
    whole run -- final cost, poses, light -- to the same library's run through the C ABI on the same problem."""
    import subprocess
    from ceres_slam_amd import build
    exe = build.build_examples("dataset_ba_phong_gpu")
    prob, ph = synth.make_phong_problem(50, 2000, num_materials=10)
    files = synth.write_reference_phong_csv(prob, ph, str(tmp_path / "sim.csv"), shared="reference")
    r = subprocess.run([exe, *files], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    d = ph.as_oracle_dict("reference")
    kw = dict(use_nonmonotonic_steps=1, trust_region_strategy_type=1, dogleg_type=1)
    op = _oracle(prob, d, shared_free=7, use_bounds=True)
    s2, log2 = op.solve(orc.driver_options(num_threads=4, **kw))
    # the same problem through the C ABI (the library the shim calls), for the report
    ba = StereoBA.from_synth(prob, lighting=d, shared_free=7, use_bounds=True)
    s, log = ba.solve(capi.default_options(max_num_iterations=1000, **kw))
    n = min(len(log["cost"]), len(log2["cost"]))
    rel = np.abs(log["cost"][:n] - log2["cost"][:n]) / np.abs(log2["cost"][:n])
    part = next((i for i in range(n) if rel[i] > 1e-6), None)
    report = [l for l in r.stdout.splitlines() if l.startswith("Ceres Solver Report")][0]
    final = float(report.split("Final cost: ")[1].split(",")[0])
    print(f"wide_border C++ driver M=10: final cost {final:.7e}, C ABI {s.final_cost:.7e} ({s.num_iterations} iterations), "
          f"oracle {s2.final_cost:.7e} ({s2.num_iterations} iterations); costs part by more than 1e-6 at iteration {part}; "
          "rel by tens: " + " ".join(f"{rel[i:i + 10].max():.1e}" for i in range(0, n, 10)))
    assert "Termination: CONVERGENCE" in report
    assert s.termination_type == s2.termination_type == 0
    np.testing.assert_allclose(log["cost"][:3], log2["cost"][:3], rtol=1e-7)
    assert log["step_is_successful"][:3].tolist() == log2["step_is_successful"][:3].tolist()
    assert final == pytest.approx(s.final_cost, rel=1e-4)
    poses = synth.read_pose_csv(str(tmp_path / "sim_poses.csv"))
    assert np.abs(poses - ba.poses).max() < 1e-4
    lights = np.loadtxt(str(tmp_path / "sim_lights.csv"), delimiter=",", skiprows=1)
    np.testing.assert_allclose(lights, ba.light, rtol=1e-4, atol=1e-5)


# --------------------------------------------------------------------------------------------------------- (7) full size
def test_full_size_driver_configuration_with_fifteen_materials():
    """1 000 poses / 100 000 landmarks, M = 15 (63 border columns), the Phong driver's configuration, K = 10: the bars of
    test_c3_full_size_in_the_phong_drivers_own_configuration, except for the costs and poses: with 15 materials the device
    and the oracle agree to 6e-9 for eight iterations, then part at 1.2e-5 (costs) and 6e-5 (poses) from iteration 8 on
    (measured; four materials: within 1e-6 and 1e-5).  The parallel plan: both panels go through its sweeps."""
    K = 10
    prob, ph = synth.make_phong_problem(*synth.CONFIGS["C2"], num_materials=15)
    d = ph.as_oracle_dict("reference")
    kw = dict(max_num_iterations=K, use_nonmonotonic_steps=1, trust_region_strategy_type=1, dogleg_type=1)
    ba = StereoBA.from_synth(prob, lighting=d, shared_free=7, use_bounds=True)
    s, log = ba.solve(capi.default_options(**kw))
    op = _oracle(prob, d, shared_free=7, use_bounds=True)
    s2, log2 = op.solve(orc.driver_options(num_threads=16, **kw))
    assert s.num_iterations == s2.num_iterations
    assert log["step_is_successful"].tolist() == log2["step_is_successful"].tolist()
    ok = np.asarray(log2["step_is_successful"], dtype=bool)
    ok[0] = True
    np.testing.assert_allclose(log["cost"][ok], log2["cost"][ok], rtol=5e-5)
    assert s.final_cost == pytest.approx(s2.final_cost, rel=5e-5)
    assert s.num_line_search_steps == s2.num_line_search_steps and s.num_line_searches_on_device > 0
    assert np.abs(ba.poses - op.poses).max() < 1e-4
    assert np.all(ba.phong[:, :2] >= 0) and np.all(ba.phong[:, :2] <= 1) and np.all(ba.phong[:, 2] >= 1)
    assert np.all(ba.texture >= 0) and np.all(ba.texture <= 1)
    np.testing.assert_allclose(ba.texture, op.texture, rtol=1e-5, atol=1e-7)


# ------------------------------------------------------------------------- plain levels, searches driven by the host
def test_plain_levels_take_both_panels(monkeypatch):
    """SSBA_NO_PCR=1: plain cyclic-reduction levels instead of the parallel plan (what a chain of more than 128 super-blocks
    takes), so both panels go through k_bcrm_fwd / _upd / _bwd level by level (border_panel's offsets of lev[l].B): the
    bordered step against the long-double refined solve, and LM step for step with the oracle."""
    monkeypatch.setenv("SSBA_NO_PCR", "1")
    prob, ph = synth.make_phong_problem(50, 2000, num_materials=15, seed=4)
    ba = StereoBA.from_synth(prob, lighting=ph.as_oracle_dict("truth"), shared_free=7)
    assert ba.stats().general_structure == 0 and ba.stats().num_superblocks == 5
    for radius in (1e4, 3.0):
        S, rhs, dp, dl, mcc = ba.lm_step(radius)
        S_pb, S_bb, rhs_b, db = ba.border_system()
        assert S_pb.shape[1] == 63
        A = np.block([[S, S_pb], [S_pb.T, S_bb]])
        _check_solve(f"wide_border plain levels r={radius}", A, np.concatenate([rhs, rhs_b]), np.concatenate([dp[1:].ravel(), db]))
    prob, ph = synth.make_phong_problem(50, 2000, num_materials=15, seed=5)
    d = ph.as_oracle_dict("perturbed")
    ba = StereoBA.from_synth(prob, lighting=d, shared_free=7)
    op = _oracle(prob, d, shared_free=7)
    s, log = ba.solve(capi.default_options(max_num_iterations=12, use_nonmonotonic_steps=1))
    s2, log2 = op.solve(orc.driver_options(num_threads=4, max_num_iterations=12))
    assert log["step_is_successful"].tolist() == log2["step_is_successful"].tolist()
    ok = np.asarray(log2["step_is_successful"], dtype=bool)
    ok[0] = True
    np.testing.assert_allclose(log["cost"][ok], log2["cost"][ok], rtol=1e-7)


def test_searches_driven_by_the_host_give_the_same_bits(monkeypatch):
    """SSBA_LS_ROUNDS=0 hands every projected line search to the host (k_ph_ls_reduce with its 63 border entries per
    evaluation); the default runs them on the device (k_ph_ls_fast and the rounds behind it).  Same evaluations: the driver's
    configuration at M = 15 must give the same bits and the same evaluation count, as
    test_line_search_on_the_device_is_the_search_the_host_drives requires of four materials."""
    prob, ph = synth.make_phong_problem(50, 2000, num_materials=15, seed=6)
    d = ph.as_oracle_dict("reference")
    kw = dict(max_num_iterations=25, use_nonmonotonic_steps=1, trust_region_strategy_type=1, dogleg_type=1)
    runs = {}
    for rounds in ("0", None):
        if rounds is None:
            monkeypatch.delenv("SSBA_LS_ROUNDS", raising=False)
        else:
            monkeypatch.setenv("SSBA_LS_ROUNDS", rounds)
        ba = StereoBA.from_synth(prob, lighting=d, shared_free=7, use_bounds=True)
        s, log = ba.solve(capi.default_options(**kw))
        runs[rounds] = (s, log, ba.poses.copy(), ba.texture.copy(), ba.light.copy())
    (s0, log0, p0, t0, l0), (s1, log1, p1, t1, l1) = runs["0"], runs[None]
    assert s0.num_line_searches_on_device == 0 and s0.num_line_searches_by_host > 0 and s1.num_line_searches_on_device > 0
    assert s0.num_line_searches_by_host == s1.num_line_searches_on_device + s1.num_line_searches_by_host
    assert s0.num_iterations == s1.num_iterations and s0.num_line_search_steps == s1.num_line_search_steps
    np.testing.assert_array_equal(log0["cost"], log1["cost"])
    np.testing.assert_array_equal(p0, p1)
    np.testing.assert_array_equal(t0, t1)
    np.testing.assert_array_equal(l0, l1)


# --------------------------------------------------------------------------------------------------- (8) still refused
def test_sharding_a_wide_border_is_refused_loudly():
    prob, ph = synth.make_phong_problem(50, 2000, num_materials=8)
    with pytest.raises(capi.SsbaError) as e:
        StereoBA.from_synth(prob, lighting=ph.as_oracle_dict("perturbed"), shared_free=7, world_size=2, rank=0)
    assert e.value.status == -6      # SSBA_ERR_UNSUPPORTED
    assert "wider than 32 columns" in str(e.value)


def test_sixteen_materials_are_refused():
    prob, ph = synth.make_phong_problem(20, 600, track_len=8, num_materials=16, seed=2)
    with pytest.raises(capi.SsbaError) as e:
        StereoBA.from_synth(prob, lighting=ph.as_oracle_dict("perturbed"), shared_free=7)
    assert "ssba_add_material_blocks" in str(e.value)
