"""Multi-rank path: landmark sharding + exchange of the pose system.
CPU part: world_size-2 gloo processes, oracle as compute.  GPU part (marked gpu): two ranks
drive the HIP library on one device and exchange through torch.distributed."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from ceres_slam_amd import sharding, synth
from oracle import oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_ranks(mode, out, world=2, timeout=300, size=None, extra_env=None):
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2")
        if size:
            env["SSBA_TEST_SIZE"] = ",".join(str(v) for v in size)
        env.update(extra_env or {})
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "dist_worker.py"), mode, out], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = [p.communicate(timeout=timeout)[0].decode(errors="replace") for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    return [json.load(open(f"{out}.{r}.json")) for r in range(world)]


def test_landmark_ranges_partition_and_balance():
    prob = synth.make_problem(40, 3000, track_len=8, seed=2)
    for world in (1, 2, 3, 8):
        ranges = sharding.landmark_ranges(prob.obs_point, prob.num_points, world)
        assert ranges[0][0] == 0 and ranges[-1][1] == prob.num_points
        assert all(ranges[i][1] == ranges[i + 1][0] for i in range(world - 1))
        counts = [int(((prob.obs_point >= b) & (prob.obs_point < e)).sum()) for b, e in ranges]
        assert sum(counts) == prob.num_obs
        assert max(counts) - min(counts) <= 0.02 * prob.num_obs + 16      # balanced by observations
    # every observation lands in exactly one shard, indices remapped consistently
    shards = [sharding.shard_by_landmarks(prob, 3, r) for r in range(3)]
    assert sum(s.obs_pose.shape[0] for s in shards) == prob.num_obs
    for s in shards:
        np.testing.assert_array_equal(s.points, prob.points_init[s.point_ids])
        assert s.obs_point.max() < s.points.shape[0]


def test_two_rank_gloo_sum_of_shard_systems_equals_unsharded(tmp_path):
    res = _run_ranks("cpu", str(tmp_path / "cpu"))
    prob = synth.make_problem(16, 400, track_len=6, seed=21)
    op = orc.OracleProblem.from_synth(prob)
    cost, g_p, g_l, H_pp, H_ll = op.linearize()
    for r in res:      # every rank holds the same all-reduced sums
        assert r["cost"] == pytest.approx(cost, rel=1e-12)
        np.testing.assert_allclose(np.array(r["g_p"]).reshape(-1, 6), g_p, rtol=1e-10, atol=1e-8)
        assert r["H_pp_trace"] == pytest.approx(np.trace(H_pp.sum(0)), rel=1e-12)
        assert r["gmax_l"] == pytest.approx(np.abs(g_l).max(), rel=1e-12)
    assert sum(r["num_local_obs"] for r in res) == prob.num_obs


@pytest.mark.gpu
def test_two_rank_sharded_gpu_solve_matches_unsharded_oracle(tmp_path):
    res = _run_ranks("gpu", str(tmp_path / "gpu"))
    prob = synth.make_problem(16, 400, track_len=6, seed=21)
    op = orc.OracleProblem.from_synth(prob)
    s, log = op.solve(orc.driver_options(num_threads=2))
    for r in res:
        assert r["termination"] == 0
        assert r["num_iterations"] == s.num_iterations
        np.testing.assert_allclose(r["cost"], log["cost"], rtol=1e-9)
        assert r["final_cost"] == pytest.approx(s.final_cost, rel=1e-6)
        assert np.abs(np.array(r["poses"]) - op.poses).max() < 1e-6          # poses replicated
        assert np.abs(np.array(r["points"]) - op.points[r["point_ids"]]).max() < 1e-5
    np.testing.assert_array_equal(res[0]["poses"], res[1]["poses"])          # ranks agree bit for bit


@pytest.mark.gpu
@pytest.mark.parametrize("world,size", [(2, (60, 2400, 20)), (3, (130, 3900, 24))])
def test_sharded_long_tracks_match_unsharded_oracle(tmp_path, world, size):
    """Landmark sharding of a problem whose tracks have 13..24 observations (ssba_wide.hip): every rank forms the 144-row
    super-blocks of ITS landmarks, they are summed over the ranks next to the gradient vectors, every rank runs the same
    parallel cyclic reduction.  Same iterates as the unsharded oracle, ranks bit-identical."""
    K = 25
    res = _run_ranks("gpu", str(tmp_path / "wide"), world, size=size, extra_env={"SSBA_TEST_MAXIT": str(K)})
    prob = synth.make_problem(size[0], size[1], track_len=size[2], seed=21)
    assert np.bincount(prob.obs_point).max() > 12
    op = orc.OracleProblem.from_synth(prob)
    s, log = op.solve(orc.driver_options(num_threads=2, max_num_iterations=K))
    for r in res:
        assert r["num_iterations"] == s.num_iterations
        assert r["accept"] == log["step_is_successful"].tolist()
        ok = np.asarray(log["step_is_successful"], dtype=bool)
        ok[0] = True
        np.testing.assert_allclose(np.asarray(r["cost"])[ok], log["cost"][ok], rtol=1e-8)
        assert r["final_cost"] == pytest.approx(s.final_cost, rel=1e-6)
        assert np.abs(np.array(r["poses"]) - op.poses).max() < 1e-6
        assert np.abs(np.array(r["points"]) - op.points[r["point_ids"]]).max() < 1e-5
    for r in res[1:]:
        np.testing.assert_array_equal(res[0]["poses"], r["poses"])


@pytest.mark.gpu
@pytest.mark.parametrize("world,size,dogleg,mode", [(2, (16, 400, 6), 0, "gpu"), (3, (40, 1600, 12), 1, "gpu"), (2, (60, 2400, 20), 1, "gpu"),
                                                    (2, (60, 2400, 12), 1, "gpu_phong"), (2, (60, 2400, 12), 1, "gpu_phongfree"),
                                                    (3, (60, 2400, 12), 0, "gpu_phongfree")])
def test_sharded_dogleg_solve_matches_unsharded_oracle(tmp_path, world, size, dogleg, mode):
    """The trust-region strategy of the reference's BA driver (tests/dataset_ba_phong.cpp:85-86: DOGLEG, SUBSPACE_DOGLEG) with
    landmark sharding: the six sums of the dogleg model (|gradient|^2, |gn|^2, gradient.gn, |Jv|^2, |Jgn|^2, Jv.Jgn) are
    per-rank partial sums that the ranks add at one more exchange point; windowed layout, long tracks (144-row super-blocks)
    and lighting terms with constant shared blocks.  Same iterates as the unsharded oracle, ranks bit-identical."""
    K = 25
    res = _run_ranks(mode, str(tmp_path / "dl"), world, size=size, extra_env={"SSBA_TEST_MAXIT": str(K), "SSBA_TEST_DOGLEG": str(dogleg)})
    okw = dict(num_threads=2, max_num_iterations=K, trust_region_strategy_type=1, dogleg_type=dogleg)
    if mode in ("gpu_phong", "gpu_phongfree"):     # gpu_phongfree: light, Phong and texture blocks free (the driver's problem; its border part of the sums is counted by one rank)
        free = mode == "gpu_phongfree"
        prob, ph = synth.make_phong_problem(size[0], size[1], track_len=size[2], seed=21)
        op = orc.OracleProblem(prob.camera, prob.poses_init, prob.points_init, prob.obs_pose, prob.obs_point, prob.obs_uvd,
                               prob.stiffness(), lighting=ph.as_oracle_dict("perturbed" if free else "truth"), shared_free=7 if free else 0)
    else:
        prob = synth.make_problem(size[0], size[1], track_len=size[2], seed=21)
        op = orc.OracleProblem.from_synth(prob)
    s, log = op.solve(orc.driver_options(**okw))
    for r in res:
        assert r["num_iterations"] == s.num_iterations
        assert r["accept"] == log["step_is_successful"].tolist()
        ok = np.asarray(log["step_is_successful"], dtype=bool)
        ok[0] = True
        # (SUBSPACE_DOGLEG on lighting problems amplifies rounding to ~1e-8 in its first iteration -- the Gauss-Newton solve with
        # mu = 1e-8 --: tools/fuzz_parity.py conditioned_agreement; the unsharded lighting tests compare at 1e-6 too)
        np.testing.assert_allclose(np.asarray(r["cost"])[ok], log["cost"][ok], rtol=1e-6 if mode.startswith("gpu_phong") else 1e-8)
        assert r["final_cost"] == pytest.approx(s.final_cost, rel=1e-6)
        assert np.abs(np.array(r["poses"]) - op.poses).max() < 1e-6
    for r in res[1:]:
        np.testing.assert_array_equal(res[0]["poses"], r["poses"])


@pytest.mark.gpu
@pytest.mark.parametrize("world,dogleg,huber", [(2, None, 0.0), (3, 1, 0.5)])
def test_sharded_solve_with_pose_factors_matches_unsharded_oracle(tmp_path, world, dogleg, huber):
    """Pose prior + sun-sensor blocks (tests/dataset_vo_sun.cpp:80-124: no constant pose, the prior anchors the window;
    HuberLoss on the sun blocks; the driver's SUBSPACE_DOGLEG) with landmark sharding: the poses are replicated, ONE rank
    adds the unary blocks to the sums the ranks exchange, every rank evaluates them at the candidate."""
    from test_oracle_pose_factors import _sun_problem
    K = 20
    env = {"SSBA_TEST_MAXIT": str(K), "SSBA_TEST_HUBER": str(huber)}
    okw = dict(num_threads=2, max_num_iterations=K)
    if dogleg is not None:
        env["SSBA_TEST_DOGLEG"] = str(dogleg)
        okw.update(trust_region_strategy_type=1, dogleg_type=dogleg)
    res = _run_ranks("gpu_sun", str(tmp_path / "sun"), world, size=(30, 1500, 5), extra_env=env)
    prob, factors = _sun_problem(P=30, L=1500, seed=5, huber=huber)
    op = orc.OracleProblem(prob.camera, prob.poses_init, prob.points_init, prob.obs_pose, prob.obs_point, prob.obs_uvd, prob.stiffness(),
                           pose_const=np.zeros(prob.num_poses, dtype=np.uint8), pose_factors=factors)
    s, log = op.solve(orc.driver_options(**okw))
    for r in res:
        assert r["num_iterations"] == s.num_iterations
        assert r["accept"] == log["step_is_successful"].tolist()
        ok = np.asarray(log["step_is_successful"], dtype=bool)
        ok[0] = True
        np.testing.assert_allclose(np.asarray(r["cost"])[ok], log["cost"][ok], rtol=1e-7)
        assert r["final_cost"] == pytest.approx(s.final_cost, rel=1e-6)
        assert np.abs(np.array(r["poses"]) - op.poses).max() < 1e-5
    for r in res[1:]:
        np.testing.assert_array_equal(res[0]["poses"], r["poses"])


def test_aligned_partition_cuts_at_superblock_boundaries():
    for P, L, W in ((40, 1600, 2), (60, 2400, 3), (300, 12000, 4)):
        prob = synth.make_problem(P, L)
        ranges, seps = sharding.aligned_partition(prob.obs_pose, prob.obs_point, prob.num_poses, prob.num_points, W)
        assert ranges[0][0] == 0 and ranges[-1][1] == L and all(ranges[r][1] == ranges[r + 1][0] for r in range(W - 1))
        assert seps[0] == 0 and seps[-1] == (P - 1 + 11) // 12 - 1 and np.all(np.diff(seps.astype(int)) >= 1)
        f = prob.obs_pose.astype(int) - 1          # pose 0 is constant
        for r, (b, e) in enumerate(ranges):
            sel = (prob.obs_point >= b) & (prob.obs_point < e) & (f >= 0)
            sb = f[sel] // 12
            assert sb.min() >= seps[r] and sb.max() <= seps[r + 1]
    # no aligned cut when every landmark is seen from everywhere
    rng = np.random.default_rng(0)
    op, ol = rng.integers(0, 60, 5000), rng.integers(0, 200, 5000)
    assert sharding.aligned_partition(op, ol, 60, 200, 2) is None


def test_ranges_for_separators_keep_every_rank_inside_its_chain():
    """Explicit separator lists (tests/test_gpu_hp_sharded.py): with tracks of 8 every interior super-block has a landmark cut."""
    for size, seps in (((61, 2400, 8), [0, 2, 4]), ((61, 2400, 8), [0, 1, 2, 4]), ((58, 2300, 8), [0, 1, 2, 3, 4]),
                       ((85, 3400, 8), [0, 2, 3, 4, 5, 6]), ((133, 5300, 8), [0, 6, 10])):
        prob = synth.make_problem(size[0], size[1], track_len=size[2], seed=21)
        ranges = sharding.ranges_for_separators(prob.obs_pose, prob.obs_point, prob.num_poses, prob.num_points, seps)
        assert ranges[0][0] == 0 and ranges[-1][1] == size[1] and all(ranges[r][1] == ranges[r + 1][0] for r in range(len(seps) - 2))
        f = prob.obs_pose.astype(int) - 1          # pose 0 is constant
        for r, (b, e) in enumerate(ranges):
            sb = f[(prob.obs_point >= b) & (prob.obs_point < e) & (f >= 0)] // 12
            assert sb.min() >= seps[r] and sb.max() <= seps[r + 1]
    with pytest.raises(ValueError):               # the list must end at the last super-block
        sharding.ranges_for_separators(prob.obs_pose, prob.obs_point, prob.num_poses, prob.num_points, [0, 6, 9])
    prob = synth.make_problem(60, 2400, track_len=20, seed=21)      # tracks of 20 span three super-blocks: no cut at 2
    with pytest.raises(ValueError):
        sharding.ranges_for_separators(prob.obs_pose, prob.obs_point, prob.num_poses, prob.num_points, [0, 2, 4])


@pytest.mark.gpu
@pytest.mark.parametrize("world,size,pcr_max,maxit", [(2, (40, 1600, 12), None, 0), (3, (100, 4000, 12), None, 30), (2, (300, 9000, 12), None, 30),
                                                      (4, (300, 9000, 12), None, 0), (2, (300, 9000, 12), 4, 30), (4, (300, 9000, 12), 3, 30),
                                                      (3, (420, 12000, 12), 5, 30)])
def test_partitioned_gpu_solve_matches_unsharded_oracle(tmp_path, world, size, pcr_max, maxit):
    """Partitioned reduced solve (ssba_set_partition): every rank eliminates the interior of its own chain of
    super-blocks (parallel cyclic reduction with the shared ends pinned; with SSBA_PCR_MAX_BLOCKS set, plain levels
    first), only the separator system is summed over the ranks.  Same iterates as the unsharded solve.
    maxit > 0: both runs are cut at that iteration count, before the flat tail of the convergence, and EVERYTHING is
    compared at the 1e-6 bar (landmarks, gradient norms, step norms included); maxit = 0: run to convergence."""
    env = {}
    if pcr_max:
        env["SSBA_PCR_MAX_BLOCKS"] = str(pcr_max)
    if maxit:
        env["SSBA_TEST_MAXIT"] = str(maxit)
    res = _run_ranks("gpu_part", str(tmp_path / "part"), world, size=size, extra_env=env or None)
    prob = synth.make_problem(size[0], size[1], track_len=size[2], seed=21)
    op = orc.OracleProblem.from_synth(prob)
    s2, log2 = op.solve(orc.driver_options(num_threads=2, **({"max_num_iterations": maxit} if maxit else {})))
    for r in res:
        assert r["termination"] == s2.termination_type
        assert r["num_iterations"] == s2.num_iterations
        assert r["accept"] == log2["step_is_successful"].tolist()
        ok = np.asarray(log2["step_is_successful"], dtype=bool)
        ok[0] = True
        np.testing.assert_allclose(np.asarray(r["cost"])[ok], log2["cost"][ok], rtol=1e-8)
        assert r["final_cost"] == pytest.approx(s2.final_cost, rel=1e-6)
        assert np.abs(np.asarray(r["poses"]) - op.poses).max() < 1e-6              # every rank has the whole trajectory
        ref = op.points[r["point_ids"]]
        if maxit:
            np.testing.assert_allclose(r["gmax"], log2["gradient_max_norm"], rtol=1e-6)
            np.testing.assert_allclose(r["step_norm"], log2["step_norm"], rtol=1e-6, atol=1e-12)
            assert (np.abs(np.asarray(r["points"]) - ref) / (1 + np.abs(ref))).max() < 1e-6
        else:
            # converged runs: far landmarks are weakly constrained in depth and drift along the flat tail (~70
            # iterations); their 1e-6 comparison is the job of the fixed-iteration cases above
            assert (np.abs(np.asarray(r["points"]) - ref) / (1 + np.abs(ref))).max() < 1e-4
    assert res[0]["poses"] == res[1]["poses"]                                      # bit-identical across ranks


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3])
def test_partitioned_huber_solve_with_outliers_matches_unsharded_oracle(tmp_path, world):
    """BASELINE.json configs[4] in small: HuberLoss on every block, 30 % outlier observations, landmarks sharded over
    the ranks with the partitioned reduced solve.  Both runs are cut at the same iteration count (before the flat tail
    whose stop point is rounding-sensitive): same accept / reject sequence, costs and end point at the 1e-6 bar."""
    size = (100, 4000, 12)
    K = 25
    res = _run_ranks("gpu_part", str(tmp_path / "hub"), world, size=size, extra_env={"SSBA_TEST_HUBER": "1.345", "SSBA_TEST_MAXIT": str(K)})
    prob = synth.make_problem(size[0], size[1], track_len=size[2], seed=21, outlier_fraction=0.3)
    op = orc.OracleProblem.from_synth(prob, huber_a=1.345)
    s2, log2 = op.solve(orc.driver_options(num_threads=2, max_num_iterations=K))
    for r in res:
        assert r["num_iterations"] == s2.num_iterations
        assert r["accept"] == log2["step_is_successful"].tolist()
        ok = np.asarray(log2["step_is_successful"], dtype=bool)
        ok[0] = True
        np.testing.assert_allclose(np.asarray(r["cost"])[ok], log2["cost"][ok], rtol=1e-8)
        assert r["final_cost"] == pytest.approx(s2.final_cost, rel=1e-6)
        assert np.abs(np.asarray(r["poses"]) - op.poses).max() < 1e-6
    assert res[0]["poses"] == res[1]["poses"]


_RCCL_WORLD1 = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from ceres_slam_amd import capi, sharding, synth
from ceres_slam_amd.solver import StereoBA
prob = synth.make_config("C1")
opts = dict(max_num_iterations=1000, use_nonmonotonic_steps=1)
ref = StereoBA.from_synth(prob)
s0, log0 = ref.solve(capi.default_options(**opts))
ba = StereoBA(prob.camera, prob.poses_init.copy(), prob.points_init.copy(), prob.obs_pose, prob.obs_point, prob.obs_uvd,
              prob.stiffness(), world_size=1, rank=0)
sharding.attach_rccl_exchange(ba, None)
s, log = ba.solve(capi.default_options(**opts))
json.dump(dict(it=[int(s.num_iterations), int(s0.num_iterations)], ok=[log["step_is_successful"].tolist(), log0["step_is_successful"].tolist()],
               cost=[log["cost"].tolist(), log0["cost"].tolist()], dpose=float(np.abs(ba.poses - ref.poses).max()),
               final=float(s.final_cost)), open(sys.argv[2], "w"))
"""


@pytest.mark.gpu
def test_native_rccl_exchange_world_of_one(tmp_path):
    """ssba_set_rccl: the library's own ncclAllReduce calls at the exchange points (a communicator of one rank here -- the
    test box has one GPU; more ranks use the same code with a shared unique id).  The sharded code path (all poses kept,
    kernel segments around the exchange points) must reproduce the plain single-GPU solve.
    Runs in a child process through tests/rccl_record.py: NCCL_DEBUG=INFO into a file, the library's own time limit on its
    RCCL set-up calls (SSBA_ERR_TIMEOUT names the call, the librccl.so file and version), and an outer limit that
    snapshots /proc/<pid> before killing.  A hang INSIDE the named RCCL call is an expected failure with the whole record
    in its message and under gpurun_out/rccl_records/; anything else -- including a hang somewhere else -- fails."""
    import json
    from rccl_record import library_timed_out, run
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "rccl1.json")
    rc, _, err, record, rec_dir = run([sys.executable, "-c", _RCCL_WORLD1, root, out], "world1")
    # a hang inside the RCCL call the library names is a FAILURE that carries its record (r03 turned it into an xfail, which
    # keeps `pytest -x -q` green: a recurring hang would never have turned the suite red)
    assert not (rc != 0 and library_timed_out(err)), f"RCCL set-up hang, diagnosed by the library's own time limit (record kept in {rec_dir}):\n{record}"
    assert rc == 0, f"record in {rec_dir}:\n{record}"
    res = json.load(open(out))
    assert res["it"][0] == res["it"][1]
    assert res["ok"][0] == res["ok"][1]
    np.testing.assert_allclose(res["cost"][0], res["cost"][1], rtol=1e-10)
    assert res["dpose"] < 1e-9
    op = orc.OracleProblem.from_synth(synth.make_config("C1"))
    s2, _ = op.solve(orc.driver_options(num_threads=4))
    assert res["final"] == pytest.approx(s2.final_cost, rel=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,world", [("gpu_phong", 2), ("gpu_part_phong", 3)])
def test_sharded_lighting_terms_match_unsharded_oracle(tmp_path, mode, world):
    """BASELINE.json configs[2] sharded: stereo + Phong intensity + normal blocks with the shared light /
    material / texture blocks constant, landmarks (with their lighting observations) split over the ranks -- summing the
    whole reduced system (gpu_phong) and with the partitioned reduced solve (gpu_part_phong)."""
    size, K = (60, 2400, 12), 20
    res = _run_ranks(mode, str(tmp_path / "ph"), world, size=size, extra_env={"SSBA_TEST_MAXIT": str(K)})
    prob, ph = synth.make_phong_problem(size[0], size[1], track_len=size[2], seed=21)
    d = ph.as_oracle_dict("truth")
    op = orc.OracleProblem(prob.camera, prob.poses_init, prob.points_init, prob.obs_pose, prob.obs_point, prob.obs_uvd,
                           prob.stiffness(), lighting=d)
    s2, log2 = op.solve(orc.driver_options(num_threads=2, max_num_iterations=K))
    for r in res:
        assert r["num_iterations"] == s2.num_iterations
        assert r["accept"] == log2["step_is_successful"].tolist()
        ok = np.asarray(log2["step_is_successful"], dtype=bool)
        ok[0] = True
        np.testing.assert_allclose(np.asarray(r["cost"])[ok], log2["cost"][ok], rtol=1e-8)
        assert r["final_cost"] == pytest.approx(s2.final_cost, rel=1e-6)
        assert np.abs(np.asarray(r["poses"]) - op.poses).max() < 1e-6
        assert np.abs(np.asarray(r["normals"]) - op.normals[r["point_ids"]]).max() < 1e-6
    assert res[0]["poses"] == res[1]["poses"]


@pytest.mark.gpu
def test_sharded_lighting_terms_with_free_shared_blocks(tmp_path):
    """The same with the light, Phong and texture blocks FREE: every rank forms the border sums (S_pb, S_bb, reduced border
    gradient) of its own landmarks, they are summed over the ranks next to the reduced system, and every rank solves the
    arrowhead system; the shared blocks come out identical on all ranks and equal to the unsharded oracle's."""
    size, K = (60, 2400, 12), 15
    res = _run_ranks("gpu_phongfree", str(tmp_path / "phf"), 2, size=size, extra_env={"SSBA_TEST_MAXIT": str(K)})
    prob, ph = synth.make_phong_problem(size[0], size[1], track_len=size[2], seed=21)
    d = ph.as_oracle_dict("perturbed")
    op = orc.OracleProblem(prob.camera, prob.poses_init, prob.points_init, prob.obs_pose, prob.obs_point, prob.obs_uvd,
                           prob.stiffness(), lighting=d, shared_free=7)
    s2, log2 = op.solve(orc.driver_options(num_threads=2, max_num_iterations=K))
    for r in res:
        assert r["num_iterations"] == s2.num_iterations
        assert r["accept"] == log2["step_is_successful"].tolist()
        ok = np.asarray(log2["step_is_successful"], dtype=bool)
        ok[0] = True
        np.testing.assert_allclose(np.asarray(r["cost"])[ok], log2["cost"][ok], rtol=1e-7)
        assert r["final_cost"] == pytest.approx(s2.final_cost, rel=1e-6)
        assert np.abs(np.asarray(r["poses"]) - op.poses).max() < 1e-6
        np.testing.assert_allclose(r["light"], op.light, rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(r["phong"], op.phong, rtol=1e-6, atol=1e-8)
        np.testing.assert_allclose(r["texture"], op.texture, rtol=1e-6)
    assert res[0]["poses"] == res[1]["poses"] and res[0]["light"] == res[1]["light"]


@pytest.mark.gpu
@pytest.mark.parametrize("world,dogleg", [(2, 1), (3, None)])
def test_sharded_lighting_driver_configuration_with_bounds(tmp_path, world, dogleg):
    """The BA driver's own problem on more than one rank (tests/dataset_ba_phong.cpp:84-87,142-180): free light / Phong / texture
    blocks, bounds on the Phong and texture blocks -- so every iteration ends in Ceres' projected Armijo line search -- and
    SUBSPACE_DOGLEG.  With landmark sharding the search's sums (phi, phi', |dx|^2 over the landmarks' rows; max|delta| through
    one slot per rank) are added over the ranks at every evaluation; the full step is tested on the device, a rejected one is
    searched by the host in lockstep on all ranks.  Same iterates and the same number of line-search evaluations as the
    unsharded oracle, ranks bit-identical."""
    size, K = (60, 2400, 12), 20
    env = {"SSBA_TEST_MAXIT": str(K)}
    okw = dict(num_threads=2, max_num_iterations=K)
    if dogleg is not None:
        env["SSBA_TEST_DOGLEG"] = str(dogleg)
        okw.update(trust_region_strategy_type=1, dogleg_type=dogleg)
    res = _run_ranks("gpu_phongfreeb", str(tmp_path / "phb"), world, size=size, extra_env=env)
    prob, ph = synth.make_phong_problem(size[0], size[1], track_len=size[2], seed=21)
    op = orc.OracleProblem(prob.camera, prob.poses_init, prob.points_init, prob.obs_pose, prob.obs_point, prob.obs_uvd,
                           prob.stiffness(), lighting=ph.as_oracle_dict("perturbed"), shared_free=7, use_bounds=True)
    s2, log2 = op.solve(orc.driver_options(**okw))
    assert s2.num_line_search_steps > s2.num_iterations        # (some full steps were rejected: the search itself ran)
    for r in res:
        assert r["num_iterations"] == s2.num_iterations
        assert r["accept"] == log2["step_is_successful"].tolist()
        assert r["line_search_steps"] == s2.num_line_search_steps
        ok = np.asarray(log2["step_is_successful"], dtype=bool)
        ok[0] = True
        np.testing.assert_allclose(np.asarray(r["cost"])[ok], log2["cost"][ok], rtol=1e-6)
        assert r["final_cost"] == pytest.approx(s2.final_cost, rel=1e-6)
        assert np.abs(np.asarray(r["poses"]) - op.poses).max() < 1e-6
        np.testing.assert_allclose(r["phong"], op.phong, rtol=1e-6, atol=1e-8)
        np.testing.assert_allclose(r["texture"], op.texture, rtol=1e-6)
    for r in res[1:]:
        assert res[0]["poses"] == r["poses"] and res[0]["phong"] == r["phong"]


def _bench(args, env_extra, timeout=900):
    import json
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env.update(env_extra)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), *args], capture_output=True, text=True, timeout=timeout, env=env)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    return r, [json.loads(ln) for ln in lines]


def test_bench_gpus_n_starts_its_own_ranks_and_relays_their_exit_code(torch_sees_a_gpu):
    """`python bench.py --gpus 2` typed without a launcher starts two ranks as child processes (before the parent touches a
    GPU).  On this CPU-only box every rank stops with the library's "no CPU fallback" message; the parent must relay a
    non-zero exit code and print no bench line."""
    if torch_sees_a_gpu:
        pytest.skip("CPU-only check of the launcher (the GPU rehearsal below covers the working path)")
    r, lines = _bench(["--gpus", "2", "--steps", "2", "--warmup", "1", "--no-cpu-baseline"], {"SSBA_BENCH_BACKEND": "gloo"}, timeout=600)
    assert r.returncode != 0
    assert not lines
    assert "needs an MI355X" in r.stderr


@pytest.mark.gpu
def test_bench_two_rank_rehearsal_on_one_device():
    """The command the driver types for the scaling runs, rehearsed on the one-GPU box: two ranks started by bench.py itself,
    both on cuda:0, collectives over gloo (SSBA_BENCH_BACKEND=gloo).  One JSON line, exit code 0, the partitioned reduced
    solve, `value` in C2-sized units (2 per iteration of the 2 x C2 problem)."""
    r, lines = _bench(["--gpus", "2", "--steps", "20", "--warmup", "5"], {"SSBA_BENCH_BACKEND": "gloo"})
    assert r.returncode == 0, r.stderr[-3000:]
    assert len(lines) == 1
    b = lines[0]
    assert b["n_gpus"] == 2 and b["steps"] == 20 and b["warmup"] == 5
    assert b["config"]["poses"] == 2000 and b["config"]["landmarks"] == 200000
    assert b["config"]["reduced_solve"].startswith("partitioned")
    assert b["config"]["exchange"] == "torch.distributed (gloo)" and b["config"]["rccl_ranks"] == 0
    assert b["value"] == pytest.approx(2 * b["config"]["joint_iters_per_sec"])
    assert b["ms_per_step"] > 0
    # what the line says about scaling: N x C2 is weak-scaled; the same joint problem measured on one GPU by rank 0 is the
    # denominator of the factor beside `value`; BASELINE.json's metric problem (C2 itself) cut into two shards rides along
    assert b["scaling"] == "weak" and b["unit"] == "C2-units/s"
    one = b["single_gpu_same_problem"]
    assert b["speedup_vs_1gpu_same_problem"] == pytest.approx(b["config"]["joint_iters_per_sec"] / one["joint_iters_per_sec"])
    st = b["strong_scaling_C2"]
    assert st["scaling"] == "strong" and st["partitioned"] and st["iters_per_sec"] > 0
    assert st["speedup_vs_1gpu_same_problem"] == pytest.approx(st["iters_per_sec"] / st["single_gpu_iters_per_sec"])


_RCCL_TIMEOUT = r"""
import sys
sys.path.insert(0, sys.argv[1])
from ceres_slam_amd import capi
from ceres_slam_amd.solver import StereoBA
print("DESCRIBE", StereoBA.rccl_describe())
try:
    StereoBA.rccl_unique_id()
    print("RESULT no timeout")
except capi.SsbaError as e:
    print("RESULT", e.status, str(e))
import time
time.sleep(5.0)      # the abandoned helper thread is still inside ncclGetUniqueId: let it return before the process is torn down
"""


@pytest.mark.gpu
def test_rccl_set_up_time_limit_leaves_a_record():
    """SSBA_RCCL_TIMEOUT_S: with a limit no RCCL call can meet (100 microseconds) ssba_rccl_unique_id must come back with
    SSBA_ERR_TIMEOUT and say which call it was waiting for and which librccl.so the process uses -- the record a real
    set-up hang would leave.  The abandoned helper thread finishes in the background (a communicator that completes late is
    destroyed by that thread); the child waits for it before it exits, so its exit code is checked too."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SSBA_RCCL_TIMEOUT_S="0.0001")
    r = subprocess.run([sys.executable, "-c", _RCCL_TIMEOUT, root], capture_output=True, text=True, timeout=240, env=env)
    out = r.stdout
    assert r.returncode == 0, out + r.stderr[-2000:]
    assert "DESCRIBE librccl: " in out and "version" in out, out + r.stderr[-2000:]
    line = [ln for ln in out.splitlines() if ln.startswith("RESULT")][0]
    assert "-8" in line and "SSBA_ERR_TIMEOUT" in line, line
    assert "ncclGetUniqueId did not return within" in line and "librccl: /" in line and "HSA_ENABLE_IPC_MODE_LEGACY=" in line, line
