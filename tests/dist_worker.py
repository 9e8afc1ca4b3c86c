"""Worker for the multi-process tests (one process per rank; RANK / WORLD_SIZE / MASTER_* in env).

mode "cpu": gloo on CPU tensors -- the sharding logic + the all-reduce of the shard-local
            normal-equation sums, with the CPU oracle as the compute (no GPU needed);
mode "gpu": every rank drives the HIP library on its landmark shard (all ranks on cuda:0 when
            only one GPU exists) and the exchange points go through torch.distributed.
mode "step" / "step_phongfree": one launch runs a list of one-iteration cases (JSON in SSBA_TEST_CASES) and records the
            whole iteration log, the written-back blocks and ssba_stats of each (tests/test_gpu_hp_sharded.py).
Each rank writes a JSON result file: <out>.<rank>.json
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _step_problem(mode, size, case):
    """The problem of one `step` case: (prob, lighting dict or None, shared_free)."""
    from ceres_slam_amd import synth
    P, Lm, T = size
    if mode == "step_phongfree":
        prob, ph = synth.make_phong_problem(P, Lm, track_len=T, seed=21, light_type=int(case.get("light_type", 0)))
        return prob, ph.as_oracle_dict("perturbed"), 7
    huber = float(case.get("huber", 0.0))
    return synth.make_problem(P, Lm, track_len=T, seed=21, outlier_fraction=0.3 if huber > 0 else 0.0), None, 0


def _step_mode(mode, out, rank, world, dist, size):
    """One trust-region iteration per case from prob.*_init on this rank's shard: radius (initial_trust_region_radius), huber
    (with it 30 % outliers), strategy / dogleg, partition (None: all-reduce mode over sharding.landmark_ranges; a list of
    separator super-blocks: ssba_set_partition over sharding.ranges_for_separators), env (variables the library reads at
    finalize, set for this case only).  Floats go through JSON, which round-trips them exactly."""
    import torch
    from ceres_slam_amd import capi, sharding
    from ceres_slam_amd.solver import StereoBA
    torch.cuda.set_device(0)
    results = []
    for case in json.loads(os.environ["SSBA_TEST_CASES"]):
        prob, lighting, shared_free = _step_problem(mode, size, case)
        huber = float(case.get("huber", 0.0))
        ranges = partition = None
        if case.get("partition") is not None:
            partition = np.asarray(case["partition"], dtype=np.uint32)
            ranges = sharding.ranges_for_separators(prob.obs_pose, prob.obs_point, prob.num_poses, prob.num_points, partition)
        shard = sharding.shard_by_landmarks(prob, world, rank, ranges=ranges)
        if partition is not None:       # pose 0 is constant: free index = pose - 1, twelve per super-block
            sb = (shard.obs_pose[shard.obs_pose > 0].astype(np.int64) - 1) // 12
            assert sb.min() >= partition[rank] and sb.max() <= partition[rank + 1], (rank, int(sb.min()), int(sb.max()), partition.tolist())
        lt = None
        if lighting is not None:
            sel = np.isin(prob.obs_point, shard.point_ids)
            lt = dict(lighting, normals=lighting["normals"][shard.point_ids], material_of_point=lighting["material_of_point"][shard.point_ids],
                      intensity=lighting["intensity"][sel], normal_obs=lighting["normal_obs"][sel])
        saved = {k: os.environ.get(k) for k in case.get("env") or {}}
        os.environ.update(case.get("env") or {})
        try:
            ba = StereoBA(prob.camera, shard.poses, shard.points, shard.obs_pose, shard.obs_point, shard.obs_uvd, prob.stiffness(), device=0,
                          world_size=world, rank=rank, partition=partition, huber_a=huber, lighting=lt, shared_free=shared_free)
        finally:
            for k, v in saved.items():
                if v is None:
                    del os.environ[k]
                else:
                    os.environ[k] = v
        sharding.attach_torch_exchange(ba, dist)
        res = {"tag": case.get("tag"), "point_ids": shard.point_ids.tolist()}
        st = ba.stats()
        res["stats"] = {k: int(getattr(st, k)) for k in ("wide_superblocks", "general_structure", "num_free_poses", "num_superblocks",
                                                         "pcr_blocks", "pcr_fused")}
        try:
            s, log = ba.solve(capi.default_options(max_num_iterations=1, initial_trust_region_radius=float(case["radius"]),
                                                   trust_region_strategy_type=int(case.get("strategy", 0)),
                                                   dogleg_type=int(case.get("dogleg", 0))))
            res.update(status=0, termination=int(s.termination_type), num_iterations=int(s.num_iterations),
                       log={k: np.asarray(v, np.float64).tolist() for k, v in log.items()},
                       poses=ba.poses.tolist(), points=ba.points.tolist())
            if lt is not None:
                res.update(normals=ba.normals.tolist(), light=np.asarray(ba.light).tolist(), phong=np.asarray(ba.phong).tolist(),
                           texture=np.asarray(ba.texture).tolist())
        except capi.SsbaError as e:     # a combination ssba_solve_begin refuses: the status it documents, on every rank alike
            res.update(status=int(e.status), message=str(e))
        ba.close()
        results.append(res)
    with open(f"{out}.{rank}.json", "w") as f:
        json.dump({"rank": rank, "cases": results}, f)
    dist.barrier()
    dist.destroy_process_group()


def main():
    mode, out = sys.argv[1], sys.argv[2]
    import torch
    import torch.distributed as dist
    from ceres_slam_amd import sharding, synth
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    import datetime
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=180))
    P, Lm, T = [int(v) for v in os.environ.get("SSBA_TEST_SIZE", "16,400,6").split(",")]
    if mode in ("step", "step_phongfree"):
        return _step_mode(mode, out, rank, world, dist, (P, Lm, T))
    huber_a = float(os.environ.get("SSBA_TEST_HUBER", "0"))      # with it: 30 % outlier observations (BASELINE.json configs[4])
    lighting = None
    shared_free = 0
    pose_factors = None
    use_bounds = False
    if mode.endswith("_phong") or mode.endswith("_phongfree") or mode.endswith("_phongfreeb"):     # BASELINE.json configs[2] sharded: lighting terms of a landmark live on its rank
        use_bounds = mode.endswith("b")        # tests/dataset_ba_phong.cpp:142-180: bounds on the Phong and texture blocks -> projected line search
        shared_free = 7 if (mode.endswith("free") or use_bounds) else 0
        mode = mode[:mode.rindex("_")]
        prob, ph = synth.make_phong_problem(P, Lm, track_len=T, seed=21)
        # shared light / Phong / texture blocks constant, or free (their border sums ride next to the reduced system)
        lighting = ph.as_oracle_dict("perturbed" if shared_free else "truth")
    elif mode.endswith("_sun"):        # unary pose residual blocks (pose prior + sun sensor, tests/dataset_vo_sun.cpp:80-124), no constant pose
        mode = mode[:mode.rindex("_")]
        from test_oracle_pose_factors import _sun_problem
        prob, pose_factors = _sun_problem(P=P, L=Lm, seed=5, huber=huber_a)
        huber_a = 0.0
    else:
        prob = synth.make_problem(P, Lm, track_len=T, seed=21, outlier_fraction=0.3 if huber_a > 0 else 0.0)
    partition = None
    if mode == "gpu_part":      # super-block-aligned landmark ranges + partitioned reduced solve
        cut = sharding.aligned_partition(prob.obs_pose, prob.obs_point, prob.num_poses, prob.num_points, world)
        if cut is None:         # no super-block-aligned cut exists: plain landmark sharding, whole reduced system summed (as bench.py does)
            shard = sharding.shard_by_landmarks(prob, world, rank)
        else:
            ranges, partition = cut
            shard = sharding.shard_by_landmarks(prob, world, rank, ranges=ranges)
    else:
        shard = sharding.shard_by_landmarks(prob, world, rank)
    res = {"rank": rank, "num_local_obs": int(shard.obs_pose.shape[0]), "num_local_points": int(shard.points.shape[0])}
    if mode == "cpu":
        from oracle import oracle as orc     # checker as compute: this is a test of the host logic
        op = orc.OracleProblem(prob.camera, shard.poses, shard.points, shard.obs_pose, shard.obs_point,
                               shard.obs_uvd, prob.stiffness())
        cost, g_p, g_l, H_pp, H_ll = op.linearize()
        buf = torch.from_numpy(np.concatenate([[cost], g_p.ravel(), H_pp.ravel()]))
        dist.all_reduce(buf, op=dist.ReduceOp.SUM)
        gmax = torch.tensor([np.abs(g_l).max()], dtype=torch.float64)
        dist.all_reduce(gmax, op=dist.ReduceOp.MAX)
        res.update(cost=float(buf[0]), g_p=buf[1:1 + g_p.size].tolist(), H_pp_trace=float(np.trace(buf[1 + g_p.size:].numpy().reshape(-1, 6, 6).sum(0))),
                   gmax_l=float(gmax[0]))
    else:
        from ceres_slam_amd import capi
        from ceres_slam_amd.solver import StereoBA
        torch.cuda.set_device(0)
        lt = None
        if lighting is not None:        # this rank's landmarks and observations
            sel = np.isin(prob.obs_point, shard.point_ids)
            lt = dict(lighting, normals=lighting["normals"][shard.point_ids], material_of_point=lighting["material_of_point"][shard.point_ids],
                      intensity=lighting["intensity"][sel], normal_obs=lighting["normal_obs"][sel])
        ba = StereoBA(prob.camera, shard.poses, shard.points, shard.obs_pose, shard.obs_point, shard.obs_uvd,
                      prob.stiffness(), device=0, world_size=world, rank=rank, partition=partition, huber_a=huber_a, lighting=lt,
                      shared_free=shared_free, use_bounds=use_bounds, pose_factors=pose_factors,
                      pose_const=np.zeros(prob.num_poses, dtype=np.uint8) if pose_factors else None)
        sharding.attach_torch_exchange(ba, dist)
        okw = dict(max_num_iterations=int(os.environ.get("SSBA_TEST_MAXIT", "1000")), use_nonmonotonic_steps=1)
        if "SSBA_TEST_DOGLEG" in os.environ:        # 0 TRADITIONAL_DOGLEG, 1 SUBSPACE_DOGLEG (tests/dataset_ba_phong.cpp:85-86)
            okw.update(trust_region_strategy_type=1, dogleg_type=int(os.environ["SSBA_TEST_DOGLEG"]))
        s, log = ba.solve(capi.default_options(**okw))
        res.update(termination=int(s.termination_type), num_iterations=int(s.num_iterations),
                   final_cost=float(s.final_cost), initial_cost=float(s.initial_cost), cost=log["cost"].tolist(),
                   poses=ba.poses.tolist(), points=ba.points.tolist(), point_ids=shard.point_ids.tolist(),
                   partition=None if partition is None else partition.tolist(), accept=log["step_is_successful"].tolist(),
                   gmax=log["gradient_max_norm"].tolist(), step_norm=log["step_norm"].tolist())
        if use_bounds:
            res["line_search_steps"] = int(s.num_line_search_steps)
        if lt is not None:
            res["normals"] = ba.normals.tolist()
            res["light"] = np.asarray(ba.light).tolist()
            res["phong"] = np.asarray(ba.phong).tolist()
            res["texture"] = np.asarray(ba.texture).tolist()
    with open(f"{out}.{rank}.json", "w") as f:
        json.dump(res, f)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
