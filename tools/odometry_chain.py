"""Odometry blocks between consecutive states on C2: ms per solver iteration with and without the 999-block chain.

BASELINE C2 (1 000 poses / 100 000 landmarks) plus one RelativePoseErrorAutomatic block between every pair of consecutive
states and the prior that holds the gauge (synth.make_odometry_factors), through the public Python API.  The chain keeps
the windowed layout (ssba_stats.general_structure == 0); a build of the library from before that rule lays the same
problem out on the general path, which is what --library is for: the same script, generator and Python layer time another
commit's libssba.so (the C ABI is the same).  SSBA_FORCE_DENSE=1 in the environment selects the general layout of this build.

    python tools/odometry_chain.py --label windowed
    python tools/odometry_chain.py --label plain_c2 --no-chain
    python tools/odometry_chain.py --label parent_general --library <other build>/libssba.so
    python tools/odometry_chain.py --label windowed_kernels --kernel-timing      # HIP events around every launch: a run of its own

Timed like bench.py's region: one solve to convergence (warm-up, gives the restart period), ssba_solve_begin with
ignore_convergence, the graph captures, --warmup steps, then --repeats windows of --steps iterations, each between two
device synchronisations, restarting from the initial values every period.  Every invocation adds its windows to the
label's samples in --out (profiles/odometry_chain.json): run the labels alternately to see the spread between them.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", required=True)
    ap.add_argument("--poses", type=int, default=1000)
    ap.add_argument("--landmarks", type=int, default=100000)
    ap.add_argument("--no-chain", action="store_true", help="the same problem without the relative-pose blocks (state 0 constant)")
    ap.add_argument("--huber", type=float, default=0.0, help="HuberLoss scale on the relative-pose blocks")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kernel-timing", action="store_true", help="per-kernel-class HIP-event times instead of the graph-replay windows")
    ap.add_argument("--library", default=None, help="time this libssba.so instead of the tree's")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "odometry_chain.json"))
    args = ap.parse_args()

    import numpy as np
    from ceres_slam_amd import capi, synth
    if args.library:
        capi.LIB_PATH = os.path.abspath(args.library)
    from ceres_slam_amd.solver import StereoBA

    prob = synth.make_problem(args.poses, args.landmarks, track_len=12)
    if args.no_chain:
        ba = StereoBA.from_synth(prob)
    else:
        ba = StereoBA(prob.camera, prob.poses_init.copy(), prob.points_init.copy(), prob.obs_pose, prob.obs_point, prob.obs_uvd, prob.stiffness(),
                      pose_const=np.zeros(prob.num_poses, np.uint8), pose_factors=synth.make_odometry_factors(prob, huber=args.huber))
    st = ba.stats()
    opts = capi.default_options(max_num_iterations=1000, use_nonmonotonic_steps=1)
    s, _ = ba.solve(opts)
    period = max(int(s.num_iterations) - 1, 1)
    ba.poses[:] = prob.poses_init
    ba.points[:] = prob.points_init

    def run(n):
        done = 0
        while done < n:
            if done and done % period == 0:
                ba.restart()
            k = min(n - done, period - done % period)
            ba.step(k)
            done += k

    ba.solve_begin(opts, ignore_convergence=True)
    ba.step(17)             # captures the two graphs the production path replays (see bench.py)
    ba.synchronize()
    ba.restart()
    run(args.warmup)
    ba.synchronize()
    samples, kernels = [], None
    if args.kernel_timing:
        ba.restart()
        ba.set_kernel_timing(True)
        run(args.steps)
        ba.synchronize()
        kernels = {k: round(ms / args.steps, 5) for k, (n, ms) in sorted(ba.kernel_times().items()) if n}
    else:
        for _ in range(args.repeats):
            ba.restart()
            ba.synchronize()
            t0 = time.perf_counter()
            run(args.steps)
            ba.synchronize()
            samples.append(round(1e3 * (time.perf_counter() - t0) / args.steps, 5))
    ba.solve_end()

    doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
    doc.setdefault("tool", "tools/odometry_chain.py")
    doc.setdefault("runs", {})
    r = doc["runs"].setdefault(args.label, {})
    r.update(poses=args.poses, landmarks=args.landmarks, chain=not args.no_chain, relative_pose_blocks=0 if args.no_chain else args.poses - 1,
             huber=args.huber, library="tree" if not args.library else "--library", steps=args.steps, warmup=args.warmup,
             general_structure=int(st.general_structure), solve_iterations=int(s.num_iterations), final_cost=float(s.final_cost),
             stats={k: int(getattr(st, k)) for k in ("num_free_poses", "num_active_points", "num_observations", "num_windows", "num_superblocks",
                                                     "num_reduced_blocks", "pose_bandwidth", "pcr_blocks", "pcr_fused")})
    if kernels is not None:
        r["kernel_ms_per_iteration"] = kernels
        r["kernel_ms_sum"] = round(sum(kernels.values()), 5)
    else:
        r["ms_per_iteration_samples"] = r.get("ms_per_iteration_samples", []) + samples
        a = r["ms_per_iteration_samples"]
        r["ms_per_iteration"] = dict(median=round(statistics.median(a), 5), min=min(a), max=max(a), windows=len(a))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps({"label": args.label, **{k: v for k, v in r.items() if k != "stats"}}), flush=True)


if __name__ == "__main__":
    main()
