"""Constant point blocks at C2 size: ms per solver iteration with no and with every third point held constant (every point
constant is another layout: tools/pose_only_bench.py).

BASELINE C2 (1 000 poses / 100 000 landmarks / track 12) through the public Python API, Levenberg-Marquardt.  A handle without
constant points launches the kernels it always launched; a handle with some launches their CP instantiations
(DESIGN.md section 4.2a), the same number of launches.  This script says what those cost.

    python tools/const_points_bench.py

Timed like tools/odometry_chain.py: per mask one solve to convergence (warm-up, gives the restart period), ssba_solve_begin with
ignore_convergence, the graph captures, --warmup steps; then --rounds rounds in which the masks take turns, one window of
--steps graph-replayed iterations each, between two device synchronisations, restarting from the initial values every
period.  Result: profiles/const_points_c2.json and one JSON line.
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
    ap.add_argument("--poses", type=int, default=1000)
    ap.add_argument("--landmarks", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "const_points_c2.json"))
    args = ap.parse_args()

    import numpy as np
    from ceres_slam_amd import capi, synth
    from ceres_slam_amd.solver import StereoBA

    prob = synth.make_problem(args.poses, args.landmarks, track_len=12)
    L = prob.num_points
    masks = {"none": None, "every_third": np.arange(L) % 3 == 0}
    opts = capi.default_options(max_num_iterations=1000, use_nonmonotonic_steps=1)
    runs = {}
    for name, m in masks.items():
        ba = StereoBA.from_synth(prob, point_const=m)
        st = ba.stats()
        s, _ = ba.solve(opts)
        period = max(int(s.num_iterations) - 1, 1)
        ba.poses[:] = prob.poses_init
        ba.points[:] = prob.points_init
        ba.solve_begin(opts, ignore_convergence=True)
        ba.step(17)             # captures the two graphs the production path replays (see bench.py)
        ba.synchronize()
        runs[name] = dict(ba=ba, period=period, samples=[], general_structure=int(st.general_structure), solve_iterations=int(s.num_iterations),
                          final_cost=float(s.final_cost), constant_points=0 if m is None else int(m.sum()))

    def run(r, n):
        ba, period, done = r["ba"], r["period"], 0
        while done < n:
            if done and done % period == 0:
                ba.restart()
            k = min(n - done, period - done % period)
            ba.step(k)
            done += k

    for r in runs.values():
        r["ba"].restart()
        run(r, args.warmup)
        r["ba"].synchronize()
    for _ in range(args.rounds):
        for r in runs.values():
            r["ba"].restart()
            r["ba"].synchronize()
            t0 = time.perf_counter()
            run(r, args.steps)
            r["ba"].synchronize()
            r["samples"].append(round(1e3 * (time.perf_counter() - t0) / args.steps, 5))
    doc = dict(tool="tools/const_points_bench.py", poses=args.poses, landmarks=args.landmarks, steps=args.steps, warmup=args.warmup, runs={})
    for name, r in runs.items():
        r["ba"].solve_end()
        a = r["samples"]
        doc["runs"][name] = dict(constant_points=r["constant_points"], general_structure=r["general_structure"], solve_iterations=r["solve_iterations"],
                                 final_cost=r["final_cost"], restart_period=r["period"], ms_per_iteration_samples=a,
                                 ms_per_iteration=dict(median=round(statistics.median(a), 5), min=min(a), max=max(a), windows=len(a)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps({k: v["ms_per_iteration_samples"] for k, v in doc["runs"].items()}), flush=True)


if __name__ == "__main__":
    main()
