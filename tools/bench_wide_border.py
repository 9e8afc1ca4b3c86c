"""Time the Phong driver's configuration (free light / Phong / texture blocks, bounds, SUBSPACE_DOGLEG, non-monotonic steps) at
C3 size (1 000 poses / 100 000 landmarks) for several material counts: M = 7 is the widest border of one panel (31 columns),
M >= 8 takes two panels (3 + 4M columns, ssba_border.hip).  The protocol of bench.py: one solve to convergence gives the
restart period, the production graphs are captured, `--warmup` iterations, then `--steps` timed iterations between
synchronisations, restarting from the initial values every period.  One JSON line per M on stdout.

    python tools/bench_wide_border.py [--materials 7 8 12 15] [--steps 200] [--warmup 20]

Under rocprofv3 keep one M per process and --steps 20 --warmup 5: the profiler faults past 16 384 graph-replayed dispatches
in a process, and a two-panel iteration replays about a hundred."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(M, steps, warmup, P=1000, L=100_000):
    from ceres_slam_amd import capi, synth
    from ceres_slam_amd.solver import StereoBA
    prob, ph = synth.make_phong_problem(P, L, num_materials=M)
    d = ph.as_oracle_dict("perturbed")
    ba = StereoBA.from_synth(prob, lighting=d, shared_free=7, use_bounds=True)
    opts = capi.default_options(max_num_iterations=1000, use_nonmonotonic_steps=1, trust_region_strategy_type=1, dogleg_type=1)
    s_conv, _ = ba.solve(opts)
    period = max(int(s_conv.num_iterations) - 1, 1)

    def reset_params():
        ba.poses[:] = prob.poses_init
        ba.points[:] = prob.points_init
        ba.normals[:] = d["normals"]
        ba.phong[:], ba.texture[:], ba.light[:] = d["phong"], d["texture"], d["light"]

    def run(n):
        done = 0
        while done < n:
            if done and done % period == 0:
                ba.restart()
            k = min(n - done, period - done % period)
            ba.step(k)
            done += k

    reset_params()
    ba.set_kernel_timing(False)
    ba.solve_begin(opts, ignore_convergence=True)
    ba.step(17)          # captures the batched and the single-iteration graphs (bench.py)
    ba.synchronize()
    ba.restart()
    run(warmup)
    ba.synchronize()
    ba.restart()
    ba.synchronize()
    t0 = time.perf_counter()
    run(steps)
    ba.synchronize()
    dt = time.perf_counter() - t0
    ba.solve_end()
    nb = ba.border_system()[0].shape[1]
    ba.close()
    return {"config": "C3 driver configuration (shared_free=7, bounds, SUBSPACE_DOGLEG, non-monotonic)", "poses": P, "landmarks": L,
            "materials": M, "border_columns": nb, "panels": 2 if nb > 32 else 1, "steps": steps, "warmup": warmup,
            "ms_per_step": 1e3 * dt / steps, "restart_period_iters": period, "solve_iterations": int(s_conv.num_iterations),
            "final_cost": float(s_conv.final_cost), "line_search_evaluations": int(s_conv.num_line_search_steps),
            # the line-search work per iteration differs between the problems (it is not a property of the border route)
            "line_search_evaluations_per_iteration": int(s_conv.num_line_search_steps) / max(int(s_conv.num_iterations), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--materials", type=int, nargs="+", default=[7, 8, 12, 15])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    for M in args.materials:
        print(json.dumps(measure(M, args.steps, args.warmup)), flush=True)


if __name__ == "__main__":
    main()
