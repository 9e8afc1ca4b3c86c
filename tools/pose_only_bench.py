"""Pose-only layout against the windowed route of the same library, at C2's shape with every point constant.

BASELINE C2 (1 000 poses / 100 000 landmarks / track 12), every point block held constant (localisation against a fixed map),
Levenberg-Marquardt, through the public Python API.  Two handles in one process: the pose-only layout
(ssba_stats.general_structure == 3: k_po_step . k_po_eval . k_decide . k_best) and, with SSBA_NO_POSE_ONLY=1 at ssba_finalize,
the windowed layout with every landmark flagged constant (12 launches, Schur and reduction steps on zeros).

    python tools/pose_only_bench.py

Per handle: one solve to convergence (warm-up; gives the restart period, the same for both routes), ssba_solve_begin with
ignore_convergence, the graph captures, --warmup steps.  Then --rounds rounds in which the two routes take turns: --steps
graph-replayed iterations between two device events on the handle's stream, restarting from the initial values every period
(the solve converges in three iterations, so the restart -- six device copies and the state reset -- is inside the window
every second iteration, for both routes alike; --period N times N iterations per restart instead, steps after convergence
included).  Result: profiles/pose_only_c2.json and one JSON line.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Hip:
    def __init__(self):
        self.lib = C.CDLL("libamdhip64.so")

    def check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what}: hipError {rc}")

    def stream(self):
        s = C.c_void_p()
        self.check(self.lib.hipStreamCreate(C.byref(s)), "hipStreamCreate")
        return s

    def event(self):
        e = C.c_void_p()
        self.check(self.lib.hipEventCreate(C.byref(e)), "hipEventCreate")
        return e

    def record(self, e, s):
        self.check(self.lib.hipEventRecord(e, s), "hipEventRecord")

    def elapsed_ms(self, a, b):
        self.check(self.lib.hipEventSynchronize(b), "hipEventSynchronize")
        ms = C.c_float()
        self.check(self.lib.hipEventElapsedTime(C.byref(ms), a, b), "hipEventElapsedTime")
        return float(ms.value)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=1000)
    ap.add_argument("--landmarks", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--period", type=int, default=0, help="iterations per restart (default: the solve's own iteration count - 1)")
    ap.add_argument("--kernel-timing", action="store_true", help="per-kernel-class HIP-event times of one window per route instead (a run of its own)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_only_c2.json"))
    args = ap.parse_args()

    import numpy as np
    from ceres_slam_amd import capi, synth
    from ceres_slam_amd.solver import StereoBA

    hip = Hip()
    prob = synth.make_problem(args.poses, args.landmarks, track_len=12)
    opts = capi.default_options(max_num_iterations=1000, use_nonmonotonic_steps=1)
    runs = {}
    for name, env in (("pose_only", "0"), ("windowed", "1")):
        os.environ["SSBA_NO_POSE_ONLY"] = env
        ba = StereoBA.from_synth(prob, points_const=True)
        os.environ.pop("SSBA_NO_POSE_ONLY")
        st = ba.stats()
        assert st.general_structure == (3 if name == "pose_only" else 0), st.general_structure
        stream = hip.stream()
        ba.set_stream(stream.value)
        s, _ = ba.solve(opts)
        period = args.period or max(int(s.num_iterations) - 1, 1)
        ba.poses[:] = prob.poses_init
        ba.solve_begin(opts, ignore_convergence=True)
        ba.step(17)             # captures the two graphs the production path replays (see bench.py)
        ba.synchronize()
        runs[name] = dict(ba=ba, stream=stream, period=period, samples=[], a=hip.event(), b=hip.event(), general_structure=int(st.general_structure),
                          solve_iterations=int(s.num_iterations), final_cost=float(s.final_cost), device_bytes=int(st.device_bytes))

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
    kernels = {}
    if args.kernel_timing:
        for name, r in runs.items():
            r["ba"].restart()
            r["ba"].set_kernel_timing(True)
            run(r, args.steps)
            r["ba"].synchronize()
            kernels[name] = {k: dict(launches_per_iteration=round(n / args.steps, 3), ms_per_iteration=round(ms / args.steps, 5))
                             for k, (n, ms) in sorted(r["ba"].kernel_times().items()) if n}
    else:
        for _ in range(args.rounds):
            for r in runs.values():
                r["ba"].restart()
                r["ba"].synchronize()
                hip.record(r["a"], r["stream"])
                run(r, args.steps)
                hip.record(r["b"], r["stream"])
                r["samples"].append(round(hip.elapsed_ms(r["a"], r["b"]) / args.steps, 5))
    doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
    doc.update(tool="tools/pose_only_bench.py", poses=args.poses, landmarks=args.landmarks, observations=int(prob.num_obs), steps=args.steps, warmup=args.warmup)
    doc.setdefault("runs", {})
    for name, r in runs.items():
        r["ba"].solve_end()
        e = doc["runs"].setdefault(name, {})
        e.update(general_structure=r["general_structure"], solve_iterations=r["solve_iterations"], final_cost=r["final_cost"], device_bytes=r["device_bytes"])
        if args.kernel_timing:
            e["kernel_classes"] = kernels[name]
        else:
            a = r["samples"]
            e.update(restart_period=r["period"], ms_per_iteration_samples=a, ms_per_iteration=dict(median=round(statistics.median(a), 5), min=min(a), max=max(a), windows=len(a)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps({k: (v.get("kernel_classes") if args.kernel_timing else v["ms_per_iteration_samples"]) for k, v in doc["runs"].items()}), flush=True)


if __name__ == "__main__":
    main()
