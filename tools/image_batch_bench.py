"""Batched against sequential dense alignment at the driver's size: writes profiles/image_batch.json.

n handles of make_image_pair(94, 310, seed = k), BILINEAR, free and constant disparities.  Per configuration and n = 1, 4, 16, 64:
  batch        one ssba_image_solve_batch(ignore_convergence, max_num_iterations = ITERS) over the n handles
  sequential   the same n handles one after another: ssba_solve_begin / ssba_solve_step(ITERS) / ssba_solve_end
alternating, three windows each after a warm-up window of WARMUP iterations; wall time around the calls (each ends in a
synchronise).  Reported: ms per (handle . iteration) of both, their ratio, and the spread (max - min over the windows) of each.
These are FORCED-ITERATION figures: nothing terminates, no termination word is read, ten rounds go into one graph replay.

--parent-tree DIR: the sequential side runs in a child process on the package and library found in DIR (a checkout of the parent
commit with its own build), alternating with the batch of this build window by window.  Without it the sequential side runs on
this build, whose solo kernels are those of the parent.

"converging" rows: the loop every real solve takes (one round per replay, the termination words copied and awaited one round
behind): n = 16 handles, max_num_iterations = 50, one ssba_image_solve_batch against 16 ssba_solve calls; wall ms per call.

Per-kernel medians come from a run of their own (no counters with it):
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/image_batch_bench.py --trace-run --out /dev/null
    python tools/image_batch_bench.py --merge-trace DIR/.../*_kernel_trace.csv       # medians per kernel into the JSON (no GPU)

    python tools/image_batch_bench.py [--out profiles/image_batch.json] [--iters 200] [--warmup 20] [--parent-tree DIR]"""
import argparse
import collections
import csv
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.environ.get("SSBA_BENCH_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ceres_slam_amd import capi, synth  # noqa: E402
from ceres_slam_amd.solver import ImageAlignment  # noqa: E402


def handles(n, const):
    out = []
    for k in range(n):
        pair = synth.make_image_pair(94, 310, seed=k)
        out.append((pair, ImageAlignment.from_synth(pair, interpolation=capi.IMAGE_BILINEAR, disparity_const=const)))
    return out


def reset(hs):
    for pair, h in hs:
        h.pose[:] = pair.pose_init
        h.disparity[:] = pair.disparity


def run_batch(hs, iters, forced=True):
    from ceres_slam_amd.solver import solve_image_batch
    reset(hs)
    o = capi.default_options(max_num_iterations=iters, use_nonmonotonic_steps=1)
    t = time.perf_counter()
    solve_image_batch([h for _, h in hs], o, ignore_convergence=forced)
    return time.perf_counter() - t


def run_sequential(hs, iters, forced=True):
    reset(hs)
    o = capi.default_options(max_num_iterations=iters, use_nonmonotonic_steps=1)
    t = time.perf_counter()
    for _, h in hs:
        if forced:
            h.solve_begin(o, ignore_convergence=True)
            h.step(iters)
            h.solve_end()
        else:
            h.solve(o)
    return time.perf_counter() - t


def worker():
    """Child process of --parent-tree: 'make n const' builds the handles, 'run iters forced' answers the seconds of one window."""
    hs = []
    for line in sys.stdin:
        w = line.split()
        if not w or w[0] == "quit":
            break
        if w[0] == "make":
            for _, h in hs:
                h.close()
            hs = handles(int(w[1]), w[2] == "1")
            print("ok", flush=True)
        elif w[0] == "run":
            print(repr(run_sequential(hs, int(w[1]), w[2] == "1")), flush=True)


class Sequential:
    """The sequential side: in this process, or in a child on another tree."""

    def __init__(self, tree):
        self.child = None
        self.hs = []
        if tree:
            env = dict(os.environ, SSBA_BENCH_ROOT=os.path.abspath(tree))
            self.child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker"], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=env)

    def ask(self, msg):
        self.child.stdin.write(msg + "\n")
        self.child.stdin.flush()
        return self.child.stdout.readline().strip()

    def make(self, n, const, own):
        if self.child:
            assert self.ask(f"make {n} {int(const)}") == "ok"
        else:
            self.hs = own

    def run(self, iters, forced=True):
        if self.child:
            return float(self.ask(f"run {iters} {int(forced)}"))
        return run_sequential(self.hs, iters, forced)

    def close(self):
        if self.child:
            self.child.stdin.write("quit\n")
            self.child.stdin.flush()
            self.child.wait(timeout=60)


def summarise_trace(path):
    """Median duration (us) of every k_imb_* / k_im_* kernel in a rocprofv3 kernel trace."""
    acc = collections.defaultdict(list)
    for row in csv.DictReader(open(path)):
        name = row["Kernel_Name"].split("(")[0].split("::")[-1]
        if name.startswith(("k_imb_", "k_im_", "k_decide", "k_best")):
            acc[name].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return {"n = 16, free disparities": {k: dict(median_us=statistics.median(v), launches=len(v)) for k, v in sorted(acc.items())}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_batch.json"))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sizes", default="1,4,16,64")
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--trace-run", action="store_true", help="one batch of 16 (free disparities, 60 forced iterations) and the same sequentially: for rocprofv3")
    ap.add_argument("--merge-trace", metavar="CSV", default=None)
    a = ap.parse_args()
    if a.worker:
        return worker()
    if a.merge_trace:
        doc = json.load(open(a.out))
        doc["kernels"] = summarise_trace(a.merge_trace)
        doc["kernel_times_from"] = "rocprofv3 --kernel-trace --stats, a run of its own"
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        print(json.dumps(doc["kernels"], indent=1))
        return
    if a.trace_run:
        hs = handles(16, False)
        run_batch(hs, 60)
        run_sequential(hs[:4], 60)
        return
    seq = Sequential(a.parent_tree)
    rows, conv = [], []
    for const in (False, True):
        for n in [int(x) for x in a.sizes.split(",")]:
            hs = handles(n, const)
            seq.make(n, const, hs)
            run_batch(hs, a.warmup)
            seq.run(a.warmup)
            tb, ts = [], []
            for _ in range(3):
                tb.append(run_batch(hs, a.iters))
                ts.append(seq.run(a.iters))
            per = 1e3 / (n * a.iters)
            mb, ms = sorted(tb)[1] * per, sorted(ts)[1] * per
            row = dict(disparities="constant" if const else "free", n=n, iterations=a.iters,
                       batch_ms_per_handle_iteration=mb, sequential_ms_per_handle_iteration=ms, ratio_sequential_over_batch=ms / mb,
                       batch_spread_ms=(max(tb) - min(tb)) * per, sequential_spread_ms=(max(ts) - min(ts)) * per,
                       batch_windows_s=tb, sequential_windows_s=ts)
            rows.append(row)
            print(json.dumps({k: v for k, v in row.items() if not k.endswith("_s")}), flush=True)
            if n == 16:      # the converging loop
                run_batch(hs, 50, False)
                seq.run(50, False)
                cb, cs = [], []
                for _ in range(3):
                    cb.append(run_batch(hs, 50, False))
                    cs.append(seq.run(50, False))
                c = dict(disparities="constant" if const else "free", n=n, max_num_iterations=50, batch_ms_per_call=sorted(cb)[1] * 1e3,
                         sequential_ms_for_the_n_solves=sorted(cs)[1] * 1e3, ratio_sequential_over_batch=sorted(cs)[1] / sorted(cb)[1],
                         batch_spread_ms=(max(cb) - min(cb)) * 1e3, sequential_spread_ms=(max(cs) - min(cs)) * 1e3)
                conv.append(c)
                print("converging", json.dumps(c), flush=True)
            for _, h in hs:
                h.close()
    seq.close()
    with open(a.out, "w") as f:
        json.dump(dict(shape="310x94", interpolation="BILINEAR", sequential_side="parent tree, child process" if a.parent_tree else "this build",
                       rows=rows, converging=conv), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
