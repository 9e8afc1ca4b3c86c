"""A stereo sequence prepared once against pair by pair: writes profiles/image_sequence.json.

Shapes (synth.make_stereo_sequence):
  a   F = 17 frames of 310 x 93, three levels, the matcher at level 0 with D 64 and block 15 (the driver's size; one chunk)
  b   F = 5 frames of 1242 x 375, D 128, block 15, the default workspace: one pair per chunk, so the matcher chunks
Per shape, alternating, three windows each after one warm-up window; wall time around calls that end in a synchronise:
  sequence     one ImageSequence.create over the F frames                          against
  pairs        F - 1 ImagePyramid.create_stereo(left_k, right_k, left_k+1) calls
  sgbm_batch   one stereo_sgbm_batch over the F - 1 pairs                          against
  sgbm_solo    F - 1 stereo_sgbm calls
Reported: the median window of each in ms, the ratio, and the spread (max - min over the windows) of each.

--parent-tree DIR: the pair-by-pair side runs in a child process on the package and library found in DIR (a checkout of the parent
commit with its own build), taking turns with this build window by window.  Without it that side runs on this build.

--example EXE RAW: the whole-process time of examples/dense_stereo_sequence_gpu on the file RAW (written by --write-raw) with and
without --sequence, three alternating windows after one warm-up each.

Per-kernel medians come from a run of their own (no counters with it):
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/image_sequence_bench.py --trace-run
    python tools/image_sequence_bench.py --merge-trace DIR/.../*_kernel_trace.csv      # medians per kernel into the JSON (no GPU)

    python tools/image_sequence_bench.py [--out profiles/image_sequence.json] [--shapes a,b] [--parent-tree DIR] [--example EXE RAW]"""
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
from ceres_slam_amd.solver import ImagePyramid, stereo_sgbm  # noqa: E402

SHAPES = {"a": dict(frames=17, rows=93, cols=310, levels=3, params=dict(num_disparities=64, block_size=15)),
          "b": dict(frames=5, rows=375, cols=1242, levels=3, params=dict(num_disparities=128, block_size=15))}
KW = dict(disparity_level=0, gradient_source=capi.GRADIENT_OF_TRACKED, gradient_scale=0.125)


def frames_of(name):
    s = SHAPES[name]
    return synth.make_stereo_sequence(s["rows"], s["cols"], s["frames"], seed=10, motion=1.0, min_wavelength_px=8.0)


def run_pairs(seq, name):
    s = SHAPES[name]
    t = time.perf_counter()
    pyrs = [ImagePyramid.create_stereo(seq.left[k], seq.right[k], seq.left[k + 1], s["levels"], params=s["params"], **KW) for k in range(s["frames"] - 1)]
    dt = time.perf_counter() - t
    for p in pyrs:
        p.close()
    return dt


def run_sgbm_solo(seq, name):
    s = SHAPES[name]
    t = time.perf_counter()
    for k in range(s["frames"] - 1):
        stereo_sgbm(seq.left[k], seq.right[k], **s["params"])
    return time.perf_counter() - t


def run_sequence(seq, name):
    from ceres_slam_amd.solver import ImageSequence
    s = SHAPES[name]
    t = time.perf_counter()
    q = ImageSequence.create(seq.left, seq.right, s["levels"], params=s["params"], **KW)
    dt = time.perf_counter() - t
    q.close()
    return dt


def run_sgbm_batch(seq, name):
    from ceres_slam_amd.solver import stereo_sgbm_batch
    s = SHAPES[name]
    t = time.perf_counter()
    stereo_sgbm_batch(seq.left[:-1], seq.right[:-1], **s["params"])
    return time.perf_counter() - t


def worker():
    """Child process of --parent-tree: 'make a' renders the frames, 'pairs' / 'sgbm' answer the seconds of one window."""
    seq, name = None, None
    for line in sys.stdin:
        w = line.split()
        if not w or w[0] == "quit":
            break
        if w[0] == "make":
            name = w[1]
            seq = frames_of(name)
            print("ok", flush=True)
        elif w[0] == "pairs":
            print(repr(run_pairs(seq, name)), flush=True)
        elif w[0] == "sgbm":
            print(repr(run_sgbm_solo(seq, name)), flush=True)


class PairByPair:
    """The pair-by-pair side: in this process, or in a child on another tree."""

    def __init__(self, tree):
        self.child = None
        if tree:
            env = dict(os.environ, SSBA_BENCH_ROOT=os.path.abspath(tree))
            self.child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker"], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=env)

    def ask(self, msg):
        self.child.stdin.write(msg + "\n")
        self.child.stdin.flush()
        return self.child.stdout.readline().strip()

    def make(self, name, seq):
        self.seq, self.name = seq, name
        if self.child:
            assert self.ask(f"make {name}") == "ok"

    def pairs(self):
        return float(self.ask("pairs")) if self.child else run_pairs(self.seq, self.name)

    def sgbm(self):
        return float(self.ask("sgbm")) if self.child else run_sgbm_solo(self.seq, self.name)

    def close(self):
        if self.child:
            self.child.stdin.write("quit\n")
            self.child.stdin.flush()
            self.child.wait(timeout=60)


def compare(new, old, label_new, label_old):
    new(), old()                                   # warm-up window
    tn, to = [], []
    for _ in range(3):
        tn.append(new())
        to.append(old())
    mn, mo = sorted(tn)[1], sorted(to)[1]
    sn, so = max(tn) - min(tn), max(to) - min(to)
    return {label_new + "_ms": mn * 1e3, label_old + "_ms": mo * 1e3, "ratio_" + label_old + "_over_" + label_new: mo / mn,
            label_new + "_spread_ms": sn * 1e3, label_old + "_spread_ms": so * 1e3,
            "faster_outside_three_spreads": bool(mo - mn > 3 * max(sn, so)),
            label_new + "_windows_s": tn, label_old + "_windows_s": to}


def run_example(exe, raw, extra):
    t = time.perf_counter()
    r = subprocess.run([exe, raw] + extra, capture_output=True, timeout=300)
    dt = time.perf_counter() - t
    if r.returncode != 0:
        raise SystemExit(r.stdout.decode() + r.stderr.decode())
    return dt, r.stdout


def summarise_trace(path):
    """Median duration (us) of every pyramid and matcher kernel in a rocprofv3 kernel trace."""
    acc = collections.defaultdict(list)
    for row in csv.DictReader(open(path)):
        name = row["Kernel_Name"].split("(")[0].split("::")[-1].split("<")[0]
        if name.startswith(("k_sgbm_", "k_pyr_")):
            acc[name].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return {k: dict(median_us=statistics.median(v), total_us=sum(v), launches=len(v)) for k, v in sorted(acc.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_sequence.json"))
    ap.add_argument("--shapes", default="a,b")
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--write-raw", metavar="RAW", default=None, help="write shape a as the file the example reads, and stop")
    ap.add_argument("--example", nargs=2, metavar=("EXE", "RAW"), default=None)
    ap.add_argument("--trace-run", action="store_true", help="shape a once each way, after a warm-up of each: for rocprofv3")
    ap.add_argument("--merge-trace", metavar="CSV", default=None)
    a = ap.parse_args()
    if a.worker:
        return worker()
    if a.write_raw:
        s = SHAPES["a"]
        synth.write_stereo_sequence(a.write_raw, frames_of("a"), s["levels"], 0, bytes(capi.sgbm_params(**s["params"])))
        return
    if a.merge_trace:
        doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
        doc["kernels_shape_a"] = summarise_trace(a.merge_trace)
        doc["kernel_times_from"] = "rocprofv3 --kernel-trace --stats, a run of its own: two ImageSequence.create and two rounds of 16 create_stereo calls"
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        print(json.dumps(doc["kernels_shape_a"], indent=1))
        return
    if a.trace_run:
        seq = frames_of("a")
        for _ in range(2):
            run_sequence(seq, "a")
            run_pairs(seq, "a")
        return
    old = PairByPair(a.parent_tree)
    doc = dict(pair_by_pair_side="parent tree, child process" if a.parent_tree else "this build", shapes={})
    if os.path.exists(a.out):
        doc.update({k: v for k, v in json.load(open(a.out)).items() if k.startswith("kernel")})
    for name in a.shapes.split(","):
        s = SHAPES[name]
        seq = frames_of(name)
        old.make(name, seq)
        row = dict(s, pair_bytes=capi.sgbm_pair_bytes(s["rows"], s["cols"], s["params"]["num_disparities"]),
                   pairs_per_chunk=capi.sgbm_chunk_pairs(s["frames"] - 1, 0, s["rows"], s["cols"], s["params"]["num_disparities"]))
        row["create"] = compare(lambda: run_sequence(seq, name), old.pairs, "sequence", "pairs")
        row["matcher"] = compare(lambda: run_sgbm_batch(seq, name), old.sgbm, "sgbm_batch", "sgbm_solo")
        doc["shapes"][name] = row
        print(name, json.dumps({k: {x: y for x, y in v.items() if not x.endswith("_s")} for k, v in row.items() if isinstance(v, dict) and k != "params"}),
              flush=True)
    old.close()
    if a.example:
        exe, raw = a.example
        base = run_example(exe, raw, [])[1]
        assert run_example(exe, raw, ["--sequence"])[1] == base, "--sequence printed other bytes"
        doc["example_shape_a"] = compare(lambda: run_example(exe, raw, ["--sequence"])[0], lambda: run_example(exe, raw, [])[0], "with_sequence", "default")
        print("example", json.dumps({k: v for k, v in doc["example_shape_a"].items() if not k.endswith("_s")}), flush=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
