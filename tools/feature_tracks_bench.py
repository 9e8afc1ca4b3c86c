"""Feature tracks from raw frames (tracks.track_sequence): writes profiles/feature_tracks.json.

Shapes (synth.make_stereo_sequence, seed 10, min_wavelength_px 8, fast_threshold 10):
  a   F = 17 frames of 310 x 93, max_features 1000
  b   F = 5 frames of 1242 x 375, max_features 2048
  c2, c5, c17   F = 2, 5, 17 frames of 310 x 93: the launch count against F
Wall time: a host clock around track_sequence, which ends in a synchronise; one warm-up window, then three windows of --calls
calls each; reported are the median window per call in ms and the spread (max - min over the windows).  Nothing on the parent does
this work, so there is no ratio.

Per-kernel medians and launch counts come from runs of their own (no timing window in them):
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/feature_tracks_bench.py --trace-run a
    python tools/feature_tracks_bench.py --merge-trace a DIR/.../*_kernel_trace.csv      # into the JSON (no GPU)
--trace-run makes exactly ONE track_sequence call, so the rows of the trace are the launches of one call: the library's k_tr_*
kernels, and apart from them the copy kernels the HIP runtime itself launches for some of the transfers.

    python tools/feature_tracks_bench.py [--out profiles/feature_tracks.json] [--shapes a,b] [--calls 10]"""
import argparse
import collections
import csv
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ceres_slam_amd import synth, tracks  # noqa: E402

SHAPES = {"a": dict(frames=17, rows=93, cols=310, max_features=1000),
          "b": dict(frames=5, rows=375, cols=1242, max_features=2048),
          "c2": dict(frames=2, rows=93, cols=310, max_features=1000),
          "c5": dict(frames=5, rows=93, cols=310, max_features=1000),
          "c17": dict(frames=17, rows=93, cols=310, max_features=1000)}
FAST_THRESHOLD = 10


def frames_of(name):
    s = SHAPES[name]
    return synth.make_stereo_sequence(s["rows"], s["cols"], s["frames"], seed=10, motion=1.0, min_wavelength_px=8.0)


def run(seq, name):
    t = time.perf_counter()
    out = tracks.track_sequence(seq.left, seq.right, fast_threshold=FAST_THRESHOLD, max_features=SHAPES[name]["max_features"])
    return time.perf_counter() - t, out


def load(path):
    return json.load(open(path)) if os.path.exists(path) else {}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feature_tracks.json"))
    ap.add_argument("--shapes", default="a,b")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--trace-run")
    ap.add_argument("--merge-trace", nargs=2)
    a = ap.parse_args()
    if a.trace_run:
        run(frames_of(a.trace_run), a.trace_run)
        return
    doc = load(a.out)
    if a.merge_trace:
        name, path = a.merge_trace
        per = collections.defaultdict(list)
        for row in csv.DictReader(open(path)):
            found = re.search(r"k_tr_\w+", row["Kernel_Name"])
            per[found.group(0) if found else row["Kernel_Name"]].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
        doc.setdefault(name, {}).update(SHAPES[name])
        doc[name]["launches_per_call"] = sum(len(v) for k, v in per.items() if k.startswith("k_tr_"))      # the library's own kernels
        doc[name]["runtime_copy_kernels_per_call"] = sum(len(v) for k, v in per.items() if not k.startswith("k_tr_"))
        doc[name]["kernels_us"] = {k: dict(launches=len(v), median_us=round(statistics.median(v), 2), total_us=round(sum(v), 2)) for k, v in sorted(per.items())}
    else:
        for name in a.shapes.split(","):
            seq = frames_of(name)
            _, out = run(seq, name)                                            # warm-up window
            for _ in range(a.calls - 1):
                run(seq, name)
            windows = [statistics.mean(run(seq, name)[0] for _ in range(a.calls)) * 1e3 for _ in range(3)]
            doc.setdefault(name, {}).update(SHAPES[name])
            doc[name].update(fast_threshold=FAST_THRESHOLD, calls_per_window=a.calls, track_sequence_ms=round(statistics.median(windows), 4),
                             spread_ms=round(max(windows) - min(windows), 4), windows_ms=[round(w, 4) for w in windows],
                             observations=int(len(out[1])), tracks=int(out[3]), observations_per_frame=[int(x) for x in (out[0][1:] - out[0][:-1])])
            print(name, doc[name])
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
