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

    python tools/feature_tracks_bench.py [--out profiles/feature_tracks.json] [--shapes a,b] [--calls 10]

--subpixel measures tracks.track_sequence_subpixel against tracks.track_sequence on the same frames in the same process, the two
calls taking turns window by window (track_sequence's code is the parent's, so it is the parent's figure), checks that with
nothing dropped the two calls name the same observations, and writes profiles/feature_tracks_subpixel.json; with --trace-run the
one call is the sub-pixel one, and --merge-trace counts k_tr_anchor and k_tr_refine with the rest.

--stream measures tracks.TrackStream (frames pushed one by one) and writes profiles/feature_track_stream.json.  The frames are 17
of the shape's sequence, walked back and forth so that consecutive pushes are neighbours.  Per shape, whole pixel and sub-pixel:
  push_ms           one push; then per W in 2, 5, 17: push + window(W) against what a live caller does without a stream, the batch
                    call (track_sequence / track_sequence_subpixel, whose code is the parent's) on the W most recent frames after
                    every new frame, on the same frames.  One warm-up window, three timed windows of --calls frames each, the two
                    labels taking turns window by window in one process; median window per frame in ms and the spread.
  history           one stream of 50 pushes with a host clock around each: the pushes at indices 5 ... 14 against 40 ... 49.
--stream --odometry measures a stream with odometry enabled (a pose with every push) and writes profiles/feature_track_odometry.json:
  (a) push_plain / push_odometry   two streams on the same frames taking turns in one process: the cost of the added launches
  (b) live_caller                  what a caller did for the same output before: push + window(2) + ssba_frontend_vo + a two-state
                                   StereoBA solve with pose 0 constant, against push_odometry
With --stream, --trace-run makes ONE stream push 17 frames with a window call after each, and --merge-trace splits the trace at
k_ts_emit (the last launch of a push) and k_ts_window into the launches of every push and of every window call."""
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


def run(seq, name, subpixel=False):
    call = tracks.track_sequence_subpixel if subpixel else tracks.track_sequence
    t = time.perf_counter()
    out = call(seq.left, seq.right, fast_threshold=FAST_THRESHOLD, max_features=SHAPES[name]["max_features"])
    return time.perf_counter() - t, out


def compare(seq, name, calls):
    """Whole-pixel and sub-pixel calls in alternating windows: one warm-up window each, then three timed windows each."""
    outs = {}
    for sub in (False, True):
        for _ in range(calls):
            _, outs[sub] = run(seq, name, sub)
    windows = {False: [], True: []}
    for _ in range(3):
        for sub in (False, True):
            windows[sub].append(statistics.mean(run(seq, name, sub)[0] for _ in range(calls)) * 1e3)
    whole, fine = outs[False], outs[True]
    same = bool(fine[4] == 0 and whole[0].tobytes() == fine[0].tobytes() and whole[1].tobytes() == fine[1].tobytes())
    med = {sub: statistics.median(w) for sub, w in windows.items()}
    return dict(fast_threshold=FAST_THRESHOLD, calls_per_window=calls, track_sequence_ms=round(med[False], 4), track_sequence_subpixel_ms=round(med[True], 4),
                ratio=round(med[True] / med[False], 4), spread_ms=round(max(windows[False]) - min(windows[False]), 4),
                spread_subpixel_ms=round(max(windows[True]) - min(windows[True]), 4), windows_ms=[round(w, 4) for w in windows[False]],
                windows_subpixel_ms=[round(w, 4) for w in windows[True]], observations=int(len(whole[1])), observations_subpixel=int(len(fine[1])),
                dropped=int(fine[4]), tracks=int(fine[3]), same_observations_as_track_sequence=same,
                largest_move_px=round(float(abs(fine[2][:, :2] - whole[2][:, :2]).max()), 4) if same else None)


STREAM_FRAMES, STREAM_WINDOWS = 17, (2, 5, 17)


def walk(n, frames=STREAM_FRAMES):
    """n frame indices 0, 1, ..., frames - 1, frames - 2, ..., 1, 0, 1, ...: neighbours follow each other"""
    period = list(range(frames)) + list(range(frames - 2, 0, -1))
    return [period[k % len(period)] for k in range(n)]


def stream_frames(name):
    s = SHAPES[name]
    return synth.make_stereo_sequence(s["rows"], s["cols"], STREAM_FRAMES, seed=10, motion=1.0, min_wavelength_px=8.0)


def stream_compare(seq, name, calls, sub):
    """Per-frame cost of a stream against the batch call on the last W frames, and the push time early and late in a stream."""
    shape, kw = SHAPES[name], dict(fast_threshold=FAST_THRESHOLD, max_features=SHAPES[name]["max_features"])
    refine = {} if sub else None
    batch = tracks.track_sequence_subpixel if sub else tracks.track_sequence
    order = walk(4 * calls + max(STREAM_WINDOWS))
    left, right = seq.left[order], seq.right[order]                     # the caller's frames in arrival order: a slice is the last W
    out = dict(calls_per_window=calls)

    def timed(step, first):
        t = time.perf_counter()
        for k in range(first, first + calls):
            step(k)
        return (time.perf_counter() - t) / calls * 1e3

    def summary(windows):
        return dict(ms=round(statistics.median(windows), 4), spread_ms=round(max(windows) - min(windows), 4), windows_ms=[round(w, 4) for w in windows])

    with tracks.TrackStream(shape["rows"], shape["cols"], 2, refine=refine, **kw) as st:
        push = lambda k: st.push(left[k], right[k])
        timed(push, 0)
        out["push"] = summary([timed(push, (1 + i) * calls) for i in range(3)])
    for W in STREAM_WINDOWS:
        with tracks.TrackStream(shape["rows"], shape["cols"], W, refine=refine, **kw) as st:
            for k in range(W - 1):                                       # both callers start with W - 1 frames behind them
                st.push(left[k], right[k])

            def streamed(k):
                st.push(left[k], right[k])
                return st.window(W)

            def batched(k):
                return batch(left[k + 1 - W:k + 1], right[k + 1 - W:k + 1], **kw)

            first = W - 1
            timed(streamed, first)
            timed(batched, first)
            windows = {"stream": [], "batch": []}
            for i in range(3):
                windows["stream"].append(timed(streamed, first + (1 + i) * calls))
                windows["batch"].append(timed(batched, first + (1 + i) * calls))
            last = first + 4 * calls - 1
            got, want = st.window(W), batched(last)
            entry = dict(push_and_window=summary(windows["stream"]), batch_on_last_w=summary(windows["batch"]), observations=int(len(got[1])), tracks=int(got[3]))
            entry["batch_over_stream"] = round(entry["batch_on_last_w"]["ms"] / entry["push_and_window"]["ms"], 3)
            if not sub:                                                  # whole pixel: the window is the batch call on its frames, byte for byte
                entry["same_bytes_as_batch"] = bool(all(a.tobytes() == b.tobytes() for a, b in zip(got[:3], want[:3])) and got[3] == want[3])
            out[f"w{W}"] = entry
    order = walk(50)
    with tracks.TrackStream(shape["rows"], shape["cols"], 5, refine=refine, **kw) as st:
        each = []
        for k in order:
            t = time.perf_counter()
            st.push(seq.left[k], seq.right[k])
            each.append((time.perf_counter() - t) * 1e3)
    for label, part in (("pushes_5_to_14", each[5:15]), ("pushes_40_to_49", each[40:50])):
        out[label] = dict(median_ms=round(statistics.median(part), 4), spread_ms=round(max(part) - min(part), 4))
    return out


def odometry_compare(seq, name, calls, sub):
    """(a) and (b) of the module docstring, medians of three alternating windows of `calls` pushes each."""
    import ctypes as C

    import numpy as np

    from ceres_slam_amd import capi, frontend
    from ceres_slam_amd.solver import StereoBA

    shape, kw = SHAPES[name], dict(fast_threshold=FAST_THRESHOLD, max_features=SHAPES[name]["max_features"])
    refine = {} if sub else None
    order = walk(4 * calls + 2)
    left, right = seq.left[order], seq.right[order]
    identity = np.array([0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1.0])
    variant = 1                                                         # which libstdc++ draw sequence: no matter for the time

    def summary(windows):
        return dict(ms=round(statistics.median(windows), 4), spread_ms=round(max(windows) - min(windows), 4), windows_ms=[round(w, 4) for w in windows])

    def timed(step, first):
        t = time.perf_counter()
        for k in range(first, first + calls):
            step(k)
        return (time.perf_counter() - t) / calls * 1e3

    def solve_window(start, ids, uvd, num_points):
        obs_state = np.repeat(np.arange(2, dtype=np.uint32), np.diff(start.astype(np.int64)))
        poses, points, init, _ = frontend.compute_initial_guess_device(seq.camera, 2, num_points, obs_state, ids, uvd, identity, variant=variant)
        sel, keep = init[ids], np.nonzero(init)[0]
        remap = np.full(num_points, -1, np.int64)
        remap[keep] = np.arange(len(keep))
        ba = StereoBA(seq.camera, poses.copy(), points[keep].copy(), obs_state[sel], remap[ids[sel]].astype(np.uint32), uvd[sel], np.eye(3) / 2.0)
        options, summ = capi.default_options(max_num_iterations=20), capi.Summary()
        ba.lib.ssba_solve(ba.h, C.byref(options), C.byref(summ))
        out = ba.poses.copy()
        ba.close()
        return out

    infos = []
    with tracks.TrackStream(shape["rows"], shape["cols"], 2, refine=refine, **kw) as plain, \
            tracks.TrackStream(shape["rows"], shape["cols"], 2, refine=refine, odometry=dict(camera=seq.camera), **kw) as odo, \
            tracks.TrackStream(shape["rows"], shape["cols"], 2, refine=refine, **kw) as live:
        def push_plain(k):
            plain.push(left[k], right[k])

        def push_odometry(k):
            odo.push(left[k], right[k])
            infos.append(odo.pose()[2])

        def live_caller(k):
            live.push(left[k], right[k])
            if live.pushed > 1:
                solve_window(*live.window(2))

        steps = dict(push_plain=push_plain, push_odometry=push_odometry, live_caller=live_caller)
        for step in steps.values():
            timed(step, 0)
        windows = {k: [] for k in steps}
        for i in range(3):
            for k, step in steps.items():
                windows[k].append(timed(step, (1 + i) * calls))
    out = {k: summary(w) for k, w in windows.items()}
    out["calls_per_window"] = calls
    out["odometry_minus_plain_ms"] = round(out["push_odometry"]["ms"] - out["push_plain"]["ms"], 4)
    out["live_caller_over_push_odometry"] = round(out["live_caller"]["ms"] / out["push_odometry"]["ms"], 3)
    timed_infos = infos[calls:]
    out["status_counts"] = {str(k): int(v) for k, v in sorted(collections.Counter(i["status"] for i in timed_infos).items())}
    for key in ("num_matches", "num_inliers", "num_iterations"):
        out["median_" + key] = int(statistics.median(i[key] for i in timed_infos))
    return out


def stream_trace_run(name, sub):
    seq, shape = stream_frames(name), SHAPES[name]
    with tracks.TrackStream(shape["rows"], shape["cols"], STREAM_FRAMES, refine={} if sub else None, fast_threshold=FAST_THRESHOLD,
                            max_features=shape["max_features"]) as st:
        for k in range(STREAM_FRAMES):
            st.push(seq.left[k], seq.right[k])
            st.window(k + 1)


def stream_merge_trace(path):
    """The library's launches of every push and of every window call, in the order of the trace."""
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    pushes, windows, current, per = [], [], [], collections.defaultdict(list)
    for row in rows:
        found = re.search(r"k_t[rs]_\w+", row["Kernel_Name"])
        if not found:
            continue
        per[found.group(0)].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
        current.append(found.group(0))
        if found.group(0) in ("k_ts_emit", "k_ts_window"):
            (pushes if found.group(0) == "k_ts_emit" else windows).append(current)
            current = []
    return dict(launches_per_push=[len(p) for p in pushes], launches_per_window_call=[len(w) for w in windows],
                launches_at_pushes_2_5_17=[len(pushes[k - 1]) for k in (2, 5, 17) if k <= len(pushes)], kernels_of_push_2=pushes[1] if len(pushes) > 1 else [],
                kernels_us={k: dict(launches=len(v), median_us=round(statistics.median(v), 2), total_us=round(sum(v), 2)) for k, v in sorted(per.items())})


def load(path):
    return json.load(open(path)) if os.path.exists(path) else {}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--subpixel", action="store_true")
    ap.add_argument("--stream", action="store_true")
    ap.add_argument("--odometry", action="store_true")
    ap.add_argument("--shapes", default="a,b")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--trace-run")
    ap.add_argument("--merge-trace", nargs=2)
    a = ap.parse_args()
    if a.odometry and not a.stream:
        ap.error("--odometry goes with --stream")
    a.out = a.out or os.path.join(ROOT, "profiles", "feature_track_odometry.json" if a.odometry else "feature_track_stream.json" if a.stream else "feature_tracks_subpixel.json" if a.subpixel else "feature_tracks.json")
    if a.odometry:
        doc = load(a.out)
        for name in a.shapes.split(","):
            seq = stream_frames(name)
            doc.setdefault(name, {}).update(SHAPES[name], frames=STREAM_FRAMES, fast_threshold=FAST_THRESHOLD)
            for sub in (False, True):
                doc[name]["subpixel" if sub else "whole_pixel"] = odometry_compare(seq, name, a.calls, sub)
                print(name, "subpixel" if sub else "whole_pixel", doc[name]["subpixel" if sub else "whole_pixel"])
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
        return
    if a.stream:
        if a.trace_run:
            stream_trace_run(a.trace_run, a.subpixel)
            return
        doc = load(a.out)
        if a.merge_trace:
            name, path = a.merge_trace
            doc.setdefault(name, {}).update(SHAPES[name])
            doc[name]["trace_subpixel" if a.subpixel else "trace_whole_pixel"] = stream_merge_trace(path)
        else:
            for name in a.shapes.split(","):
                seq = stream_frames(name)
                doc.setdefault(name, {}).update(SHAPES[name], frames=STREAM_FRAMES, fast_threshold=FAST_THRESHOLD)
                for sub in (False, True):
                    doc[name]["subpixel" if sub else "whole_pixel"] = stream_compare(seq, name, a.calls, sub)
                    print(name, "subpixel" if sub else "whole_pixel", doc[name]["subpixel" if sub else "whole_pixel"])
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
        return
    if a.trace_run:
        run(frames_of(a.trace_run), a.trace_run, a.subpixel)
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
        for name in a.shapes.split(",") if a.subpixel else []:
            doc.setdefault(name, {}).update(SHAPES[name])
            doc[name].update(compare(frames_of(name), name, a.calls))
            print(name, doc[name])
        for name in [] if a.subpixel else a.shapes.split(","):
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
