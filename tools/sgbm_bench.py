"""The semi-global matcher on the device (ssba_stereo_sgbm, ssba_image_pyramid_create_stereo): what it costs.

    python tools/sgbm_bench.py                        # wall time per call, both shapes, three alternated windows
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/sgbm_bench.py --calls 20 --windows 1 --no-pyramid --out /dev/null
                                                      # per-kernel times, a run of its own; then
    python tools/sgbm_bench.py --merge-trace DIR/.../*_kernel_trace.csv       # medians per kernel and shape into the JSON (no GPU)
    python tools/sgbm_bench.py --numpy                # the numpy reference's wall time on the same shapes, for scale (no GPU)

Shapes: 310 x 93 with 64 disparities and block 15 (the reference driver's own call, after its two halvings of a 1242 x 375 pair) and
1242 x 375 with 128 disparities and block 15; the rendered plane of ceres_slam_amd.synth.make_stereo_triple in 8 bit.

ssba_stereo_sgbm is synchronous and owns its stream: a window is the wall time of --calls calls after --warmup, the two shapes
taking turns.  The matcher inside ssba_image_pyramid_create_stereo (one level, so that nothing but the matcher differs): the same
windows of create_stereo / destroy against create / destroy with the matcher's map handed in, taking turns; the difference is the
matcher's share of the call (its kernels plus the pool allocations of its volumes, minus the upload of the map it replaces).  A
pyramid has no timing hook and its stream is its own, so no device events bracket the kernels there: the device time is the sum
of the per-kernel medians of the trace.

Next to the times: what each kernel must move (bytes_* below) against 8 TB/s."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = {"310x93 D64 b15": (93, 310, 64, 15), "1242x375 D128 b15": (375, 1242, 128, 15)}
HBM_BYTES_PER_S = 8.0e12
CLOCK_HZ = 2.4e9


def kernel_bytes(rows, cols, D):
    """What each launch must move.  n volume entries of 16 bits, npx computable pixels, img pixels.  hcost reads three rows of both
    images per row (neighbouring work-groups share them in cache: counted once) and writes the row sums; vcost re-reads its 2r + 1
    rows from cache (counted once); the path kernel reads C once per direction (five work-groups' worth of waves, far apart in
    time: counted five times) and writes five volumes; select reads them and writes 8 bytes per pixel; lr reads those and writes
    both outputs."""
    W = cols - D
    n, npx, img = rows * W * D, rows * W, rows * cols
    return dict(k_sgbm_hcost=2 * img + 2 * n, k_sgbm_vcost=4 * n, k_sgbm_paths=20 * n, k_sgbm_select=10 * n + 8 * npx, k_sgbm_lr=8 * npx + 10 * img)


def summarise_trace(path):
    import collections
    import csv
    grids = {}
    for label, (rows, cols, D, _) in SHAPES.items():
        W = cols - D
        grids[(2 * rows + W + 2 * (W + rows - 1) + 3) // 4 * 256] = label       # the path kernel's grid names the shape of a run
    acc = collections.defaultdict(list)
    current = None
    rows_ = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    # a call is hcost, vcost, paths, select, lr in stream order: label all five by the path kernel's grid
    calls, call = [], []
    for row in rows_:
        name = row["Kernel_Name"].split("(")[0].split("::")[-1].split("<")[0]
        if not name.startswith("k_sgbm"):
            continue
        call.append((name, row))
        if name == "k_sgbm_lr":
            calls.append(call)
            call = []
    for call in calls:
        label = None
        for name, row in call:
            if name == "k_sgbm_paths":
                label = grids.get(int(row["Grid_Size_X"]) if row.get("Grid_Size_X") else int(row.get("Grid_Size", 0)))
        if label is None:
            continue
        for name, row in call:
            acc[(label, name)].append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
    out = {}
    for (label, name), v in sorted(acc.items()):
        rows, cols, D, _ = SHAPES[label]
        b = kernel_bytes(rows, cols, D)[name]
        med = statistics.median(v) / 1e3
        e = dict(launches=len(v), median_us=round(med, 2), min_us=round(min(v) / 1e3, 2), bytes=b, bound_us=round(b / HBM_BYTES_PER_S * 1e6, 3),
                 share_of_bound=round(b / HBM_BYTES_PER_S * 1e6 / med, 4))
        if name == "k_sgbm_paths":
            steps = max(cols - D, rows)
            e["longest_chain_steps"] = steps
            e["cycles_per_step_at_2.4GHz"] = round(med * 1e-6 / steps * CLOCK_HZ, 1)
        out.setdefault(label, {})[name] = e
    for label in out:
        out[label]["sum_of_medians_us"] = round(sum(e["median_us"] for e in out[label].values()), 2)
    return out


def write(doc, path):
    if path == "/dev/null":
        return
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--no-pyramid", action="store_true")
    ap.add_argument("--numpy", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sgbm.json"))
    ap.add_argument("--merge-trace", metavar="CSV", default=None)
    args = ap.parse_args()
    if args.merge_trace:
        doc = json.load(open(args.out))
        doc["kernels"] = summarise_trace(args.merge_trace)
        doc["kernel_times_from"] = "rocprofv3 --kernel-trace --stats, a run of its own"
        write(doc, args.out)
        print(json.dumps(doc["kernels"]))
        return

    import numpy as np

    from ceres_slam_amd import synth
    triples = {k: synth.make_stereo_triple(r, c, seed=0, min_wavelength_px=8.0) for k, (r, c, _, _) in SHAPES.items()}

    if args.numpy:
        import sgbm_reference as sr
        doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
        doc["numpy_reference_wall_s"] = {}
        for k, (r, c, D, bs) in SHAPES.items():
            t0 = time.perf_counter()
            sr.sgbm(triples[k].left0, triples[k].right0, num_disparities=D, block_size=bs)
            doc["numpy_reference_wall_s"][k] = round(time.perf_counter() - t0, 2)
        doc["numpy_reference_note"] = "tests/sgbm_reference.py on a CPU, one run per shape: for scale only, not a competitor"
        write(doc, args.out)
        print(json.dumps(doc["numpy_reference_wall_s"]))
        return

    from ceres_slam_amd import capi
    from ceres_slam_amd.solver import ImagePyramid, stereo_sgbm

    doc = json.load(open(args.out)) if os.path.exists(args.out) and args.out != "/dev/null" else {}
    doc.update(tool="tools/sgbm_bench.py", calls_per_window=args.calls, warmup=args.warmup, shapes={})
    maps, samples = {}, {k: [] for k in SHAPES}
    for k, (r, c, D, bs) in SHAPES.items():
        for _ in range(args.warmup):
            _, maps[k] = stereo_sgbm(triples[k].left0, triples[k].right0, num_disparities=D, block_size=bs)
    for _ in range(args.windows):
        for k, (r, c, D, bs) in SHAPES.items():
            t0 = time.perf_counter()
            for _ in range(args.calls):
                stereo_sgbm(triples[k].left0, triples[k].right0, num_disparities=D, block_size=bs)
            samples[k].append(round((time.perf_counter() - t0) / args.calls * 1e3, 4))
    for k, (r, c, D, bs) in SHAPES.items():
        exact = triples[k].pair.disparity[:, D:]
        got = maps[k][:, D:]
        ok = np.isfinite(got)
        b = kernel_bytes(r, c, D)
        doc["shapes"][k] = dict(rows=r, cols=c, num_disparities=D, block_size=bs, ms_per_call_samples=samples[k],
                                ms_per_call=dict(median=statistics.median(samples[k]), min=min(samples[k]), max=max(samples[k]), windows=len(samples[k])),
                                valid_of_computable=round(float(ok.mean()), 4), within_1px=round(float((np.abs(got[ok] - exact[ok]) <= 1).mean()), 4),
                                bytes=b, bound_us={n: round(v / HBM_BYTES_PER_S * 1e6, 3) for n, v in b.items()},
                                volume_bytes=12 * r * (c - D) * D)

    if not args.no_pyramid:
        pyr = {k: dict(stereo=[], given=[]) for k in SHAPES}

        def stereo(k):
            r, c, D, bs = SHAPES[k]
            ImagePyramid.create_stereo(triples[k].left0, triples[k].right0, triples[k].left1, 1, params=dict(num_disparities=D, block_size=bs)).close()

        def given(k):
            ImagePyramid(triples[k].left0, triples[k].left1, maps[k], 1).close()
        for k in SHAPES:
            for _ in range(args.warmup):
                stereo(k), given(k)
        for _ in range(args.windows):
            for k in SHAPES:
                for name, fn in (("stereo", stereo), ("given", given)):
                    t0 = time.perf_counter()
                    for _ in range(args.calls):
                        fn(k)
                    pyr[k][name].append(round((time.perf_counter() - t0) / args.calls * 1e3, 4))
        for k in SHAPES:
            a, b = pyr[k]["stereo"], pyr[k]["given"]
            doc["shapes"][k]["create_stereo_one_level"] = dict(ms_per_create_stereo_samples=a, ms_per_create_samples=b,
                                                               matcher_ms=dict(median=round(statistics.median(a) - statistics.median(b), 4),
                                                                               min=round(min(x - y for x, y in zip(a, b)), 4),
                                                                               max=round(max(x - y for x, y in zip(a, b)), 4)))
    write(doc, args.out)
    print(json.dumps(doc), flush=True)


if __name__ == "__main__":
    main()
