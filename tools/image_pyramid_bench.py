"""The dense driver's pre-processing on the device (ssba_image_pyramid_create) and the coarse-to-fine solve: what they cost.

    python tools/image_pyramid_bench.py               # builds of a 1242 x 375 pair with 3 and 4 levels, then one align from level 2
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/image_pyramid_bench.py --builds 20 --windows 1 --no-align --out /dev/null
                                                      # per-kernel times, a run of its own; then
    python tools/image_pyramid_bench.py --merge-trace DIR/.../*_kernel_trace.csv      # medians per kernel and grid into the JSON (no GPU)

Builds: ssba_image_pyramid_create is synchronous and owns its stream, so a window is the wall time of --builds create / destroy
pairs after --warmup, the two level counts taking turns, --windows windows each; device memory and the stream come from the
library's pool after the first build.  The disparity map belongs to level 2, as in the reference driver.  Next to the times: the
launches of a build (2 n - 1 for n levels) and the bytes it must move (uploads, and per level what the two kernels read and
write) against 8 TB/s, as a bound.

Align: the synthetic pair of ceres_slam_amd.synth.make_image_pair at 1242 x 375 in 8 bit, the disparity map at level 0, constant
disparities, levels 2 -> 1 -> 0.  Route A is the device: one pyramid, one ssba_image_pyramid_align.  Route B is what a user of the
previous interface has: the pre-processing in numpy (tests/pyramid_reference.py), then one ssba_add_image_blocks handle per level
with its host uploads.  Both end at the same pose (reported).  Result: profiles/image_pyramid.json and one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ROWS, COLS = 375, 1242
HBM_BYTES_PER_S = 8.0e12


def build_bytes(levels: int, disparity_level: int) -> dict:
    """Bytes a build must move.  Upload: the pair (2 bytes per pixel) and the map (8 per pixel of its level).  k_pyr_down reads the
    finer level once (2 images) and writes the coarser one; k_pyr_finish reads the two 8-bit images (the Sobel neighbours come
    from the same lines) and writes four doubles, and above disparity_level reads and writes one disparity per pixel."""
    up = 2 * ROWS * COLS + 8 * (ROWS >> disparity_level) * (COLS >> disparity_level)
    dev = 0
    for l in range(levels):
        n = (ROWS >> l) * (COLS >> l)
        if l > 0:
            dev += 2 * (ROWS >> (l - 1)) * (COLS >> (l - 1)) + 2 * n
        dev += 2 * n + 32 * n + (16 * n if l > disparity_level else 0)
    return dict(upload_bytes=up, device_bytes=dev, device_bound_us=round(dev / HBM_BYTES_PER_S * 1e6, 3), launches=2 * levels - 1)


def summarise_trace(path: str) -> dict:
    import collections
    import csv
    acc = collections.defaultdict(list)
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"].split("(")[0].split("::")[-1]
            if name.startswith("k_pyr"):
                grid = "x".join(str(int(row[k])) for k in ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z") if row.get(k)) or row.get("Grid_Size", "")
                acc[f"{name} grid {grid}"].append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
    return {k: dict(launches=len(v), median_us=round(statistics.median(v) / 1e3, 2), min_us=round(min(v) / 1e3, 2)) for k, v in sorted(acc.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--builds", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--align-repeats", type=int, default=5)
    ap.add_argument("--no-align", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_pyramid.json"))
    ap.add_argument("--merge-trace", metavar="CSV", default=None)
    args = ap.parse_args()
    if args.merge_trace:
        doc = json.load(open(args.out))
        doc["kernels"] = summarise_trace(args.merge_trace)
        doc["kernel_times_from"] = "rocprofv3 --kernel-trace, a run of its own"
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1, sort_keys=True)
            fh.write("\n")
        print(json.dumps(doc["kernels"]))
        return

    import numpy as np

    import pyramid_reference as pr
    from ceres_slam_amd import capi, synth
    from ceres_slam_amd.solver import ImageAlignment, ImagePyramid

    pair = synth.make_image_pair(ROWS, COLS, seed=0, motion=1.0, min_wavelength_px=8.0)      # about 8 pixels at this width
    ref_u8, track_u8 = pr.quantise(pair.ref), pr.quantise(pair.track)
    d2 = pr.disparity_down(pr.disparity_down(pair.disparity))
    doc = dict(tool="tools/image_pyramid_bench.py", rows=ROWS, cols=COLS, builds_per_window=args.builds, warmup=args.warmup, builds={})

    def build(levels):
        ImagePyramid(ref_u8, track_u8, d2, levels, disparity_level=2, gradient_source=capi.GRADIENT_OF_REFERENCE, gradient_scale=1.0).close()
    samples = {3: [], 4: []}
    for levels in samples:
        for _ in range(args.warmup):
            build(levels)
    for _ in range(args.windows):
        for levels in samples:
            t0 = time.perf_counter()
            for _ in range(args.builds):
                build(levels)
            samples[levels].append(round((time.perf_counter() - t0) / args.builds * 1e3, 5))
    for levels, a in samples.items():
        doc["builds"][f"{levels} levels"] = dict(ms_per_build_samples=a, ms_per_build=dict(median=statistics.median(a), min=min(a), max=max(a), windows=len(a)),
                                                 **build_bytes(levels, 2))

    if not args.no_align:
        o = capi.default_options(max_num_iterations=50, use_nonmonotonic_steps=1)

        def route_device():
            t0 = time.perf_counter()
            pyr = ImagePyramid(ref_u8, track_u8, pair.disparity, 3, disparity_level=0, gradient_source=capi.GRADIENT_OF_TRACKED, gradient_scale=0.125,
                               camera=pair.camera)
            t1 = time.perf_counter()
            pose, disp = pair.pose_init.copy(), pair.disparity.copy()
            rc, sums = pyr.align(pose, disp, coarsest_level=2, disparity_const=True, options=o)
            t2 = time.perf_counter()
            pyr.close()
            return pose, dict(build_ms=(t1 - t0) * 1e3, align_ms=(t2 - t1) * 1e3, total_ms=(t2 - t0) * 1e3,
                              iterations=[s.num_iterations - 1 for s in sums], final_cost=sums[-1].final_cost)

        def route_host():
            t0 = time.perf_counter()
            lv = pr.build(ref_u8, track_u8, pair.disparity, 3, 0, pr.OF_TRACKED, 0.125)
            t1 = time.perf_counter()
            pose, its, cost = pair.pose_init.copy(), [], 0.0
            for l in (2, 1, 0):
                L = lv[l]
                ba = ImageAlignment(pr.level_camera(pair.camera, l), pose, L["disparity"].copy(), L["ref"], L["track"], L["gradx"], L["grady"],
                                    interpolation=capi.IMAGE_BILINEAR, disparity_const=True)
                s, _ = ba.solve(o)
                pose = ba.pose.copy()
                its.append(s.num_iterations - 1)
                cost = s.final_cost
                ba.close()
            t2 = time.perf_counter()
            return pose, dict(preprocess_ms=(t1 - t0) * 1e3, solves_ms=(t2 - t1) * 1e3, total_ms=(t2 - t0) * 1e3, iterations=its, final_cost=cost)
        runs = {"device": [], "host": []}
        poses = {}
        for rep in range(args.align_repeats + 1):       # the first repeat warms both routes up
            for name, fn in (("device", route_device), ("host", route_host)):
                poses[name], r = fn()
                if rep:
                    runs[name].append(r)
        doc["align"] = {name: {k: (round(statistics.median(x[k] for x in a), 3) if k.endswith("_ms") else a[-1][k]) for k in a[0]} for name, a in runs.items()}
        doc["align"]["repeats"] = args.align_repeats
        doc["align"]["pose_difference_between_routes"] = float(np.abs(poses["device"] - poses["host"]).max())
        doc["align"]["translation_error"] = float(np.linalg.norm(poses["device"][:3] - pair.pose_true[:3]))
    if args.out != "/dev/null":
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1, sort_keys=True)
            fh.write("\n")
    print(json.dumps(doc), flush=True)


if __name__ == "__main__":
    main()
