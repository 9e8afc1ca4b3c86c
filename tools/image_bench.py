"""Dense photometric alignment (ssba_add_image_blocks): time per Levenberg-Marquardt iteration at the reference driver's sizes.

Sizes: 310 x 94 (a KITTI frame after the two pyrDown calls of tests/dense_stereo_test.cpp:52-59) and 1242 x 375 (the full
frame), on the synthetic pair of ceres_slam_amd.synth.make_image_pair, BILINEAR, with free and with constant disparities.

    python tools/image_bench.py                      # device events: --steps graph-replayed iterations after --warmup, --rounds windows
    python tools/image_bench.py --kernel-timing      # per-kernel-class HIP-event times instead (a run of its own)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/image_bench.py --rounds 1 --out /dev/null
                                                     # per-kernel times, a run of its own; then
    python tools/image_bench.py --merge-trace DIR/.../*_kernel_trace.csv      # medians, bounds and shares into the JSON (no GPU)
    python tools/image_bench.py --loss-fraction 0.1 --parent-tree DIR --out profiles/image_loss.json
                                                     # every configuration also under ceres::HuberLoss(a), a correcting about a tenth of
                                                     # the rows; the windows alternate with a build of the parent commit in DIR

Per handle: ssba_solve_begin with ignore_convergence, 17 steps (the graph captures), --warmup steps; then --rounds windows of
--steps iterations between two device events on the handle's stream, the configurations taking turns.  The iterations run on
from wherever the solve is (after convergence every step is still one full linearisation, solve and evaluation: the launch
chain has no data-dependent work).  Next to the times the tool writes the bytes and fp64 operations per block that the kernels
need, counted from the shapes below, so that a kernel time gives its share of the bound.  Result: profiles/image_alignment.json
and one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"310x94": (94, 310), "1242x375": (375, 1242)}


def per_block_counts(free: bool) -> dict:
    """Bytes to and from memory and fp64 operations per residual block, from the shapes of ssba_image.hip (BILINEAR).

    k_im_lin reads the block's pixel index (4), its disparity (8), the reference pixel (8) and 3 x 4 samples of the tracked image
    and the two gradient images (96, neighbouring lanes share most of those lines), and writes the row (64); with free
    disparities also the committed disparity (8 written on accepted steps; counted) and the Jacobi scale (8 read).
    k_im_eval reads the pixel index, the row (64), the disparity, 4 samples of the tracked image (32) and the reference pixel,
    and with free disparities the scale, and writes the candidate disparity.
    Operations (adds and multiplies counted one each, divides one): projection 30, three bilinear samples 3 x 11, row 45,
    products into the sums 27 x 2 (free: 39 x 2 + the elimination 12); evaluation: projection 30, one sample 11, step 25."""
    lin_bytes = 4 + 8 + 8 + 96 + 64 + (16 if free else 0)
    eval_bytes = 4 + 64 + 8 + 32 + 8 + (16 if free else 0)
    lin_ops = 30 + 33 + 45 + (39 * 2 + 12 if free else 27 * 2)
    eval_ops = 30 + 11 + 25
    return dict(k_im_lin=dict(bytes=lin_bytes, fp64_ops=lin_ops), k_im_eval=dict(bytes=eval_bytes, fp64_ops=eval_ops))


HBM_BYTES_PER_S = 8.0e12        # MI355X peaks as DESIGN.md section 5 uses them
FP64_OPS_PER_S = 78.6e12


def summarise_trace(path: str) -> dict:
    """(kernel name without its argument list, grid size) -> (launches, median microseconds) from a rocprofv3 kernel trace csv."""
    import collections
    import csv
    acc = collections.defaultdict(list)
    with open(path) as f:
        for row in csv.DictReader(f):
            acc[(row["Kernel_Name"].split("(")[0], int(row.get("Grid_Size_X") or row["Grid_Size"]))].append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
    return {k: (len(v), statistics.median(v) / 1e3) for k, v in acc.items()}


def merge_kernels(doc: dict, table: dict) -> None:
    """Per configuration of doc["runs"]: the median time of k_im_lin and k_im_eval (told apart by instantiation and grid size), the
    least time the hardware could take for the bytes and operations per_block_counts gives, which of the two bounds, and the
    share of it reached.  The single-work-group launches (k_im_solve, k_decide) do not depend on the configuration; k_best by grid."""
    for name, e in doc["runs"].items():
        n_wg = (e["blocks"] + 255) // 256
        free = "true" if e["free_disparities"] else "false"
        out = {}
        for kern, grid in (("k_im_lin", n_wg * 256), ("k_im_eval", (n_wg + 1) * 256)):
            hit = [v for (k, g), v in table.items() if g == grid and k.endswith(f"{kern}<{free}>")]
            if not hit:
                continue
            c = e["per_block"][kern]
            t_bytes, t_ops = e["blocks"] * c["bytes"] / HBM_BYTES_PER_S * 1e6, e["blocks"] * c["fp64_ops"] / FP64_OPS_PER_S * 1e6
            out[kern] = dict(launches=hit[0][0], median_us=round(hit[0][1], 2), bound="hbm" if t_bytes >= t_ops else "fp64", bound_us=round(max(t_bytes, t_ops), 2),
                             share_of_bound=round(max(t_bytes, t_ops) / hit[0][1], 3))
        e["kernels"] = out
    small = {}
    for (k, g), v in sorted(table.items()):
        if any(k.endswith(s) for s in ("k_im_solve", "k_decide", "k_best")):
            small[f"{k.split('::')[-1]} grid {g}"] = dict(launches=v[0], median_us=round(v[1], 2))
    doc["control_kernels"] = small
    doc["kernel_times_from"] = "rocprofv3 --kernel-trace, a run of its own; bounds at 8 TB/s and 78.6 TFLOP/s fp64"


def alternate(args):
    """--parent-tree: `rounds` windows of this tree and of the parent's, alternating, one process each (two builds of one library
    cannot share a process); every window is a full run of this tool with --child --rounds 1."""
    runs = {}
    for _ in range(args.rounds):
        for who, tree in (("this", ROOT), ("parent", os.path.abspath(args.parent_tree))):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--rounds", "1", "--package-root", tree, "--sizes", args.sizes,
                   "--steps", str(args.steps), "--warmup", str(args.warmup)]
            if who == "this" and args.loss_fraction > 0.0:
                cmd += ["--loss-fraction", str(args.loss_fraction)]
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if out.returncode != 0:
                raise RuntimeError(f"window of the {who} tree failed:\n{out.stdout[-2000:]}{out.stderr[-2000:]}")
            for name, r in json.loads(out.stdout.strip().splitlines()[-1]).items():
                e = runs.setdefault(name, dict(blocks=r["blocks"]))
                e.setdefault(who, []).extend(r["samples"])
                if r.get("huber_a") is not None:
                    e.update(huber_a=r["huber_a"], corrected_at_start=r["corrected_at_start"])

    def summary(a):
        return dict(median=round(statistics.median(a), 5), min=min(a), max=max(a), windows=len(a))
    doc = dict(tool="tools/image_bench.py --parent-tree", steps=args.steps, warmup=args.warmup, interpolation="BILINEAR", loss_fraction=args.loss_fraction, runs={})
    for name, e in runs.items():
        d = dict(blocks=e["blocks"], ms_per_iteration_samples=e["this"], ms_per_iteration=summary(e["this"]))
        if "parent" in e:
            d.update(parent=dict(ms_per_iteration_samples=e["parent"], ms_per_iteration=summary(e["parent"])))
        if "huber_a" in e:
            base = runs[name[:-len("/huber")]]["this"]
            d.update(huber_a=e["huber_a"], corrected_at_start=e["corrected_at_start"],
                     loss_costs_ms_per_iteration=round(statistics.median(e["this"]) - statistics.median(base), 5))
        doc["runs"][name] = d
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps({k: (v["ms_per_iteration"]["median"], v.get("parent", {}).get("ms_per_iteration", {}).get("median")) for k, v in doc["runs"].items()}), flush=True)


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
    ap.add_argument("--sizes", default="310x94,1242x375")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernel-timing", action="store_true", help="per-kernel-class HIP-event times of one window per configuration instead")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_alignment.json"))
    ap.add_argument("--merge-trace", metavar="CSV", default=None, help="no run: merge the per-kernel medians of a rocprofv3 kernel trace into --out")
    ap.add_argument("--loss-fraction", type=float, default=0.0,
                    help="also time every configuration under ceres::HuberLoss(a), a = the width that corrects about this fraction of the rows at the start "
                         "(the matching quantile of |r| of a NULL-loss ssba_image_step); runs named <size>/<free|constant>/huber")
    ap.add_argument("--parent-tree", metavar="DIR", default=None,
                    help="a checkout of the parent commit with its library built: the windows alternate between this tree and that one, one process per "
                         "window; the parent's figures go under 'parent' of every run it can time (it has no loss on image blocks)")
    ap.add_argument("--package-root", metavar="DIR", default=ROOT, help="where ceres_slam_amd is imported from (a window of --parent-tree)")
    ap.add_argument("--child", action="store_true", help="a window of --parent-tree: print the samples as one JSON line, write nothing")
    args = ap.parse_args()
    if args.parent_tree:
        return alternate(args)
    if args.merge_trace:
        doc = json.load(open(args.out))
        merge_kernels(doc, summarise_trace(args.merge_trace))
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1, sort_keys=True)
            fh.write("\n")
        print(json.dumps({k: v.get("kernels") for k, v in doc["runs"].items()}))
        return

    sys.path.insert(0, os.path.abspath(args.package_root))
    from ceres_slam_amd import capi, synth
    from ceres_slam_amd.solver import ImageAlignment

    hip = Hip()
    opts = capi.default_options(max_num_iterations=1000, use_nonmonotonic_steps=1)
    runs = {}
    for size in args.sizes.split(","):
        rows, cols = SIZES[size]
        pair = synth.make_image_pair(rows, cols, seed=0, invalid_fraction=0.03)
        for const, loss in [(c, l) for c in (False, True) for l in ((False, True) if args.loss_fraction > 0.0 else (False,))]:
            name = f"{size}/{'constant' if const else 'free'}" + ("/huber" if loss else "")
            ba = ImageAlignment.from_synth(pair, interpolation=capi.IMAGE_BILINEAR, disparity_const=const)
            width = corrected = None
            if loss:
                blk = np.isfinite(pair.disparity) & (pair.disparity > 0)
                r0 = np.abs(ba.image_step(1e4).residuals[blk])
                width = float(np.quantile(r0[r0 > 0], 1.0 - args.loss_fraction))
                ba.set_huber_loss(width)
                corrected = float((np.abs(ba.image_step(1e4).residuals[blk]) != r0).mean())
            st = ba.stats()
            assert st.general_structure == 4
            stream = hip.stream()
            ba.set_stream(stream.value)
            if args.kernel_timing:
                ba.set_kernel_timing(True)
            ba.solve_begin(opts, ignore_convergence=True)
            ba.step(17)         # the single-iteration graph and the batch of ten
            ba.step(args.warmup)
            ba.synchronize()
            runs[name] = dict(ba=ba, stream=stream, a=hip.event(), b=hip.event(), samples=[], blocks=int(st.num_observations), rows=rows, cols=cols,
                              free=not const, device_bytes=int(st.device_bytes), huber_a=width, corrected_at_start=corrected)
    kernels = {}
    if args.kernel_timing:
        for name, r in runs.items():
            before = r["ba"].kernel_times()
            r["ba"].step(args.steps)
            r["ba"].synchronize()
            after = r["ba"].kernel_times()
            kernels[name] = {k: dict(launches_per_iteration=round((after[k][0] - before.get(k, (0, 0.0))[0]) / args.steps, 3),
                                     ms_per_iteration=round((after[k][1] - before.get(k, (0, 0.0))[1]) / args.steps, 5))
                             for k in sorted(after) if after[k][0] - before.get(k, (0, 0.0))[0]}
    else:
        for _ in range(args.rounds):
            for r in runs.values():
                r["ba"].synchronize()
                hip.record(r["a"], r["stream"])
                r["ba"].step(args.steps)
                hip.record(r["b"], r["stream"])
                r["samples"].append(round(hip.elapsed_ms(r["a"], r["b"]) / args.steps, 5))
    if args.child:
        for r in runs.values():
            r["ba"].solve_end()
        print(json.dumps({k: dict(samples=r["samples"], blocks=r["blocks"], huber_a=r["huber_a"], corrected_at_start=r["corrected_at_start"])
                          for k, r in runs.items()}), flush=True)
        return
    doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
    doc.update(tool="tools/image_bench.py", steps=args.steps, warmup=args.warmup, interpolation="BILINEAR")
    doc.setdefault("runs", {})
    for name, r in runs.items():
        s = r["ba"].solve_end()
        e = doc["runs"].setdefault(name, {})
        e.update(rows=r["rows"], cols=r["cols"], blocks=r["blocks"], free_disparities=r["free"], device_bytes=r["device_bytes"],
                 per_block=per_block_counts(r["free"]))
        if r["huber_a"] is not None:
            e.update(huber_a=r["huber_a"], corrected_at_start=r["corrected_at_start"])
        if args.kernel_timing:
            e["kernel_classes"] = kernels[name]
        else:
            a = r["samples"]
            e.update(ms_per_iteration_samples=a, ms_per_iteration=dict(median=round(statistics.median(a), 5), min=min(a), max=max(a), windows=len(a)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps({k: (v.get("kernel_classes") if args.kernel_timing else v.get("ms_per_iteration_samples")) for k, v in doc["runs"].items()}), flush=True)


if __name__ == "__main__":
    main()
