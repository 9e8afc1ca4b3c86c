"""ssba_covariance_blocks: every pose and landmark marginal of one window in one call.

One JSON line per configuration: the host-clock time of the call (warmed up, median of 5; the call returns after the
copy back), the per-class kernel times of one more call with kernel timing on (linearisation, Schur assembly, BCR factor;
the selected inversion, the landmark kernel and the column gather are the "small" class -- a rocprofv3 --kernel-trace
--stats run splits them by kernel name), and ssba_pose_covariance per pose averaged over 20 poses for comparison.

usage: python tools/bench_covariance.py [--configs c2,c4]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ceres_slam_amd import capi, synth  # noqa: E402
from ceres_slam_amd.solver import StereoBA  # noqa: E402

CONFIGS = {"c2": (1000, 100_000), "c4": (10_000, 1_000_000)}


def run(name):
    P, L = CONFIGS[name]
    prob = synth.make_problem(P, L, track_len=12, seed=42)
    ba = StereoBA.from_synth(prob, device=0)
    ba.solve(capi.default_options(max_num_iterations=5, use_nonmonotonic_steps=1))
    L = ba.points.shape[0]
    # the request array and the output buffer are built once: the host clock is around the C call only
    req = np.zeros((P + L, 4), dtype=np.uint32)
    req[:P, 1] = req[:P, 3] = np.arange(P)
    req[P:, 0] = req[P:, 2] = capi.COV_POINT
    req[P:, 1] = req[P:, 3] = np.arange(L)
    out = np.zeros(36 * P + 9 * L)
    rp = req.ctypes.data_as(ctypes.POINTER(capi.CovBlock))

    def call():
        t0 = time.perf_counter()
        capi.check(ba.lib.ssba_covariance_blocks(ba.h, rp, P + L, capi.dptr(out)), "ssba_covariance_blocks")
        return 1e3 * (time.perf_counter() - t0)

    call()
    times = [call() for _ in range(5)]
    ba.set_kernel_timing(True)
    timed = call()
    kt = {k: round(v[1], 4) for k, v in ba.kernel_times().items() if v[0]}
    ba.set_kernel_timing(False)
    ks = list(range(1, P, max(1, P // 20)))[:20]
    ba.pose_covariance(ks[0])
    t0 = time.perf_counter()
    for k in ks:
        ba.pose_covariance(k)
    pc = 1e3 * (time.perf_counter() - t0) / len(ks)
    out_mb = (36 * P + 9 * L) * 8 / 1e6
    return dict(config=name, poses=P, points=L, blocks=P + L, ms_per_call_median=round(float(np.median(times)), 3),
                ms_per_call_all=[round(t, 3) for t in times], ms_with_kernel_timing=round(timed, 3), kernel_ms=kt,
                output_mb=round(out_mb, 2), pose_covariance_ms_per_pose=round(pc, 3),
                pose_covariance_ms_for_all_poses=round(pc * P, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2")
    a = ap.parse_args()
    for c in a.configs.split(","):
        print(json.dumps(run(c)), flush=True)


if __name__ == "__main__":
    main()
