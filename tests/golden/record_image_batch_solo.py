"""Writes tests/golden/image_batch_solo.json: pose, disparity map and every column of ssba_iteration_log of solo ssba_solve runs
on the shapes 40x30, 8x6 and blocks1025 of tests/test_gpu_image_alignment.py (both interpolations, free and constant
disparities, max_num_iterations = 50, non-monotonic steps), as the bytes of the float64 / int32 arrays in hex.  Run once on the
GPU, from the repository root of the commit whose results are to be kept:
    python tests/golden/record_image_batch_solo.py [output.json]"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import test_gpu_image_alignment as shapes  # noqa: E402
from ceres_slam_amd import capi  # noqa: E402

LOG_COLUMNS = ("cost", "cost_change", "gradient_max_norm", "step_norm", "relative_decrease", "trust_region_radius", "step_is_successful")


def record(name, interp, const):
    ba = shapes._handle(name, interp, const)
    s, log = ba.solve(capi.default_options(max_num_iterations=50, use_nonmonotonic_steps=1))
    out = dict(pose=ba.pose.tobytes().hex(), disparity=ba.disparity.tobytes().hex(), num_iterations=int(s.num_iterations),
               termination_type=int(s.termination_type), log={k: log[k].tobytes().hex() for k in LOG_COLUMNS})
    ba.close()
    return out


if __name__ == "__main__":
    out = {}
    for name in ("40x30", "8x6", "blocks1025"):
        for interp in (0, 1):
            for const in (False, True):
                out[f"{name}/{'bilinear' if interp else 'nearest'}/{'const' if const else 'free'}"] = record(name, interp, const)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "image_batch_solo.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(path, {k: v["num_iterations"] for k, v in out.items()})
