"""Writes tests/golden/pcr_store_deal_costs.json and pcr_store_deal_poses.npz: the cost column (hex floats) and the final
poses of the chains of tests/test_gpu_pcr_store_deal.py.  Run once on the GPU, from the repository root of the commit whose
results are to be kept:  python tests/golden/record_pcr_store_deal_costs.py [output directory]"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from ceres_slam_amd import capi, synth  # noqa: E402
from ceres_slam_amd.solver import StereoBA  # noqa: E402


def problem(blocks):
    if blocks == 86:        # two workgroups per block
        return synth.make_problem(1022, 10 * 1022, track_len=12, seed=7)
    n = 12 * (blocks - 1) + 2
    return synth.make_problem(n, 30 * n, track_len=12, seed=3)


costs, poses = {}, {}
for blocks in (3, 5, 9, 86):
    ba = StereoBA.from_synth(problem(blocks))
    s, log = ba.solve(capi.default_options(max_num_iterations=1000, use_nonmonotonic_steps=1))
    st = ba.stats()
    assert st.pcr_blocks == blocks and st.pcr_fused == 1
    costs[str(blocks)] = [float(c).hex() for c in log["cost"]]
    poses[str(blocks)] = np.array(ba.poses, dtype=np.float64)
    ba.close()
out = sys.argv[1] if len(sys.argv) > 1 else HERE
with open(os.path.join(out, "pcr_store_deal_costs.json"), "w") as f:
    json.dump(costs, f, indent=1)
    f.write("\n")
np.savez(os.path.join(out, "pcr_store_deal_poses.npz"), **poses)
print(out, {k: len(v) for k, v in costs.items()})
