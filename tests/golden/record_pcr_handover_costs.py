"""Writes tests/golden/pcr_handover_costs.json: the cost column of the 5- and 9-block chains of
tests/test_gpu_pcr_handover.py as hex floats.  Run once on the GPU, from the repository root of the commit whose costs
are to be kept:  python tests/golden/record_pcr_handover_costs.py [output.json]"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from ceres_slam_amd import capi, synth  # noqa: E402
from ceres_slam_amd.solver import StereoBA  # noqa: E402

out = {}
for blocks in (5, 9):
    n = 12 * (blocks - 1) + 2
    ba = StereoBA.from_synth(synth.make_problem(n, 30 * n, track_len=12, seed=3))
    s, log = ba.solve(capi.default_options(max_num_iterations=1000, use_nonmonotonic_steps=1))
    st = ba.stats()
    assert st.pcr_blocks == blocks and st.pcr_fused == 1
    out[str(blocks)] = [float(c).hex() for c in log["cost"]]
    ba.close()
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "pcr_handover_costs.json")
with open(path, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(path, {k: len(v) for k, v in out.items()})
