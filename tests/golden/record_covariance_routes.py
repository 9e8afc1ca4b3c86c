"""Writes tests/golden/covariance_routes.npz: what ssba_pose_covariance and ssba_covariance_blocks return, values and status
codes, on the handles of tests/test_gpu_covariance_routes.py (that module builds them; this script only stores what they give).
Run once on the GPU, from the repository root of the commit whose results are to be kept, with the test module of the commit
that checks them:  python tests/golden/record_covariance_routes.py [output directory]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import test_gpu_covariance_routes as routes  # noqa: E402

got = {f"{route}.{k}": np.asarray(v) for route, run in routes.ROUTES.items() for k, v in run().items()}
out = sys.argv[1] if len(sys.argv) > 1 else HERE
np.savez(os.path.join(out, "covariance_routes.npz"), **got)
for k, v in got.items():
    print(k, v.shape, v if v.ndim == 0 else float(np.abs(v).max()))
