"""The members of the batches of tests/test_gpu_image_batch.py, shared with tests/test_image_batch_inputs.py, which pins on the
numpy loop alone that they end at different iterations.  Every array is shared between tests and never written."""
import functools

import numpy as np

import image_reference as ir
from ceres_slam_amd import synth

MAX_ITER = 50

#: name -> (make_image_pair arguments, keywords, interpolation, constant disparities, log entries of ImageProblem.solve)
MEMBERS = {
    "s1": ((30, 40), dict(seed=1), ir.BILINEAR, True, 6),
    "s4": ((30, 40), dict(seed=4), ir.BILINEAR, True, 8),
    "s0": ((30, 40), dict(seed=0), ir.BILINEAR, True, 9),
    "8x6": ((6, 8), dict(seed=2, min_wavelength_px=4.0), ir.BILINEAR, True, 18),
    "s0free": ((30, 40), dict(seed=0), ir.BILINEAR, False, MAX_ITER + 1),      # runs to the cap
}
FIVE = ["s1", "s4", "s0", "8x6", "s0free"]


@functools.lru_cache(maxsize=None)
def member(name):
    """(pair, start pose, interpolation, constant disparities)"""
    if name == "blocks1025":        # tests/test_gpu_image_alignment.py: 5 work-groups, one lane in the last
        pair = synth.make_image_pair(30, 40, seed=1)
        rng = np.random.Generator(np.random.PCG64(1025))
        idx = rng.choice(1200, size=1200 - 1025, replace=False)
        pair.disparity.reshape(-1)[idx] = np.array([np.nan, 0.0, -2.0])[np.arange(idx.shape[0]) % 3]
        interp, const = ir.NEAREST, True
    elif name.startswith("tiny"):   # 8 x 6 with another seed
        pair = synth.make_image_pair(6, 8, seed=int(name[4:]), min_wavelength_px=4.0)
        interp, const = ir.BILINEAR, True
    else:
        shape, kw, interp, const, _ = MEMBERS[name]
        pair = synth.make_image_pair(*shape, **kw)
    start = pair.pose_init.copy()
    for a in (pair.ref, pair.track, pair.gradx, pair.grady, pair.disparity, start):
        a.setflags(write=False)
    return pair, start, interp, const


@functools.lru_cache(maxsize=None)
def reference_log_length(name):
    pair, start, interp, const = member(name)
    pr = ir.ImageProblem(pair.camera, pair.ref, pair.track, pair.gradx, pair.grady, pair.disparity, interp, disp_const=const)
    return len(pr.solve(start, pair.disparity, max_iter=MAX_ITER)[2])
