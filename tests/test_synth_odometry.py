"""synth.make_odometry_factors is the generator of tools/odometry_chain.py and the documentation: the same construction as the
tests' own _odometry_factors (noisy T_2_1 between consecutive states from poses_gt, SPD stiffness, the prior on state 0)."""
import numpy as np

from ceres_slam_amd import synth
from test_oracle_pose_factors import _odometry_factors


def test_make_odometry_factors_is_the_tests_construction():
    prob = synth.make_problem(9, 300, track_len=5, seed=6)
    for loop in (False, True):
        a, b = _odometry_factors(prob, seed=3, loop=loop, huber=0.05), synth.make_odometry_factors(prob, seed=3, huber=0.05, loop=loop)
        assert len(a) == len(b) == 1 + 8 + int(loop)
        for x, y in zip(a, b):
            assert x["type"] == y["type"] and x["pose"] == y["pose"] and x.get("pose2") == y.get("pose2") and x.get("huber", 0.0) == y.get("huber", 0.0)
            np.testing.assert_allclose(np.asarray(x["data"]), np.asarray(y["data"]), rtol=0, atol=1e-15)      # (two Rodrigues formulas: the last bit)
            np.testing.assert_array_equal(np.asarray(x["stiffness"]).ravel(), np.asarray(y["stiffness"]).ravel())
    chain = synth.make_odometry_factors(prob, prior=False)
    assert len(chain) == 8 and all(f["type"] == 2 and f["pose2"] == f["pose"] + 1 for f in chain)
    for f in chain:       # SPD stiffness, a rigid transform close to the true T_2_1
        S = np.asarray(f["stiffness"]).reshape(6, 6)
        assert np.allclose(S, S.T) and np.linalg.eigvalsh(S).min() > 0
        R = np.asarray(f["data"])[3:].reshape(3, 3)
        np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-12)
