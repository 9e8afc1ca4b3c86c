"""The fused plan of the parallel cyclic reduction keeps its private operands (assembled blocks, Gram products, kept
couplings) as 16-byte tile images (ssba_types.h, PcrFused); the two-launch plan (SSBA_NO_PCR_FUSED=1) never touches
them.  Both must solve alike, at the bar of test_fused_and_two_launch_steps_of_the_parallel_plan_agree
(tests/test_gpu_edge_cases.py), on the smallest chains that reach every loader and store branch of the images."""
import numpy as np
import pytest

from ceres_slam_amd import capi, synth
from ceres_slam_amd.solver import StereoBA

pytestmark = pytest.mark.gpu
DRIVER = dict(max_num_iterations=1000, use_nonmonotonic_steps=1)


def _fused_against_two_launch(monkeypatch, prob, blocks):
    ba = StereoBA.from_synth(prob)
    s, log = ba.solve(capi.default_options(**DRIVER))
    st = ba.stats()
    assert st.general_structure == 0 and st.num_superblocks == blocks and st.pcr_blocks == blocks and st.pcr_fused == 1
    monkeypatch.setenv("SSBA_NO_PCR_FUSED", "1")
    ba2 = StereoBA.from_synth(prob)
    s2, log2 = ba2.solve(capi.default_options(**DRIVER))
    assert s.termination_type == s2.termination_type
    assert s.num_iterations == s2.num_iterations
    assert log["step_is_successful"].tolist() == log2["step_is_successful"].tolist()
    ok = np.asarray(log2["step_is_successful"], dtype=bool)
    ok[0] = True
    np.testing.assert_allclose(log["cost"][ok], log2["cost"][ok], rtol=1e-10)
    np.testing.assert_allclose(log["cost"], log2["cost"], rtol=1e-7)      # rejected candidates far outside the trust region are ill-conditioned
    assert np.abs(ba.poses - ba2.poses).max() < 1e-9
    ba.close()
    ba2.close()


@pytest.mark.parametrize("blocks", [2, 3, 5, 9, 25])
def test_short_chains_reach_every_image_branch(monkeypatch, blocks):
    """12 (k - 1) + 1 free poses (the first pose is constant): k super-blocks, the last one holding a single pose, so the
    identity rows of its padding go through the images.  2, 3: one or two steps, end blocks only (one Gram product each,
    the first step's operands row-major, the second's images).  5: a block with both couplings -- the two orientations of
    YU^T YL are written and consumed.  9, 25: couplings renewed over three and five steps, the assembled block read back
    as an image from the third step on."""
    prob = synth.make_problem(12 * (blocks - 1) + 2, 30 * (12 * (blocks - 1) + 2), track_len=12, seed=3)
    _fused_against_two_launch(monkeypatch, prob, blocks)


@pytest.mark.parametrize("num_poses,blocks", [(1022, 86), (1530, 128)])
def test_two_workgroups_per_block(monkeypatch, num_poses, blocks):
    """More than 85 blocks: two workgroups per block share the Gram tiles (86: the first such chain; 128: the longest plan)."""
    prob = synth.make_problem(num_poses, 10 * num_poses, track_len=12, seed=7)
    _fused_against_two_launch(monkeypatch, prob, blocks)
