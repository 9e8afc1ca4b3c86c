"""What a fused step of the parallel cyclic reduction hands to the next one: its operands are resolved on the host and
passed with the launch (FusedStep, ssba_bcr_mfma.hip), and the tile images leave write-through.  The two-launch plan
(SSBA_NO_PCR_FUSED=1) knows nothing of either, so both must solve alike, at the bars of tests/test_gpu_pcr_tile_images.py;
and since the change only moves bytes and addresses, the costs of the short chains are the ones recorded before it, bit
for bit."""
import json
import os

import numpy as np
import pytest

from ceres_slam_amd import capi, synth
from ceres_slam_amd.solver import StereoBA

pytestmark = pytest.mark.gpu
DRIVER = dict(max_num_iterations=1000, use_nonmonotonic_steps=1)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pcr_handover_costs.json")


def chain_problem(blocks):
    """12 (k - 1) + 2 poses, 30 landmarks per pose, tracks of 12: k super-blocks, the last one holding a single free pose."""
    n = 12 * (blocks - 1) + 2
    return synth.make_problem(n, 30 * n, track_len=12, seed=3)


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


@pytest.mark.parametrize("blocks", [3, 5, 9])
def test_short_chains(monkeypatch, blocks):
    """3: end blocks only, no YU^T YL is produced.  5: the first chain with a block that has both couplings -- both
    orientations of YU^T YL are read once.  9: couplings renewed over three steps, both image sets in turn."""
    _fused_against_two_launch(monkeypatch, chain_problem(blocks), blocks)


def test_two_workgroups_per_block(monkeypatch):
    """86 blocks: two workgroups per block, the other deal of the Gram tiles."""
    _fused_against_two_launch(monkeypatch, synth.make_problem(1022, 10 * 1022, track_len=12, seed=7), 86)


@pytest.mark.parametrize("blocks", [5, 9])
def test_costs_are_the_recorded_ones(blocks):
    """The cost column of the whole solve against tests/golden/pcr_handover_costs.json (hex floats, written by
    tests/golden/record_pcr_handover_costs.py on the commit before this hand-over): bit for bit."""
    with open(GOLDEN) as f:
        want = json.load(f)[str(blocks)]
    ba = StereoBA.from_synth(chain_problem(blocks))
    s, log = ba.solve(capi.default_options(**DRIVER))
    st = ba.stats()
    assert st.pcr_blocks == blocks and st.pcr_fused == 1
    got = [float(c).hex() for c in log["cost"]]
    ba.close()
    assert got == want
