"""The fused steps of the parallel cyclic reduction keep ONE image of YU^T YL (the block that needs its transpose turns it
on load) and share out their end-of-step stores.  All of that moves bytes, addresses and which wave or workgroup issues a
store; no floating-point operation changes.  So whole solves give the costs and the poses recorded on the commit before
(tests/golden/record_pcr_store_deal_costs.py), bit for bit."""
import json
import os

import numpy as np
import pytest

from ceres_slam_amd import capi, synth
from ceres_slam_amd.solver import StereoBA

pytestmark = pytest.mark.gpu
DRIVER = dict(max_num_iterations=1000, use_nonmonotonic_steps=1)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def chain_problem(blocks):
    """As in tests/test_gpu_pcr_handover.py: k super-blocks, the last one holding a single free pose."""
    n = 12 * (blocks - 1) + 2
    return synth.make_problem(n, 30 * n, track_len=12, seed=3)


def _problem(blocks):
    return synth.make_problem(1022, 10 * 1022, track_len=12, seed=7) if blocks == 86 else chain_problem(blocks)


_solved = {}


def _solve(blocks):
    """One solve per chain, shared by the cost and the pose test."""
    if blocks not in _solved:
        ba = StereoBA.from_synth(_problem(blocks))
        s, log = ba.solve(capi.default_options(**DRIVER))
        st = ba.stats()
        _solved[blocks] = (int(st.pcr_blocks), int(st.pcr_fused), [float(c).hex() for c in log["cost"]], np.array(ba.poses, dtype=np.float64))
        ba.close()
    return _solved[blocks]


CASES = [3, 5, 9, 86]


@pytest.mark.parametrize("blocks", CASES)
def test_costs_are_the_recorded_ones(blocks):
    """3: end blocks only, no tile of YU^T YL exists.  5: the first block with both couplings -- the transposed read
    happens once.  9: three steps, both image sets in turn.  86: two workgroups per block, the other deal."""
    with open(os.path.join(GOLDEN, "pcr_store_deal_costs.json")) as f:
        want = json.load(f)[str(blocks)]
    n, fused, got, _ = _solve(blocks)
    assert n == blocks and fused == 1
    assert got == want


@pytest.mark.parametrize("blocks", CASES)
def test_poses_are_the_recorded_ones(blocks):
    with np.load(os.path.join(GOLDEN, "pcr_store_deal_poses.npz")) as z:
        want = z[str(blocks)]
    n, fused, _, got = _solve(blocks)
    assert n == blocks and fused == 1
    assert np.array_equal(got, want)
