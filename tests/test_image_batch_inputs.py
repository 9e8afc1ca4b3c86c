"""What tests/test_gpu_image_batch.py relies on, asserted on the numpy loop tests/image_reference.py alone: the members of its
batch end at different iterations (BILINEAR, start pose_init, max_iter = 50), so a batch that stopped every member at the
first termination, or ran every member to the last, could not pass there."""
import pytest

import image_batch_members as bm


@pytest.mark.parametrize("name", bm.FIVE)
def test_log_entries_of_the_reference_loop(name):
    assert bm.reference_log_length(name) == bm.MEMBERS[name][4]


def test_the_counts_differ_and_one_member_runs_to_the_cap():
    counts = [bm.MEMBERS[n][4] for n in bm.FIVE]
    assert counts == [6, 8, 9, 18, 51]
    assert len(set(counts)) == len(counts) and max(counts) == bm.MAX_ITER + 1
