"""What solver.ImageSequence and solver.stereo_sgbm_batch hand to the C calls, and the chunk arithmetic of the batched matcher
(include/ssba.h: 12 bytes per (row, computable column, disparity) and pair; capi.sgbm_chunk_pairs mirrors sgbm_chunk_pairs of
ceres_slam_amd/csrc/ssba_sgbm.hip).  No device is needed."""
import numpy as np
import pytest

from ceres_slam_amd import capi, synth
from ceres_slam_amd.solver import pack_frames


def test_frame_major_packing():
    seq = synth.make_stereo_sequence(24, 40, 4, seed=2)
    lefts, rights = [seq.left[k] for k in range(4)], [seq.right[k] for k in range(4)]
    L, R = pack_frames(lefts, rights)
    assert L.shape == (4, 24, 40) and R.shape == (3, 24, 40) and L.dtype == R.dtype == np.uint8
    assert L.flags.c_contiguous and R.flags.c_contiguous
    flat = L.reshape(-1)
    for k in range(4):                                            # frame k starts at k * rows * cols: one stride
        assert flat[k * 960:(k + 1) * 960].tobytes() == lefts[k].tobytes()
    for k in range(3):
        assert R.reshape(-1)[k * 960:(k + 1) * 960].tobytes() == rights[k].tobytes()
    L2, R2 = pack_frames(lefts, rights[:3])                       # the last right frame is never needed
    assert L2.tobytes() == L.tobytes() and R2.tobytes() == R.tobytes()
    La, Ra = pack_frames(seq.left, seq.right)                     # stacked arrays
    assert La.tobytes() == L.tobytes() and Ra.tobytes() == R.tobytes()
    strided = [a[:, ::2] for a in lefts]                          # non-contiguous views are packed, not passed on
    Ls, _ = pack_frames(strided, [a[:, ::2] for a in rights])
    assert Ls.flags.c_contiguous and Ls[2].tobytes() == np.ascontiguousarray(strided[2]).tobytes()


def test_packing_refusals():
    a = np.zeros((24, 40), np.uint8)
    for lefts, rights in [([a], [a]), ([a, a, a], [a]), ([a, a], [a, a, a]), ([a, a], [a[:, :30]]), ([a, a.astype(np.float64)], [a]),
                          ([a, a], [np.zeros((2, 24, 40), np.uint8)])]:
        with pytest.raises(ValueError):
            pack_frames(lefts, rights)


def test_pair_bytes_are_the_recorded_figures():
    """17.6 MB at 310 x 93 with D 64, 642 MB at 1242 x 375 with D 128 (six 16-bit volumes)."""
    assert capi.sgbm_pair_bytes(93, 310, 64) == 12 * 93 * 246 * 64 == 17570304
    assert capi.sgbm_pair_bytes(375, 1242, 128) == 12 * 375 * 1114 * 128 == 641664000
    assert round(17570304 / 1e6, 1) == 17.6 and round(641664000 / 1e6) == 642
    assert capi.sgbm_pair_bytes(18, 120, 48, min_disparity=4) == 12 * 18 * 68 * 48


def test_chunk_arithmetic():
    small, large = 17570304, 641664000
    assert capi.sgbm_chunk_pairs(16, 0, 93, 310, 64) == 16                       # 1 GiB holds 61 such pairs: one chunk
    assert (1 << 30) // small == 61
    assert capi.sgbm_chunk_pairs(100, 0, 93, 310, 64) == 61
    assert capi.sgbm_chunk_pairs(4, 0, 375, 1242, 128) == 1                      # the default holds one large pair: it chunks
    assert capi.sgbm_chunk_pairs(4, 2 * large, 375, 1242, 128) == 2
    assert capi.sgbm_chunk_pairs(4, 2 * large - 1, 375, 1242, 128) == 1
    assert capi.sgbm_chunk_pairs(4, large, 375, 1242, 128) == 1
    assert capi.sgbm_chunk_pairs(5, 2 * small, 93, 310, 64) == 2                 # chunks of 2, 2, 1
    assert capi.sgbm_chunk_pairs(1, 1 << 40, 93, 310, 64) == 1
    assert capi.sgbm_chunk_pairs(10 ** 6, 1 << 62, 9, 17, 16) == capi.SGBM_MAX_CHUNK == 65535
    with pytest.raises(ValueError, match=str(large)):
        capi.sgbm_chunk_pairs(4, large - 1, 375, 1242, 128)
    with pytest.raises(ValueError):
        capi.sgbm_chunk_pairs(0, 0, 93, 310, 64)
    with pytest.raises(ValueError):
        capi.sgbm_chunk_pairs(2, 0, 8, 16, 16)                                   # no computable column
