"""Inputs shared by tests/test_tracks_odometry_reference.py (CPU: the statement alone, and that the seeds chosen here keep the
reference's ambiguous cases within the cap) and tests/test_gpu_track_odometry.py (the device against the statement)."""
import functools

import numpy as np

import hp_frontend as hp
import tracks_odometry_reference as orf
import tracks_stream_reference as sr
from ceres_slam_amd import synth

CAM = dict(fu=700.0, fv=710.0, cu=600.0, cv=180.0, b=0.5)          # fu != fv on purpose
THRESHOLD = 4.0
SIZES = (3, 4, 63, 64, 65, 255, 256, 257, 1025, 4096)               # where the strides (64, 256) and the scans turn over
RANSAC_CASES = ((3, 1),) + tuple((n, 64) for n in SIZES)            # (n, H); with n = 3 the one draw is forced
REFINE_SIZES = (3, 40, 257, 4096)
SEED = {3: 2, 4: 0, 63: 0, 64: 0, 65: 0, 255: 0, 256: 0, 257: 0, 1025: 0, 4096: 0, 40: 0}
FRAME = 5                                                           # the frame index of the synthetic cases' draws


@functools.lru_cache(maxsize=None)
def synthetic(n, outliers=True, noise_px=None):
    """n matches of two states of hp.make_sequence (every landmark seen twice, so half of each state matches): uvd_prev, uvd_cur,
    the true T_1_0.  From n = 63 on every fifth match is an outlier, 25 pixels off in u.  The noise is 0.2 pixel, and 0.01 pixel
    for n = 3 and 4: three points 8 to 40 m away whose disparities are 0.2 pixel off are no congruent triangles any more, and
    the one hypothesis there is would have no inlier."""
    noise_px = (0.01 if n <= 4 else 0.2) if noise_px is None else noise_px
    s = hp.make_sequence(CAM, 2, per_state=2 * n, track=2, noise_px=noise_px, seed=SEED[n])
    a0, a1, a2 = (int(v) for v in s["state_start"])
    ka, kb = hp.match_states(s["point_id"][a0:a1], s["point_id"][a1:a2])
    prev, cur = s["uvd"][a0 + ka].copy(), s["uvd"][a1 + kb].copy()
    assert len(prev) == n
    if outliers and n >= 63:
        cur[::5, 0] += 25.0
    g = s["poses_gt"]
    truth = hp.se3_compose(g[1], np.asarray(oracle_inverse(g[0])))
    for a in (prev, cur):
        a.setflags(write=False)
    return prev, cur, np.asarray(truth, np.float64)


def oracle_inverse(T):
    R, t = np.asarray(T[3:]).reshape(3, 3), np.asarray(T[:3])
    return np.concatenate([-R.T @ t, R.T.ravel()])


@functools.lru_cache(maxsize=None)
def synthetic_reference(n, hypotheses):
    prev, cur, _ = synthetic(n)
    return orf.ransac(CAM, prev, cur, FRAME, hypotheses, THRESHOLD)


def refine_case(m):
    """m matches that are all inliers of the winner (0.02 pixel of noise, no outlier): the refinement runs over exactly m points."""
    return synthetic(m, False, 0.02)


def _uvd(points):
    return np.asarray(hp._project(CAM, hp._f(points)), np.float64)


def degenerate(kind):
    """Lists on which the alignment or the selection meets its edge: (uvd_prev, uvd_cur, hypotheses)."""
    rng = np.random.default_rng(7)
    if kind == "collinear":           # three matches on a line: rank W = 1
        p0 = np.array([[-1.0, 0.2, 10.0], [0.0, 0.2, 12.0], [1.0, 0.2, 14.0]])
        return _uvd(p0), _uvd(p0 + [0.05, 0.0, -0.1]), 1
    if kind == "coincident":          # three times the same match: W = 0
        p0 = np.tile([0.4, -0.3, 9.0], (3, 1))
        return _uvd(p0), _uvd(p0 + [0.05, 0.0, -0.1]), 1
    if kind == "outliers":            # no rigid motion maps any triangle of the one cloud near its partner in the other
        z0, z1 = rng.uniform(6, 30, 24), rng.uniform(6, 30, 24)
        p0 = np.stack([rng.uniform(-0.4, 0.4, 24) * z0, rng.uniform(-0.2, 0.2, 24) * z0, z0], 1)
        p1 = np.stack([rng.uniform(-0.4, 0.4, 24) * z1, rng.uniform(-0.2, 0.2, 24) * z1, z1], 1)
        return _uvd(p0), _uvd(p1), 64
    if kind == "two":
        p0 = np.array([[-1.0, 0.2, 10.0], [1.0, -0.2, 14.0]])
        return _uvd(p0), _uvd(p0 + [0.05, 0.0, -0.1]), 64
    raise KeyError(kind)


def rejected_step_case():
    """A refinement whose first step is rejected: 40 matches of which every fifth is 25 pixels off, all of them declared inliers
    by a threshold of 1e9, so that the minimiser starts from a pose fitted to three points in a cost dominated by the outliers."""
    prev, cur, _ = synthetic(40, outliers=False)
    cur = cur.copy()
    cur[::5, 0] += 25.0
    cur[1::7, 2] *= 0.5
    return prev, cur, 1e9


# ---- the image sequences of the stream tests ---------------------------------------------------------------------------------
PARAMS = dict(fast_threshold=10)
SHAPES = {(64, 96): 6, (96, 128): 4}
HYPOTHESES = 64


@functools.lru_cache(maxsize=None)
def sequence(rows, cols):
    seq = synth.make_stereo_sequence(rows, cols, SHAPES[rows, cols], seed=1)
    for a in (seq.left, seq.right):
        a.setflags(write=False)
    return seq


@functools.lru_cache(maxsize=None)
def statement_pushes(rows, cols, subpixel):
    """The numpy stream's pushes of the sequence with right images."""
    s = sequence(rows, cols)
    st = sr.Stream(SHAPES[rows, cols], refine={} if subpixel else None, **PARAMS)
    return [st.push(s.left[f], right=s.right[f]) for f in range(SHAPES[rows, cols])]
