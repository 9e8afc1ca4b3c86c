"""The statement of the streaming odometry of libssba_tracks.so (include/ssba_tracks.h, "Odometry").

The draws are exact integers.  Hypotheses, counts, bands and the winner come from hp_frontend (long double): align3 / ransac_pair.
The refinement is the C oracle's Levenberg-Marquardt on the two-view problem: poses (identity, T) with pose_const = [1, 0], one
point per inlier started at its triangulation in frame k - 1, the 2 m observations, stiffness I / sqrt(variance), solved under
oracle.default_options(max_num_iterations=...)."""
import numpy as np

import hp_frontend as hp
from oracle import oracle

OK, FIRST_FRAME, FEW_MATCHES, FEW_INLIERS, NUMERICAL = range(5)
IDENTITY = hp.IDENTITY
M32 = 0xFFFFFFFF


def mix(x):
    """The 32-bit mixer, on an array of Python-int-valued uint64s."""
    x = np.asarray(x, dtype=np.uint64) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(M32)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    return x


def draws(frame_index, hypotheses, n):
    """(hypotheses, 3) int64: three distinct indices below n >= 3 per hypothesis, counter c = 3 (f H + h) mod 2^32."""
    assert n >= 3
    h = np.arange(hypotheses, dtype=np.uint64)
    c = (np.uint64(3) * ((np.uint64(frame_index & M32) * np.uint64(hypotheses) + h) & np.uint64(M32))) & np.uint64(M32)
    i0 = (mix(c) % np.uint64(n)).astype(np.int64)
    i1 = (mix((c + np.uint64(1)) & np.uint64(M32)) % np.uint64(n - 1)).astype(np.int64)
    i1 += i1 >= i0
    i2 = (mix((c + np.uint64(2)) & np.uint64(M32)) % np.uint64(n - 2)).astype(np.int64)
    i2 += i2 >= np.minimum(i0, i1)
    i2 += i2 >= np.maximum(i0, i1)
    return np.stack([i0, i1, i2], axis=1)


def matches(prev_push, cur_push):
    """The ids present in both pushes' outputs, in the current push's order: (uvd_prev, uvd_cur), paired by position.
    A push is (ids, uvd, dropped)."""
    where = {int(t): k for k, t in enumerate(prev_push[0].tolist())}
    cur = [k for k, t in enumerate(cur_push[0].tolist()) if int(t) in where]
    prev = [where[int(cur_push[0][k])] for k in cur]
    return np.ascontiguousarray(prev_push[1][prev]).reshape(-1, 3), np.ascontiguousarray(cur_push[1][cur]).reshape(-1, 3)


def triangulate64(cam, uvd):
    """StereoCamera::triangulate in IEEE doubles, the operations in the device's order (no sum follows a product, so nothing can
    be contracted): the device's points to the bit."""
    uvd = np.asarray(uvd, dtype=np.float64).reshape(-1, 3)
    bod = cam["b"] / uvd[:, 2]
    return np.stack([(uvd[:, 0] - cam["cu"]) * bod, (uvd[:, 1] - cam["cv"]) * bod * (cam["fu"] / cam["fv"]), cam["fu"] * bod], axis=1)


def ransac(cam, uvd_prev, uvd_cur, frame_index, hypotheses, threshold):
    """hp.ransac_pair over this rule's draws, on the fp64 points; None below three matches."""
    n = len(uvd_prev)
    if n < 3:
        return None
    with np.errstate(all="ignore"):
        p0, p1 = triangulate64(cam, uvd_prev), triangulate64(cam, uvd_cur)
        r = hp.ransac_pair(cam, p0, p1, draws(frame_index, hypotheses, n), threshold)
    r["p0"], r["p1"] = p0, p1
    return r


def refine(cam, uvd_prev, uvd_cur, inlier, T_start, variance=4.0, iterations=20):
    """The oracle's solve of the two-view problem over the flagged matches.  Returns (summary, log, T)."""
    idx = np.nonzero(np.asarray(inlier))[0]
    m = len(idx)
    pts = triangulate64(cam, np.asarray(uvd_prev)[idx])
    obs_pose = np.tile(np.array([0, 1], np.uint32), m)
    obs_point = np.repeat(np.arange(m, dtype=np.uint32), 2)
    obs_uvd = np.stack([np.asarray(uvd_prev, np.float64)[idx], np.asarray(uvd_cur, np.float64)[idx]], axis=1).reshape(-1, 3)
    prob = oracle.OracleProblem(cam, np.stack([IDENTITY, np.asarray(T_start, np.float64)]), pts, obs_pose, obs_point, obs_uvd, np.eye(3) / np.sqrt(variance),
                                pose_const=np.array([1, 0], np.uint8))
    summary, log = prob.solve(oracle.default_options(max_num_iterations=int(iterations)))
    return summary, log, prob.poses[1].copy()


def compose(Ta, Tb):
    """Ta o Tb in fp64, the device's order of operations up to contraction."""
    return np.asarray(hp.se3_compose(np.asarray(Ta, np.float64), np.asarray(Tb, np.float64)), np.float64)


def pose_error(T, truth):
    """(max |dt|, max |dR|)"""
    d = np.abs(np.asarray(T, np.float64) - np.asarray(truth, np.float64))
    return float(d[:3].max()), float(d[3:].max())
