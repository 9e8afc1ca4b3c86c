"""ssba_pose_covariance and ssba_covariance_blocks take their columns of Sigma from one sweep routine per layout, and every
begin sequence is one function.  That moved host code only: which unit column goes where, the order of the sweeps and every
kernel are as they were.  So on every layout both calls return the values and the status codes recorded on the commit before
(tests/golden/record_covariance_routes.py writes tests/golden/covariance_routes.npz), bit for bit.

Shapes: the smallest that cross every chunk boundary of the sweeps -- a window of 48 poses with six far columns (two sweeps of
5), 30 columns on the general layout (three solves of 10), nine on a solved wide handle (two sweeps of 8) -- and the smallest
problems of the pose-only and the image tests."""
import functools
import os

import numpy as np
import pytest

from ceres_slam_amd import capi, synth
from ceres_slam_amd.solver import StereoBA

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "covariance_routes.npz")


def _status(call):
    try:
        call()
    except capi.SsbaError as e:
        return np.array(e.status)
    return np.array(0)


def _diag(poses):
    return [(("pose", int(k)), ("pose", int(k))) for k in poses]


def _windowed():
    """47 free poses in four super-blocks of 12.  The request: blocks inside the band; six (pose, pose) blocks from super-block
    0 to six different poses of super-blocks 2 and 3, whose columns take a sweep of 5 and a sweep of 1; one (pose, point) and
    one (point, point) block.  Handle a asks ssba_pose_covariance first, handle b ssba_covariance_blocks: either call adds the
    multi-right-hand-side buffers, and the second request on each handle finds them there."""
    prob = synth.make_problem(48, 30 * 48, track_len=12, seed=5)
    j = int(prob.obs_point[np.nonzero(prob.obs_pose == 10)[0][0]])
    pairs = _diag([1, 24, 47]) + [(("pose", 11), ("pose", 14)), (("pose", 30), ("pose", 20))]
    pairs += [(("pose", a), ("pose", b)) for a, b in [(1, 30), (2, 31), (3, 40), (41, 4), (5, 45), (6, 47)]]
    pairs += [(("pose", 10), ("point", j)), (("point", j), ("point", j))]
    out = {}
    for name in "ab":
        ba = StereoBA.from_synth(prob, device=0)
        assert ba.stats().general_structure == 0 and ba.stats().num_free_poses == 47
        ba.solve(capi.default_options(max_num_iterations=1000, use_nonmonotonic_steps=1))
        if name == "a":
            for k in (1, 24, 47):
                out[f"a_pose_{k}"] = ba.pose_covariance(k)
            out["a_status_constant_pose"] = _status(lambda: ba.pose_covariance(0))
        for ask in (1, 2):
            for i, blk in enumerate(ba.covariance_blocks(pairs)):
                out[f"{name}_blocks{ask}_{i}"] = blk
        if name == "b":
            out["b_pose_1"] = ba.pose_covariance(1)
        ba.close()
    return out


def _general():
    """The 30-pose problem of test_pose_covariance_on_the_general_path: per-point stiffness, no constant pose, a prior."""
    from test_gpu_general_structure import _per_point_stiffness
    from test_oracle_pose_factors import _sun_problem
    P = 30
    prob, factors = _sun_problem(P=P, L=60 * P, seed=7)
    ba = StereoBA(prob.camera, prob.poses_init.copy(), prob.points_init.copy(), prob.obs_pose, prob.obs_point, prob.obs_uvd,
                  _per_point_stiffness(prob, seed=3), pose_const=np.zeros(P, dtype=np.uint8), pose_factors=factors)
    assert ba.stats().general_structure == 1
    ba.solve(capi.default_options(max_num_iterations=1000, use_nonmonotonic_steps=1, trust_region_strategy_type=1, dogleg_type=1))
    out = {f"pose_{k}": ba.pose_covariance(k) for k in (1, P // 2, P - 1)}
    out["diagonal"] = np.array(ba.covariance_blocks(_diag(range(P))))
    ba.close()
    return out


def _wide():
    """13 free poses on one 144-row super-block, after the solve (the handle is shared with tests/test_gpu_wide_covariance.py
    and only read)."""
    from test_gpu_wide_covariance import CASES, _solved_wide
    case = min(c for c in CASES if c[0] - 1 >= 9)
    prob, ba = _solved_wide(case)
    assert ba.stats().wide_superblocks > 0
    out = {f"pose_{k}": ba.pose_covariance(k) for k in (1, case[0] - 1)}
    out["diagonal"] = np.array(ba.covariance_blocks(_diag(range(1, 10))))
    return out


def _pose_only():
    from test_gpu_pose_only import _shape
    prob, const = _shape("1x30")
    ba = StereoBA(prob.camera, prob.poses_init.copy(), prob.points_init.copy(), prob.obs_pose, prob.obs_point, prob.obs_uvd,
                  prob.stiffness(), pose_const=const, points_const=True)
    assert ba.stats().general_structure == 3
    out = {"pose_0": ba.pose_covariance(0), "blocks_0": ba.covariance_blocks(_diag([0]))[0]}
    ba.close()
    return out


def _image():
    import image_reference as ir
    from test_gpu_image_alignment import _handle
    out = {}
    for name in ("8x6", "40x30"):
        ba = _handle(name, ir.BILINEAR, True)
        out[f"pose_{name}"] = ba.pose_covariance(0)
        if name == "8x6":
            out["status_covariance_blocks"] = _status(lambda: ba.covariance_blocks(_diag([0])))
        ba.close()
    ba = _handle("8x6", ir.BILINEAR, False)
    out["status_free_disparities"] = _status(lambda: ba.pose_covariance(0))
    ba.close()
    return out


ROUTES = dict(windowed=_windowed, general=_general, wide=_wide, pose_only=_pose_only, image=_image)


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("route", list(ROUTES))
def test_route_returns_the_recorded_bits(route):
    got = ROUTES[route]()
    want = {k[len(route) + 1:]: v for k, v in _golden().items() if k.startswith(route + ".")}
    assert sorted(got) == sorted(want)
    for k in sorted(got):
        assert np.array_equal(np.asarray(got[k]), want[k]), (route, k)
    assert any(np.asarray(v).any() for v in got.values())
