"""CPU checks of the numpy statement of the ImageError blocks (tests/image_reference.py), the truth of
tests/test_gpu_image_alignment.py: its Jacobians against central differences where bilinear sampling is exact, and its
Levenberg-Marquardt loop on the synthetic pair (ceres_slam_amd.synth.make_image_pair)."""
import numpy as np
import pytest

from ceres_slam_amd import synth

import image_reference as ir


def _ramp_problem(rows=24, cols=32):
    """A linear-ramp tracked image with constant gradient images: bilinear sampling is exact, so the residual is a smooth
    function of the pose and the disparity and the analytic Jacobians are its derivatives."""
    gx, gy = 0.013, -0.021
    v, u = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing="ij")
    track = 0.2 + gx * u + gy * v
    rng = np.random.Generator(np.random.PCG64(3))
    ref = rng.random((rows, cols))
    cam = dict(fu=0.6 * cols, fv=0.55 * cols, cu=0.5 * (cols - 1), cv=0.5 * (rows - 1), b=0.54)
    disp = 1.0 + rng.random((rows, cols))
    T = synth.pose_pack(np.array([0.03, -0.02, 0.05]), synth.so3_exp(np.array([0.01, -0.02, 0.015])))
    pr = ir.ImageProblem(cam, ref, track, np.full((rows, cols), gx), np.full((rows, cols), gy), disp, ir.BILINEAR)
    return pr, T, disp


def test_jacobians_equal_central_differences_on_a_ramp():
    pr, T, disp = _ramp_problem()
    r, Jp, Jd, inb = pr.rows(T, disp)
    assert inb.sum() > 0.5 * inb.size and (~inb).sum() > 0       # both kinds of block are present
    h = 1e-6
    # blocks that stay in bounds under every probe (the residual jumps to 0 at the edge)
    keep = inb.copy()
    num_p = np.zeros_like(Jp)
    for c in range(6):
        e = np.zeros(6)
        e[c] = h
        (rp, _), (rm, _) = pr.residuals(ir.se3_plus(T, e, np.float64), disp), pr.residuals(ir.se3_plus(T, -e, np.float64), disp)
        keep &= pr.rows(ir.se3_plus(T, e, np.float64), disp)[3] & pr.rows(ir.se3_plus(T, -e, np.float64), disp)[3]
        num_p[:, c] = (rp - rm) / (2 * h)
    (rp, _), (rm, _) = pr.residuals(T, disp + h), pr.residuals(T, disp - h)
    keep &= pr.rows(T, disp + h)[3] & pr.rows(T, disp - h)[3]
    num_d = (rp - rm) / (2 * h)
    assert keep.sum() > 0.5 * keep.size
    ep, ed = np.abs(Jp - num_p)[keep].max(), np.abs(Jd - num_d)[keep].max()
    print(f"ramp: max |J_pose - central difference| = {ep:.3e}, max |J_disp - central difference| = {ed:.3e}")
    assert ep <= 1e-6 and ed <= 1e-6
    # out of bounds: exact zeros
    assert not r[~inb].any() and not Jp[~inb].any() and not Jd[~inb].any()


def test_elimination_equals_the_full_normal_equations():
    """The closed-form elimination of the disparities against the dense (6 + n) x (6 + n) damped system."""
    pair = synth.make_image_pair(12, 16, seed=1, invalid_fraction=0.1)
    pr = ir.ImageProblem(pair.camera, pair.ref, pair.track, pair.gradx, pair.grady, pair.disparity, ir.BILINEAR)
    st = pr.lm_step(pair.pose_init, pair.disparity, 3.0)
    n = pr.blk.shape[0]
    J = np.zeros((n, 6 + n))
    J[:, :6] = st["Jp"]
    J[np.arange(n), 6 + np.arange(n)] = st["Jd"]
    s = np.concatenate(st["scale"])
    D = np.clip((J * J).sum(0) * s * s, 1e-6, 1e32) / (3.0 * s * s)
    delta = np.linalg.solve(J.T @ J + np.diag(D), -J.T @ st["r"])
    assert np.abs(delta[:6] - st["dp"]).max() <= 1e-10 * np.abs(delta[:6]).max()
    assert np.abs(delta[6:] - st["dd"]).max() <= 1e-10 * np.abs(delta[6:]).max()
    Jd = J @ delta
    assert abs(-(Jd * (st["r"] + Jd / 2)).sum() - st["mcc"]) <= 1e-10 * abs(st["mcc"])


@pytest.mark.parametrize("shape", [(30, 40), (64, 96)])
def test_the_loop_converges_on_the_synthetic_pair(shape):
    pair = synth.make_image_pair(*shape, seed=0)
    pr = ir.ImageProblem(pair.camera, pair.ref, pair.track, pair.gradx, pair.grady, pair.disparity, ir.BILINEAR, disp_const=True)
    T, _, log = pr.solve(pair.pose_init, pair.disparity, max_iter=50)
    err = np.abs(T - pair.pose_true).max()
    print(f"{shape}: {len(log) - 1} iterations, cost {log[0][0]:.4e} -> {log[-1][0]:.4e}, max |pose - true| = {err:.3e}")
    assert len(log) - 1 <= 10
    assert err <= 2e-2


def test_float64_statement_against_long_double():
    """How far the float64 statement sits from the same statement in long double: the floor of what the device bars can show."""
    pair = synth.make_image_pair(64, 96, seed=0, invalid_fraction=0.05)
    out = {}
    for dt in (np.float64, np.longdouble):
        pr = ir.ImageProblem(pair.camera, pair.ref, pair.track, pair.gradx, pair.grady, pair.disparity, ir.BILINEAR, dtype=dt)
        out[dt] = pr.lm_step(pair.pose_init, pair.disparity, 1e4)
    a, b = out[np.float64], out[np.longdouble]
    eS = float(np.abs(a["S"] - b["S"]).max() / np.abs(b["S"]).max())
    ep = float(np.abs(a["dp"] - b["dp"]).max() / np.abs(b["dp"]).max())
    ed = float(np.abs(a["dd"] - b["dd"]).max() / np.abs(b["dd"]).max())
    print(f"float64 against long double at 96 x 64, radius 1e4: S {eS:.2e}, delta_pose {ep:.2e}, delta_disp {ed:.2e}")
    assert eS <= 1e-11 and ep <= 1e-9 and ed <= 1e-9      # a tenth of the device bars (1e-10, 1e-8)
