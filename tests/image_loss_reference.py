"""ImageError blocks under ceres::HuberLoss(a), on top of tests/image_reference.py: the truth for the LOSS = true kernels of
ceres_slam_amd/csrc/ssba_image.hip.  Ceres applies a loss through its corrector; with rho'' <= 0 (Huber) that is a plain scaling
of the block's row, exactly as on the stereo rows (ssba_device.h: obs_linearize_S).  For an in-bounds block with raw residual r:

    r^2 > a^2 (strictly):  sc = sqrt(max(DBL_MIN, a / |r|)),  r~ = sc r,  J~_pose = sc J_pose,  J~_disp = sc J_disp,
                           the block's cost is 1/2 rho = 1/2 (2 a |r| - a^2)
    otherwise              the row is unchanged, the block's cost is 1/2 r^2

Out-of-bounds rows (r = 0, J = 0) stay as they are; a <= 0 is the NULL loss and gives image_reference's numbers bit for bit.
The step and the loop are image_reference's, fed with the corrected rows: sums, Jacobi scales, damping, V, the elimination of the
disparity, delta_d, the gradient max norm and the model cost change.  The cost of an iterate or a candidate is 1/2 sum rho of its
raw residuals.  Every function takes the dtype of the problem, as that file does.

min_loss_margin records the least | |r| - a | over every in-bounds row the problem evaluated (rows and candidate residuals), as
min_margin does for NEAREST: a test asserts on it that its inputs sit away from the branch."""
import numpy as np

import image_reference as ir
import pyramid_reference as pyr

DBL_MIN = np.finfo(np.float64).tiny


def half_rho(r, a, dtype):
    """1/2 rho(r^2) per row for raw residuals r (a > 0)."""
    r = np.asarray(r, dtype=dtype)
    a = dtype(a)
    return np.where(r * r > a * a, (2 * a * np.abs(r) - a * a) / 2, r * r / 2)


def corrector_scale(r, a, dtype):
    """sc per row: 1 where the row is left alone."""
    r = np.asarray(r, dtype=dtype)
    a = dtype(a)
    sc = np.ones(r.shape, dtype=dtype)
    k = r * r > a * a
    sc[k] = np.sqrt(np.maximum(dtype(DBL_MIN), a / np.abs(r[k])))
    return sc


class ImageLossProblem(ir.ImageProblem):
    def __init__(self, cam, ref, track, gradx, grady, disparity, interp=ir.BILINEAR, disp_const=False, dtype=np.float64, huber_a=0.0):
        super().__init__(cam, ref, track, gradx, grady, disparity, interp, disp_const, dtype)
        self.huber_a = float(huber_a) if huber_a > 0 else 0.0
        self.min_loss_margin = np.inf

    def _note_loss_margin(self, r, inb):
        if self.huber_a > 0 and inb.any():
            m = np.abs(np.abs(r[inb].astype(np.float64)) - self.huber_a).min()
            self.min_loss_margin = min(self.min_loss_margin, float(m))

    def raw_rows(self, T, disp):
        return super().rows(T, disp)

    def residuals(self, T, disp):
        """The raw residuals of every block and the cost 1/2 sum rho."""
        r, cost = super().residuals(T, disp)
        if self.huber_a > 0:
            d = np.asarray(disp, dtype=self.dtype).reshape(-1)[self.blk]
            _, _, u, v = self.project(T, d)
            self._note_loss_margin(r, self.in_bounds(u, v))
            cost = half_rho(r, self.huber_a, self.dtype).sum()
        return r, cost

    def rows(self, T, disp):
        """The corrected rows r~ (n), J~_pose (n, 6), J~_disp (n) and the in-bounds mask."""
        r, Jp, Jd, inb = super().rows(T, disp)
        self._raw_cost = (r * r).sum() / 2
        if self.huber_a > 0:
            self._note_loss_margin(r, inb)
            self._raw_cost = half_rho(r, self.huber_a, self.dtype).sum()
            sc = corrector_scale(r, self.huber_a, self.dtype)
            r, Jp, Jd = r * sc, Jp * sc[:, None], Jd * sc
        return r, Jp, Jd, inb

    def lm_step(self, T, disp, radius, scale=None, min_diag=1e-6, max_diag=1e32):
        """image_reference's step on the corrected rows; out["cost"] is 1/2 sum rho at (T, disp)."""
        out = super().lm_step(T, disp, radius, scale, min_diag, max_diag)
        out["cost"] = self._raw_cost
        return out


def coarse_to_fine(levels, cam0, pose0, coarsest, base, interp=ir.BILINEAR, disp_const=True, max_iter=50, huber_a=0.0):
    """pyramid_reference.coarse_to_fine with one width on every level's blocks (intensities do not scale with the level).
    Returns (pose, base disparity, [log per level], least loss margin over the levels)."""
    T = np.asarray(pose0, dtype=np.float64).copy()
    logs, d, margin = [], levels[base]["disparity"], np.inf
    for l in range(coarsest, base - 1, -1):
        L = levels[l]
        pr = ImageLossProblem(pyr.level_camera(cam0, l), L["ref"], L["track"], L["gradx"], L["grady"], L["disparity"], interp,
                              disp_const=True if l > base else disp_const, huber_a=huber_a)
        T, d, log = pr.solve(T, L["disparity"], max_iter=max_iter)
        logs.append(log)
        margin = min(margin, pr.min_loss_margin)
    return T, d, logs, margin
