"""CPU reference for stereo problems with constant point blocks (ssba_set_point_constant).

A constant point is not part of x, as in Ceres: its Jacobian columns leave the problem, its residual blocks stay in the cost.
np_reference.NumpyBA already selects the landmark columns through its `active` mask (lm_step, solve, dogleg_linearize and
dogleg_solve all go through it), so the reference for any subset is that class with the constant points cleared from the
mask.  tests/test_const_points_reference.py pins it against the C oracle where the oracle has a switch (every point constant).
dense_reduced_system is the reduced camera system the device assembles: H_pp over ALL observations minus W V^-1 W^T over the
free landmarks only, in the unscaled coordinates of ssba_lm_step.
"""
import numpy as np

import np_reference as npr


class ConstPointsBA(npr.NumpyBA):
    def __init__(self, cam, poses, points, obs_pose, obs_point, obs_uvd, S, pose_const=None, huber_a=0.0, point_const=None):
        super().__init__(cam, poses, points, obs_pose, obs_point, obs_uvd, S, pose_const=pose_const, huber_a=huber_a)
        L = points.shape[0]
        self.point_const = np.zeros(L, dtype=bool) if point_const is None else np.asarray(point_const, dtype=bool).copy()
        assert self.point_const.shape == (L,)
        self.active = self.active & ~self.point_const

    @classmethod
    def from_synth(cls, prob, point_const=None, pose_const=None, huber_a=0.0):
        return cls(prob.camera, prob.poses_init, prob.points_init, prob.obs_pose, prob.obs_point, prob.obs_uvd, prob.stiffness(),
                   pose_const=pose_const, huber_a=huber_a, point_const=point_const)


def dense_reduced_system(ba, poses, points, radius, scale=None, min_diag=1e-6, max_diag=1e32, extra_S=None, extra_rhs=None):
    """(S, rhs, dp, dl, scale) of one LM step at `radius` in unscaled coordinates, dense algebra:
         S   = H_pp + D_p - W (V + D_l)^-1 W^T,   rhs = -(g_p - W (V + D_l)^-1 g_l),   S dp = rhs,   dl = -(V + D_l)^-1 (g_l + W^T dp)
    with D = clamp(diag(J^T J) s^2, min, max) / (radius s^2) and the Jacobi scale s = 1 / (1 + sqrt(diag(J^T J))) of this point
    (or the one passed in).  H_pp and g_p sum over every observation of a free pose; W, V, g_l have the columns of the free
    (`active`) landmarks only.  dp is (P, 6), dl (L, 3) with zero rows for constant blocks.
    extra_S / extra_rhs: what residual blocks on poses alone (priors, sun sensor, odometry) add to S and rhs -- their J^T J
    with its damping and -J^T r, which touch no landmark column and so pass through the elimination unchanged."""
    _, r, Jp, Jl = ba.residuals(poses, points, jac=True)
    J = ba.sparse_jacobian(Jp, Jl).toarray()
    nf, L, P = ba.nf, points.shape[0], poses.shape[0]
    keep = np.concatenate([np.ones(6 * nf, bool), np.repeat(ba.active, 3)])
    J = J[:, keep]
    colsq = (J * J).sum(0)
    if scale is None:
        scale = 1.0 / (1.0 + np.sqrt(colsq))
    s2 = scale * scale
    damp = np.clip(colsq * s2, min_diag, max_diag) / (radius * s2)
    H = J.T @ J + np.diag(damp)
    g = J.T @ r.reshape(-1)
    n = 6 * nf
    Hpp, W, V = H[:n, :n], H[:n, n:], H[n:, n:]
    if V.shape[0]:
        Vi = np.linalg.inv(V)       # block diagonal (3 x 3 per landmark)
        S = Hpp - W @ Vi @ W.T
        rhs = -(g[:n] - W @ Vi @ g[n:])
    else:
        Vi = np.zeros((0, 0))
        S, rhs = Hpp.copy(), -g[:n]
    if extra_S is not None:
        S = S + extra_S
    if extra_rhs is not None:
        rhs = rhs + extra_rhs
    x = np.linalg.solve(S, rhs)
    y = -Vi @ (g[n:] + W.T @ x)
    dp = np.zeros((P, 6))
    dp[ba.free] = x.reshape(nf, 6)
    dl = np.zeros((L, 3))
    dl[ba.active] = y.reshape(-1, 3)
    return S, rhs, dp, dl, scale


def undamped_reduced_system(ba, poses, points):
    """S at radius -> infinity (no damping): its inverse holds the pose blocks of the covariance."""
    return dense_reduced_system(ba, poses, points, 1e300, scale=np.ones(6 * ba.nf + 3 * int(ba.active.sum())), min_diag=0.0)[0]


# ---- SUBSPACE_DOGLEG [Ceres 1.x dogleg_strategy.cc: ComputeSubspaceModel, ComputeSubspaceDoglegStep], in the D-scaled space
# ---- of np_reference.dogleg_linearize; np_reference has the TRADITIONAL loop only
def subspace_model(state):
    """Orthonormal basis of span(gradient_, gauss_newton_step_) (the longer vector first, as the pivoted QR takes them), the
    gradient g and the Hessian B of the model restricted to it.  one_dim: the two vectors are parallel."""
    D, grad, gn, Js = (state[k] for k in ("D", "grad", "gn", "Js"))
    a, b = (grad, gn) if grad @ grad >= gn @ gn else (gn, grad)
    an = np.linalg.norm(a)
    if not an > 0:
        return None
    e0 = a / an
    w = b - (e0 @ b) * e0
    wn = np.linalg.norm(w)
    if wn <= 2.0 * np.finfo(float).eps * an:
        return dict(one_dim=True)
    basis = np.stack([e0, w / wn], 1)
    JB = Js @ (basis / D[:, None])
    return dict(one_dim=False, basis=basis, g=basis.T @ grad, B=JB.T @ JB)


def subspace_boundary_minimum(model, radius):
    """FindMinimumOnTrustRegionBoundary: the candidates are -(B + y I)^-1 g for the real parts y of the roots of the boundary
    polynomial, compared after projection onto the boundary; the unprojected one is returned, as Ceres does."""
    B, g = model["B"], model["g"]
    detB, trB, r2 = B[0, 0] * B[1, 1] - B[0, 1] ** 2, B[0, 0] + B[1, 1], radius * radius
    Badj = np.array([[B[1, 1], -B[0, 1]], [-B[0, 1], B[0, 0]]])
    poly = [r2, 2.0 * r2 * trB, r2 * (trB * trB + 2.0 * detB) - g @ g, -2.0 * (g @ Badj @ g - r2 * detB * trB),
            r2 * detB * detB - (Badj @ g) @ (Badj @ g)]
    best, arg = np.inf, None
    for y in np.roots(poly).real:
        x = -np.linalg.solve(B + y * np.eye(2), g)
        nx = np.linalg.norm(x)
        if nx > 0:
            sx = radius / nx * x
            f = 0.5 * sx @ B @ sx + g @ sx
            if f < best:
                best, arg = f, x
    return arg


def dogleg_subspace_step(state, model, radius):
    """ComputeSubspaceDoglegStep: (step in D-scaled space, the same in Jacobi-scaled parameters, model cost change,
    dogleg_step_norm_)."""
    D, grad, gn, Js, rv = (state[k] for k in ("D", "grad", "gn", "Js", "rv"))
    gnorm, nnorm = np.linalg.norm(grad), np.linalg.norm(gn)
    if nnorm <= radius:
        step, norm = gn.copy(), nnorm
    elif model["one_dim"]:
        step, norm = -(radius / gnorm) * grad, radius
    else:
        m = subspace_boundary_minimum(model, radius)
        if m is None:
            step, _, _ = npr.dogleg_traditional_step(state, radius)
            norm = np.linalg.norm(step)
        else:
            step, norm = model["basis"] @ m, radius
    step_js = step / D
    mdl = Js @ step_js
    return step, step_js, -mdl @ (rv + 0.5 * mdl), norm


def dogleg_solve(ba, dogleg_type=0, max_iter=1000, nonmonotonic=True, f_tol=1e-6, p_tol=1e-8, min_rd=1e-3, min_diag=1e-6, max_diag=1e32):
    """np_reference.dogleg_solve for TRADITIONAL_DOGLEG (0); the same trust-region loop with the subspace step for
    SUBSPACE_DOGLEG (1).  Returns (poses, points, [(cost, step_is_successful)])."""
    if dogleg_type == 0:
        return npr.dogleg_solve(ba, max_iter=max_iter, nonmonotonic=nonmonotonic, f_tol=f_tol, p_tol=p_tol, min_rd=min_rd,
                                min_diag=min_diag, max_diag=max_diag)
    x_p, x_l = ba.poses.copy(), ba.points.copy()
    radius, mu, reuse, scale = 1e4, 1e-8, False, None
    max_nm = 5 if nonmonotonic else 0
    x_cost, _ = ba.residuals(x_p, x_l)
    minimum = current = reference = candidate = x_cost
    acc_ref = acc_cand = 0.0
    n_nm = 0
    log = [(x_cost, False)]
    nf, L = ba.nf, x_l.shape[0]
    keep = np.concatenate([np.ones(6 * nf, bool), np.repeat(ba.active, 3)])
    x_norm = np.linalg.norm(np.concatenate([x_p[ba.free].ravel(), x_l[ba.active].ravel()]))
    state = model = None
    for it in range(1, max_iter + 1):
        failed = False
        if not reuse:
            reuse = True
            state = npr.dogleg_linearize(ba, x_p, x_l, keep, scale, mu, min_diag, max_diag)
            scale = state["scale"]
            model = subspace_model(state)
            failed = model is None                     # LINEAR_SOLVER_FAILURE
        if not failed:
            step, step_js, mcc, step_norm_scaled = dogleg_subspace_step(state, model, radius)
        if failed or not (mcc > 0):
            mu *= 10.0
            reuse = False
            log.append((x_cost, False))
            continue
        delta = np.zeros(6 * nf + 3 * L)
        delta[keep] = step_js * scale
        dp = np.zeros((x_p.shape[0], 6))
        dp[ba.free] = delta[: 6 * nf].reshape(nf, 6)
        c_p, c_l = ba.plus(x_p, x_l, dp, delta[6 * nf:].reshape(L, 3))
        c_cost, _ = ba.residuals(c_p, c_l)
        stepn = np.sqrt(((c_p[ba.free] - x_p[ba.free]) ** 2).sum() + ((c_l[ba.active] - x_l[ba.active]) ** 2).sum())
        if stepn <= p_tol * (x_norm + p_tol) or abs(x_cost - c_cost) <= f_tol * x_cost:
            break
        rd = max((current - c_cost) / mcc, (reference - c_cost) / (acc_ref + mcc))
        if rd > min_rd:
            x_p, x_l, x_cost = c_p, c_l, c_cost
            x_norm = np.linalg.norm(np.concatenate([x_p[ba.free].ravel(), x_l[ba.active].ravel()]))
            if rd < 0.25:
                radius *= 0.5
            if rd > 0.75:
                radius = max(radius, 3.0 * step_norm_scaled)
            mu = max(1e-8, 2.0 * mu / 10.0)
            reuse = False
            current = c_cost
            acc_cand += mcc
            acc_ref += mcc
            if current < minimum:
                minimum, n_nm, candidate, acc_cand = current, 0, current, 0.0
            else:
                n_nm += 1
                if current > candidate:
                    candidate, acc_cand = current, 0.0
            if n_nm == max_nm:
                reference, acc_ref = candidate, acc_cand
            log.append((x_cost, True))
        else:
            radius *= 0.5
            reuse = True
            log.append((c_cost, False))
    return x_p, x_l, log
