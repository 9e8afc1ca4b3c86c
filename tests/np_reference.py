"""Independent numpy/scipy restatement used to cross-check the C oracle.

Deliberately written a different way from oracle/ssba_oracle.c: residuals are
evaluated through the reference's *global* 12+3 parameterisation and the
Jacobians come from complex-step differentiation through ``Plus`` (the route
Ceres's AutoDiffCostFunction + AutoDiffLocalParameterization take), the damped
normal equations are solved WITHOUT a Schur complement by a sparse direct solve,
and the trust-region loop is re-implemented on top of that.

Citations are into /root/reference.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

EPS = np.finfo(np.float64).eps


def wedge(phi):
    # so3group.hpp:248-254
    return np.array([[0, -phi[2], phi[1]], [phi[2], 0, -phi[0]], [-phi[1], phi[0], 0]], dtype=phi.dtype)


def so3_exp(phi):
    # so3group.hpp:273-291; complex-safe (norm via sqrt of sum of squares)
    angle = np.sqrt(phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2])
    if abs(angle) <= EPS:
        return np.eye(3, dtype=phi.dtype) + wedge(phi)
    a = phi / angle
    return np.cos(angle) * np.eye(3) + (1 - np.cos(angle)) * np.outer(a, a) + np.sin(angle) * wedge(a)


def se3_plus(T, eps):
    # perturbations.hpp:61-62 with se3group.hpp:176-183,323-325
    t, R = T[:3], T[3:].reshape(3, 3)
    E = so3_exp(eps[3:])
    return np.concatenate([E @ t + eps[:3], (E @ R).reshape(9)])


def residual_global(cam, T, p, z, S):
    # stereo_reprojection_error.hpp:38-50 ; stereo_camera.hpp:79-84
    t, R = T[:3], T[3:].reshape(3, 3)
    q = R @ p + t
    iz = 1.0 / q[2]
    pred = np.array([cam["fu"] * q[0] * iz + cam["cu"], cam["fv"] * q[1] * iz + cam["cv"], cam["fu"] * cam["b"] * iz])
    return S @ (pred - z)


def jacobians_complex_step(cam, T, p, z, S, h=1e-30):
    """Local Jacobians d r / d eps (3x6) and d r / d p (3x3) by complex step.

    At eps = 0 the first-order branch of so3_exp is taken, exactly as when Ceres
    evaluates the plus-Jacobian with Jets.
    """
    Jp, Jl = np.zeros((3, 6)), np.zeros((3, 3))
    Tc, pc = T.astype(complex), p.astype(complex)
    for c in range(6):
        e = np.zeros(6, dtype=complex)
        e[c] = 1j * h
        Jp[:, c] = residual_global(cam, se3_plus(Tc, e), pc, z, S).imag / h
    for c in range(3):
        d = pc.copy()
        d[c] += 1j * h
        Jl[:, c] = residual_global(cam, Tc, d, z, S).imag / h
    return Jp, Jl


def huber(a, s):
    # [Ceres loss_function.cc]
    b = a * a
    if s > b:
        r = np.sqrt(s)
        rho1 = max(np.finfo(np.float64).tiny, a / r)
        return 2 * a * r - b, rho1, -rho1 / (2 * s)
    return s, 1.0, 0.0


class NumpyBA:
    """Whole-problem evaluation with vectorised closed forms + sparse algebra."""

    def __init__(self, cam, poses, points, obs_pose, obs_point, obs_uvd, S, pose_const=None, huber_a=0.0):
        self.cam = cam
        self.poses, self.points = poses.copy(), points.copy()
        self.k, self.j = obs_pose.astype(np.int64), obs_point.astype(np.int64)
        self.z, self.S = obs_uvd, np.asarray(S).reshape(3, 3)
        P, L = poses.shape[0], points.shape[0]
        if pose_const is None:
            pose_const = np.zeros(P, dtype=bool)
            pose_const[0] = True
        seen = np.bincount(self.k, minlength=P) > 0
        self.free = (~np.asarray(pose_const, dtype=bool)) & seen
        self.free_idx = np.full(P, -1)
        self.free_idx[self.free] = np.arange(self.free.sum())
        self.active = np.bincount(self.j, minlength=L) > 0
        self.nf = int(self.free.sum())
        self.huber_a = huber_a

    def residuals(self, poses, points, jac=False):
        cam = self.cam
        t, R = poses[self.k, :3], poses[self.k, 3:].reshape(-1, 3, 3)
        p = points[self.j]
        q = np.einsum("nij,nj->ni", R, p) + t
        iz = 1.0 / q[:, 2]
        pred = np.stack([cam["fu"] * q[:, 0] * iz + cam["cu"], cam["fv"] * q[:, 1] * iz + cam["cv"], cam["fu"] * cam["b"] * iz], 1)
        r = (pred - self.z) @ self.S.T
        sq = (r * r).sum(1)
        if self.huber_a > 0:
            a, b = self.huber_a, self.huber_a ** 2
            out = sq > b
            rho0 = np.where(out, 2 * a * np.sqrt(np.where(out, sq, 1.0)) - b, sq)
            rho1 = np.where(out, a / np.sqrt(np.where(out, sq, 1.0)), 1.0)
            cost = 0.5 * rho0.sum()
        else:
            rho1 = np.ones_like(sq)
            cost = 0.5 * sq.sum()
        if not jac:
            return cost, r * np.sqrt(rho1)[:, None]
        N = q.shape[0]
        Jpi = np.zeros((N, 3, 3))
        Jpi[:, 0, 0] = cam["fu"] * iz
        Jpi[:, 0, 2] = -cam["fu"] * q[:, 0] * iz * iz
        Jpi[:, 1, 1] = cam["fv"] * iz
        Jpi[:, 1, 2] = -cam["fv"] * q[:, 1] * iz * iz
        Jpi[:, 2, 2] = -cam["fu"] * cam["b"] * iz * iz
        A = np.einsum("ij,njk->nik", self.S, Jpi)
        G = np.zeros((N, 3, 6))
        G[:, 0, 0] = G[:, 1, 1] = G[:, 2, 2] = 1.0
        G[:, 0, 4], G[:, 0, 5] = q[:, 2], -q[:, 1]
        G[:, 1, 3], G[:, 1, 5] = -q[:, 2], q[:, 0]
        G[:, 2, 3], G[:, 2, 4] = q[:, 1], -q[:, 0]
        Jp = np.einsum("nij,njk->nik", A, G)
        Jl = np.einsum("nij,njk->nik", A, R)
        # Huber (rho'' <= 0 always): scale by sqrt(rho')  [Ceres corrector.cc]
        s1 = np.sqrt(rho1)
        return cost, r * s1[:, None], Jp * s1[:, None, None], Jl * s1[:, None, None]

    def sparse_jacobian(self, Jp, Jl):
        """J over [free poses (6 each) | all landmarks (3 each)] as CSR."""
        N = Jp.shape[0]
        nf, L = self.nf, self.points.shape[0]
        rows = np.arange(3 * N).reshape(N, 3)
        f = self.free_idx[self.k]
        m = f >= 0
        rp = np.repeat(rows[m][:, :, None], 6, axis=2).reshape(-1)
        cp = (6 * f[m][:, None, None] + np.arange(6)[None, None, :]).repeat(3, axis=1).reshape(-1)
        vp = Jp[m].reshape(-1)
        rl = np.repeat(rows[:, :, None], 3, axis=2).reshape(-1)
        cl = (6 * nf + 3 * self.j[:, None, None] + np.arange(3)[None, None, :]).repeat(3, axis=1).reshape(-1)
        vl = Jl.reshape(-1)
        J = sp.csr_matrix((np.concatenate([vp, vl]), (np.concatenate([rp, rl]), np.concatenate([cp, cl]))),
                          shape=(3 * N, 6 * nf + 3 * L))
        return J

    def lm_step(self, poses, points, radius, scale=None, min_diag=1e-6, max_diag=1e32):
        """One Ceres LM step; returns (dp (P,6), dl (L,3), model_cost_change, scale)."""
        cost, r, Jp, Jl = self.residuals(poses, points, jac=True)
        J = self.sparse_jacobian(Jp, Jl)
        nf, L = self.nf, points.shape[0]
        keep = np.concatenate([np.ones(6 * nf, bool), np.repeat(self.active, 3)])
        J = J[:, keep]
        colsq = np.asarray(J.multiply(J).sum(0)).ravel()
        if scale is None:
            scale = 1.0 / (1.0 + np.sqrt(colsq))
        Js = J @ sp.diags(scale)
        diag = np.clip(np.asarray(Js.multiply(Js).sum(0)).ravel(), min_diag, max_diag)
        H = (Js.T @ Js + sp.diags(diag / radius)).tocsc()
        y = spla.spsolve(H, Js.T @ r.reshape(-1))
        delta = -y * scale
        Jd = J @ delta
        mcc = -Jd @ (r.reshape(-1) + 0.5 * Jd)
        full = np.zeros(6 * nf + 3 * L)
        full[keep] = delta
        dp = np.zeros((poses.shape[0], 6))
        dp[self.free] = full[: 6 * nf].reshape(nf, 6)
        dl = full[6 * nf:].reshape(L, 3)
        return dp, dl, mcc, scale, cost

    def plus(self, poses, points, dp, dl):
        out = poses.copy()
        for k in np.nonzero(self.free)[0]:
            out[k] = se3_plus(poses[k], dp[k])
        pts = points.copy()
        pts[self.active] += dl[self.active]
        return out, pts

    def solve(self, max_iter=1000, nonmonotonic=True, f_tol=1e-6, p_tol=1e-8, min_rd=1e-3):
        """Independent re-implementation of the trust-region loop (cost log only)."""
        x_p, x_l = self.poses.copy(), self.points.copy()
        radius, dec = 1e4, 2.0
        scale = None
        max_nm = 5 if nonmonotonic else 0
        cost0, _ = self.residuals(x_p, x_l)
        x_cost = cost0
        minimum = current = reference = candidate = x_cost
        acc_ref = acc_cand = 0.0
        n_nm = 0
        log = [(x_cost, False)]
        xs = np.concatenate([x_p[self.free].ravel(), x_l[self.active].ravel()])
        x_norm = np.linalg.norm(xs)
        for it in range(1, max_iter + 1):
            dp, dl, mcc, scale, _ = self.lm_step(x_p, x_l, radius, scale)
            if not (mcc > 0):
                radius /= dec
                dec *= 2
                log.append((x_cost, False))
                continue
            c_p, c_l = self.plus(x_p, x_l, dp, dl)
            c_cost, _ = self.residuals(c_p, c_l)
            step = np.sqrt(((c_p[self.free] - x_p[self.free]) ** 2).sum() + ((c_l[self.active] - x_l[self.active]) ** 2).sum())
            if step <= p_tol * (x_norm + p_tol):
                break
            if abs(x_cost - c_cost) <= f_tol * x_cost:
                break
            rd = max((current - c_cost) / mcc, (reference - c_cost) / (acc_ref + mcc))
            if rd > min_rd:
                x_p, x_l, x_cost = c_p, c_l, c_cost
                xs = np.concatenate([x_p[self.free].ravel(), x_l[self.active].ravel()])
                x_norm = np.linalg.norm(xs)
                radius = min(1e16, radius / max(1 / 3, 1 - (2 * rd - 1) ** 3))
                dec = 2.0
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
                radius /= dec
                dec *= 2
                log.append((c_cost, False))
        return x_p, x_l, log


# ---- unary pose rows of the sun-aided driver (tests/dataset_vo_sun.cpp:80-124) ------------------------------
def _dot(a, b):
    return a @ b if a.ndim == 1 else (a * b).sum(-1)


def _mv(R, p):
    return R @ p if R.ndim == 2 else np.einsum("...ij,...j->...i", R, p)


def _keep(pert):
    return (lambda name, v: v) if pert is None else pert


def _rot(T):
    return T[..., 3:].reshape(T.shape[:-1] + (3, 3))


# The pose-factor formulas take one block (1-D pose, 2-D rotation) or a stack of them (leading dimensions), in complex (the
# fp64 complex step) or np.clongdouble (tests/hp_reference.py: numpy carries the type of the inputs through every operation
# here, so no `dtype` argument is needed); the one-block fp64 path is the original arithmetic, bit for bit.  `pert(name,
# value)`, when given, returns a replacement for the intermediates the formulas store (R_res, t_res, R_12, v, axis,
# sin_angle, cos_angle, angle, s_c, the four sun angles) and sees the guard quantities (angle, raz, raz_wrapped, rzen).
def so3_log(R, pert=None):
    """so3group.hpp:293-348 (works on complex matrices for complex-step differentiation)."""
    keep = _keep(pert)
    axis = keep("axis", np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], -1))
    sin_a = keep("sin_angle", 0.5 * np.sqrt((axis * axis).sum(-1)))
    cos_a = keep("cos_angle", 0.5 * (R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2] - 1.0))
    # atan2 for complex arguments: angle + first-order imaginary part
    ang = np.arctan2(sin_a.real, cos_a.real)
    d = (cos_a.real * sin_a.imag - sin_a.real * cos_a.imag) / (sin_a.real ** 2 + cos_a.real ** 2) if np.iscomplexobj(R) else 0.0
    angle = keep("angle", ang + 1j * d if np.iscomplexobj(R) else ang)
    small = abs(ang) <= np.finfo(float).eps     # first-order branch: vee(C - I)
    if R.ndim == 2:
        if small:
            return 0.5 * axis
        return 0.5 * angle * axis / sin_a
    return np.where(small[..., None], 0.5 * axis, 0.5 * angle[..., None] * axis / np.where(small, 1.0, sin_a)[..., None])


def pose_prior_residual(T, T_ref, S, pert=None):
    """PoseErrorAutomatic (pose_error.hpp:22-55): S [t_ref - R_res t ; log(R_ref R^T)] (complex-step safe)."""
    keep = _keep(pert)
    R, Rr = _rot(T), _rot(T_ref)
    Rres = keep("R_res", Rr @ np.swapaxes(R, -1, -2))
    e = np.concatenate([keep("t_res", T_ref[..., :3] - _mv(Rres, T[..., :3])), so3_log(Rres, pert)], -1)
    return _mv(S, e)


def relative_pose_residual(T1, T2, T_ref, S, pert=None):
    """RelativePoseErrorAutomatic (relative_pose_error.hpp:22-40): S log(T_ref T1 T2^-1) with the reference's
    log = [translation ; axis-angle] (complex-step safe)."""
    keep = _keep(pert)
    R1, R2, Rr = _rot(T1), _rot(T2), _rot(T_ref)
    R12 = keep("R_12", R1 @ np.swapaxes(R2, -1, -2))
    t = keep("t_res", _mv(Rr, keep("v", T1[..., :3] - _mv(R12, T2[..., :3]))) + T_ref[..., :3])
    return _mv(S, np.concatenate([t, so3_log(keep("R_res", Rr @ R12), pert)], -1))


def sun_sensor_residual(T, oc, eg, S, taz, tzen, pert=None):
    """SunSensorErrorAutomatic (sun_sensor_error.hpp:35-104): azimuth / zenith differences (complex-step safe)."""
    keep = _keep(pert)
    R = _rot(T)
    if T.ndim == 1:
        oc, eg = oc / np.linalg.norm(oc), eg / np.linalg.norm(eg)
    else:
        oc, eg = oc / np.sqrt((oc * oc).sum(-1))[..., None], eg / np.sqrt((eg * eg).sum(-1))[..., None]
    sc = keep("s_c", _mv(R, eg))

    def azzen(v):
        y = v[..., 1]
        zen = np.arccos(-y.real) + (1j * y.imag / np.sqrt(1 - y.real ** 2) if np.iscomplexobj(v) else 0.0)
        x, z = v[..., 0], v[..., 2]
        az = np.arctan2(x.real, z.real) + (1j * (z.real * x.imag - x.real * z.imag) / (x.real ** 2 + z.real ** 2) if np.iscomplexobj(v) else 0.0)
        return az, zen
    eaz, ezen = azzen(sc)
    oaz, ozen = azzen(oc)
    eaz, ezen, oaz, ozen = keep("eaz", eaz), keep("ezen", ezen), keep("oaz", oaz), keep("ozen", ozen)
    raz, rzen = keep("raz", eaz - oaz), keep("rzen", ezen - ozen)
    if T.ndim == 1:
        if raz.real > np.pi:
            raz -= 2 * np.pi
        elif raz.real < -np.pi:
            raz += 2 * np.pi
        if abs(raz.real) > taz:
            raz = 0.0
        if abs(rzen.real) > tzen:
            rzen = 0.0
        return S @ np.array([raz, rzen])
    raz = keep("raz_wrapped", np.where(raz.real > np.pi, raz - 2 * np.pi, np.where(raz.real < -np.pi, raz + 2 * np.pi, raz)))
    raz = np.where(np.abs(raz.real) > np.real(taz), 0.0, raz)
    rzen = np.where(np.abs(rzen.real) > np.real(tzen), 0.0, rzen)
    return _mv(S, np.stack([raz, rzen], -1))


def se3_complex_step_jacobian(fun, T, h=1e-30):
    """d fun(Plus(T, eps)) / d eps at eps = 0 by complex step (rows x 6)."""
    J = []
    for c in range(6):
        e = np.zeros(6, dtype=complex)
        e[c] = 1j * h
        J.append(fun(se3_plus(T.astype(complex), e)).imag / h)
    return np.array(J).T


# ---- Phong lighting rows: forward formulas only (complex-step differentiable) ----------------
# They take one observation (1-D vectors) or a stack of them (leading dimensions), and `dtype`: complex (the fp64 complex
# step) or np.clongdouble (the long-double reference, tests/hp_reference.py).  The one-observation fp64 path is the original
# arithmetic, bit for bit.  `pert(name, value)`, when given, returns a replacement for the intermediate unit vectors
# (nc, ell, cd, m) and for q: hp_reference perturbs them to measure how the rows depend on their rounding.
def _fmax0(col):      # utils/utils.hpp:16-19 with a = 0
    return np.where(0.0 >= col.real, 0.0 * col, col)


def _fmin1(col):      # utils/utils.hpp:22-25 with a = 1
    return np.where(1.0 <= col.real, 1.0 + 0.0 * col, col)


def phong_shade(nc, ell, cd, kd, ks, alpha, dtype=complex, pert=None):
    """lighting/phong.hpp:25-51,59-104,136-139 (ambient = 0)."""
    nc, ell, cd = (np.asarray(v, dtype=dtype) for v in (nc, ell, cd))
    kd, ks, alpha = (np.asarray(v, dtype=dtype) for v in (kd, ks, alpha))
    ldn = _dot(ell, nc)
    lit = np.isfinite(ell).all(-1) & ~(ldn.real <= 0)
    diffuse = np.where(lit, kd * ldn, 0.0)
    mt = 2 * ldn[..., None] * nc - ell
    mu2 = _dot(mt, mt)
    seen = ~(mu2.real <= 0)
    m = mt / np.sqrt(np.where(seen, mu2, 1.0))[..., None]
    if pert is not None:
        m = pert("m", m)
    s = _dot(m, cd)
    seen &= ~(s.real <= 0)
    specular = np.where(seen, ks * np.where(seen, s, 1.0) ** alpha, 0.0)
    col = 1.0 * (0.0 + diffuse + specular) + 0j
    return _fmin1(_fmax0(col))


def unit_vector_plus(x, delta):
    """perturbations.hpp:98-102"""
    y = x + delta - (_dot(delta, x) / _dot(x, x))[..., None] * x
    return y / np.sqrt(_dot(y, y))[..., None]


def intensity_residual(light_type, T, p, n, phong, kd, light, colour, stiffness, dtype=complex, pert=None):
    """intensity_error_point_light.hpp:24-96 / intensity_error_directional_light.hpp:24-96"""
    t, R = T[..., :3], T[..., 3:].reshape(T.shape[:-1] + (3, 3))
    keep = (lambda name, v: v) if pert is None else pert
    q, nc = keep("q", _mv(R, p) + t), keep("nc", _mv(R, n))
    if light_type == 0:
        v = (_mv(R, light) + t) - q                    # point_light.hpp:79-81
        ell = v / np.sqrt(_dot(v, v))[..., None]
    else:
        d = _mv(R, light)                              # directional_light.hpp:32-35 normalises
        ell = d / np.sqrt(_dot(d, d))[..., None]
    cd = -q / np.sqrt(_dot(q, q))[..., None]
    ell, cd = keep("ell", ell), keep("cd", cd)
    return stiffness * (phong_shade(nc, ell, cd, kd, phong[..., 1], phong[..., 2], dtype, pert) - colour)


def intensity_jacobian_complex_step(light_type, T, p, n, phong, kd, light, colour, stiffness, h=1e-30):
    """[pose(6) | point(3) | normal(3) | phong(3) | texture(1) | light(3)] local Jacobian the way
    Ceres forms it: through SE3Perturbation / UnitVectorPerturbation Plus at delta = 0."""
    J = np.zeros(19)
    c = lambda a: np.asarray(a, dtype=complex)
    T, p, n, phong, light = c(T), c(p), c(n), c(phong), c(light)
    base = dict(light_type=light_type, T=T, p=p, n=n, phong=phong, kd=kd + 0j, light=light, colour=colour, stiffness=stiffness)

    def f(**kw):
        a = dict(base)
        a.update(kw)
        return intensity_residual(**a).imag / h
    for k in range(6):
        e = np.zeros(6, dtype=complex); e[k] = 1j * h
        J[k] = f(T=se3_plus(T, e))
    for k in range(3):
        e = np.zeros(3, dtype=complex); e[k] = 1j * h
        J[6 + k] = f(p=p + e)
        J[9 + k] = f(n=unit_vector_plus(n, e))
        J[12 + k] = f(phong=phong + e)
        J[16 + k] = f(light=(light + e) if light_type == 0 else unit_vector_plus(light, e))
    J[15] = f(kd=kd + 1j * h)
    return J


# ---- traditional dogleg [Ceres 1.x dogleg_strategy.cc], written directly in the Jacobi-scaled
# ---- space the way Ceres does (the C oracle works in unscaled coordinates)
def dogleg_linearize(ba: "NumpyBA", x_p, x_l, keep, scale, mu, min_diag=1e-6, max_diag=1e32):
    """DoglegStrategy's work at a new linearisation point, in Jacobi-scaled coordinates: J_s, D, gradient_, the Cauchy step
    length alpha and the Gauss-Newton step (D-scaled).  scale: the Jacobi scale of the first point, or None to take it here."""
    cost, r, Jp, Jl = ba.residuals(x_p, x_l, jac=True)
    J = ba.sparse_jacobian(Jp, Jl)[:, keep]
    if scale is None:
        scale = 1.0 / (1.0 + np.sqrt(np.asarray(J.multiply(J).sum(0)).ravel()))
    Js = J @ sp.diags(scale)
    rv = r.reshape(-1)
    D = np.sqrt(np.clip(np.asarray(Js.multiply(Js).sum(0)).ravel(), min_diag, max_diag))
    grad = (Js.T @ rv) / D                                   # ComputeGradient
    Jg = Js @ (grad / D)
    alpha = (grad @ grad) / (Jg @ Jg)                        # ComputeCauchyPoint
    H = (Js.T @ Js + sp.diags(mu * D * D)).tocsc()           # ComputeGaussNewtonStep
    gn = -D * spla.spsolve(H, Js.T @ rv)
    return dict(Js=Js, rv=rv, D=D, grad=grad, alpha=alpha, gn=gn, scale=scale)


def dogleg_traditional_step(state, radius):
    """ComputeTraditionalDoglegStep: the step in D-scaled space, the same in Jacobi-scaled parameters (step / D) and its model
    cost change -model . (r + model / 2), model = J_s step / D."""
    D, grad, alpha, gn, Js, rv = (state[k] for k in ("D", "grad", "alpha", "gn", "Js", "rv"))
    gnorm, nnorm = np.linalg.norm(grad), np.linalg.norm(gn)
    if nnorm <= radius:
        step = gn.copy()
    elif gnorm * alpha >= radius:
        step = -(radius / gnorm) * grad
    else:
        b_dot_a = -alpha * (grad @ gn)
        a_sq = (alpha * gnorm) ** 2
        bma = a_sq - 2 * b_dot_a + nnorm ** 2
        c = b_dot_a - a_sq
        d = np.sqrt(c * c + bma * (radius ** 2 - a_sq))
        beta = (d - c) / bma if c <= 0 else (radius ** 2 - a_sq) / (d + c)
        step = (-alpha * (1 - beta)) * grad + beta * gn
    step_js = step / D
    model = Js @ step_js
    return step, step_js, -model @ (rv + 0.5 * model)


def dogleg_solve(ba: "NumpyBA", max_iter=1000, nonmonotonic=True, f_tol=1e-6, p_tol=1e-8, min_rd=1e-3,
                 min_diag=1e-6, max_diag=1e32):
    x_p, x_l = ba.poses.copy(), ba.points.copy()
    radius, mu, reuse = 1e4, 1e-8, False
    scale = None
    max_nm = 5 if nonmonotonic else 0
    x_cost, _ = ba.residuals(x_p, x_l)
    minimum = current = reference = candidate = x_cost
    acc_ref = acc_cand = 0.0
    n_nm = 0
    log = [(x_cost, False)]
    nf, L = ba.nf, x_l.shape[0]
    keep = np.concatenate([np.ones(6 * nf, bool), np.repeat(ba.active, 3)])
    xs = np.concatenate([x_p[ba.free].ravel(), x_l[ba.active].ravel()])
    x_norm = np.linalg.norm(xs)
    state = {}
    for it in range(1, max_iter + 1):
        if not reuse:
            reuse = True
            state = dogleg_linearize(ba, x_p, x_l, keep, scale, mu, min_diag, max_diag)
            scale = state["scale"]
        step, step_js, mcc = dogleg_traditional_step(state, radius)
        step_norm_scaled = np.linalg.norm(step)
        if not (mcc > 0):
            mu *= 10.0
            reuse = False
            log.append((x_cost, False))
            continue
        delta = np.zeros(6 * nf + 3 * L)
        delta[keep] = step_js * scale
        dp = np.zeros((x_p.shape[0], 6))
        dp[ba.free] = delta[: 6 * nf].reshape(nf, 6)
        dl = delta[6 * nf:].reshape(L, 3)
        c_p, c_l = ba.plus(x_p, x_l, dp, dl)
        c_cost, _ = ba.residuals(c_p, c_l)
        stepn = np.sqrt(((c_p[ba.free] - x_p[ba.free]) ** 2).sum() + ((c_l[ba.active] - x_l[ba.active]) ** 2).sum())
        if stepn <= p_tol * (x_norm + p_tol):
            break
        if abs(x_cost - c_cost) <= f_tol * x_cost:
            break
        rd = max((current - c_cost) / mcc, (reference - c_cost) / (acc_ref + mcc))
        if rd > min_rd:
            x_p, x_l, x_cost = c_p, c_l, c_cost
            xs = np.concatenate([x_p[ba.free].ravel(), x_l[ba.active].ravel()])
            x_norm = np.linalg.norm(xs)
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


# ---- config 3 (stereo + intensity + normal residual blocks, landmark block = [position | normal]) ----
def phong_lm_step(cam, poses, points, normals, obs_pose, obs_point, obs_uvd, S, ph, radius, pose_const=None,
                  min_diag=1e-6, max_diag=1e32, shared_free=0):
    """One Ceres LM step of the config-3 problem with a dense/sparse direct solve and complex-step
    Jacobians through the reference's Plus operators (slow: small problems only).
    `shared_free` frees the shared blocks (bit 0 light, bit 1 Phong parameters, bit 2 textures); their
    columns follow the landmark columns in the order light, Phong parameters, textures.
    Returns dp (P,6), dl (L,6), model_cost_change, cost [, db when shared_free]."""
    P, L, N = poses.shape[0], points.shape[0], obs_pose.shape[0]
    if pose_const is None:
        pose_const = np.zeros(P, bool)
        pose_const[0] = True
    seen = np.bincount(obs_pose, minlength=P) > 0
    free = (~pose_const) & seen
    fidx = np.full(P, -1)
    fidx[free] = np.arange(free.sum())
    active = np.bincount(obs_point, minlength=L) > 0
    nf = int(free.sum())
    M = len(ph["texture"])
    b_light = b_phong = b_tex = -1
    nb = 0
    if shared_free & 1:
        b_light, nb = nb, nb + 3
    if shared_free & 2:
        b_phong, nb = nb, nb + 3 * M
    if shared_free & 4:
        b_tex, nb = nb, nb + M
    ncol = 6 * nf + 6 * L + nb
    rows, cols, vals, r = [], [], [], np.zeros(7 * N)
    Sn = np.asarray(ph["normal_stiffness"]).reshape(3, 3)
    h = 1e-30
    for i in range(N):
        k, j = int(obs_pose[i]), int(obs_point[i])
        T, p, n = poses[k], points[j], normals[j]
        m = int(ph["material_of_point"][j])
        r[7 * i: 7 * i + 3] = residual_global(cam, T, p, obs_uvd[i], S)
        Jp3, Jl3 = jacobians_complex_step(cam, T, p, obs_uvd[i], S)
        r[7 * i + 3] = intensity_residual(ph["light_type"], T, p, n, ph["phong"][m], ph["texture"][m], ph["light"],
                                          ph["intensity"][i], ph["int_stiffness"]).real
        J19 = intensity_jacobian_complex_step(ph["light_type"], T, p, n, ph["phong"][m], ph["texture"][m], ph["light"],
                                              ph["intensity"][i], ph["int_stiffness"])
        R = T[3:].reshape(3, 3)
        r[7 * i + 4: 7 * i + 7] = Sn @ (R @ n - ph["normal_obs"][i])
        Jnp, Jnn = np.zeros((3, 6)), np.zeros((3, 3))
        for c in range(6):
            e = np.zeros(6, dtype=complex); e[c] = 1j * h
            Tn = se3_plus(T.astype(complex), e)
            Jnp[:, c] = (Sn @ (Tn[3:].reshape(3, 3) @ n - ph["normal_obs"][i])).imag / h
        for c in range(3):
            e = np.zeros(3, dtype=complex); e[c] = 1j * h
            Jnn[:, c] = (Sn @ (R @ unit_vector_plus(n.astype(complex), e) - ph["normal_obs"][i])).imag / h
        Jp = np.vstack([Jp3, J19[None, :6], Jnp])                       # 7 x 6
        Jl = np.zeros((7, 6))
        Jl[:3, :3] = Jl3
        Jl[3, :] = J19[6:12]
        Jl[4:, 3:] = Jnn
        for a in range(7):
            if fidx[k] >= 0:
                for c in range(6):
                    rows.append(7 * i + a); cols.append(6 * fidx[k] + c); vals.append(Jp[a, c])
            for c in range(6):
                rows.append(7 * i + a); cols.append(6 * nf + 6 * j + c); vals.append(Jl[a, c])
        b0 = 6 * nf + 6 * L
        if b_phong >= 0:
            for c in range(3):
                rows.append(7 * i + 3); cols.append(b0 + b_phong + 3 * m + c); vals.append(J19[12 + c])
        if b_tex >= 0:
            rows.append(7 * i + 3); cols.append(b0 + b_tex + m); vals.append(J19[15])
        if b_light >= 0:
            for c in range(3):
                rows.append(7 * i + 3); cols.append(b0 + b_light + c); vals.append(J19[16 + c])
    J = sp.csr_matrix((vals, (rows, cols)), shape=(7 * N, ncol))
    keep = np.concatenate([np.ones(6 * nf, bool), np.repeat(active, 6), np.ones(nb, bool)])
    J = J[:, keep]
    colsq = np.asarray(J.multiply(J).sum(0)).ravel()
    scale = 1.0 / (1.0 + np.sqrt(colsq))
    Js = J @ sp.diags(scale)
    diag = np.clip(np.asarray(Js.multiply(Js).sum(0)).ravel(), min_diag, max_diag)
    H = (Js.T @ Js + sp.diags(diag / radius)).tocsc()
    y = spla.spsolve(H, Js.T @ r)
    delta = -y * scale
    Jd = J @ delta
    mcc = -Jd @ (r + 0.5 * Jd)
    full = np.zeros(ncol)
    full[keep] = delta
    dp = np.zeros((P, 6))
    dp[free] = full[: 6 * nf].reshape(nf, 6)
    if shared_free:
        return dp, full[6 * nf: 6 * nf + 6 * L].reshape(L, 6), mcc, 0.5 * r @ r, full[6 * nf + 6 * L:]
    return dp, full[6 * nf:].reshape(L, 6), mcc, 0.5 * r @ r
