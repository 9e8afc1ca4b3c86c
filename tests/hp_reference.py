"""Extended-precision reference for the reduced camera system (CPU only).

Everything that cancels -- the stereo rows, their Gram products and the landmark elimination of the Schur complement -- is
evaluated in ``np.longdouble`` (80-bit on x86-64: unit roundoff 2^-64 against fp64's 2^-53) from the fp64 inputs the device
received, which long double holds exactly.  The system is the one the device factorises (``k_assemble_reduced`` /
``k_finish_reduced``): UNSCALED coordinates, the Jacobi scale s = 1 / (1 + sqrt(diag H)) taken at the linearisation point,
the Levenberg-Marquardt diagonal clamp(diag(H) s^2, 1e-6, 1e32) / (radius s^2) on pose and landmark blocks, and

    S = A_pp - sum_j W_j V_j^-1 W_j^T,    rhs = -(g_p - sum_j W_j V_j^-1 g_l,j),    S delta_p = rhs.

Unary pose rows (prior, sun sensor) are passed in as fp64 blocks; their rounding enters the bounds as c u |H_unary|.  Or the
pose-only residual blocks (prior, sun sensor, relative pose) come in long double as well: pose_factor_rows, PoseFactorSums.

The bars derived here all use u = 2^-53 (the precision of the side under test):

* backward error  eta = |rhs - S x|_inf / (|S|_inf |x|_inf + |rhs|_inf), residual in long double;
* entrywise assembly bound  E = (m + c) u (|A_pp| + sum_j kappa(V_j) |W_j| |V_j^-1| |W_j|^T), m the number of terms summed into
  the entry -- large exactly where the Schur complement cancels, which a fixed relative bar is not;
* covariance bound  |S^-1| E |S^-1| (first-order propagation) plus the solve term.

Imports neither torch nor libssba.so.
"""
from __future__ import annotations

import numpy as np
import scipy.linalg as sla

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "long double is not extended precision on this platform: the reference would be fp64"

U = 2.0 ** -53            # unit roundoff of the side under test
C_TERMS = 16              # the c of gamma = (m + c) u: the rounding of one row / one 3x3 inverse, independent of m
SOLVE_C = 4096            # eta <= SOLVE_C u;  |x - x*| / |x*| <= SOLVE_C u kappa_2
DENSE_EIG_MAX = 2000      # kappa_2 from eigvalsh up to this size, from the extreme eigenvalues of the band above


# ---------------------------------------------------------------------------------------------------------------- stereo rows
def huber_weight(sq, a, dtype=LD):
    """sqrt(rho') of the Huber loss at s = |r|^2 (Ceres corrector with rho'' <= 0: r and J scaled by sqrt(rho'))."""
    sq = np.asarray(sq, dtype=dtype)
    if not a > 0:
        return np.ones_like(sq)
    a = dtype(a)
    out = sq > a * a
    return np.where(out, np.sqrt(a / np.sqrt(np.where(out, sq, dtype(1)))), dtype(1))


def stereo_rows(cam, poses, points, obs_pose, obs_point, obs_uvd, stiffness, huber_a=0.0, dtype=LD, jacobians=True):
    """Residuals and closed-form local Jacobians (the route of np_reference.NumpyBA.residuals) in `dtype`.

    stiffness: one 3x3 matrix or one per observation (N, 3, 3).  Returns a dict with cost, r (N,3), Jp (N,3,6), Jl (N,3,3)
    -- corrected by sqrt(rho') -- and the magnitudes the fp64 rounding of each row is relative to: rabs (N,3) for the
    residual (pred - z cancels), Jpa / Jla for the Jacobians (q = R p + t cancels when the point is far from the origin).
    """
    f = lambda v: np.asarray(v, dtype=dtype)
    k, j = np.asarray(obs_pose, np.int64), np.asarray(obs_point, np.int64)
    T, p, z = f(poses)[k], f(points)[j], f(obs_uvd)
    S = f(stiffness)
    S = np.broadcast_to(S.reshape(3, 3), (k.shape[0], 3, 3)) if S.size == 9 else S.reshape(-1, 3, 3)
    fu, fv, cu, cv, b = (dtype(cam[n]) for n in ("fu", "fv", "cu", "cv", "b"))
    t, R = T[:, :3], T[:, 3:].reshape(-1, 3, 3)
    q = np.einsum("nij,nj->ni", R, p) + t
    iz = dtype(1) / q[:, 2]
    pred = np.stack([fu * q[:, 0] * iz + cu, fv * q[:, 1] * iz + cv, fu * b * iz], 1)
    r = np.einsum("nij,nj->ni", S, pred - z)
    sq = (r * r).sum(1)
    w = huber_weight(sq, huber_a, dtype)
    if huber_a > 0:
        a = dtype(huber_a)
        rho0 = np.where(sq > a * a, 2 * a * np.sqrt(sq) - a * a, sq)
    else:
        rho0 = sq
    N = q.shape[0]
    if not jacobians:       # cost, residuals and their magnitudes only (a C2-sized cost: the Jacobians are 18 of 24 values per row)
        q64, R64, p64, t64 = (np.asarray(v, np.float64) for v in (q, R, p, t))
        alpha = 1.0 + (np.abs(R64) @ np.abs(p64)[..., None])[..., 0].max(1) / np.abs(q64[:, 2]) + np.abs(t64).max(1) / np.abs(q64[:, 2])
        rabs = np.einsum("nij,nj->ni", np.abs(np.asarray(S, np.float64)),
                         alpha[:, None] * np.abs(np.asarray(pred, np.float64)) + np.abs(np.asarray(z, np.float64))) * np.asarray(w, np.float64)[:, None]
        return dict(cost=dtype(0.5) * rho0.sum(), r=r * w[:, None], rabs=rabs, alpha=alpha)
    Jpi = np.zeros((N, 3, 3), dtype=dtype)
    Jpi[:, 0, 0] = fu * iz
    Jpi[:, 0, 2] = -fu * q[:, 0] * iz * iz
    Jpi[:, 1, 1] = fv * iz
    Jpi[:, 1, 2] = -fv * q[:, 1] * iz * iz
    Jpi[:, 2, 2] = -fu * b * iz * iz
    A = np.einsum("nij,njk->nik", S, Jpi)
    G = np.zeros((N, 3, 6), dtype=dtype)
    G[:, 0, 0] = G[:, 1, 1] = G[:, 2, 2] = 1
    G[:, 0, 4], G[:, 0, 5] = q[:, 2], -q[:, 1]
    G[:, 1, 3], G[:, 1, 5] = -q[:, 2], q[:, 0]
    G[:, 2, 3], G[:, 2, 4] = q[:, 1], -q[:, 0]
    Jp = np.einsum("nij,njk->nik", A, G) * w[:, None, None]
    Jl = np.einsum("nij,njk->nik", A, R) * w[:, None, None]
    # magnitudes (fp64 is enough): alpha = how much larger the terms of q are than q itself
    q64, R64, p64, t64 = (np.asarray(v, np.float64) for v in (q, R, p, t))
    alpha = 1.0 + (np.abs(R64) @ np.abs(p64)[..., None])[..., 0].max(1) / np.abs(q64[:, 2]) + np.abs(t64).max(1) / np.abs(q64[:, 2])
    Jp64, Jl64, w64 = np.abs(np.asarray(Jp, np.float64)), np.abs(np.asarray(Jl, np.float64)), np.asarray(w, np.float64)
    rabs = np.einsum("nij,nj->ni", np.abs(np.asarray(S, np.float64)),
                     alpha[:, None] * np.abs(np.asarray(pred, np.float64)) + np.abs(np.asarray(z, np.float64))) * w64[:, None]
    Jpa = Jp64 + alpha[:, None, None] * Jp64.max((1, 2))[:, None, None]
    Jla = Jl64 + alpha[:, None, None] * Jl64.max((1, 2))[:, None, None]
    return dict(cost=dtype(0.5) * rho0.sum(), r=r * w[:, None], Jp=Jp, Jl=Jl, rabs=rabs, Jpa=Jpa, Jla=Jla, alpha=alpha)


# ----------------------------------------------------------------------------------------------------------- lighting rows
H_CS = 2.0 ** -100        # complex step: exact power of two, so value + i h f' carries f' to long-double accuracy
DELTA_MAG = 2.0 ** -52    # relative perturbation for the rounding magnitudes (below fp64's own u: no guard is crossed
                          # unless the row is within fp64 rounding of it, where either branch is a correct fp64 answer)
C_ROW = 16                # the c of the row bar c u mag


def _dot3(a, b):
    return (a * b).sum(-1)


def _se3_columns(T, h):
    """SE3Perturbation Plus at eps = i h e_c, c = 0..5, on stacked poses (N, 12): (6, N, 12).  At eps = 0 Ceres takes the
    first-order branch of so3_exp (np_reference.jacobians_complex_step), so Plus(T, eps) = [(I + eps_r^) t + eps_t, (I + eps_r^) R]."""
    N = T.shape[0]
    out = np.repeat(T[None], 6, axis=0)
    t, R = T[:, :3], T[:, 3:].reshape(N, 3, 3)
    for c in range(3):
        out[c, :, c] = out[c, :, c] + 1j * h
        phi = np.zeros(3)
        phi[c] = 1.0
        W = np.array([[0, -phi[2], phi[1]], [phi[2], 0, -phi[0]], [-phi[1], phi[0], 0]]) * (1j * h)
        out[3 + c, :, :3] = t + np.einsum("ij,nj->ni", W, t)
        out[3 + c, :, 3:] = (R + np.einsum("ij,njk->nik", W, R)).reshape(N, 9)
    return out


def _phong_eval(light_type, x, pert, cdt):
    """(r_int (N,), J_int (N,19), r_nrm (N,3), J_nrm (N,3,9) = [pose 6 | normal 3]) by complex step in `cdt` through the
    forward formulas of np_reference and the reference's Plus operators, at the inputs `x` (already in `cdt`)."""
    import np_reference as npr
    h = H_CS
    T, p, n, ph, kd, light, col, st, nobs, Sn = (x[k] for k in ("T", "p", "n", "phong", "kd", "light", "colour",
                                                                "stiffness", "nobs", "Sn"))
    N = T.shape[0]
    e3 = np.eye(3) * (1j * h)

    def f_int(T=T, p=p, n=n, ph=ph, kd=kd, light=light):
        return npr.intensity_residual(light_type, T, p, n, ph, kd, light, col, st, dtype=cdt, pert=pert)

    def f_nrm(T=T, n=n):
        R = T[:, 3:].reshape(N, 3, 3)
        nc = np.einsum("nij,nj->ni", R, n)
        if pert is not None:
            nc = pert("nc", nc)
        return np.einsum("nij,nj->ni", Sn, nc - nobs)

    Ts = _se3_columns(T, h)
    r0 = f_int()
    # Ceres chains d r / d x at the block's value x with the plus-Jacobian (I - x x^T / |x|^2) / |x| of
    # UnitVectorPerturbation: the same as the complex step through Plus only when |x| = 1, since Plus(x, 0) = x / |x|
    plus = lambda v, e: v + (e - (_dot3(e, v) / _dot3(v, v))[:, None] * v) / np.sqrt(_dot3(v, v))[:, None]
    J = np.zeros((N, 19), dtype=LD if cdt == np.clongdouble else np.float64)
    for c in range(6):
        J[:, c] = f_int(T=Ts[c]).imag / h
    for c in range(3):
        J[:, 6 + c] = f_int(p=p + e3[c]).imag / h
        J[:, 9 + c] = f_int(n=plus(n, np.broadcast_to(e3[c], n.shape))).imag / h
        J[:, 12 + c] = f_int(ph=ph + e3[c]).imag / h
        J[:, 16 + c] = f_int(light=(light + e3[c]) if light_type == 0 else plus(light, np.broadcast_to(e3[c], light.shape))).imag / h
    J[:, 15] = f_int(kd=kd + 1j * h).imag / h
    rn = f_nrm()
    Jn = np.zeros((N, 3, 9), dtype=J.dtype)
    for c in range(6):
        Jn[:, :, c] = f_nrm(T=Ts[c]).imag / h
    for c in range(3):
        Jn[:, :, 6 + c] = f_nrm(n=plus(n, np.broadcast_to(e3[c], n.shape))).imag / h
    return r0.real, J, rn.real, Jn


_PH_INPUTS = (("T", 12), ("p", 3), ("n", 3), ("phong", 3), ("kd", 1), ("light", 3), ("colour", 1), ("stiffness", 1),
              ("nobs", 3), ("Sn", 9))
_PH_UNITS = ("q", "nc", "ell", "cd", "m")


def phong_rows(light_type, poses, points, normals, phong, texture, light, colour, stiffness, normal_obs, normal_stiffness,
               dtype=LD, mags=True):
    """The intensity row (point light: light_type 0, directional: 1) and the three normal rows of every observation, with
    their local Jacobians, in `dtype` -- by complex step in the matching complex type through np_reference's forward
    formulas (and so through their branches: ldn <= 0, mu2 <= 0 and s <= 0 guards, the fmax 0 / fmin 1 clamp with a zero
    gradient where it fires, the normalised directional light) and the reference's Plus operators.

    Arguments per observation as for capi.phong_evaluate: poses (N,12), points, normals (N,3), phong (N,3), texture (N,),
    colour (N,); light (3), stiffness (scalar), normal_obs (N,3), normal_stiffness (3,3).  Returns r_int (N,), J_int
    (N,19) = [pose 6 | position 3 | normal 3 | Phong 3 | texture 1 | light 3], r_nrm (N,3), J_np (N,3,6), J_nn (N,3,3),
    the branch flags of every row, and (mags=True) a rounding magnitude of each value: mag_r_int, mag_J_int, mag_r_nrm,
    mag_J_np, mag_J_nn.

    The bar on an fp64 evaluation is |fp64 - truth| <= C_ROW u mag, where mag is the first-order sensitivity of the
    quantity Q (a residual or one Jacobian entry) to relative perturbations of each of its inputs x_k and of its
    intermediate vectors y_k (q = R p + t, nc = R n, ell, cd, the mirror direction m), component by component:

        mag = |Q| + sum_k |x_k dQ/dx_k| + sum_k |y_k dQ/dy_k|.

    fp64 evaluates Q as the exact function of inputs and intermediates each carrying a relative error of at most a few u
    (one rounding per stored value, the two or three of a 3-term dot product, the few ulps of log, exp, the rsqrt of
    ph_rsqrt / ph_rcp); to first order |fp64 - Q| <= sum_k gamma_k |x_k dQ/dx_k| with gamma_k <= 4 u for all of them.  The
    perturbation of an input x_k stands for the rounding of the first products formed from it (R p + t cancels when the
    point is far: then |p dQ/dp| is large), that of the intermediates for the rounding of the normalisations, the dot
    products (ldn = ell.nc, s = m.cd: |m_i cd_i| / s is large for s near 0) and the differences (mt = 2 ldn nc - ell,
    v = light - q).  exp(alpha log s) has the relative error |alpha log s| u of the logarithm, which is exactly the relative
    sensitivity to alpha.  C_ROW = 16 = 4 x 4 u: four such terms adding in the same direction beyond the bound on each.
    Where a clamp fires both Q and mag are 0 except d r / d colour, d r / d stiffness: the bar is then exact zero gradients.
    The derivatives are measured, not derived: one extra complex-step evaluation per perturbation at x_k (1 + DELTA_MAG)
    in long double, so mag carries a relative error of 2^-64 / DELTA_MAG = 2^-12.
    """
    cdt = np.clongdouble if dtype == LD else complex
    c = lambda v: np.asarray(v, dtype=cdt)
    N = np.asarray(poses).shape[0]
    x = dict(T=c(poses), p=c(points), n=c(normals), phong=c(phong).reshape(N, 3), kd=c(texture).reshape(N),
             light=c(np.broadcast_to(np.asarray(light, np.float64), (N, 3))), colour=c(colour).reshape(N),
             stiffness=c(stiffness), nobs=c(normal_obs), Sn=c(np.broadcast_to(np.asarray(normal_stiffness, np.float64).reshape(3, 3), (N, 3, 3))))
    x["stiffness"] = np.broadcast_to(x["stiffness"], (N,)).copy()
    r, J, rn, Jn = _phong_eval(light_type, x, None, cdt)
    out = dict(r_int=r, J_int=J, r_nrm=rn, J_np=Jn[:, :, :6], J_nn=Jn[:, :, 6:])
    out.update(_phong_branches(light_type, x))
    if not mags:
        return out
    base = [np.abs(np.asarray(v, np.float64)) for v in (r, J, rn, Jn)]
    acc = [b.copy() for b in base]
    ref = [np.asarray(v, LD) for v in (r, J, rn, Jn)]

    def add(res, rel):
        for a, v, r0 in zip(acc, res, ref):
            d = np.abs(np.asarray((np.asarray(v, LD) - r0), np.float64))
            a += d / rel.reshape((-1,) + (1,) * (d.ndim - 1))

    for name, width in _PH_INPUTS:
        flat = x[name].reshape(N, -1)
        for k in range(flat.shape[1]):
            y = dict(x)
            f2 = flat.copy()
            f2[:, k] = f2[:, k] * (1 + DELTA_MAG)
            xr = np.abs(np.asarray(flat[:, k].real, np.float64))
            if not np.any(xr > 0):
                continue
            rel = np.abs(np.asarray((f2[:, k] - flat[:, k]).real, np.float64)) / np.maximum(xr, 1e-300)
            y[name] = f2.reshape(x[name].shape)
            add(_phong_eval(light_type, y, None, cdt), np.where(xr > 0, rel, np.inf))
    for name in _PH_UNITS:
        for k in range(3):
            def pert(nm, v, name=name, k=k):
                if nm != name:
                    return v
                v = v.copy()
                v[..., k] = v[..., k] * (1 + DELTA_MAG)
                return v
            add(_phong_eval(light_type, x, pert, cdt), np.full(N, DELTA_MAG))
    acc[1][:, :6] += _pose_chain_terms(light_type, x, J, cdt)
    acc[1][:, 9:12] += _projection_terms(light_type, x, "n", cdt)
    if light_type == 1:
        acc[1][:, 16:19] += _projection_terms(light_type, x, "light", cdt)
    acc[3][:, :, 6:] += _normal_row_projection_terms(x)
    out.update(mag_r_int=acc[0], mag_J_int=acc[1], mag_r_nrm=acc[2], mag_J_np=acc[3][:, :, :6], mag_J_nn=acc[3][:, :, 6:])
    return out


def _pose_chain_terms(light_type, x, J, cdt):
    """|d r / d eps| through q alone, through nc alone, and through the light alone, for the six pose columns.  The pose
    Jacobian is the sum of these three chains and cancels where the row is invariant (a rigid motion of the camera moves
    q, nc and a point light together: the rotation columns are exactly 0; the translation columns lose the light chain),
    so its rounding is relative to the terms, which no perturbation of an input sees: the symmetry survives every one."""
    import np_reference as npr
    h = H_CS
    N = x["T"].shape[0]
    out = np.zeros((N, 6))
    for c in range(6):
        e = np.zeros(3)
        e[c % 3] = 1.0
        step = lambda v: (np.broadcast_to(e * (1j * h), v.shape) if c < 3 else np.cross(e * (1j * h), v))
        parts = []
        for target in ("q", "nc"):
            if target == "nc" and c < 3:
                parts.append(np.zeros(N, LD))
                continue
            pert = lambda nm, v, target=target: v + step(v) if nm == target else v
            parts.append(np.asarray(npr.intensity_residual(light_type, x["T"], x["p"], x["n"], x["phong"], x["kd"], x["light"],
                                                           x["colour"], x["stiffness"], dtype=cdt, pert=pert).imag / h, LD))
        rest = np.asarray(J[:, c], LD) - parts[0] - parts[1]
        out[:, c] = sum(np.abs(np.asarray(v, np.float64)) for v in (parts[0], parts[1], rest))
    return out


def _projection_terms(light_type, x, name, cdt):
    """|g| + |g.x| |x| / |x|^2 of the UnitVectorPerturbation plus-Jacobian (I - x x^T / |x|^2) / |x| applied to the
    gradient g with respect to the raw vector x (the normal, or a directional light): the two terms cancel where g is
    nearly parallel to x, which no relative perturbation of x sees."""
    import np_reference as npr
    h = H_CS
    v = np.asarray(x[name].real, LD)
    g = np.zeros(v.shape, LD)
    for c in range(3):
        y = dict(x)
        e = np.zeros(3)
        e[c] = 1.0
        y[name] = x[name] + e * (1j * h)
        g[:, c] = np.asarray(npr.intensity_residual(light_type, y["T"], y["p"], y["n"], y["phong"], y["kd"], y["light"], y["colour"],
                                                    y["stiffness"], dtype=cdt).imag / h, LD)
    n2 = (v * v).sum(1)
    proj = np.abs((g * v).sum(1))[:, None] * np.abs(v) / n2[:, None]
    return np.asarray((np.abs(g) + proj) / np.sqrt(n2)[:, None], np.float64)


def _normal_row_projection_terms(x):
    """The same two terms for the normal rows: g = Sn R (rows of Sn R against the unit normal)."""
    n = np.asarray(x["n"].real, LD)
    R = np.asarray(x["T"].real, LD)[:, 3:].reshape(-1, 3, 3)
    G = np.einsum("nij,njk->nik", np.asarray(x["Sn"].real, LD), R)
    n2 = (n * n).sum(1)
    proj = np.abs(np.einsum("nij,nj->ni", G, n))[:, :, None] * np.abs(n)[:, None, :] / n2[:, None, None]
    return np.asarray((np.abs(G) + proj) / np.sqrt(n2)[:, None, None], np.float64)


def _phong_branches(light_type, x):
    """Which side of each guard every intensity row is on, in long double (for the tests that build edge batches)."""
    R = np.asarray(x["T"].real, LD)[:, 3:].reshape(-1, 3, 3)
    t = np.asarray(x["T"].real, LD)[:, :3]
    q = np.einsum("nij,nj->ni", R, np.asarray(x["p"].real, LD)) + t
    nc = np.einsum("nij,nj->ni", R, np.asarray(x["n"].real, LD))
    lc = np.einsum("nij,nj->ni", R, np.asarray(x["light"].real, LD))
    v = lc + t - q if light_type == 0 else lc
    ell = v / np.sqrt((v * v).sum(1))[:, None]
    cd = -q / np.sqrt((q * q).sum(1))[:, None]
    ldn = (ell * nc).sum(1)
    mt = 2 * ldn[:, None] * nc - ell
    mu2 = (mt * mt).sum(1)
    s = (mt * cd).sum(1) / np.sqrt(np.where(mu2 > 0, mu2, 1))
    ph = np.asarray(x["phong"].real, LD)
    kd = np.asarray(x["kd"].real, LD)
    col = np.where(ldn > 0, kd * ldn, 0) + np.where((mu2 > 0) & (s > 0), ph[:, 1] * np.where(s > 0, s, 1) ** ph[:, 2], 0)
    return dict(ldn=ldn, mu2=mu2, s=s, col=col)


def phong_observation_rows(cam, poses, points, normals, obs_pose, obs_point, obs_uvd, stiffness, lighting, huber_a=0.0,
                           shared_free=0, dtype=LD, phong=None):
    """The seven rows of every observation of a config-3 problem (stereo 3 with the Huber corrector, intensity 1, normal
    3), as SchurSystem takes them: r (N,7), Jp (N,7,6), Jl (N,7,6) = [position | normal], and the border Jb (N,7,nb) of the
    free shared blocks in the order of np_reference.phong_lm_step and ssba_border_system: light 3, Phong 3M, textures M.
    With the rounding magnitudes rabs, Jpa, Jla, Jba of the rows (stereo_rows; phong_rows).  `phong`: the "phong" entry of
    an earlier call on the same observations (the lighting rows do not depend on the loss or on which blocks are free)."""
    k, j = np.asarray(obs_pose, np.int64), np.asarray(obs_point, np.int64)
    lt = lighting
    st = stereo_rows(cam, poses, points, obs_pose, obs_point, obs_uvd, stiffness, huber_a, dtype)
    mat = np.asarray(lt["material_of_point"], np.int64)[j]
    ph = phong if phong is not None else phong_rows(lt["light_type"], np.asarray(poses)[k], np.asarray(points)[j], np.asarray(normals)[j],
                    np.asarray(lt["phong"])[mat], np.asarray(lt["texture"])[mat], lt["light"], lt["intensity"],
                    lt["int_stiffness"], lt["normal_obs"], lt["normal_stiffness"], dtype)
    N = k.shape[0]
    M = len(lt["texture"])
    r = np.zeros((N, 7), dtype=dtype)
    Jp, Jl = np.zeros((N, 7, 6), dtype=dtype), np.zeros((N, 7, 6), dtype=dtype)
    rabs, Jpa, Jla = np.zeros((N, 7)), np.zeros((N, 7, 6)), np.zeros((N, 7, 6))
    r[:, :3], Jp[:, :3], Jl[:, :3, :3] = st["r"], st["Jp"], st["Jl"]
    rabs[:, :3], Jpa[:, :3], Jla[:, :3, :3] = st["rabs"], st["Jpa"], st["Jla"]
    r[:, 3], Jp[:, 3], Jl[:, 3] = ph["r_int"], ph["J_int"][:, :6], ph["J_int"][:, 6:12]
    rabs[:, 3], Jpa[:, 3], Jla[:, 3] = ph["mag_r_int"], ph["mag_J_int"][:, :6], ph["mag_J_int"][:, 6:12]
    r[:, 4:], Jp[:, 4:], Jl[:, 4:, 3:] = ph["r_nrm"], ph["J_np"], ph["J_nn"]
    rabs[:, 4:], Jpa[:, 4:], Jla[:, 4:, 3:] = ph["mag_r_nrm"], ph["mag_J_np"], ph["mag_J_nn"]
    cols = []
    if shared_free & 1:
        cols += [(np.zeros(N, np.int64) + c, 16 + c) for c in range(3)]
    nb = 3 if shared_free & 1 else 0
    if shared_free & 2:
        cols += [(nb + 3 * mat + c, 12 + c) for c in range(3)]
        nb += 3 * M
    if shared_free & 4:
        cols += [(nb + mat, 15)]
        nb += M
    Jb, Jba = np.zeros((N, 7, nb), dtype=dtype), np.zeros((N, 7, nb))
    for col, src in cols:
        Jb[np.arange(N), 3, col] = ph["J_int"][:, src]
        Jba[np.arange(N), 3, col] = ph["mag_J_int"][:, src]
    return dict(cost=st["cost"] + LD(0.5) * ((r[:, 3:] ** 2).sum()), r=r, Jp=Jp, Jl=Jl, rabs=rabs, Jpa=Jpa, Jla=Jla,
                Jb=Jb, Jba=Jba, phong=ph)


# ------------------------------------------------------------------------------------------------------------ Schur assembly
def inv3(V):
    """Inverses of a stack of 3x3 matrices by the adjugate (numpy.linalg does not take long double)."""
    a, b, c = V[:, 0, 0], V[:, 0, 1], V[:, 0, 2]
    d, e, f = V[:, 1, 0], V[:, 1, 1], V[:, 1, 2]
    g, h, i = V[:, 2, 0], V[:, 2, 1], V[:, 2, 2]
    C = np.stack([e * i - f * h, c * h - b * i, b * f - c * e,
                  f * g - d * i, a * i - c * g, c * d - a * f,
                  d * h - e * g, b * g - a * h, a * e - b * d], 1).reshape(-1, 3, 3)
    det = a * C[:, 0, 0] + b * C[:, 1, 0] + c * C[:, 2, 0]
    return C / det[:, None, None]


def inv_spd(V):
    """Inverses of a stack of symmetric positive definite matrices by Cholesky, in the dtype of V (long double)."""
    n = V.shape[-1]
    Lf = np.zeros_like(V)
    for i in range(n):
        for j in range(i + 1):
            t = V[:, i, j] - (Lf[:, i, :j] * Lf[:, j, :j]).sum(1)
            Lf[:, i, j] = np.sqrt(t) if i == j else t / Lf[:, j, j]
    Li = np.zeros_like(V)                     # L^-1 by forward substitution
    for i in range(n):
        Li[:, i, i] = 1 / Lf[:, i, i]
        for j in range(i):
            Li[:, i, j] = -(Lf[:, i, j:i] * Li[:, j:i, j]).sum(1) / Lf[:, i, i]
    return np.einsum("nki,nkj->nij", Li, Li)


def _segments(keys):
    """Sorted order of `keys` and the segment starts of equal keys (for np.add.reduceat)."""
    order = np.argsort(keys, kind="stable")
    ks = keys[order]
    starts = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]])) if ks.size else np.zeros(0, np.int64)
    return order, ks, starts


def _damping(h, s, radius):
    if radius is None:
        return np.zeros_like(h)
    s2 = s * s
    return np.clip(h * s2, LD(1e-6), LD(1e32)) / (LD(radius) * s2)


class SchurSystem:
    """The damped (radius) or undamped (radius=None) reduced camera system in long double, stored as 6x6 blocks.

    free_idx: free index of every pose (-1 constant).  H_unary / g_unary (n x n and n, fp64, free-pose coordinates): unary
    pose rows already summed; Ha_unary their magnitude sum |J|^T |J| (unary_pose_blocks).  factor_sums (PoseFactorSums): the
    long-double blocks of the pose-only residual blocks instead -- H with the off-diagonal 6x6 blocks J_1^T J_2 of the relative
    blocks, g, and their bars: the sums of magnitudes join those of the stereo terms under (m + c) u with the blocks' rows
    counted in m, and the rounding of the row values (C_TERMS u (mag |J| + |J| mag)) is added to E.  The Schur terms are summed in
    chunks into the distinct 6x6 blocks, so a C2-sized system (14 million observation pairs) fits in memory.

    E is a bound on the fp64 rounding of each entry, not a relative bar: where a landmark is nearly unobserved in depth
    (undamped V_j, kappa(V_j) ~ 1e12 and more) its terms exceed S itself and the check only bounds the cancellation.
    """

    def __init__(self, rows, obs_pose, obs_point, free_idx, num_points, radius=None, H_unary=None, g_unary=None,
                 Ha_unary=None, factor_sums=None):
        k = np.asarray(obs_pose, np.int64)
        j = np.asarray(obs_point, np.int64)
        fidx = np.asarray(free_idx, np.int64)
        self.nf = nf = int((fidx >= 0).sum())
        self.n = 6 * nf
        f = fidx[k]
        Jp, Jl, r = rows["Jp"], rows["Jl"], rows["r"]
        Jpa, Jla, rabs = rows["Jpa"], rows["Jla"], rows["rabs"]
        fr = f >= 0
        # ---- landmark blocks (undamped Gram, scale, damping, inverse)
        V_i = np.einsum("nai,naj->nij", Jl, Jl)
        g_i = np.einsum("nai,na->ni", Jl, r)
        order, lk, st = _segments(j)
        self.lm = lk[st]                                            # landmarks present
        V = np.add.reduceat(V_i[order], st, axis=0)
        gl = np.add.reduceat(g_i[order], st, axis=0)
        hl = np.diagonal(V, axis1=1, axis2=2).copy()
        sl = LD(1) / (LD(1) + np.sqrt(hl))
        d = Jl.shape[-1]
        self.d = d
        V[:, range(d), range(d)] += _damping(hl, sl, radius)
        Vinv = inv3(V) if d == 3 else inv_spd(V)
        self.V, self.Vinv, self.gl = V, Vinv, gl
        slot = np.full(num_points, -1, np.int64)
        slot[self.lm] = np.arange(self.lm.shape[0])
        self.slot_of_obs = slot[j]
        V64 = np.asarray(V, np.float64)
        self.kappa_V = np.linalg.cond(V64)
        Via = np.abs(np.asarray(Vinv, np.float64))
        # ---- pose blocks
        Hp_i = np.einsum("nai,naj->nij", Jp, Jp)
        gp_i = np.einsum("nai,na->ni", Jp, r)
        Hpa_i = np.einsum("nai,naj->nij", Jpa, Jpa)
        gpa_i = np.einsum("nai,na->ni", Jpa, rabs)
        n = self.n
        Hd = np.zeros((nf, 6, 6), dtype=LD)
        gp = np.zeros((nf, 6), dtype=LD)
        Hda = np.zeros((nf, 6, 6))
        gpa = np.zeros((nf, 6))
        m_diag = np.zeros(nf)
        o2, fk, st2 = _segments(f[fr])
        if fk.size:
            sel = np.flatnonzero(fr)[o2]
            fu = fk[st2]
            Hd[fu] = np.add.reduceat(Hp_i[sel], st2, axis=0)
            gp[fu] = np.add.reduceat(gp_i[sel], st2, axis=0)
            Hda[fu] = np.add.reduceat(Hpa_i[sel], st2, axis=0)
            gpa[fu] = np.add.reduceat(gpa_i[sel], st2, axis=0)
            m_diag[fu] = np.diff(np.concatenate([st2, [fk.size]]))
        if H_unary is not None:
            for a in range(nf):
                Hd[a] += np.asarray(H_unary[6 * a: 6 * a + 6, 6 * a: 6 * a + 6], LD)
                gp[a] += np.asarray(g_unary[6 * a: 6 * a + 6], LD)
                Hda[a] += Ha_unary[6 * a: 6 * a + 6, 6 * a: 6 * a + 6]
                gpa[a] += np.abs(g_unary[6 * a: 6 * a + 6])
        fs = self.factor_sums = factor_sums
        free_poses = np.flatnonzero(fidx >= 0)
        gv = np.zeros((nf, 6))
        if fs is not None:
            a = fidx[free_poses]
            Hd[a] += fs.H[free_poses]
            gp[a] += fs.g[free_poses]
            Hda[a] += fs.Hs[free_poses]
            gpa[a] += fs.gs[free_poses]
            m_diag[a] += fs.m[free_poses]
            gv[a] = fs.gv[free_poses]
        hp = np.diagonal(Hd, axis1=1, axis2=2).copy()
        self.sp = LD(1) / (LD(1) + np.sqrt(hp))
        dmp = _damping(hp, self.sp, radius)
        Hd[:, range(6), range(6)] += dmp
        Hda[:, range(6), range(6)] += np.asarray(dmp, np.float64)
        # ---- Schur terms: every ordered pair of free observations of one landmark
        W = np.einsum("nai,naj->nij", Jp, Jl)                       # 6x3 per observation
        Wa = np.einsum("nai,naj->nij", Jpa, Jla)
        self.W = W
        s_of = self.slot_of_obs
        X = np.einsum("nij,njk->nik", W, Vinv[s_of])               # W V^-1
        Xa = np.einsum("nij,njk->nik", Wa, Via[s_of] * self.kappa_V[s_of][:, None, None])
        # rhs: rhs = -(g_p - sum W V^-1 g_l)
        rl = np.zeros((nf, 6), dtype=LD)
        rla = np.zeros((nf, 6))
        gla = np.zeros((self.lm.shape[0], d))
        np.add.at(gla, s_of, np.einsum("nai,na->ni", Jla, rabs))
        obs_f = np.flatnonzero(fr)
        if obs_f.size:
            o3, fk3, st3 = _segments(f[obs_f])
            sel = obs_f[o3]
            fu = fk3[st3]
            rl[fu] = np.add.reduceat(np.einsum("nij,nj->ni", X[sel], gl[s_of[sel]]), st3, axis=0)
            rla[fu] = np.add.reduceat(np.einsum("nij,nj->ni", Xa[sel], gla[s_of[sel]]), st3, axis=0)
        self.rhs = -(gp - rl).reshape(n)
        tmax = float(np.diff(np.concatenate([st, [lk.size]])).max()) if lk.size else 0.0
        m_rhs = np.repeat(m_diag * (1.0 + tmax), 6)
        # Schur blocks: every ordered pair (a, b) of free observations of one landmark, summed into the distinct blocks
        oj, lj, stj = _segments(s_of[obs_f])
        obs_sorted = obs_f[oj]
        cnt = np.diff(np.concatenate([stj, [obs_sorted.size]]))
        pairs = []
        for t in np.unique(cnt):
            idx = obs_sorted[stj[cnt == t][:, None] + np.arange(t)[None, :]]          # (n_t, t)
            pairs.append((np.repeat(idx, t, axis=1).ravel(), np.tile(idx, (1, t)).ravel()))
        pa = np.concatenate([p[0] for p in pairs]) if pairs else np.zeros(0, np.int64)
        pb = np.concatenate([p[1] for p in pairs]) if pairs else np.zeros(0, np.int64)
        pkeys = f[pa] * nf + f[pb]
        diag_keys = np.arange(nf) * (nf + 1)
        cross = [] if fs is None else [(fidx[k1], fidx[k2], X) for (k1, k2), X in fs.cross.items() if fidx[k1] >= 0 and fidx[k2] >= 0]
        cross_keys = np.array([k for a, b, _ in cross for k in (a * nf + b, b * nf + a)], np.int64)
        self.keys = np.unique(np.concatenate([pkeys, diag_keys, cross_keys]))
        K = self.keys.size
        blocks = np.zeros((K, 6, 6), dtype=LD)
        blocka = np.zeros((K, 6, 6))
        counts = np.zeros(K)
        CH = 1 << 18
        for c0 in range(0, pa.size, CH):
            aa, bb = pa[c0: c0 + CH], pb[c0: c0 + CH]
            slot_k = np.searchsorted(self.keys, pkeys[c0: c0 + CH])
            o, ks, stc = _segments(slot_k)
            u = ks[stc]
            blocks[u] -= np.add.reduceat(np.einsum("nij,nkj->nik", X[aa[o]], W[bb[o]]), stc, axis=0)
            blocka[u] += np.add.reduceat(np.einsum("nij,nkj->nik", Xa[aa[o]], Wa[bb[o]]), stc, axis=0)
            counts[u] += np.diff(np.concatenate([stc, [o.size]]))
        dslot = np.searchsorted(self.keys, diag_keys)
        blocks[dslot] += Hd
        blocka[dslot] += Hda
        counts[dslot] += m_diag
        Ev = np.zeros((K, 6, 6))
        for a, b, X in cross:       # J_1^T J_2 at (a, b), its transpose at (b, a): no landmark need fill them
            for key, T in ((a * nf + b, lambda M: M), (b * nf + a, lambda M: M.T)):
                i = int(np.searchsorted(self.keys, key))
                blocks[i] += T(X[0])
                Ev[i] += T(X[1])
                blocka[i] += T(X[2])
                counts[i] += X[3]
        if fs is not None:
            Ev[dslot[fidx[free_poses]]] += fs.Hv[free_poses]
        self.blocks = blocks
        self.m = counts
        self.E_blocks = ((self.m + C_TERMS) * U)[:, None, None] * blocka + Ev
        if H_unary is not None:      # unary rows: rounding of the device's closed forms, c u |H_unary|
            for i, key in enumerate(self.keys):
                a, b = key // nf, key % nf
                self.E_blocks[i] += C_TERMS * U * Ha_unary[6 * a: 6 * a + 6, 6 * b: 6 * b + 6]
        self.E_rhs = (m_rhs + C_TERMS) * U * (gpa + rla).reshape(n) + gv.reshape(n)
        self.rows = rows
        self._k, self._j, self._f = k, j, f
        self.nb = 0
        if "Jb" in rows and rows["Jb"].shape[-1]:
            self._border(rows, radius, X, Xa, Via, gla, fr, m_rhs)

    def _border(self, rows, radius, X, Xa, Via, gla, fr, m_rhs):
        """The border of free shared columns (light 3, Phong 3M, textures M: np_reference.phong_lm_step's order):
            S_pb = A_pb - sum_j W_j V_j^-1 Y_j^T,  S_bb = A_bb + D_b - sum_j Y_j V_j^-1 Y_j^T,
            rhs_b = -(g_b - sum_j Y_j V_j^-1 g_l,j),  Y_j = sum over the observations of j of J_b^T J_l,
        damped as ssba_border_system reports it: the Jacobi scale s_b = 1 / (1 + sqrt(diag A_bb)) of the undamped border
        diagonal and D_b = clamp(h s_b^2, 1e-6, 1e32) / (radius s_b^2).  E extends to the border as to S: every border entry
        sums over all observations and landmarks, so m = N + L there."""
        Jb, Jba, Jl, Jla, Jp, Jpa, r, rabs = (rows[k] for k in ("Jb", "Jba", "Jl", "Jla", "Jp", "Jpa", "r", "rabs"))
        nb, nf, L = Jb.shape[-1], self.nf, self.lm.shape[0]
        self.nb = nb
        so = self.slot_of_obs
        Y = np.zeros((L, nb, self.d), dtype=LD)
        Ya = np.zeros((L, nb, self.d))
        np.add.at(Y, so, np.einsum("nab,nai->nbi", Jb, Jl))
        np.add.at(Ya, so, np.einsum("nab,nai->nbi", Jba, Jla))
        self.Y = Y
        A_bb = np.einsum("nab,nac->bc", Jb, Jb)
        A_bba = np.einsum("nab,nac->bc", Jba, Jba)
        g_b = np.einsum("nab,na->b", Jb, r)
        g_ba = np.einsum("nab,na->b", Jba, rabs)
        hb = np.diagonal(A_bb).copy()
        self.sb = LD(1) / (LD(1) + np.sqrt(hb))
        Db = _damping(hb, self.sb, radius)
        YVi = np.einsum("lbi,lij->lbj", Y, self.Vinv)
        YVia = np.einsum("lbi,lij->lbj", Ya, Via * self.kappa_V[:, None, None])
        self.S_bb = A_bb + np.diag(Db) - np.einsum("lbj,lcj->bc", YVi, Y)
        self.rhs_b = -(g_b - np.einsum("lbj,lj->b", YVi, self.gl))
        S_pb = np.zeros((nf, 6, nb), dtype=LD)
        S_pba = np.zeros((nf, 6, nb))
        fo = np.flatnonzero(fr)
        fk = self._f[fo]
        np.add.at(S_pb, fk, np.einsum("nai,nab->nib", Jp[fo], Jb[fo]) - np.einsum("nij,nbj->nib", X[fo], Y[so[fo]]))
        np.add.at(S_pba, fk, np.einsum("nai,nab->nib", Jpa[fo], Jba[fo]) + np.einsum("nij,nbj->nib", Xa[fo], Ya[so[fo]]))
        self.S_pb = S_pb.reshape(6 * nf, nb)
        m = float(Jb.shape[0] + L + C_TERMS)
        self.E_bb = m * U * (A_bba + np.diag(np.asarray(Db, np.float64)) + np.einsum("lbj,lcj->bc", YVia, Ya))
        self.E_pb = m * U * S_pba.reshape(6 * nf, nb)
        self.E_rhs_b = m * U * (g_ba + np.einsum("lbj,lj->b", YVia, gla))

    def border_excess(self, S_pb, S_bb, rhs_b):
        """max |dev - truth| / E over S_pb, S_bb and rhs_b (<= 1 passes)."""
        out = []
        for dev, ref, E in ((S_pb, self.S_pb, self.E_pb), (S_bb, self.S_bb, self.E_bb), (rhs_b, self.rhs_b, self.E_rhs_b)):
            dd = np.abs(np.asarray(np.asarray(dev, LD) - ref, np.float64))
            out.append(float((dd / np.maximum(E, 1e-300)).max()))
        return tuple(out)

    def bordered(self):
        """[S S_pb; S_pb^T S_bb] and [rhs; rhs_b] as dense long-double arrays."""
        return (np.block([[self.dense(), self.S_pb], [self.S_pb.T, self.S_bb]]), np.concatenate([self.rhs, self.rhs_b]))

    # ---- views
    def dense(self, dtype=LD):
        """S as a dense n x n array (small systems)."""
        M = np.zeros((self.n, self.n), dtype=dtype)
        nf = self.nf
        for key, B in zip(self.keys, self.blocks):
            a, b = key // nf, key % nf
            M[6 * a: 6 * a + 6, 6 * b: 6 * b + 6] = B
        return M

    def dense_bound(self):
        M = np.zeros((self.n, self.n))
        nf = self.nf
        for key, B in zip(self.keys, self.E_blocks):
            a, b = key // nf, key % nf
            M[6 * a: 6 * a + 6, 6 * b: 6 * b + 6] = B
        return M

    def assembly_excess(self, S_dev, rhs_dev):
        """max over entries of |S_dev - S| / E and |rhs_dev - rhs| / E_rhs (<= 1 passes); inf if S_dev has a non-zero entry
        outside the blocks the reference forms."""
        nf = self.nf
        a, b = self.keys // nf, self.keys % nf
        r6 = np.arange(6)
        ri = (6 * a)[:, None, None] + r6[None, :, None]
        ci = (6 * b)[:, None, None] + r6[None, None, :]
        Sd = np.asarray(S_dev)
        d = np.abs(np.asarray(Sd[ri, ci], LD) - self.blocks).astype(np.float64)
        worst = float((d / np.maximum(self.E_blocks, 1e-300)).max())
        covered = np.zeros((nf, nf), bool)
        covered[a, b] = True
        outside = ~np.repeat(np.repeat(covered, 6, axis=0), 6, axis=1)
        if np.any(Sd[outside] != 0):
            return float("inf"), float("inf")
        d = np.abs(np.asarray(rhs_dev, LD) - self.rhs).astype(np.float64)
        return worst, float((d / np.maximum(self.E_rhs, 1e-300)).max())

    # ---- back-substitution and the model cost change from a given pose step
    def back_substitute(self, dp_free, db=None):
        """delta_l = V^-1 (-g_l - W^T delta_p - Y^T delta_b) in long double from the free-pose step (nf*6) and the border
        step; (landmarks present, d)."""
        x = np.asarray(dp_free, LD).reshape(-1, 6)
        Wt = np.zeros((self.lm.shape[0], self.d), dtype=LD)
        if self.nb:
            Wt += np.einsum("lbi,b->li", self.Y, np.asarray(db, LD))
        fr = self._f >= 0
        np.add.at(Wt, self.slot_of_obs[fr], np.einsum("nij,ni->nj", self.W[fr], x[self._f[fr]]))
        return np.einsum("nij,nj->ni", self.Vinv, -self.gl - Wt)

    def model_cost_change(self, dp_free, dl_present, db=None):
        """-J delta . (r + J delta / 2) in long double and the magnitude sum of its terms."""
        x = np.asarray(dp_free, LD).reshape(-1, 6)
        y = np.asarray(dl_present, LD)
        fr = self._f >= 0
        Jd = np.einsum("nai,ni->na", self.rows["Jl"], y[self.slot_of_obs])
        if self.nb:
            Jd += np.einsum("nab,b->na", self.rows["Jb"], np.asarray(db, LD))
        Jd[fr] += np.einsum("nai,ni->na", self.rows["Jp"][fr], x[self._f[fr]])
        r = self.rows["r"]
        terms = -(Jd * (r + LD(0.5) * Jd))
        total, mag, count = terms.sum(), float(np.abs(np.asarray(Jd * r, np.float64)).sum() + 0.5 * np.abs(np.asarray(Jd * Jd, np.float64)).sum()), terms.size
        if self.factor_sums is not None:
            # the rows of the pose-only blocks, with their magnitudes in place of the absolute values: C_ROW u on J and on r
            # costs 2 C_ROW u (mag_J |x|) mag_r to first order, which (n + c) u times that product covers from n >= 16 rows on
            fidx = np.full(self.factor_sums.H.shape[0], -1, np.int64)
            fidx[self.factor_sums.free_poses] = np.arange(self.nf)
            for a in self.factor_sums.rows:
                jd, jm = np.zeros(a["r"].shape[0], LD), np.zeros(a["r"].shape[0])
                for (k, J), (_, Jm) in zip(a["blocks"], a["mag_blocks"]):
                    if fidx[k] >= 0:
                        jd += J @ x[fidx[k]]
                        jm += Jm @ np.abs(np.asarray(x[fidx[k]], np.float64))
                total += -(jd * (a["r"] + LD(0.5) * jd)).sum()
                mag += float((jm * a["mag_r"]).sum() + 0.5 * (jm * jm).sum())
                count += jd.size
        return total, mag, count


def free_index(num_poses, obs_pose, pose_const, factor_poses=None):
    """Free index of every pose (-1: constant, or touched by nothing).  factor_poses: the poses that a pose-only residual block
    touches -- a state without observations is free through its odometry blocks alone."""
    seen = np.bincount(np.asarray(obs_pose, np.int64), minlength=num_poses) > 0
    if factor_poses is not None:
        seen[np.asarray(list(factor_poses), np.int64)] = True
    free = ~np.asarray(pose_const, bool) & seen
    fidx = np.full(num_poses, -1, np.int64)
    fidx[free] = np.arange(int(free.sum()))
    return fidx


# ------------------------------------------------------------------------------------------------------------ refined solve
def _band_lower(S64, bw):
    n = S64.shape[0]
    ab = np.zeros((bw + 1, n))
    for d in range(bw + 1):
        ab[d, : n - d] = np.diagonal(S64, -d)
    return ab


def _band_matvec(abL, x):
    """y = S x for symmetric S given by its lower band (long double)."""
    y = abL[0] * x
    n = x.shape[0]
    for d in range(1, abL.shape[0]):
        y[d:] += abL[d, : n - d] * x[: n - d]
        y[: n - d] += abL[d, : n - d] * x[d:]
    return y


def bandwidth(S):
    """Lower bandwidth of a dense symmetric matrix."""
    rows, cols = np.nonzero(np.asarray(S) != 0)
    return int((rows - cols).max()) if rows.size else 0


def refined_solve(S, rhs, band=None, max_iter=40):
    """x with S x = rhs: fp64 Cholesky (banded when `band` -- the lower bandwidth -- is given) and iterative refinement
    with the residual in long double; stops when the correction stalls.  Returns (x in long double, kappa_2 estimate).

    The result is as accurate as the long-double residual allows: componentwise, cond(S, x) 2^-64 plus the last
    correction (Skeel); normwise at worst kappa_2 2^-64, 2^11 times below the fp64 bar 4096 u kappa_2 the tests use.
    """
    S = np.asarray(S)
    S64 = np.asarray(S, np.float64)
    b = np.asarray(rhs, LD)
    if band is None:
        fac = sla.cho_factor(S64, lower=True)
        solve = lambda v: sla.cho_solve(fac, v)
        SL = np.asarray(S, LD)
        matvec = lambda v: SL @ v
    else:
        ab = _band_lower(S64, band)
        abL = _band_lower(np.asarray(S, LD), band) if S.dtype == LD else ab.astype(LD)
        cb = sla.cholesky_banded(ab, lower=True)
        solve = lambda v: sla.cho_solve_banded((cb, True), v)
        matvec = lambda v: _band_matvec(abL, v)
    x = np.asarray(solve(np.asarray(b, np.float64)), LD)
    prev = np.inf
    for _ in range(max_iter):
        res = b - matvec(x)
        dx = solve(np.asarray(res, np.float64))
        x = x + np.asarray(dx, LD)
        nd = float(np.abs(dx).max())
        if nd <= 2.0 ** -66 * float(np.abs(x).max()) or nd >= 0.5 * prev:
            break
        prev = nd
    return x, kappa2(S64, band)


def kappa2(S64, band=None):
    n = S64.shape[0]
    if n <= DENSE_EIG_MAX or band is None:
        w = np.linalg.eigvalsh(0.5 * (S64 + S64.T))
        return float(w[-1] / w[0])
    ab = _band_lower(S64, band)
    lo = sla.eigvals_banded(ab, lower=True, select="i", select_range=(0, 0))[0]
    hi = sla.eigvals_banded(ab, lower=True, select="i", select_range=(n - 1, n - 1))[0]
    return float(hi / lo)


# ------------------------------------------------------------------------------------------------------------ bound helpers
def backward_error(S, rhs, x):
    """eta = |rhs - S x|_inf / (|S|_inf |x|_inf + |rhs|_inf), residual in long double."""
    SL, b, xl = np.asarray(S, LD), np.asarray(rhs, LD), np.asarray(x, LD)
    res = np.abs(np.asarray(b - SL @ xl, np.float64)).max()
    Sn = np.abs(np.asarray(S, np.float64)).sum(1).max()
    return float(res / (Sn * np.abs(np.asarray(x, np.float64)).max() + np.abs(np.asarray(rhs, np.float64)).max()))


def backward_error_banded(S, rhs, x, band):
    abL = _band_lower(np.asarray(S, np.float64), band).astype(LD)
    res = np.abs(np.asarray(np.asarray(rhs, LD) - _band_matvec(abL, np.asarray(x, LD)), np.float64)).max()
    A = np.abs(_band_lower(np.asarray(S, np.float64), band))
    rs = A[0].copy()
    n = rs.shape[0]
    for d in range(1, A.shape[0]):
        rs[d:] += A[d, : n - d]
        rs[: n - d] += A[d, : n - d]
    return float(res / (rs.max() * np.abs(np.asarray(x, np.float64)).max() + np.abs(np.asarray(rhs, np.float64)).max()))


def forward_error(x, x_true):
    x_true = np.asarray(x_true, LD)
    return float(np.sqrt(((np.asarray(x, LD) - x_true) ** 2).sum() / (x_true ** 2).sum()))


def solve_bars(kappa, oracle_bar=1e-8):
    """(eta bar, forward-error bar): SOLVE_C u and SOLVE_C u kappa_2, never looser than the oracle parity bar."""
    return SOLVE_C * U, min(SOLVE_C * U * kappa, oracle_bar)


def covariance_truth(S_ld, f, band=None):
    """6x6 block of S^-1 of free pose f from six refined solves (S in long double)."""
    n = S_ld.shape[0]
    cols = []
    for c in range(6):
        e = np.zeros(n)
        e[6 * f + c] = 1.0
        x, kap = refined_solve(S_ld, e, band)
        cols.append(x[6 * f: 6 * f + 6])
    return np.stack(cols, 1), kap


def covariance_bound(S64, E, f, kappa, cov_true):
    """Entrywise bound on |cov_dev - cov_true| for a device covariance formed from an S within E of the truth: the first-
    order propagation |S^-1| E |S^-1| of the assembly error, plus the solve term SOLVE_C u kappa_2 max|cov|."""
    Si = np.abs(np.linalg.inv(S64))
    rows = Si[6 * f: 6 * f + 6]
    return rows @ E @ rows.T + SOLVE_C * U * kappa * float(np.abs(np.asarray(cov_true, np.float64)).max())


def unary_pose_blocks(poses, factors, fidx):
    """H = J^T J, g = J^T r and |J|^T |J| of pose-prior (type 0) and sun-sensor (type 1) rows in fp64, free-pose
    coordinates: the reference formulas of np_reference with complex-step Jacobians through SE3 Plus.  Without a loss."""
    import np_reference as npr
    n = 6 * int((np.asarray(fidx) >= 0).sum())
    H, g, Ha = np.zeros((n, n)), np.zeros(n), np.zeros((n, n))
    for fct in factors:
        assert fct.get("huber", 0.0) == 0.0 and fct["type"] in (0, 1)
        k = fct["pose"]
        if fct["type"] == 0:
            fun = lambda X: npr.pose_prior_residual(X, np.asarray(fct["data"]), np.asarray(fct["stiffness"]).reshape(6, 6))
        else:
            d = np.asarray(fct["data"])
            fun = lambda X: npr.sun_sensor_residual(X, d[:3], d[3:6], np.asarray(fct["stiffness"]).reshape(2, 2), d[6], d[7])
        r, J = fun(poses[k]).real, npr.se3_complex_step_jacobian(fun, poses[k])
        sl = slice(6 * int(fidx[k]), 6 * int(fidx[k]) + 6)
        H[sl, sl] += J.T @ J
        g[sl] += J.T @ r
        Ha[sl, sl] += np.abs(J).T @ np.abs(J)
    return H, g, Ha


# ------------------------------------------------------------------------------------------------------- pose-factor rows
_PF_INPUTS = {0: ("T", "ref", "S"), 1: ("T", "oc", "eg", "S"), 2: ("T", "T2", "ref", "S")}
_PF_UNITS = {0: (("R_res", 9), ("t_res", 3), ("axis", 3), ("sin_angle", 1), ("cos_angle", 1), ("angle", 1)),
             1: (("s_c", 3), ("eaz", 1), ("ezen", 1), ("oaz", 1), ("ozen", 1)),
             2: (("R_12", 9), ("v", 3), ("R_res", 9), ("t_res", 3), ("axis", 3), ("sin_angle", 1), ("cos_angle", 1), ("angle", 1))}
_PF_GUARDS = {0: ("angle",), 1: ("raz", "raz_wrapped", "rzen"), 2: ("angle",)}


def _pf_eval(tp, x, pert, outlier=None):
    """One type of pose factor on stacked blocks `x` (complex arrays): [r (N,m), J per pose touched (N,m,6)..., the
    uncorrected r (N,m), |r|^2 (N,), the guard quantities (N,)...] and the Huber decision.  Complex step through the forward
    formulas of np_reference and SE3Perturbation's Plus (_se3_columns); the corrector sqrt(rho') multiplies r and J where
    `outlier` (the decision of the unperturbed long-double |r|^2 when the magnitudes are measured)."""
    import np_reference as npr
    h = H_CS
    seen = {}

    def hook(name, v):
        if pert is not None:
            v = pert(name, v)
        seen.setdefault(name, v)        # the first evaluation is the one at the pose itself
        return v

    if tp == 0:
        funs = [(x["T"], lambda T: npr.pose_prior_residual(T, x["ref"], x["S"], hook))]
    elif tp == 1:
        funs = [(x["T"], lambda T: npr.sun_sensor_residual(T, x["oc"], x["eg"], x["S"], x["taz"], x["tzen"], hook))]
    else:
        funs = [(x["T"], lambda T: npr.relative_pose_residual(T, x["T2"], x["ref"], x["S"], hook)),
                (x["T2"], lambda T: npr.relative_pose_residual(x["T"], T, x["ref"], x["S"], hook))]
    r = funs[0][1](funs[0][0]).real
    Js = []
    for T, f in funs:
        cols = _se3_columns(T, h)
        Js.append(np.stack([f(cols[c]).imag / h for c in range(6)], -1))
    sq = (r * r).sum(-1)
    a = x["huber"].real
    if outlier is None:
        outlier = (a > 0) & (sq > a * a)
    w = np.where(outlier, np.sqrt(np.where(outlier, a, 1) / np.sqrt(np.where(outlier, sq, 1))), 1)
    return [r * w[:, None]] + [J * w[:, None, None] for J in Js] + [r, sq] + [seen[g].real for g in _PF_GUARDS[tp]], outlier


def pose_factor_rows(poses, factors, dtype=LD, mags=True):
    """Rows of the pose-only residual blocks -- pose prior (type 0), sun sensor (1), relative pose between `pose` and
    `pose2` (2) -- in `dtype` (LD, or np.float64: the fp64 evaluation the bars are proved on), by complex step in the
    matching complex type through np_reference's forward formulas and SE3Perturbation's Plus, as phong_rows does it.  The
    formulas' own branches and constants are followed: the fp64 DBL_EPSILON guard of the logarithm (first-order branch
    vee(C - I) / 2), the fp64 value of pi in the wrap of the azimuth residual, the thresholds that zero a residual angle
    together with its gradient, and the Huber corrector sqrt(rho') on r and J, decided on |r|^2 in `dtype`.

    One dict per factor, in order: r (m), blocks [(pose, J (m x 6))], cost = rho(|r|^2) / 2, sq = |r|^2 before the corrector,
    outlier, guards {angle | raz, raz_wrapped, rzen}; and (mags=True) a rounding magnitude of every value: mag_r, mag_blocks,
    mag_r_raw (of the uncorrected r), mag_sq, mag_guards.  The bar on an fp64 evaluation is C_ROW u mag.

    mag is measured as in phong_rows: |Q| plus the first-order sensitivities of Q to relative perturbations DELTA_MAG of
    each input (poses, the reference pose or the two directions, the stiffness) and of each intermediate that the
    reference's formula stores, component by component.  What each intermediate stands for:
      R_res      the 3-term dot products of R_ref R^T (R_ref R_12), which every entry of the logarithm reads; and, in
                 t_ref - R_res t, the product whose rotation columns cancel against the motion of t (d / d eps_r of the
                 translation rows is exactly zero: a rigid rotation moves R_res and t together) -- no perturbation of an
                 input sees that cancellation, since Plus carries it along, but a rounded R_res breaks it;
      R_12, v    (relative) the same for R_1 R_2^T and v = t_1 - R_12 t_2: R_12 t_2 does not change with a rotation of pose 2,
                 and v cancels where both poses are far from the origin and close to each other;
      t_res      the sum t_ref - R_res t (R_ref v + t_ref): cancels where the pose is far from the origin;
      axis       the differences C_kj - C_jk, of size 2 sin(angle): near pi they cancel to the rounding of C;
      sin_angle  the square root of the sum of squares; cos_angle: the trace minus one, which cancels near angle = 2 pi / 3
                 and whose rounding moves atan2 by |d cos| sin near pi / 2;
      angle      atan2 itself (added to the list the rows were first measured with: a relative change of sin_angle moves the
                 angle and the quotient angle / sin_angle together, so at small angles it cancels out of the logarithm,
                 while the rounding of atan2 and that of the division are independent; the off-diagonal entries of
                 d log / d eps, ~angle / 2 beside a diagonal of 1, are differences of terms of size 1 that only this sees);
      s_c        R e_g: 1 - y^2 and x^2 + z^2 of the angle gradients read it -- 1 / sqrt(1 - y^2) has the relative sensitivity
                 y^2 / (1 - y^2) to y, which is the loss of 1 - y^2 as the zenith tends to 0 or pi;
      the four angles  acos and atan2 (a few ulps each) and the differences e - o, which cancel for a small residual.
    The Huber scale is a function of the row (w = sqrt(a / |r|)) and is perturbed with it.  Where a threshold zeroes an angle,
    Q and mag are 0 for that angle's share: the bar is then an exact zero.  The derivatives are measured with one extra
    evaluation per perturbation, so mag carries a relative error of 2^-64 / DELTA_MAG = 2^-12 in long double."""
    cdt = np.clongdouble if dtype == LD else complex
    poses = np.asarray(poses, np.float64)
    out = [None] * len(factors)
    for tp in (0, 1, 2):
        idx = [i for i, f in enumerate(factors) if f["type"] == tp]
        if not idx:
            continue
        N = len(idx)
        fs = [factors[i] for i in idx]
        dat = np.stack([np.asarray(f["data"], np.float64).ravel()[:12 if tp != 1 else 8] for f in fs])
        m = 2 if tp == 1 else 6
        c = lambda v: np.asarray(v, dtype=cdt)
        x = dict(T=c(poses[[f["pose"] for f in fs]]), S=c(np.stack([np.asarray(f["stiffness"], np.float64).reshape(m, m) for f in fs])),
                 huber=c([f.get("huber", 0.0) for f in fs]))
        if tp == 1:
            x.update(oc=c(dat[:, :3]), eg=c(dat[:, 3:6]), taz=c(dat[:, 6]), tzen=c(dat[:, 7]))
        else:
            x["ref"] = c(dat)
        if tp == 2:
            x["T2"] = c(poses[[f["pose2"] for f in fs]])
        res, outlier = _pf_eval(tp, x, None)
        nj = 2 if tp == 2 else 1
        acc = None
        if mags:
            ref = [np.asarray(v, LD) for v in res]
            acc = [np.abs(np.asarray(v, np.float64)) for v in res]

            def add(res2, rel):
                for a, v, r0 in zip(acc, res2, ref):
                    d = np.abs(np.asarray(np.asarray(v, LD) - r0, np.float64))
                    a += d / rel.reshape((-1,) + (1,) * (d.ndim - 1))

            for name in _PF_INPUTS[tp]:
                flat = x[name].reshape(N, -1)
                for k in range(flat.shape[1]):
                    xr = np.abs(np.asarray(flat[:, k].real, np.float64))
                    if not np.any(xr > 0):
                        continue
                    f2 = flat.copy()
                    f2[:, k] = f2[:, k] * (1 + DELTA_MAG)
                    rel = np.abs(np.asarray((f2[:, k] - flat[:, k]).real, np.float64)) / np.maximum(xr, 1e-300)
                    y = dict(x)
                    y[name] = f2.reshape(x[name].shape)
                    add(_pf_eval(tp, y, None, outlier)[0], np.where(xr > 0, rel, np.inf))
            for name, width in _PF_UNITS[tp]:
                for k in range(width):
                    def pert(nm, v, name=name, k=k, width=width):
                        if nm != name:
                            return v
                        if width == 1:
                            return v * (1 + DELTA_MAG)
                        v = v.reshape(v.shape[:-2] + (9,)).copy() if width == 9 else v.copy()
                        v[..., k] = v[..., k] * (1 + DELTA_MAG)
                        return v.reshape(v.shape[:-1] + (3, 3)) if width == 9 else v
                    add(_pf_eval(tp, x, pert, outlier)[0], np.full(N, DELTA_MAG))
        rdt = LD if dtype == LD else np.float64
        for n, i in enumerate(idx):
            f = fs[n]
            ks = [f["pose"]] + ([f["pose2"]] if tp == 2 else [])
            sq, a = res[nj + 2][n], rdt(f.get("huber", 0.0))
            rho = 2 * a * np.sqrt(sq) - a * a if outlier[n] else sq
            d = dict(r=np.asarray(res[0][n], rdt), blocks=[(k, np.asarray(res[1 + b][n], rdt)) for b, k in enumerate(ks)],
                     cost=rdt(0.5) * rho, sq=sq, outlier=bool(outlier[n]),
                     guards={g: res[nj + 3 + q][n] for q, g in enumerate(_PF_GUARDS[tp])})
            if mags:
                d.update(mag_r=acc[0][n], mag_blocks=[(k, acc[1 + b][n]) for b, k in enumerate(ks)], mag_r_raw=acc[nj + 1][n],
                         mag_sq=acc[nj + 2][n], mag_guards={g: acc[nj + 3 + q][n] for q, g in enumerate(_PF_GUARDS[tp])})
            out[i] = d
    return out


def _pf_product(A, Am, B, Bm):
    """A^T B over the rows of one block with the two parts of its bar: (value, value rounding, sum of magnitudes)."""
    f = lambda v: np.abs(np.asarray(v, np.float64))
    return A.T @ B, C_TERMS * U * (Am.T @ f(B) + f(A).T @ Bm), f(A).T @ f(B)


def factor_poses(factors):
    return sorted({k for f in factors for k in ([f["pose"]] + ([f["pose2"]] if f["type"] == 2 else []))})


class PoseFactorSums:
    """What the device sums from the pose-only residual blocks, in long double from pose_factor_rows (with magnitudes) and in
    list order: per pose H = sum J^T J and g = sum J^T r, per pair of poses of a relative block J_1^T J_2 (cross[(k1, k2)]),
    and the cost.  `free_poses`: the poses that are free (for SchurSystem.model_cost_change); default all.

    Bars.  A row value carries C_ROW u mag, so a sum of m products a_i b_i carries, to first order,
        C_TERMS u sum (mag_a |b| + |a| mag_b)  +  (m + C_TERMS) u sum |a| |b|:
    the rounding of the values (C_ROW = C_TERMS; Hv, gv, cross[..][1]) and the gamma_m of the summation with the c of the
    products' own arithmetic (Hs, gs, cross[..][2] are the sums of magnitudes, m / cross[..][3] the numbers of terms), as in
    test_pose_graph_only_with_a_prior_exactly_on_its_pose.  The cost: C_TERMS u sum |r| mag_r + (n + C_TERMS) u sum |term|
    over the n blocks (cost_at)."""

    def __init__(self, P, factors, rows, free_poses=None):
        f = lambda v: np.abs(np.asarray(v, np.float64))
        self.rows = rows
        self.free_poses = np.arange(P) if free_poses is None else np.asarray(free_poses, np.int64)
        self.H, self.g = np.zeros((P, 6, 6), LD), np.zeros((P, 6), LD)
        self.Hv, self.Hs, self.gv, self.gs = np.zeros((P, 6, 6)), np.zeros((P, 6, 6)), np.zeros((P, 6)), np.zeros((P, 6))
        self.m = np.zeros(P)
        self.cross = {}
        self.cost, self.cost_v, self.cost_s = LD(0), 0.0, 0.0
        for fct, a in zip(factors, rows):
            r, rm = a["r"], a["mag_r"]
            for (k, J), (_, Jm) in zip(a["blocks"], a["mag_blocks"]):
                for tgt, (val, v, s) in (((self.H, self.Hv, self.Hs), _pf_product(J, Jm, J, Jm)),
                                         ((self.g, self.gv, self.gs), _pf_product(J, Jm, r[:, None], rm[:, None]))):
                    tgt[0][k] += val.reshape(tgt[0][k].shape)
                    tgt[1][k] += v.reshape(tgt[1][k].shape)
                    tgt[2][k] += s.reshape(tgt[2][k].shape)
                self.m[k] += r.shape[0]
            if fct["type"] == 2:
                (k1, J1), (k2, J2) = a["blocks"]
                (_, M1), (_, M2) = a["mag_blocks"]
                val, v, s = _pf_product(J1, M1, J2, M2)
                X = self.cross.setdefault((k1, k2), [np.zeros((6, 6), LD), np.zeros((6, 6)), np.zeros((6, 6)), 0])
                X[0] += val
                X[1] += v
                X[2] += s
                X[3] += 6
            self.cost += a["cost"]
            self.cost_v += C_TERMS * U * float((f(r) * rm).sum())
            self.cost_s += abs(float(a["cost"]))
        self.n = len(factors)

    def H_bar(self, extra_m=0.0):
        return self.Hv + ((self.m + extra_m + C_TERMS) * U)[:, None, None] * self.Hs

    def g_bar(self, extra_m=0.0):
        return self.gv + ((self.m + extra_m + C_TERMS) * U)[:, None] * self.gs

    def cross_bar(self, key):
        X = self.cross[key]
        return X[1] + (X[3] + C_TERMS) * U * X[2]

    def cost_bar(self):
        return self.cost_v + (self.n + C_TERMS) * U * self.cost_s


# ---------------------------------------------------------------------------------------------------------------- dogleg
# Ceres' DoglegStrategy (dogleg_strategy.cc) written in Jacobi-scaled coordinates, as Ceres writes it: J_s = J diag(s) with
# s = 1 / (1 + sqrt(diag(J^T J))) at the linearisation point, D^2 = clamp(diag(J_s^T J_s), min_lm_diagonal, max_lm_diagonal),
# gradient_ = J_s^T r / D, the Gauss-Newton step of (J_s^T J_s + mu D^2) in D-scaled space, the Cauchy point, TRADITIONAL_DOGLEG
# and SUBSPACE_DOGLEG; steps are returned in unscaled coordinates, delta = beta delta_gn + gamma v with v = s^2 g / D^2.
# The device (k_dogleg_vec / k_dogleg_gn / k_dogleg_interp) restates all of this in unscaled coordinates and takes the
# row-space products from an expanded identity; here every J x is formed row by row.
C_DL_ROW = 16             # c_row: rounding of one row value J x (one 3- to 19-term dot product and the row's own rounding)


def _rel_residual(T1, T2, T_ref, S):
    """RelativePoseErrorAutomatic: S log(T_ref T1 T2^-1) with the reference's log = [translation ; axis-angle]."""
    import np_reference as npr
    R1, R2, Rr = T1[3:].reshape(3, 3), T2[3:].reshape(3, 3), T_ref[3:].reshape(3, 3)
    R12 = R1 @ R2.T
    t = Rr @ (T1[:3] - R12 @ T2[:3]) + T_ref[:3]
    return S @ np.concatenate([t, npr.so3_log(Rr @ R12)])


def unary_rows(poses, factors):
    """Rows of the pose-only residual blocks (prior 0, sun 1, relative 2 between pose and pose2): one entry per block with
    r (m), and (pose, J (m x 6)) per pose it touches -- fp64 complex-step Jacobians through SE3 Plus, Huber-corrected like the
    stereo rows (sqrt(rho') on r and J)."""
    import np_reference as npr
    out = []
    for fct in factors:
        S = np.asarray(fct["stiffness"], np.float64)
        d = np.asarray(fct["data"], np.float64)
        if fct["type"] == 0:
            fun = lambda X: npr.pose_prior_residual(X, d[:12], S.reshape(6, 6))
            r, blocks = fun(poses[fct["pose"]]).real, [(fct["pose"], npr.se3_complex_step_jacobian(fun, poses[fct["pose"]]))]
        elif fct["type"] == 1:
            fun = lambda X: npr.sun_sensor_residual(X, d[:3], d[3:6], S.reshape(2, 2), d[6], d[7])
            r, blocks = fun(poses[fct["pose"]]).real, [(fct["pose"], npr.se3_complex_step_jacobian(fun, poses[fct["pose"]]))]
        else:
            k1, k2 = fct["pose"], fct["pose2"]
            T1, T2 = poses[k1], poses[k2]
            r = _rel_residual(T1, T2, d[:12], S.reshape(6, 6)).real
            J1 = npr.se3_complex_step_jacobian(lambda X: _rel_residual(X, T2.astype(complex), d[:12], S.reshape(6, 6)), T1)
            J2 = npr.se3_complex_step_jacobian(lambda X: _rel_residual(T1.astype(complex), X, d[:12], S.reshape(6, 6)), T2)
            blocks = [(k1, J1), (k2, J2)]
        w = float(huber_weight(np.float64((r * r).sum()), fct.get("huber", 0.0), np.float64))
        out.append(dict(r=np.asarray(r * w, LD), blocks=[(k, np.asarray(J * w, LD)) for k, J in blocks]))
    return out


class DoglegReference:
    """J of one linearisation point as row groups over one parameter vector [free poses (6 nf) | landmarks present (d each) |
    free shared blocks (nb)] in long double, and the dogleg quantities of Ceres computed from it.

    rows: stereo_rows / phong_observation_rows; unary: unary_rows (or None); mu: the Levenberg-Marquardt regulariser of the
    Gauss-Newton step (SchurSystem at radius 1 / mu).  Unary rows carry fp64 Jacobians (complex step): their rounding enters
    every bar through the magnitude Ja = |J| with c_row."""

    def __init__(self, rows, obs_pose, obs_point, fidx, num_points, mu, unary=None, min_diag=1e-6, max_diag=1e32):
        fidx = np.asarray(fidx, np.int64)
        self.mu, self.min_diag, self.max_diag = mu, min_diag, max_diag
        unary = unary or []
        nf = int((fidx >= 0).sum())
        # unary blocks summed as the SchurSystem takes them; the off-diagonal (relative-pose) blocks are added to S below
        n = 6 * nf
        Hu, gu, Hua = np.zeros((n, n), LD), np.zeros(n, LD), np.zeros((n, n))
        for b in unary:
            for k, J in b["blocks"]:
                if fidx[k] < 0:
                    continue
                a = slice(6 * fidx[k], 6 * fidx[k] + 6)
                gu[a] += J.T @ b["r"]
                for k2, J2 in b["blocks"]:
                    if fidx[k2] >= 0:
                        c = slice(6 * fidx[k2], 6 * fidx[k2] + 6)
                        Hu[a, c] += J.T @ J2
                        Hua[a, c] += np.abs(np.asarray(J, np.float64)).T @ np.abs(np.asarray(J2, np.float64))
        self.sy = sy = SchurSystem(rows, obs_pose, obs_point, fidx, num_points, 1.0 / mu, H_unary=Hu if unary else None,
                                   g_unary=gu if unary else None, Ha_unary=Hua if unary else None)
        self.nf, self.d, self.nb, self.Lp = nf, sy.d, sy.nb, sy.lm.shape[0]
        self.o_l = 6 * nf
        self.o_b = self.o_l + self.d * self.Lp
        self.N = self.o_b + self.nb
        sink = self.N                               # column of constant poses: x[sink] = 0
        f = fidx[np.asarray(obs_pose, np.int64)]
        cp = np.where(f[:, None] >= 0, 6 * f[:, None] + np.arange(6), sink)
        cl = self.o_l + self.d * sy.slot_of_obs[:, None] + np.arange(self.d)
        groups = [dict(r=rows["r"], blocks=[(rows["Jp"], rows["Jpa"], cp), (rows["Jl"], rows["Jla"], cl)])]
        if self.nb:
            cb = np.broadcast_to(self.o_b + np.arange(self.nb), (cl.shape[0], self.nb))
            groups[0]["blocks"].append((rows["Jb"], rows["Jba"], cb))
        for b in unary:
            blk = []
            for k, J in b["blocks"]:
                col = np.full((1, 6), sink) if fidx[k] < 0 else (6 * fidx[k] + np.arange(6))[None]
                blk.append((J[None], np.abs(np.asarray(J, np.float64))[None], col))
            groups.append(dict(r=b["r"][None], blocks=blk))
        self.groups = groups
        self.unary_offdiag = Hu.copy()
        for a in range(nf):
            self.unary_offdiag[6 * a: 6 * a + 6, 6 * a: 6 * a + 6] = 0
        # gradient, diag(J^T J) and their rounding magnitudes, per column
        g, h = np.zeros(self.N + 1, LD), np.zeros(self.N + 1, LD)
        ga, ha, m = np.zeros(self.N + 1), np.zeros(self.N + 1), np.zeros(self.N + 1)
        rab = rows["rabs"]
        for gi, G in enumerate(groups):
            ra = rab if gi == 0 else np.abs(np.asarray(G["r"], np.float64))
            for J, Ja, col in G["blocks"]:
                np.add.at(g, col, np.einsum("nmw,nm->nw", J, G["r"]))
                np.add.at(h, col, np.einsum("nmw,nmw->nw", J, J))
                np.add.at(ga, col, np.einsum("nmw,nm->nw", Ja, ra))
                np.add.at(ha, col, np.einsum("nmw,nmw->nw", Ja, Ja))
                np.add.at(m, col, np.ones(col.shape))
        self.g, self.h, self.ga, self.ha, self.m = g[:-1], h[:-1], ga[:-1], ha[:-1], m[:-1]
        self.s = LD(1) / (LD(1) + np.sqrt(self.h))
        self.D2 = np.clip(self.s * self.s * self.h, LD(min_diag), LD(max_diag))
        self.clamped = (self.s * self.s * self.h < LD(min_diag)) | (self.s * self.s * self.h > LD(max_diag))
        self.grad_ = self.s * self.g / np.sqrt(self.D2)            # gradient_ (D-scaled space)
        self.v = self.s * self.s * self.g / self.D2               # unscaled image of gradient_ / D
        self.t_max = int(np.bincount(sy.slot_of_obs).max()) if sy.slot_of_obs.size else 0

    # ---- vectors
    def split(self, x):
        """(poses free (nf, 6), landmarks present (Lp, d), border (nb)) of a parameter vector."""
        x = np.asarray(x)
        return x[: self.o_l].reshape(-1, 6), x[self.o_l: self.o_b].reshape(-1, self.d), x[self.o_b:]

    def pack(self, xp_free, xl_present, xb=None):
        parts = [np.asarray(xp_free, LD).ravel(), np.asarray(xl_present, LD).ravel()]
        if self.nb:
            parts.append(np.asarray(xb, LD).ravel())
        return np.concatenate(parts)

    def gauss_newton(self, band=None):
        """delta_gn (unscaled, long double) of (J^T J + mu D^2 / s^2) delta = -g, the kappa_2 of the reduced system it came
        from: the long-double SchurSystem at radius 1 / mu and a refined solve -- equivalently, in Ceres' D-scaled space,
        D delta / s solves (J_s^T J_s + mu D^2) y = -J_s^T r."""
        sy = self.sy
        if self.nb:
            A, b = sy.bordered()
            A[: sy.n, : sy.n] += self.unary_offdiag
        else:
            A, b = sy.dense(), sy.rhs
            A = A + self.unary_offdiag
        x, kap = refined_solve(A, b, band)
        xp, xb = x[: sy.n], x[sy.n:]
        xl = sy.back_substitute(xp, xb if self.nb else None)
        return self.pack(xp, xl, xb), kap

    # ---- row-space sums
    def jx(self, x):
        """J x of every row group, row by row (long double)."""
        xe = np.concatenate([np.asarray(x, LD), [LD(0)]])
        return [sum(np.einsum("nmw,nw->nm", J, xe[col]) for J, _, col in G["blocks"]) for G in self.groups]

    def jx_mag(self, x):
        """sum over blocks of Ja |x| per row (the magnitude every term of a one-pass J x sum is bounded by)."""
        xe = np.concatenate([np.abs(np.asarray(x, np.float64)), [0.0]])
        return [sum(np.einsum("nmw,nw->nm", Ja, xe[col]) for _, Ja, col in G["blocks"]) for G in self.groups]

    def c_sum(self):
        """c of the summation bar c u sum |terms| of the device's six sums: t_max observations in one lane (plus the 36 products
        of a 6x6 quadratic form and the unary rows of one pose), two 256-lane tree reductions (8 levels each), the partials
        of the final pass (ceil(parts / 256) per lane), C_TERMS for the rest."""
        parts = (self.Lp + 255) // 256 + (self.nf + 255) // 256 + 1
        return self.t_max + 36 + 16 + (parts + 255) // 256 + C_TERMS

    def row_sums(self, x, y):
        """(x.J^T J.y row by row, its bar) -- the bar (c_sum + 2 c_row) u sum_rows mag(x) mag(y) bounds every term of the
        device's expansion dl^T H dl + 2 dl.(tt - g_l) + |e|^2 and the rounding of J itself (c_row u Ja per entry)."""
        jx, jy = self.jx(x), self.jx(y)
        mx, my = self.jx_mag(x), self.jx_mag(y)
        val = sum((a * b).sum() for a, b in zip(jx, jy))
        mag = sum(float((a * b).sum()) for a, b in zip(mx, my))
        return val, (self.c_sum() + 2 * C_DL_ROW) * U * mag

    def param_sums(self, v, gn):
        """|gradient_|^2, |gn|_D^2 and gradient_ . gn in long double from the device's vectors, with bars: summation
        c_sum u |terms|, and the rounding of g (the row bar (m + C_TERMS) u ga) and of s^2 / D^2 (from diag H: (m + C_TERMS) u
        ha / h relative where unclamped, 8 u where clamped) carried through the formulas."""
        v, gn = np.asarray(v, LD), np.asarray(gn, LD)
        g, s2, D2 = self.g, self.s * self.s, self.D2
        w = s2 / D2
        eg = (self.m + C_TERMS) * U * self.ga
        ew = np.where(self.clamped, 8 * U, (self.m + C_TERMS) * U * self.ha / np.maximum(np.asarray(self.h, np.float64), 1e-300) + 8 * U)
        g64, w64, gn64 = (np.abs(np.asarray(t, np.float64)) for t in (g, w, gn))
        cs = self.c_sum() * U
        a = (w * g * g).sum()
        ea = cs * float((w64 * g64 * g64).sum()) + float((w64 * (2 * g64 * eg + ew * g64 * g64)).sum())
        b = (gn * gn / w).sum()
        eb = cs * float((gn64 * gn64 / w64).sum()) + float((ew * gn64 * gn64 / w64).sum())
        c = (g * gn).sum()
        ec = cs * float((g64 * gn64).sum()) + float((eg * gn64).sum())
        return (a, b, c), (ea, eb, ec)

    def v_bar(self):
        """Entrywise bar of the device's v = s^2 g / D^2: 8 u (its own rounding) plus the rounding of g and of s^2 / D^2."""
        w64 = np.asarray(self.s * self.s / self.D2, np.float64)
        eg = (self.m + C_TERMS) * U * self.ga
        ew = np.where(self.clamped, 8 * U, (self.m + C_TERMS) * U * self.ha / np.maximum(np.asarray(self.h, np.float64), 1e-300) + 8 * U)
        v64 = np.abs(np.asarray(self.v, np.float64))
        return 8 * U * v64 + w64 * eg + ew * v64

    def model_cost_change(self, delta):
        """-delta . g - |J delta|^2 / 2 row by row, and the magnitude |delta| . |g| + sum_rows (Ja |delta|)^2."""
        jd = self.jx(delta)
        val = -(np.asarray(delta, LD) * self.g).sum() - LD(0.5) * sum((a * a).sum() for a in jd)
        mag = float((np.abs(np.asarray(delta, np.float64)) * np.abs(np.asarray(self.g, np.float64))).sum())
        mag += sum(float((a * a).sum()) for a in self.jx_mag(delta))
        return val, mag


# ---- the scalar chain of DoglegStrategy from the six sums (long double)
def dogleg_scalars(sums, radius, dogleg_type):
    """From (|gradient_|^2, |gn|_D^2, gradient_.gn, |Jv|^2, |Jgn|^2, Jv.Jgn): dict with alpha, beta, gamma (delta = beta gn +
    gamma v, unscaled), step_norm (|delta|_D), mcc (from the sums), branch, and for SUBSPACE the model (g, B, basis) and the
    boundary minimiser.  Branches: 'gn' (Gauss-Newton step inside), 'cauchy' (Cauchy point outside), 'dogleg' (TRADITIONAL on
    the dogleg), 'one_dim', 'boundary' (SUBSPACE), 'fallback' (SUBSPACE found no minimum: TRADITIONAL, as Ceres)."""
    A, Bn, C, Jv2, Jg2, Jvg = (LD(x) for x in sums)
    r = LD(radius)
    gnorm, gn_norm = np.sqrt(A), np.sqrt(Bn)
    alpha = A / Jv2
    out = dict(alpha=alpha)

    def finish(beta, gamma, norm, branch):
        out.update(beta=LD(beta), gamma=LD(gamma), step_norm=LD(norm), branch=branch)
        out["mcc"] = -(out["beta"] * C + out["gamma"] * A) - LD(0.5) * (out["beta"] ** 2 * Jg2 + 2 * out["beta"] * out["gamma"] * Jvg
                                                                        + out["gamma"] ** 2 * Jv2)
        return out

    def traditional():
        if gn_norm <= r:
            return finish(1, 0, gn_norm, "gn")
        if alpha * gnorm >= r:
            return finish(0, -r / gnorm, r, "cauchy")
        # |a + t (b - a)| = r with a = -alpha gradient_, b = gn: the positive root of |b - a|^2 t^2 + 2 a.(b - a) t + |a|^2 - r^2
        a2, ab, b2 = alpha * alpha * A, -alpha * C, Bn
        qa, qb, qc = a2 - 2 * ab + b2, 2 * (ab - a2), a2 - r * r
        t = (-qb + np.sqrt(qb * qb - 4 * qa * qc)) / (2 * qa)
        gam, bet = -alpha * (1 - t), t
        return finish(bet, gam, np.sqrt(gam * gam * A + 2 * gam * bet * C + bet * bet * Bn), "dogleg")

    if dogleg_type == 0:
        return traditional()
    # SUBSPACE_DOGLEG: orthonormal basis of span(gradient_, gn), the longer column first (Gram-Schmidt on the 2x2 Gram)
    p_first = A >= Bn
    an2, bn2 = (A, Bn) if p_first else (Bn, A)
    an = np.sqrt(an2)
    proj = C / an
    wn = np.sqrt(max(bn2 - proj * proj, LD(0)))
    ia = 0 if p_first else 1
    e = np.zeros((2, 2), LD)
    e[0, ia] = 1 / an
    one_dim = wn <= 2 * np.finfo(np.float64).eps * an
    out["one_dim"] = bool(one_dim)
    if not one_dim:     # the model is formed at the linearisation point, whatever the radius (ComputeSubspaceModel)
        e[1, ia], e[1, 1 - ia] = -proj / (an * wn), 1 / wn
        G = np.array([[A, C], [C, Bn]], LD)
        JJ = np.array([[Jv2, Jvg], [Jvg, Jg2]], LD)
        sg = e @ G[:, 0]                                   # basis . gradient_
        sB = e @ JJ @ e.T
        out.update(sub_e=e, sub_g=sg, sub_B=sB)
    if gn_norm <= r:
        return finish(1, 0, gn_norm, "gn")
    if one_dim:
        return finish(0, -r / gnorm, r, "one_dim")
    y = boundary_minimum(sg, sB, r)
    if y is None:
        res = traditional()
        res["branch"] = "fallback"
        return res
    out["y"] = y
    gam, bet = y @ e[:, 0], y @ e[:, 1]
    return finish(bet, gam, r, "boundary")


def boundary_minimum(g, B, radius, grid=4096, newton=60):
    """argmin of g.y + y^T B y / 2 over |y| = radius, independent of the quartic Ceres (and the device) solve: a dense grid in
    theta, then Newton on f'(theta) in long double from the best grid point.  None when Newton fails to converge."""
    g, B, r = np.asarray(g, LD), np.asarray(B, LD), LD(radius)

    def f(t):
        c, s = np.cos(t), np.sin(t)
        return r * (g[0] * c + g[1] * s) + LD(0.5) * r * r * (B[0, 0] * c * c + 2 * B[0, 1] * c * s + B[1, 1] * s * s)

    def d1(t):
        c, s = np.cos(t), np.sin(t)
        return r * (-g[0] * s + g[1] * c) + r * r * ((B[1, 1] - B[0, 0]) * c * s + B[0, 1] * (c * c - s * s))

    def d2(t):
        c, s = np.cos(t), np.sin(t)
        return -r * (g[0] * c + g[1] * s) + r * r * ((B[1, 1] - B[0, 0]) * (c * c - s * s) - 4 * B[0, 1] * c * s)

    th = np.arange(grid, dtype=LD) * (2 * LD(np.pi) / grid)
    t = th[int(np.argmin(f(th)))]
    step = LD(1)
    for _ in range(newton):
        h2 = d2(t)
        if not h2 > 0:
            return None
        step = d1(t) / h2
        t = t - step
        if abs(step) <= LD(2.0) ** -60:
            break
    if not abs(step) <= LD(2.0) ** -50:      # (f' is evaluated to ~2^-64 of its terms: the last steps may stall above 2^-60)
        return None
    return np.array([r * np.cos(t), r * np.sin(t)], LD)


def propagate(fun, sums, bars, rel=LD(2.0) ** -30):
    """sum_i |d fun / d sums_i| bars_i by long-double central differences (fun: the sums -> dict of scalars)."""
    base = np.asarray(sums, LD)
    keys = None
    acc = {}
    for i in range(base.shape[0]):
        hstep = max(abs(base[i]) * rel, LD(1e-300))
        up, dn = base.copy(), base.copy()
        up[i] += hstep
        dn[i] -= hstep
        fu, fd = fun(up), fun(dn)
        if keys is None:
            keys = list(fu)
        for k in keys:
            acc[k] = acc.get(k, 0.0) + float(abs((LD(fu[k]) - LD(fd[k])) / (2 * hstep))) * float(bars[i])
    return acc


# ------------------------------------------------------------------------ the second half of a trust-region iteration
# What happens after the step exists, from the Ceres 1.x semantics the kernels cite: the Plus operators of the local
# parameterisations (SE3Perturbation, UnitVectorPerturbation, ParameterBlock::Plus with bounds), the cost 1/2 sum rho(|r|^2),
# the gradient max norm |x - Plus(x, -g)|_inf of TrustRegionMinimizer::EvaluateGradientAndJacobian, and the scalar chain of
# TrustRegionMinimizer / TrustRegionStepEvaluator / LevenbergMarquardtStrategy / DoglegStrategy.
DBL_EPSILON = 2.0 ** -52
C_PLUS = 24               # c of the se3_plus bar (derived in its docstring)
C_UNIT = 16               # c of the unit_plus bar
C_NORM = 8                # c of the step_norm / x_norm bars


def _skew(v):
    K = np.zeros(v.shape[:-1] + (3, 3), dtype=v.dtype)
    K[..., 0, 1], K[..., 0, 2] = -v[..., 2], v[..., 1]
    K[..., 1, 0], K[..., 1, 2] = v[..., 2], -v[..., 0]
    K[..., 2, 0], K[..., 2, 1] = -v[..., 1], v[..., 0]
    return K


def se3_plus(T, eps, dtype=LD):
    """SE3Perturbation: Plus(T, eps) = [E t + eps_t | E R], E = so3 exp(eps_r) = cos(a) I + (1 - cos a) n n^T + sin(a) n^ with
    a = |eps_r|, n = eps_r / a, and the first-order branch E = I + eps_r^ for a <= DBL_EPSILON.  T (..., 12) = [t | R row-major],
    eps (..., 6) = [translation | rotation]; fp64 inputs are held exactly.  Returns (Plus (N, 12), bar (N, 12)).

    The bar c u (M_E |T| + |eps|) bounds an fp64 evaluation entrywise, M_E >= |E| being the sum of the magnitudes of the terms
    of E: (|cos| + a |sin|) I + (|1 - cos| + |cos| + a |sin|) |n n^T| + (|sin| + a |cos|) |n^| -- the a |sin|, a |cos| parts carry
    the rounding of the angle into cos and sin (an absolute error 3 u a of the argument), which dominates for angles far beyond
    pi (the projected gradient of a first iteration); 1 - cos is formed from the rounded cosine, so its error is absolute in
    u |cos|, not relative to 1 - cos (a small step: 1 - cos ~ a^2 / 2, its rounding ~ u).  Relative to those magnitudes an entry of E costs: the angle 3 u (three
    squares, two sums, a square root), each n_i 4 u, cos / sin 2 u, 1 - cos 1 u, two products 2 u and the sum of the terms
    2 u: 17 u with two n_i in one term.  Each output entry is a 3-term dot product plus eps_t: 4 u more, on M_E |T| + |eps|.
    c = 24 leaves 3 u for the second-order terms.  (First-order branch: E is exact and only the 4 u remain.)"""
    T = np.asarray(T, dtype).reshape(-1, 12)
    eps = np.asarray(eps, dtype).reshape(-1, 6)
    n = T.shape[0]
    phi = eps[:, 3:]
    ang = np.sqrt((phi * phi).sum(1))
    small = ang <= dtype(DBL_EPSILON)
    safe = np.where(small, dtype(1), ang)
    a = phi / safe[:, None]
    c, s = np.cos(safe), np.sin(safe)
    I = np.broadcast_to(np.eye(3, dtype=dtype), (n, 3, 3))
    aa = a[:, :, None] * a[:, None, :]
    E = np.where(small[:, None, None], I + _skew(phi), c[:, None, None] * I + (1 - c)[:, None, None] * aa + s[:, None, None] * _skew(a))
    f = lambda v: np.abs(np.asarray(v, np.float64))
    a64, c64, s64 = f(safe), f(c), f(s)
    ME = np.where(np.asarray(small)[:, None, None], f(I + _skew(phi)),
                  (c64 + a64 * s64)[:, None, None] * f(I) + (f(1 - c) + c64 + a64 * s64)[:, None, None] * f(aa)
                  + (s64 + a64 * c64)[:, None, None] * f(_skew(a)))
    t, R = T[:, :3], T[:, 3:].reshape(n, 3, 3)
    out = np.concatenate([np.einsum("nij,nj->ni", E, t) + eps[:, :3], np.einsum("nij,njk->nik", E, R).reshape(n, 9)], 1)
    bar = C_PLUS * U * np.concatenate([np.einsum("nij,nj->ni", ME, f(t)) + f(eps[:, :3]),
                                       np.einsum("nij,njk->nik", ME, f(R)).reshape(n, 9)], 1)
    return out, bar


def se3_minus(T_new, T, dtype=LD):
    """The inverse of se3_plus: eps with Plus(T, eps) = T_new.  E = R_new R^T, eps_r = so3 log(E) = a v / |v| with
    v = vee(E - E^T) / 2 = sin(a) n and a = atan2(|v|, (tr E - 1) / 2) (accurate for small angles, where acos(cos a) loses half
    the digits, and up to pi; for a <= DBL_EPSILON it returns v, the first-order branch of se3_plus, to 1e-32 relative),
    eps_t = t_new - E t.  T_new, T (..., 12) = [t | R row-major].  Returns (eps (N, 6) = [translation | rotation], bar (N, 6)).

    The bar is for T_new an fp64 evaluation of Plus(T, eps): its entrywise se3_plus bar b = (b_t, b_R) carried through the log
    to first order.  dE = dR_new R^T, so |dE| <= b_R |R|^T entrywise, plus |E| |R R^T - I|: an fp64 R is orthonormal only to
    rounding and E inherits the defect.  d eps_r = J_l^-1(eps_r) vee(skew(dE E^T)): |vee(skew M)|_2 <= |M|_F / sqrt 2, and the
    largest singular value of J_l^-1 is (a / 2) / sin(a / 2) (1 at a = 0, 1.043 at a = 1, pi / 2 at pi), so every entry of eps_r
    is within (a / 2) / sin(a / 2) |dE|_F / sqrt 2.  d eps_t = d t_new - dE t: b_t + |dE| |t|."""
    T_new = np.asarray(T_new, dtype).reshape(-1, 12)
    T = np.asarray(T, dtype).reshape(-1, 12)
    n = T.shape[0]
    t, R = T[:, :3], T[:, 3:].reshape(n, 3, 3)
    E = np.einsum("nij,nkj->nik", T_new[:, 3:].reshape(n, 3, 3), R)
    v = np.stack([E[:, 2, 1] - E[:, 1, 2], E[:, 0, 2] - E[:, 2, 0], E[:, 1, 0] - E[:, 0, 1]], 1) / 2
    vn = np.sqrt((v * v).sum(1))
    ang = np.arctan2(vn, (E[:, 0, 0] + E[:, 1, 1] + E[:, 2, 2] - 1) / 2)
    eps_r = v * np.where(vn > 0, ang / np.where(vn > 0, vn, dtype(1)), dtype(1))[:, None]
    eps = np.concatenate([T_new[:, :3] - np.einsum("nij,nj->ni", E, t), eps_r], 1)
    f = lambda x: np.abs(np.asarray(x, np.float64))
    b = se3_plus(T, eps, dtype)[1]
    defect = f(np.einsum("nij,nkj->nik", R, R) - np.eye(3, dtype=dtype))
    dE = np.einsum("nij,nkj->nik", b[:, 3:].reshape(n, 3, 3), f(R)) + np.einsum("nij,njk->nik", f(E), defect)
    a64 = np.asarray(ang, np.float64)
    k = np.where(a64 > 1e-8, 0.5 * a64 / np.sin(0.5 * np.maximum(a64, 1e-8)), 1.0)
    bar_r = k * np.sqrt((dE * dE).sum((1, 2)) / 2)
    bar = np.concatenate([b[:, :3] + np.einsum("nij,nj->ni", dE, f(t)), np.repeat(bar_r[:, None], 3, 1)], 1)
    return eps, bar


def unit_plus(x, d, dtype=LD):
    """UnitVectorPerturbation: Plus(x, d) = y / |y|, y = x + d - (d.x / x.x) x.  x, d (..., 3).  Returns (Plus, bar), (N, 3).

    The bar on an fp64 evaluation: y sums three terms of magnitude m = |x| + |d| + s_m |x| with s_m = (|d|.|x|) / (x.x) the
    magnitude sum of the quotient; the two dot products cost 3 u each, the quotient 1 u, s x 1 u, the two sums 2 u: 10 u m on
    y.  The normalisation carries an error of y into every component (through |y|): |d out| <= |d y|_2 / |y|, plus 3 u |out| for
    |y| (1.5 u) and the quotient.  c = 16 leaves 6 u m for second-order terms."""
    x = np.asarray(x, dtype).reshape(-1, 3)
    d = np.asarray(d, dtype).reshape(-1, 3)
    s = (d * x).sum(1) / (x * x).sum(1)
    y = x + d - s[:, None] * x
    nrm = np.sqrt((y * y).sum(1))
    out = y / nrm[:, None]
    f = lambda v: np.abs(np.asarray(v, np.float64))
    sm = (f(d) * f(x)).sum(1) / f((x * x).sum(1))
    m = f(x) + f(d) + sm[:, None] * f(x)
    bar = C_UNIT * U * (np.sqrt((m * m).sum(1)) / f(nrm))[:, None] + 3 * U * f(out)
    return out, np.broadcast_to(bar, out.shape).copy()


def projected_plus(light_type, light, phong, texture, db, shared_free, bounds=None, dtype=LD):
    """ParameterBlock::Plus of the shared blocks with the border step db in the order light 3, Phong 3M, textures M (the free
    ones only, shared_free bit 0 / 1 / 2): the sum, UnitVectorPerturbation for a directional light (light_type 1), then the
    projection onto the box [lo, hi] -- bounds = (lo (4), hi (4)) for ka, ks, alpha, kd, or None.  Returns the new
    (light, phong, texture) and their bars: u |x + d| for the sum (nothing where the projection fires on both sides of the
    rounding: the bound itself is returned; u |x + d| is kept there as well, for a sum within rounding of the bound)."""
    light = np.asarray(light, dtype).reshape(3)
    phong = np.asarray(phong, dtype).reshape(-1, 3)
    texture = np.asarray(texture, dtype).reshape(-1)
    db = np.asarray(db, dtype).ravel()
    M = texture.shape[0]
    o = 0
    f = lambda v: np.abs(np.asarray(v, np.float64))
    nl, bl = light.copy(), np.zeros(3)
    if shared_free & 1:
        if light_type == 1:
            nl, bl = unit_plus(light, db[:3], dtype)
            nl, bl = nl[0], bl[0]
        else:
            nl = light + db[:3]
            bl = U * f(nl)
        o = 3
    nph, bph = phong.copy(), np.zeros(phong.shape)
    if shared_free & 2:
        nph = phong + db[o: o + 3 * M].reshape(M, 3)
        bph = U * f(nph)
        if bounds is not None:
            nph = np.minimum(np.maximum(nph, np.asarray(bounds[0], dtype)[:3]), np.asarray(bounds[1], dtype)[:3])
        o += 3 * M
    ntx, btx = texture.copy(), np.zeros(M)
    if shared_free & 4:
        ntx = texture + db[o: o + M]
        btx = U * f(ntx)
        if bounds is not None:
            ntx = np.minimum(np.maximum(ntx, dtype(bounds[0][3])), dtype(bounds[1][3]))
    return (nl, nph, ntx), (bl, bph, btx)


def _unary_magnitudes(poses, factors):
    """Rounding magnitude of every pose-only residual block (fp64): |r| + 2 sum over its poses of |d r / d T| |T|, the ambient
    Jacobian by complex step -- log(T_ref T_1 T_2^-1) and t_ref - R_res t cancel where the poses are far from the origin, and
    the reference pose in the data is as large as the poses (the factor 2).  Huber-corrected like unary_rows."""
    import np_reference as npr
    out = []
    h = 1e-30
    for fct in factors:
        S = np.asarray(fct["stiffness"], np.float64)
        d = np.asarray(fct["data"], np.float64)
        if fct["type"] == 0:
            funs = [(fct["pose"], lambda X: npr.pose_prior_residual(X, d[:12], S.reshape(6, 6)))]
        elif fct["type"] == 1:
            funs = [(fct["pose"], lambda X: npr.sun_sensor_residual(X, d[:3], d[3:6], S.reshape(2, 2), d[6], d[7]))]
        else:
            T1, T2 = poses[fct["pose"]].astype(complex), poses[fct["pose2"]].astype(complex)
            funs = [(fct["pose"], lambda X: _rel_residual(X, T2, d[:12], S.reshape(6, 6))),
                    (fct["pose2"], lambda X: _rel_residual(T1, X, d[:12], S.reshape(6, 6)))]
        r = np.asarray(funs[0][1](poses[funs[0][0]].astype(complex)).real, np.float64)
        mag = np.abs(r)
        for k, fun in funs:
            for c in range(12):
                X = poses[k].astype(complex)
                X[c] += 1j * h
                mag = mag + 2 * np.abs(np.asarray(fun(X)).imag / h) * abs(poses[k][c])
        w = float(huber_weight(np.float64((r * r).sum()), fct.get("huber", 0.0), np.float64))
        out.append(mag * w)
    return out


def cost_at(cam, poses, points, obs_pose, obs_point, obs_uvd, stiffness, huber_a=0.0, factors=None, lighting=None,
            normals=None, jacobians=True, rows=None):
    """1/2 sum rho(|r|^2) over all residual blocks at (poses, points[, normals, the shared blocks in `lighting`]) in long
    double: the stereo blocks with the Huber loss (stereo_rows), the intensity and normal blocks (phong_observation_rows; a
    NULL loss), the unary and relative pose blocks (unary_rows: fp64 values, each with its own Huber loss).  Returns a dict:
    cost, bar, rows (the stereo / lighting rows, for reuse; jacobians=False: stereo residuals and magnitudes only), n_terms.
    rows: the rows of this very point when the caller has them already (stereo_rows / phong_observation_rows).

    The bar on an fp64 evaluation, in any summation order, has two parts.
    (1) The rounding of each term.  A row value r carries c u rabs (rabs of stereo_rows: pred - z cancels; the C_ROW magnitudes
        of phong_rows; _unary_magnitudes), c = 16 = C_TERMS = C_ROW, and d (1/2 rho(|r|^2)) = rho' r . dr = (w r) . (w dr): the
        corrected rows and magnitudes as they are returned.  Twice that for the pose blocks, whose reference values are fp64.
        The term's own arithmetic (squares, 2 a sqrt(s) - a^2 <= 3 times the term's sum of magnitudes) is part of (2).
    (2) The summation: (N + C_TERMS) u sum |term| over the N residual blocks bounds any order of adding them (the lane, block and
        partial-sum trees of the device), C_TERMS covering the term's own arithmetic."""
    if lighting is not None:
        lt = dict(lighting)
        nrm = lt["normals"] if normals is None else normals
        if rows is None:
            rows = phong_observation_rows(cam, poses, points, nrm, obs_pose, obs_point, obs_uvd, stiffness, lt, huber_a, 0)
        N = rows["r"].shape[0]
        st_cost = rows["cost"] - LD(0.5) * (rows["r"][:, 3:] ** 2).sum()
        terms = [np.asarray(LD(0.5) * (rows["r"][:, 3] ** 2), LD), np.asarray(LD(0.5) * (rows["r"][:, 4:] ** 2).sum(1), LD)]
        n_terms = 3 * N
    else:
        if rows is None:
            rows = stereo_rows(cam, poses, points, obs_pose, obs_point, obs_uvd, stiffness, huber_a, jacobians=jacobians)
        N = rows["r"].shape[0]
        st_cost = rows["cost"]
        terms = []
        n_terms = N
    cost = LD(0) + rows["cost"]
    r64 = np.abs(np.asarray(rows["r"], np.float64))
    part1 = C_TERMS * U * float((r64 * rows["rabs"]).sum())
    mag = abs(float(st_cost)) + sum(float(t.sum()) for t in terms)
    if factors:
        un = unary_rows(np.asarray(poses, np.float64), factors)
        um = _unary_magnitudes(np.asarray(poses, np.float64), factors)
        for fct, b, m in zip(factors, un, um):
            sw = (b["r"] * b["r"]).sum()
            a = LD(fct.get("huber", 0.0))
            rho = 2 * sw - a * a if (a > 0 and sw > a * a) else sw
            cost = cost + LD(0.5) * rho
            mag += 0.5 * abs(float(rho))
            part1 += 2 * C_TERMS * U * float((np.abs(np.asarray(b["r"], np.float64)) * m).sum())
        n_terms += len(factors)
    return dict(cost=cost, bar=part1 + (n_terms + C_TERMS) * U * mag, rows=rows, n_terms=n_terms, part1=part1)


def gradient_max_norm(ref, fidx, poses, normals=None, shared=None):
    """max over the free blocks of |x - Plus(x, -g)|_inf [TrustRegionMinimizer::EvaluateGradientAndJacobian] from the
    long-double gradient of a DoglegReference at this point: SE3 Plus on the free poses, the plain |g_l|_inf on the landmark
    positions, UnitVectorPerturbation on the normals (6-wide landmark blocks), the projected Plus on the free shared blocks
    (shared = dict(light_type, light, phong, texture, shared_free, bounds)).  Returns (value, bar).

    The bar: the fp64 gradient carries (m + C_TERMS) u sum |J|^T |r| per entry (m rows in the column: ref.m, ref.ga).  Through
    Plus: a rotation changes by at most |d g_r|_2 per radian in every entry, so an entry of E v moves by at most |d g_r|_2
    |v|_2, the translation by |d g_t|; plus the bar of Plus itself at eps = -g.  The subtraction T - Plus(T, -g) is exact for
    nearby values and otherwise rounds to u |T - Plus|: it is absolute in u |T| through the Plus bar, not relative to the
    difference.  A maximum moves by no more than its largest entry bar."""
    fidx = np.asarray(fidx, np.int64)
    free = np.flatnonzero(fidx >= 0)
    gp, gl, gb = ref.split(ref.g)
    eg = (ref.m + C_TERMS) * U * ref.ga
    egp, egl, egb = ref.split(eg)
    best, bar = LD(0), 0.0
    if free.size:
        T = np.asarray(poses, LD)[free]
        Tn, pb = se3_plus(T, -gp)
        diff = np.abs(T - Tn)
        T64 = np.abs(np.asarray(T, np.float64))
        dr = np.sqrt((egp[:, 3:] ** 2).sum(1))
        vn = np.stack([np.sqrt((T64[:, :3] ** 2).sum(1))] * 3 + [np.sqrt((T64[:, 3:].reshape(-1, 3, 3) ** 2).sum(1))[:, c % 3]
                                                                 for c in range(9)], 1)
        eb = dr[:, None] * vn + pb + U * np.asarray(diff, np.float64)
        eb[:, :3] += egp[:, :3]
        best, bar = max(best, diff.max()), max(bar, float(eb.max()))
    if gl.size:
        best, bar = max(best, np.abs(gl[:, :3]).max()), max(bar, float(egl[:, :3].max()))
        if ref.d == 6:
            x = np.asarray(normals, LD)[ref.sy.lm]
            xn, ub = unit_plus(x, -gl[:, 3:])
            diff = np.abs(x - xn)
            # |d Plus / d delta| <= 1 / |y| in the 2-norm
            y = x - gl[:, 3:] + (((gl[:, 3:] * x).sum(1) / (x * x).sum(1))[:, None]) * x
            e2 = np.sqrt((egl[:, 3:] ** 2).sum(1)) / np.asarray(np.sqrt((y * y).sum(1)), np.float64)
            best, bar = max(best, diff.max()), max(bar, float((ub + e2[:, None] + U * np.abs(np.asarray(x, np.float64))).max()))
    if ref.nb:
        sh = shared
        neg = -gb
        (nl, nph, ntx), (bl, bph, btx) = projected_plus(sh["light_type"], sh["light"], sh["phong"], sh["texture"], neg,
                                                        sh["shared_free"], sh.get("bounds"))
        o = 0
        for on, old, new, b0, width in ((1, np.asarray(sh["light"], LD).reshape(3), nl, bl, 3),
                                        (2, np.asarray(sh["phong"], LD).ravel(), nph.ravel(), bph.ravel(), 3 * len(sh["texture"])),
                                        (4, np.asarray(sh["texture"], LD).ravel(), ntx.ravel(), btx.ravel(), len(sh["texture"]))):
            if not sh["shared_free"] & on:
                continue
            e = egb[o: o + width]
            if on == 1 and sh["light_type"] == 1:
                e = np.full(3, np.sqrt((e ** 2).sum()))      # |y| >= |x| = 1 for a unit light moved in its tangent plane
            diff = np.abs(old - new)
            best = max(best, diff.max())
            bar = max(bar, float((e + np.ravel(b0) + U * np.abs(np.asarray(old, np.float64))).max()))
            o += width
    return best, bar


def block_norms(fidx, present, x_poses, x_points, c_poses=None, c_points=None, x_normals=None, c_normals=None, x_shared=None,
                c_shared=None):
    """|x|_2 (candidate None) or |candidate - x|_2 over the blocks of the reduced program, as TrustRegionMinimizer takes them:
    12 ambient entries per free pose, 3 per landmark that has an observation (`present`), 3 per normal of such a landmark,
    the free shared blocks (x_shared: the concatenated free entries); no constant or unobserved block.  Returns (norm, bar).

    The bar: every difference (or entry) of the fp64 side carries an absolute error e_i (the candidate's own rounding, u |x_i|
    at least, passed in by the caller through the Plus bars; here u |x_i| per entry for the subtraction and the square), and
    d |v|_2 <= |e|_2 -- absolute in u |x|, which is what decides near convergence where |v| ~ 1e-6 and |x| ~ 100 -- plus the
    summation (n + C_NORM) u |v|_2 / 2 of the n squares in any order and the square root."""
    free = np.flatnonzero(np.asarray(fidx) >= 0)
    xs = [np.asarray(x_poses, LD)[free].ravel(), np.asarray(x_points, LD)[present].ravel()]
    cs = None if c_poses is None else [np.asarray(c_poses, LD)[free].ravel(), np.asarray(c_points, LD)[present].ravel()]
    if x_normals is not None:
        xs.append(np.asarray(x_normals, LD)[present].ravel())
        if cs is not None:
            cs.append(np.asarray(c_normals, LD)[present].ravel())
    if x_shared is not None:
        xs.append(np.asarray(x_shared, LD).ravel())
        if cs is not None:
            cs.append(np.asarray(c_shared, LD).ravel())
    x = np.concatenate(xs)
    v = x if cs is None else np.concatenate(cs) - x
    nrm = np.sqrt((v * v).sum())
    e = U * np.abs(np.asarray(x, np.float64)) * (0.0 if cs is None else 1.0)
    return nrm, float(np.sqrt((e * e).sum())) + (0.5 * v.size + C_NORM) * U * float(nrm)


# ---- the scalar chain
def trust_region_options(**kw):
    """Ceres 1.x Solver::Options defaults of the fields the chain reads (strategy 0 LM / 1 DOGLEG)."""
    o = dict(max_num_iterations=50, use_nonmonotonic_steps=0, max_consecutive_nonmonotonic_steps=5,
             max_num_consecutive_invalid_steps=5, max_trust_region_radius=1e16, min_trust_region_radius=1e-32,
             min_relative_decrease=1e-3, function_tolerance=1e-6, gradient_tolerance=1e-10, parameter_tolerance=1e-8,
             trust_region_strategy_type=0)
    for k in kw:
        assert k in o, k
    o.update(kw)
    return o


def trust_region_state(x_cost, radius, options):
    """The state after IterationZero: the strategy (radius, decrease_factor 2, mu 1e-8, reuse) and the step evaluator."""
    c = LD(x_cost)
    return dict(radius=LD(radius), decrease_factor=LD(2), mu=LD(1e-8), reuse=0, num_invalid=0,
                se_minimum=c, se_current=c, se_reference=c, se_candidate=c, se_acc_ref=LD(0), se_acc_cand=LD(0),
                se_num_nonmono=0,
                se_max_nonmono=options["max_consecutive_nonmonotonic_steps"] if options["use_nonmonotonic_steps"] else 0)


def can_continue(iteration, gmax, radius, options):
    """FinalizeIterationAndCheckIfMinimizerCanContinue: None, or the termination ("no_convergence", "gradient", "radius")."""
    if iteration >= options["max_num_iterations"]:
        return "no_convergence"
    if gmax <= options["gradient_tolerance"]:
        return "gradient"
    if radius <= options["min_trust_region_radius"]:
        return "radius"
    return None


def _step_quality(v, st):
    x_cost, cand, mcc = v[0], v[1], v[2]
    # the evaluator's current cost is the x_cost of a monotonic history; it is carried as an offset of x_cost so that the bar
    # of x_cost propagates into it
    cur = st["se_current"] + (x_cost - st["_x_cost0"])
    rd0 = (cur - cand) / mcc
    rd1 = (st["se_reference"] + (x_cost - st["_x_cost0"]) * st["_ref_is_x"] - cand) / (st["se_acc_ref"] + mcc)
    return rd0, rd1


def trust_region_decision(x_cost, candidate_cost, mcc, step_norm, x_norm, state, options, dl_norm=None, step_valid=True,
                          bars=None):
    """One pass of the trust-region loop after the candidate evaluation, in long double:

        step validity [ComputeTrustRegionStep: the linear solver failed or model_cost_change <= 0 -> HandleInvalidStep],
        ParameterToleranceReached  step_norm <= parameter_tolerance (x_norm + parameter_tolerance),
        FunctionToleranceReached   |x_cost - candidate_cost| <= function_tolerance x_cost,
        TrustRegionStepEvaluator::StepQuality  rho = max(rho_0, rho_1), rho_0 = (current - candidate) / mcc,
                                   rho_1 = (reference - candidate) / (accumulated_reference_model_cost_change + mcc),
        rho > min_relative_decrease -> HandleSuccessfulStep, else HandleUnsuccessfulStep,
        LevenbergMarquardtStrategy: accepted radius / max(1/3, 1 - (2 rho - 1)^3) capped by max_trust_region_radius and
                                   decrease_factor = 2; rejected or invalid radius / decrease_factor, decrease_factor * 2,
        DoglegStrategy:            accepted rho < 0.25 radius / 2, rho > 0.75 max(radius, 3 |delta|_D) (dl_norm), mu = max(1e-8,
                                   2 mu / 10); rejected radius / 2 and the step is reused; invalid mu * 10,
        TrustRegionStepEvaluator::StepAccepted (the non-monotonic bookkeeping).

    state: trust_region_state or the "state" of an earlier call (not modified).  bars: dict of the fp64 bars of x_cost,
    candidate_cost, mcc, step_norm, x_norm (default 0).  Returns a dict: valid, termination (None / "parameter" / "function"
    / "failure"), cost_change, rho, rho0, rho1, accepted, radius (the new one), state (the new one), rho_bar and radius_bar
    (the bars propagated by central differences, hp.propagate), and margins: for every comparison made, the distance of its
    left-hand side from the threshold divided by the propagated bar of that distance (inf for a zero bar) -- a comparison
    with margin <= 1 could go either way in fp64."""
    o = options
    b = dict(x_cost=0.0, candidate_cost=0.0, mcc=0.0, step_norm=0.0, x_norm=0.0)
    b.update(bars or {})
    st = dict(state)
    dog = o["trust_region_strategy_type"] == 1
    x_cost, cand, mcc, sn, xn = (LD(v) for v in (x_cost, candidate_cost, mcc, step_norm, x_norm))
    margins = {}
    ratio = lambda dist, bar: float("inf") if bar == 0 else abs(float(dist)) / bar
    out = dict(margins=margins, termination=None, accepted=False, rho=None, cost_change=None)
    margins["valid"] = ratio(mcc, b["mcc"])
    out["valid"] = bool(step_valid and mcc > 0)
    if not out["valid"]:
        st["num_invalid"] += 1
        if st["num_invalid"] >= o["max_num_consecutive_invalid_steps"]:
            out["termination"] = "failure"
        if dog:
            st["mu"], st["reuse"] = st["mu"] * 10, 0
        else:
            st["radius"], st["decrease_factor"] = st["radius"] / st["decrease_factor"], st["decrease_factor"] * 2
        out.update(radius=st["radius"], state=st, radius_bar=0.0, rho_bar=0.0)
        return out
    st["num_invalid"] = 0
    out["cost_change"] = x_cost - cand
    pt, ft = LD(o["parameter_tolerance"]), LD(o["function_tolerance"])
    margins["parameter"] = ratio(sn - pt * (xn + pt), b["step_norm"] + float(pt) * b["x_norm"])
    if sn <= pt * (xn + pt):
        out.update(termination="parameter", radius=st["radius"], state=st, radius_bar=0.0, rho_bar=0.0)
        return out
    margins["function"] = ratio(abs(x_cost - cand) - ft * x_cost, b["x_cost"] * (1 + float(ft)) + b["candidate_cost"])
    if abs(x_cost - cand) <= ft * x_cost:
        out.update(termination="function", radius=st["radius"], state=st, radius_bar=0.0, rho_bar=0.0)
        return out
    # step quality: the evaluator's current / reference costs follow x_cost where they are the same number
    q = dict(st, _x_cost0=x_cost, _ref_is_x=1 if st["se_reference"] == st["se_current"] else 0)
    rd0, rd1 = _step_quality([x_cost, cand, mcc], q)
    rho = max(rd0, rd1)
    out.update(rho=rho, rho0=rd0, rho1=rd1)

    def radius_after(rho_, radius):
        if dog:
            r = radius
            if rho_ < 0.25:
                r = r * LD(0.5)
            if rho_ > 0.75:
                r = max(r, 3 * LD(dl_norm))
            return r
        return min(LD(o["max_trust_region_radius"]), radius / max(LD(1) / 3, 1 - (2 * rho_ - 1) ** 3))

    vals, vbars = [x_cost, cand, mcc], [b["x_cost"], b["candidate_cost"], b["mcc"]]
    prop = propagate(lambda v: dict(rho=max(_step_quality(v, q)), radius=radius_after(max(_step_quality(v, q)), st["radius"])),
                     vals, vbars)
    out["rho_bar"] = prop["rho"]
    mrd = LD(o["min_relative_decrease"])
    margins["accept"] = ratio(rho - mrd, prop["rho"])
    if rho > mrd:
        out["accepted"] = True
        if dog:
            margins["rho_0.25"], margins["rho_0.75"] = ratio(rho - LD(0.25), prop["rho"]), ratio(rho - LD(0.75), prop["rho"])
            out["radius_bar"] = 0.0
            st["mu"], st["reuse"] = max(LD(1e-8), 2 * st["mu"] / 10), 0
        else:
            out["radius_bar"] = prop["radius"] + 8 * U * float(radius_after(rho, st["radius"]))
            st["decrease_factor"] = LD(2)
        st["radius"] = radius_after(rho, st["radius"])
        # TrustRegionStepEvaluator::StepAccepted
        st["se_current"] = cand
        st["se_acc_cand"] = st["se_acc_cand"] + mcc
        st["se_acc_ref"] = st["se_acc_ref"] + mcc
        if st["se_current"] < st["se_minimum"]:
            st["se_minimum"], st["se_num_nonmono"] = st["se_current"], 0
            st["se_candidate"], st["se_acc_cand"] = st["se_current"], LD(0)
        else:
            st["se_num_nonmono"] += 1
            if st["se_current"] > st["se_candidate"]:
                st["se_candidate"], st["se_acc_cand"] = st["se_current"], LD(0)
        if st["se_num_nonmono"] == st["se_max_nonmono"]:
            st["se_reference"], st["se_acc_ref"] = st["se_candidate"], st["se_acc_cand"]
    else:
        out["radius_bar"] = 0.0
        if dog:
            st["radius"], st["reuse"] = st["radius"] * LD(0.5), 1
        else:
            st["radius"], st["decrease_factor"] = st["radius"] / st["decrease_factor"], st["decrease_factor"] * 2
    out.update(radius=st["radius"], state=st)
    return out


# ------------------------------------------------------------------------------------------- the projected line search
# [Ceres 1.x TrustRegionMinimizer::DoLineSearch -> ArmijoLineSearch::DoSearch, polynomial.cc] phi(a) = cost(Plus(x, a delta)),
# phi'(a) = delta . gradient(Plus(x, a delta)): the gradient J^T r of the rows AT the trial point, in the tangent space of the
# trial point (the plus-Jacobians of SE3Perturbation / UnitVectorPerturbation are inside the rows' J), against the UNSCALED
# delta with every entry in full -- also the entries whose trial value the projection put on a bound (LineSearchFunction
# knows nothing of the projection).
class RowGradient:
    """g = J^T r, its rounding magnitude ga = |J|^T |r| (from the rows' magnitudes) and the row count m per column, over the
    parameter vector of DoglegReference -- [free poses (6 nf) | landmarks present (d each, index order) | free shared blocks
    (nb)] -- straight from the rows (stereo_rows / phong_observation_rows): no Schur system is formed, so it scales to
    thousands of poses."""

    def __init__(self, rows, obs_pose, obs_point, fidx):
        fidx = np.asarray(fidx, np.int64)
        k, j = np.asarray(obs_pose, np.int64), np.asarray(obs_point, np.int64)
        self.lm = np.unique(j)
        slot = np.searchsorted(self.lm, j)
        self.nf, self.d, self.Lp = int((fidx >= 0).sum()), rows["Jl"].shape[2], self.lm.shape[0]
        self.nb = rows["Jb"].shape[2] if "Jb" in rows else 0
        self.o_l = 6 * self.nf
        self.o_b = self.o_l + self.d * self.Lp
        self.N = self.o_b + self.nb
        f = fidx[k]
        cp = np.where(f[:, None] >= 0, 6 * f[:, None] + np.arange(6), self.N)        # constant poses: the sink column N
        cl = self.o_l + self.d * slot[:, None] + np.arange(self.d)
        self.blocks = [(rows["Jp"], rows["Jpa"], cp), (rows["Jl"], rows["Jla"], cl)]
        if self.nb:
            self.blocks.append((rows["Jb"], rows["Jba"], np.broadcast_to(self.o_b + np.arange(self.nb), (cl.shape[0], self.nb))))
        self.r, self.rabs = rows["r"], rows["rabs"]
        self.r64 = np.abs(np.asarray(self.r, np.float64))
        g, ga, m = np.zeros(self.N + 1, LD), np.zeros(self.N + 1), np.zeros(self.N + 1)
        for J, Ja, col in self.blocks:
            np.add.at(g, col, np.einsum("nmw,nm->nw", J, self.r))
            np.add.at(ga, col, np.einsum("nmw,nm->nw", Ja, self.rabs))
            np.add.at(m, col, np.full(col.shape, float(self.r.shape[1])))
        self.g, self.ga, self.m = g[:-1], ga[:-1], m[:-1]
        self.t_max = int(np.bincount(slot).max()) if slot.size else 0

    def jx(self, x):
        xe = np.concatenate([np.asarray(x, LD), [LD(0)]])
        return sum(np.einsum("nmw,nw->nm", J, xe[col]) for J, _, col in self.blocks)

    def jx_mag(self, x):
        xe = np.concatenate([np.abs(np.asarray(x, np.float64)), [0.0]])
        return sum(np.einsum("nmw,nw->nm", Ja, xe[col]) for _, Ja, col in self.blocks)

    def g_bar(self):
        """Entrywise bar of an fp64 gradient: (m + C_TERMS) u |J|^T |r| (m rows summed into the entry, in any order)."""
        return (self.m + C_TERMS) * U * self.ga

    def directional(self, delta):
        """phi' = delta . g = sum_rows r (J delta) and the bars of its two fp64 evaluations.

        Row pass (k_ph_ls_probe: sum over the rows of r times the row's J delta): every term r_i J_ic delta_c is bounded by
        T = |delta|^T |J|^T |r|.  One lane adds the 7 rows of its landmark's t_max observations in sequence, each row's dot
        product has at most 19 terms (6 pose + 6 landmark + 7 border entries), two 256-lane trees (8 levels each) and
        the final pass over the work-group partials (one per 256 landmarks, 1 024 lanes) follow: m = 7 t_max + 19 + 16 +
        ceil(parts / 1024), and (m + C_TERMS) u T bounds summation and products.  The rounding of r and J themselves
        (C_ROW u of the rows' magnitudes rabs, Ja) is carried through |J delta|: C_ROW u (rabs . |J delta| + |r| . Ja |delta|).

        Column pass (g . delta from the gradient of the linearisation, ls_out[5]): the gradient's own bar carried through
        |delta|, plus (n + C_TERMS) u sum |g| |delta| for the dot product over the n parameters in any order."""
        d = np.asarray(delta, LD)
        d64 = np.abs(np.asarray(delta, np.float64))
        jd = self.jx(d)
        val = (self.r * jd).sum()
        T = float((self.r64 * self.jx_mag(d64)).sum())
        parts = (self.Lp + 255) // 256
        m_row = 7 * self.t_max + 19 + 16 + (parts + 1023) // 1024
        row_bar = (m_row + C_TERMS) * U * T + C_ROW * U * float((self.rabs * np.abs(np.asarray(jd, np.float64))).sum() + T)
        g64 = np.abs(np.asarray(self.g, np.float64))
        col_bar = float((self.g_bar() * d64).sum()) + (self.N + C_TERMS) * U * float((g64 * d64).sum())
        return dict(value=val, row_bar=row_bar, col_bar=col_bar, via_g=(self.g * d).sum(), T=T, m_row=m_row)


def line_search_function(problem, x, ref, delta, alpha, trial=None):
    """phi*(alpha) and phi'*(alpha) of the projected line search from x along delta (a vector over ref's parameters), in long
    double.  problem: an object with rows(x) -> the rows at x, cost(x, rows=) -> cost_at dict and plus(x, ref, delta) -> (point,
    bars), with obs = (obs_pose, obs_point, ...) and fidx (the Spec of the GPU tests); ref: a DoglegReference / RowGradient at x (only
    its split of the parameter vector is used).  trial: the trial point to evaluate at -- an fp64 side's own Plus(x, alpha
    delta) -- or None for the long-double Plus.  phi* carries the cost bar of cost_at; phi'* the bars of RowGradient.directional.
    Returns a dict: alpha, trial, phi, phi_bar, dphi, dphi_bar (row pass), dphi_col_bar (column pass), grad (the RowGradient)."""
    if trial is None:
        trial = problem.plus(x, ref, LD(alpha) * np.asarray(delta, LD))[0]
    rows = problem.rows(trial)
    c = problem.cost(trial, rows=rows)
    grad = RowGradient(rows, problem.obs[0], problem.obs[1], problem.fidx)
    assert grad.N == np.asarray(delta).shape[0], (grad.N, np.asarray(delta).shape)
    dd = grad.directional(delta)
    return dict(alpha=alpha, trial=trial, phi=c["cost"], phi_bar=c["bar"], dphi=dd["value"], dphi_bar=dd["row_bar"],
                dphi_col_bar=dd["col_bar"], dphi_via_g=dd["via_g"], grad=grad)


ARMIJO = dict(sufficient_decrease=1e-4, max_step_contraction=1e-3, min_step_contraction=0.6, min_step_size=1e-9, max_num_iterations=20)
# c of the elimination term c u kappa_inf(A) |alpha| of an interior step: four times the worst |alpha_fp64 - alpha_mpmath| /
# (u kappa_inf(A) |alpha|) measured over the 40 synthetic searches of tests/test_oracle_bounds.py for the numpy restatement
# and the C oracle (tests/test_hp_reference.py: test_armijo_elimination_constant), two bits for another pivoting order and
# root finder
ARMIJO_C = 5.61           # measured: 1.4006
MP_DIGITS = 50


def interpolation_minimum(samples, lo, hi, bars=None):
    """FindInterpolatingPolynomial + MinimizeInterpolatingPolynomial at MP_DIGITS digits (mpmath).  samples: (x, value,
    gradient) triples -- the polynomial of degree 2 len(samples) - 1 through all of them -- and the candidates in Ceres' order:
    the midpoint of [lo, hi], lo, hi, the real parts of ALL roots of the derivative that fall inside [lo, hi], then the samples
    inside it with their own values; the first strictly smallest value wins.

    Returns a dict: x (float), kind ("mid" / "lo" / "hi" / "root" / "sample"), interior (kind == "root"), kappa (kappa_inf of the
    interpolation system A), and with bars (one (value bar, gradient bar) pair per sample): x_bar -- the bars carried through
    the minimiser by central differences --, rank_margin (smallest |p(other) - p(best)| over its propagated bar) and
    edge_margin (smallest distance of a root's real part from lo / hi over its propagated bar); inf where nothing competes."""
    import mpmath as mp
    with mp.workdps(MP_DIGITS):
        lo_, hi_ = mp.mpf(float(lo)), mp.mpf(float(hi))
        xs = [mp.mpf(float(s[0])) for s in samples]
        n = 2 * len(samples)

        def solve(vals):
            A, b = mp.zeros(n, n), mp.zeros(n, 1)
            for i, x in enumerate(xs):
                for jc in range(n):
                    A[2 * i, jc] = x ** (n - 1 - jc)
                    A[2 * i + 1, jc] = (n - 1 - jc) * x ** (n - 2 - jc) if jc < n - 1 else mp.mpf(0)
                b[2 * i], b[2 * i + 1] = vals[2 * i], vals[2 * i + 1]
            coef = [c for c in mp.lu_solve(A, b)]
            der = [(n - 1 - i) * coef[i] for i in range(n - 1)]
            while len(der) > 1 and der[0] == 0:
                der = der[1:]
            roots = sorted((mp.re(z) for z in mp.polyroots(der, maxsteps=500, extraprec=4 * MP_DIGITS)), key=float) if len(der) > 1 else []
            return A, coef, roots

        base = [mp.mpf(float(v)) for s in samples for v in (s[1], s[2])]
        A, coef, roots = solve(base)
        kappa = float(mp.norm(A, mp.inf) * mp.norm(mp.inverse(A), mp.inf))
        cands = [("mid", (lo_ + hi_) / 2, None), ("lo", lo_, None), ("hi", hi_, None)]
        cands += [("root", z, i) for i, z in enumerate(roots) if lo_ <= z <= hi_]
        vals = [mp.polyval(coef, x) for _, x, _ in cands]
        cands += [("sample", xs[i], i) for i in range(len(xs)) if lo_ <= xs[i] <= hi_]
        vals += [base[2 * i] for i in range(len(xs)) if lo_ <= xs[i] <= hi_]
        best = 0
        for i in range(1, len(cands)):
            if vals[i] < vals[best]:
                best = i
        out = dict(x=float(cands[best][1]), kind=cands[best][0], interior=cands[best][0] == "root", kappa=kappa,
                   x_bar=0.0, rank_margin=float("inf"), edge_margin=float("inf"))
        if bars is None:
            return out
        flat = [float(b) for pair in bars for b in pair]

        def observe(v):
            _, cf, rt = solve(v)
            assert len(rt) == len(roots)
            loc = lambda c: rt[c[2]] if c[0] == "root" else c[1]
            val = lambda c, v=v: v[2 * c[2]] if c[0] == "sample" else mp.polyval(cf, loc(c))
            o = {"x": loc(cands[best])}
            for i, c in enumerate(cands):
                if i != best:
                    o[f"rank{i}"] = val(c) - val(cands[best])
            for i, z in enumerate(rt):
                o[f"root{i}"] = z
            return o

        obs0, acc = observe(base), {}
        for i in range(len(base)):
            h = max(abs(base[i]), mp.mpf(1)) * mp.mpf(2) ** -60
            up, dn = list(base), list(base)
            up[i], dn[i] = base[i] + h, base[i] - h
            ou, od = observe(up), observe(dn)
            for k in obs0:
                acc[k] = acc.get(k, 0.0) + float(abs((ou[k] - od[k]) / (2 * h))) * flat[i]
        ratio = lambda dist, bar: float("inf") if bar == 0 else abs(float(dist)) / bar
        out["x_bar"] = acc["x"]
        ranks = [ratio(obs0[k], acc[k]) for k in obs0 if k.startswith("rank")]
        edges = [ratio(z - e, acc[f"root{i}"]) for i, z in enumerate(roots) for e in (lo_, hi_)]
        out["rank_margin"] = min(ranks) if ranks else float("inf")
        out["edge_margin"] = min(edges) if edges else float("inf")
        return out


def armijo_search(phi, dphi, dir_max_norm=1.0, initial=None):
    """ArmijoLineSearch::DoSearch with the defaults quoted at the top of csrc/ssba_linesearch.h (ARMIJO): CUBIC interpolation
    through (0, previous, current), step contraction into [1e-3, 0.6] of the current step, at most 20 iterations, minimum step
    size 1e-9 / |direction|_inf.  phi(a), dphi(a) return a value or (value, bar).  initial: ((phi(0), bar), (phi'(0), bar)) when
    they are known already.  The decisions are made on the values; the interpolating polynomial and its minimiser at
    MP_DIGITS digits (interpolation_minimum).

    Returns a dict: alphas (every step evaluated, the first is 1), kinds (None for the first, then the kind of each choice),
    interior, x_bars and kappas per chosen step, armijo_margins (|phi(a) - phi(0) - 1e-4 phi'(0) a| over its bar, per sample),
    choice_margins (min of rank and edge margin per choice), success, optimal (the accepted step or None), count (evaluations),
    samples ((a, phi, phi')), margin (the smallest of all margins)."""
    pair = lambda v: (v[0], float(v[1])) if isinstance(v, tuple) else (v, 0.0)
    o = ARMIJO
    (f0, f0b), (g0, g0b) = (pair(phi(0.0)), pair(dphi(0.0))) if initial is None else (pair(initial[0]), pair(initial[1]))
    init = (0.0, f0, g0)
    init_b = (f0b, g0b)
    prev = prev_b = None
    x = 1.0
    out = dict(alphas=[], kinds=[None], interior=[False], x_bars=[0.0], kappas=[0.0], armijo_margins=[], choice_margins=[], samples=[],
               success=False, optimal=None)
    it = 0
    ratio = lambda dist, bar: float("inf") if bar == 0 else abs(float(dist)) / bar
    while True:
        (v, vb), (g, gb) = pair(phi(x)), pair(dphi(x))
        out["alphas"].append(x)
        out["samples"].append((x, v, g))
        thr = LD(f0) + LD(o["sufficient_decrease"]) * LD(g0) * LD(x)
        out["armijo_margins"].append(ratio(LD(v) - thr, vb + f0b + o["sufficient_decrease"] * x * g0b))
        if not LD(v) > thr:
            out.update(success=True, optimal=x)
            break
        it += 1
        if it >= o["max_num_iterations"]:
            break
        lo, hi = o["max_step_contraction"] * x, o["min_step_contraction"] * x
        smp, sb = [init, (x, v, g)], [init_b, (vb, gb)]
        if prev is not None:
            smp.append(prev)
            sb.append(prev_b)
        m = interpolation_minimum(smp, lo, hi, sb)
        if m["x"] * dir_max_norm < o["min_step_size"]:
            break
        out["kinds"].append(m["kind"])
        out["interior"].append(m["interior"])
        out["x_bars"].append(m["x_bar"])
        out["kappas"].append(m["kappa"])
        out["choice_margins"].append(min(m["rank_margin"], m["edge_margin"]))
        prev, prev_b, x = (x, v, g), (vb, gb), m["x"]
    out["count"] = len(out["alphas"])
    out["margin"] = min(out["armijo_margins"] + out["choice_margins"])
    return out
