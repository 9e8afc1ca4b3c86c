"""Long-double reference for the front end (ssba_frontend.hip; CPU only, numpy only).

The front end is the reference project's ``compute_initial_guess``: reciprocal matching of consecutive states, stereo
triangulation, a 3-point RANSAC per pair (alignment by the SVD of the 3x3 cross-covariance W, stereo reprojection inlier
test, first maximum), the pose chain and the map initialisation.  Everything here is evaluated in ``np.longdouble`` (unit
roundoff 2^-64) from the fp64 inputs, which long double holds exactly; matching and selection are exact integer work.

Bars (u = 2^-53, c = 16 as in tests/hp_reference.py):

* rotation      |R - R*|_max <= c (u |E_W|_F / s2 + u).  W = (1/3) sum b_i a_i^T has rank <= 2 for three points; R is fixed by
  the two leading singular pairs, and the pair (s2, v2, u2) moves by |dW| / s2 under a perturbation dW (Wedin: the gap to
  the null direction is s2, the gap s1 - s2 to the other pair does not enter R = u1 v1^T + u2 v2^T + (u1 x u2)(v1 x v2)^T,
  which is invariant under rotations inside the leading plane).  E_W is the first-order entrywise rounding of W in fp64:
  every centred coordinate carries u (|a| + |c|), every product u |b||a|:
      E_W = (1/3) sum_i [(|b_i| + |c1|)|a_i|^T + |b_i| (|a_i| + |c0|)^T].
* translation   |t - t*| <= c ((u |E_W|_F / s2 + u) |c0|_1 + u (|c1| + |c0|_1)),  t = c1 - R c0; |c| are the means of the
  absolute coordinates, which also cover the rounding of the centroid sums.
* orthonormality |R^T R - I|_max <= c u, |det R - 1| <= c u, degenerate samples included.
* triangulation relative error <= 4 u per coordinate (a subtraction, a division, two or three products).
* inlier flag   decided only where |e^2 - thresh| > c u M, M the sum of the absolute values of the terms that cancel in e^2.
* chain         rotation of pose k within sum_{q<k} bar_R(q) + c u k; translation within
  sum_{q<k} (bar_R(q) |t_q*|_1 + bar_t(q)) + c u k |t_k*|.
"""
from __future__ import annotations

import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "long double is not extended precision on this platform: the reference would be fp64"

U = 2.0 ** -53
C_TERMS = 16
TRI_REL = 4 * U
IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1.0])


def _f(v):
    return np.asarray(v, dtype=LD)


# ------------------------------------------------------------------------------------------------------------ triangulation
def triangulate(cam, uvd):
    """StereoCamera::triangulate: (u, v, d) -> (x, y, z), b/d * (u - cu, (v - cv) fu / fv, fu)."""
    uvd = _f(uvd)
    fu, fv, cu, cv, b = (LD(cam[n]) for n in ("fu", "fv", "cu", "cv", "b"))
    bod = b / uvd[..., 2]
    return np.stack([(uvd[..., 0] - cu) * bod, (uvd[..., 1] - cv) * bod * (fu / fv), fu * bod], axis=-1)


# ---------------------------------------------------------------------------------------------------------------- alignment
def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def jacobi_svd3(W, sweeps=40):
    """One-sided Jacobi SVD of a batch of 3x3 matrices (B, 3, 3) in W's dtype.  Returns G = W V (columns orthogonal, norms =
    singular values) and V, columns sorted by descending norm."""
    G = np.array(W, copy=True)
    B = G.shape[0]
    dt = G.dtype
    V = np.broadcast_to(np.eye(3, dtype=dt), (B, 3, 3)).copy()
    eps = dt.type(np.finfo(dt).eps) / 4
    for _ in range(sweeps):
        moved = False
        for p, q in ((0, 1), (0, 2), (1, 2)):
            gp, gq = G[:, :, p], G[:, :, q]
            al, be, ga = (gp * gp).sum(1), (gq * gq).sum(1), (gp * gq).sum(1)
            act = (ga != 0) & (np.abs(ga) > eps * np.sqrt(al) * np.sqrt(be))
            if not act.any():
                continue
            moved = True
            gs = np.where(act, ga, dt.type(1))
            zeta = (be - al) / (2 * gs)
            t = np.where(zeta >= 0, dt.type(1), dt.type(-1)) / (np.abs(zeta) + np.sqrt(zeta * zeta + 1))
            c = 1 / np.sqrt(t * t + 1)
            s = t * c
            c = np.where(act, c, dt.type(1))[:, None]
            s = np.where(act, s, dt.type(0))[:, None]
            G[:, :, p], G[:, :, q] = c * gp - s * gq, s * gp + c * gq
            vp, vq = V[:, :, p].copy(), V[:, :, q].copy()
            V[:, :, p], V[:, :, q] = c * vp - s * vq, s * vp + c * vq
        if not moved:
            break
    sv = np.sqrt((G * G).sum(1))
    order = np.argsort(-sv, axis=1, kind="stable")
    G = np.take_along_axis(G, order[:, None, :], axis=2)
    V = np.take_along_axis(V, order[:, None, :], axis=2)
    return G, V, np.take_along_axis(sv, order, axis=1)


def _unit(v):
    n = np.sqrt((v * v).sum(-1, keepdims=True))
    return v / np.where(n > 0, n, 1)


def _complete(u1):
    """A unit vector orthogonal to u1: e_m - (e_m . u1) u1 with m the smallest |u1| component."""
    m = np.argmin(np.abs(u1), axis=-1)
    e = np.zeros_like(u1)
    np.put_along_axis(e, m[:, None], 1, axis=-1)
    return _unit(e - (e * u1).sum(-1, keepdims=True) * u1)


def align3(p0, p1, dtype=LD):
    """PointCloudAligner::compute_transformation for batches of 3-point samples: p0, p1 (B, 3, 3) [sample, point, xyz].

    Returns a dict: T (B, 12) [t | R row-major] in `dtype`, s1, s2, EW_F = |E_W|_F, c0abs1 = |c0|_1, c1abs (B, 3), v1, u1
    and rank (0, 1, 2: singular values above 2^-60 s1 count), the last ones for the degenerate samples."""
    p0, p1 = np.asarray(p0, dtype=dtype), np.asarray(p1, dtype=dtype)
    c0, c1 = p0.sum(1) / 3, p1.sum(1) / 3
    a, b = p0 - c0[:, None], p1 - c1[:, None]
    W = np.einsum("bir,bic->brc", b, a) / 3
    G, V, sv = jacobi_svd3(W)
    s1, s2 = sv[:, 0], sv[:, 1]
    one = dtype(1)
    v1, v2 = _unit(V[:, :, 0]), V[:, :, 1]
    v2 = _unit(v2 - (v1 * v2).sum(-1, keepdims=True) * v1)
    ok1 = s1 > 0
    e0 = np.zeros_like(v1)
    e0[:, 0] = 1
    u1 = np.where(ok1[:, None], G[:, :, 0] / np.where(ok1, s1, one)[:, None], e0)
    ok2 = s2 > dtype(2.0 ** -60) * s1
    u2 = G[:, :, 1] / np.where(ok2, s2, one)[:, None]
    u2 = u2 - (u1 * u2).sum(-1, keepdims=True) * u1
    u2 = np.where(ok2[:, None], _unit(u2), _complete(u1))
    u3, v3 = _cross(u1, u2), _cross(v1, v2)
    R = u1[:, :, None] * v1[:, None, :] + u2[:, :, None] * v2[:, None, :] + u3[:, :, None] * v3[:, None, :]
    t = c1 - np.einsum("brc,bc->br", R, c0)
    # magnitudes for the bars (fp64 accuracy is ample)
    a64, b64 = np.abs(np.asarray(a, np.float64)), np.abs(np.asarray(b, np.float64))
    c0a, c1a = np.abs(np.asarray(p0, np.float64)).mean(1), np.abs(np.asarray(p1, np.float64)).mean(1)
    EW = (np.einsum("bir,bic->brc", b64 + c1a[:, None], a64) + np.einsum("bir,bic->brc", b64, a64 + c0a[:, None])) / 3
    return dict(T=np.concatenate([t, R.reshape(-1, 9)], axis=1), s1=s1, s2=s2, EW_F=np.sqrt((EW * EW).sum((1, 2))),
                c0abs1=c0a.sum(1), c1abs=c1a, v1=v1, u1=u1, rank=ok1.astype(int) + (ok1 & ok2).astype(int))


def align_bars(ref):
    """(bar_R (B,), bar_t (B, 3)) of the module docstring from align3's dict; infinite where s2 = 0."""
    s2 = np.asarray(ref["s2"], np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        inner = np.where(s2 > 0, U * ref["EW_F"] / np.where(s2 > 0, s2, 1.0), np.inf) + U
    return C_TERMS * inner, C_TERMS * (inner[:, None] * ref["c0abs1"][:, None] + U * (ref["c1abs"] + ref["c0abs1"][:, None]))


def orthonormality(T):
    """(max |R^T R - I|, |det R - 1|) per sample, evaluated in long double from the fp64 result."""
    R = _f(T)[:, 3:].reshape(-1, 3, 3)
    G = np.einsum("bki,bkj->bij", R, R) - np.eye(3, dtype=LD)
    det = (R[:, 0] * _cross(R[:, 1], R[:, 2])).sum(-1)
    return np.abs(G).max((1, 2)).astype(np.float64), np.abs(det - 1).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------- inlier test
def reprojection_error2(cam, T, p0, p1):
    """Squared stereo reprojection error of is_inlier, (project(p1) - project(T p0))^2 over (u, v, d), broadcasting T
    (..., 12) against p0, p1 (..., 3).  Returns (e2, M): M = the sum of the absolute values of the terms that cancel, so that
    an fp64 evaluation of e2 is within c u M of it.  q2 <= 0 or p1.z <= 0 is evaluated like any other value."""
    T, p0, p1 = _f(T), _f(p0), _f(p1)
    fu, fv, cu, cv, b = (LD(cam[n]) for n in ("fu", "fv", "cu", "cv", "b"))
    R = T[..., 3:].reshape(T.shape[:-1] + (3, 3))
    terms = R * p0[..., None, :]
    q = terms.sum(-1) + T[..., :3]
    qa = np.abs(terms).sum(-1) + np.abs(T[..., :3])           # |R||p0| + |t|: what q is rounded relative to
    q0, q1, q2 = q[..., 0], q[..., 1], q[..., 2]
    a = np.stack([fu * p1[..., 0] / p1[..., 2], fv * p1[..., 1] / p1[..., 2], fu * b / p1[..., 2]], -1)
    bq = np.stack([fu * q0 / q2, fv * q1 / q2, fu * b / q2], -1)
    d = a - bq
    e2 = (d * d).sum(-1)
    # first order: d_k carries u (|a_k| + |b_k| + |c_k|) from its own operations and |b_k| (dq_k/|q_k| + dq2/|q2|) from q
    aq2 = np.abs(q2)
    rel2 = qa[..., 2] / aq2
    cvec = np.stack([np.abs(cu), np.abs(cv), LD(0)])
    db = np.stack([np.abs(fu) * qa[..., 0] / aq2 + np.abs(bq[..., 0]) * rel2, np.abs(fv) * qa[..., 1] / aq2 + np.abs(bq[..., 1]) * rel2,
                   np.abs(bq[..., 2]) * rel2], -1)
    mag = np.abs(a) + np.abs(bq) + cvec + db
    M = (2 * np.abs(d) * mag).sum(-1) + e2
    return e2, np.asarray(M, np.float64)


def inlier_decision(cam, T, p0, p1, thresh, extra_band=0.0):
    """(flag, decided): the long-double e2 < thresh, and whether |e2 - thresh| > c u M + extra_band."""
    e2, M = reprojection_error2(cam, T, p0, p1)
    flag = e2 < LD(thresh)
    band = C_TERMS * U * M + extra_band
    with np.errstate(invalid="ignore"):
        decided = np.abs(np.asarray(e2 - LD(thresh), np.float64)) > band
    return flag, decided & np.isfinite(np.asarray(e2, np.float64))


def pose_sensitivity(cam, T, p0, p1, dR, dt):
    """First-order bound of |e2(T + dT) - e2(T)| for |dR|_max <= dR and |dt| <= dt (3,), fp64."""
    T64, p0, p1 = np.asarray(T, np.float64), np.asarray(p0, np.float64), np.asarray(p1, np.float64)
    R = T64[..., 3:].reshape(T64.shape[:-1] + (3, 3))
    q = (R * p0[..., None, :]).sum(-1) + T64[..., :3]
    dq = dR * np.abs(p0).sum(-1)[..., None] + dt
    fu, fv, b = cam["fu"], cam["fv"], cam["b"]
    q2 = np.abs(q[..., 2])
    pj = lambda x: np.stack([fu * x[..., 0] / x[..., 2], fv * x[..., 1] / x[..., 2], fu * b / x[..., 2]], -1)
    d = np.abs(pj(p1) - pj(q))
    db = np.stack([fu * (dq[..., 0] + np.abs(q[..., 0]) / q2 * dq[..., 2]) / q2, fv * (dq[..., 1] + np.abs(q[..., 1]) / q2 * dq[..., 2]) / q2,
                   fu * b * dq[..., 2] / (q2 * q2)], -1)
    return (2 * d * db + db * db).sum(-1)


# ------------------------------------------------------------------------------------------------------------------ pipeline
def match_states(ids_a, ids_b):
    """Reciprocal matches in exact integers: positions kept in each list, each list's own order.  None for a pair the device
    reports as unusable (a duplicate id makes the two lists differ in length)."""
    ka = np.nonzero(np.isin(ids_a, ids_b))[0]
    kb = np.nonzero(np.isin(ids_b, ids_a))[0]
    return (ka, kb) if len(ka) == len(kb) else None


def se3_compose(Ta, Tb):
    Ra, Rb = Ta[3:].reshape(3, 3), Tb[3:].reshape(3, 3)
    return np.concatenate([Ra @ Tb[:3] + Ta[:3], (Ra @ Rb).ravel()])


def ransac_pair(cam, p0, p1, samples, thresh):
    """All hypotheses of one pair.  p0, p1 (n, 3) fp64 points as the device triangulated them (or long double), samples
    (iters, 3).  Returns a dict: ref (align3's dict over the hypotheses), count (iters,) long-double counts, lo / hi: the
    decided-inlier count and that plus the undecided points, where the band of a point is c u M plus the sensitivity of e2 to
    the hypothesis's own bars; winner (first maximum, -1 if all counts are 0), unambiguous."""
    ref = align3(np.asarray(p0)[samples], np.asarray(p1)[samples])
    bR, bt = align_bars(ref)
    T = ref["T"][:, None, :]
    sens = pose_sensitivity(cam, T, p0[None], p1[None], np.minimum(bR, 1e300)[:, None, None], np.minimum(bt, 1e300)[:, None, :])
    flag, decided = inlier_decision(cam, T, _f(p0)[None], _f(p1)[None], thresh, np.nan_to_num(sens, nan=np.inf))
    count = flag.sum(1)
    lo = (flag & decided).sum(1)
    hi = lo + (~decided).sum(1)
    w = int(np.argmax(count)) if count.max() > 0 else -1
    unamb = w >= 0 and bool(np.all(hi[:w] < lo[w]) and np.all(hi[w + 1:] <= lo[w]))
    return dict(ref=ref, bar_R=bR, bar_t=bt, count=count, lo=lo, hi=hi, winner=w, unambiguous=unamb, flag=flag, decided=decided)


def vo_pipeline(cam, state_start, point_id, uvd, num_points, first_pose, samples_of, thresh):
    """compute_initial_guess in long double.  state_start (S + 1,), point_id / uvd grouped by state; samples_of(n) -> (iters, 3)
    draw sequence for a pair of n matches.  Returns a dict with per pair: match_count, pair results (ransac_pair), T (P, 12);
    poses (S, 12) long double; map (num_points, 3), initialized, first_pair; and the accumulated chain bars chain_R (S,),
    chain_t (S,).  A pair with fewer than three matches (or mismatched lists) gets match_count 0 and stops the pipeline
    (`failed` = its index), as the device reports an error there."""
    S = len(state_start) - 1
    out = dict(match_count=np.zeros(S - 1, np.int64), pairs=[], failed=None, match_pos=[])
    poses = np.zeros((S, 12), dtype=LD)
    poses[0] = _f(first_pose)
    pmap = np.zeros((num_points, 3), dtype=LD)
    init = np.zeros(num_points, dtype=bool)
    first_pair = np.full(num_points, -1)
    map_bar = np.zeros(num_points)
    chain_R, chain_t = np.zeros(S), np.zeros(S)
    for k in range(S - 1):
        a0, a1, a2 = state_start[k], state_start[k + 1], state_start[k + 2]
        m = match_states(point_id[a0:a1], point_id[a1:a2])
        n = 0 if m is None else len(m[0])
        out["match_count"][k] = n
        out["match_pos"].append(m)
        if n < 3:
            out["failed"] = k if out["failed"] is None else out["failed"]
            out["pairs"].append(None)
            continue
    if out["failed"] is not None:
        return out
    for k in range(S - 1):
        a0, a1 = state_start[k], state_start[k + 1]
        ka, kb = out["match_pos"][k]
        p0, p1 = triangulate(cam, uvd[a0 + ka]), triangulate(cam, uvd[a1 + kb])
        # the device scores the fp64 points it triangulated: round as it does (within TRI_REL, asserted separately)
        p0, p1 = np.asarray(p0, np.float64), np.asarray(p1, np.float64)
        r = ransac_pair(cam, p0, p1, samples_of(len(ka)), thresh)
        out["pairs"].append(r)
        w = r["winner"]
        T = r["ref"]["T"][w] if w >= 0 else _f(IDENTITY)
        poses[k + 1] = se3_compose(T, poses[k])
        bR = r["bar_R"][w] if w >= 0 else 0.0
        bt = r["bar_t"][w].max() if w >= 0 else 0.0
        tq = float(np.abs(poses[k][:3]).sum())
        chain_R[k + 1] = chain_R[k] + bR + C_TERMS * U
        chain_t[k + 1] = chain_t[k] + bR * tq + bt
        if w >= 0:
            mask = r["flag"][w]
            js = point_id[a0 + ka][mask]
            new = ~init[js]
            Rk, tk = poses[k][3:].reshape(3, 3), poses[k][:3]
            pmap[js[new]] = (_f(p0)[mask][new] - tk) @ Rk
            init[js[new]] = True
            first_pair[js[new]] = k
            pk = np.abs(p0[mask][new]).sum(1) + tq
            ct = chain_t[k] + C_TERMS * U * k * float(np.abs(poses[k][:3]).max())
            map_bar[js[new]] = 3 * chain_R[k] * pk + 3 * ct + C_TERMS * U * pk
    out.update(poses=poses, map=pmap, initialized=init, first_pair=first_pair, map_bar=map_bar, chain_R=chain_R,
               chain_t=chain_t + C_TERMS * U * np.arange(S) * np.asarray(np.abs(poses[:, :3]).max(1), np.float64))
    return out


def mp_to_ld(x):
    """mpmath.mpf -> long double without passing through fp64: two fp64 pieces, each exact."""
    hi = float(x)
    return LD(hi) + LD(float(x - hi))


# ------------------------------------------------------------------------------------------------------------------- cases
CPU_LADDER = (1.4, 7.6e1, 7.6e3, 7.6e5, 7.6e7, 7.6e9, 7.6e11)
GPU_LADDER = (1.0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7)


def _rot(axis, ang):
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K


def ladder_step(kappa, count, rng, mirror=False, max_angle=0.5):
    """`count` triangles with s1 / s2 ~ kappa: base 2 L along e1, apex at height h = L sqrt(3 / kappa) along e2 (the scatter
    of that triangle has eigenvalues 2 L^2 / 3 and 2 h^2 / 9), centroid at depth 5-80 m, L = spread 0.05-5 m (log-uniform),
    rotation 0.01-max_angle rad about a random axis, translation up to 1 m, and a non-congruence of 1e-3 h in every coordinate
    of the second triangle.  mirror: the second triangle is the first one reflected in its own plane about e1 -- the best
    proper rotation then turns it over (det U det V = -1 for an SVD that returns U, V of opposite handedness).
    Returns p0, p1 (count, 3, 3) fp64."""
    p0, p1 = np.zeros((count, 3, 3)), np.zeros((count, 3, 3))
    for i in range(count):
        z = rng.uniform(5, 80)
        c = np.array([rng.uniform(-0.4, 0.4) * z, rng.uniform(-0.15, 0.15) * z, z])
        L = 0.05 * 100 ** rng.uniform()
        h = L * np.sqrt(3.0 / kappa)
        Q = np.linalg.qr(rng.normal(size=(3, 3)))[0]
        e1, e2 = Q[:, 0], Q[:, 1]
        xs = np.array([-1.0, 1.0, 0.0]) * L
        ys = np.array([-1.0, -1.0, 2.0]) * h / 3
        a = xs[:, None] * e1 + ys[:, None] * e2
        am = xs[:, None] * e1 - ys[:, None] * e2 if mirror else a
        R = _rot(rng.normal(size=3), rng.uniform(0.01, max_angle))
        p0[i] = c + a
        p1[i] = (c + am) @ R.T + rng.uniform(-1, 1, size=3) + 1e-3 * h * rng.normal(size=(3, 3))
    return p0, p1


def collinear_cases():
    """16 exactly collinear samples (dyadic coordinates, centroid and centred coordinates exact in fp64): p0_i = c + k_i d,
    p1_i = c' + k_i d', so W = (sum k~^2 / 3) d' d^T has rank 1, v1 = d / |d|, u1 = d' / |d'|.  Returns p0, p1, v1, u1 (LD)."""
    ks = [np.array(k, float) for k in ((-3, 0, 3), (0, 3, 6), (-1, -1, 2), (1, 4, -5), (0.5, 0.25, -0.75), (6, -3, -3), (2, 2, -4), (0, 1.5, 3))]
    ds = [((1, 2, 2), (2, -1, 2)), ((0.5, 0, 0), (0, 0, 0.75)), ((3, 4, 0), (0, -4, 3)), ((1, 1, 1), (-1, 2, 0.5))]
    p0, p1, v1, u1 = [], [], [], []
    for n, k in enumerate(ks):
        for m in range(2):
            d, dd = (np.array(v, float) for v in ds[(n + 2 * m) % 4])
            c, cc = np.array([2.0, -1.5, 12.0 + n]), np.array([1.25, 0.5, 11.0 + n])
            p0.append(c + k[:, None] * d)
            p1.append(cc + k[:, None] * dd)
            v1.append(_f(d) / np.sqrt((_f(d) ** 2).sum()))
            u1.append(_f(dd) / np.sqrt((_f(dd) ** 2).sum()))
    return np.array(p0), np.array(p1), np.array(v1), np.array(u1)


def coincident_cases():
    p0 = np.array([[[1.0, 2.0, 10.0]] * 3, [[-3.0, 0.5, 40.0]] * 3, [[0.0, 0.0, 5.0]] * 3, [[7.0, -2.0, 80.0]] * 3])
    p1 = np.array([[[1.5, 2.0, 9.0]] * 3, [[-3.0, 0.5, 40.0]] * 3, [[0.25, 0.0, 5.5]] * 3, [[6.0, -1.0, 79.0]] * 3])
    return p0, p1


def align_ratios(T, ref):
    """Worst |R - R*| / bar_R and |t - t*| / bar_t per sample of a fp64 result T (B, 12) against align3's dict."""
    bR, bt = align_bars(ref)
    d = np.abs(np.asarray(_f(T) - ref["T"], np.float64))
    return d[:, 3:].max(1) / bR, (d[:, :3] / bt).max(1)


def align3_eig_fp64(p0, p1):
    """The superseded algorithm in fp64 numpy: right singular vectors from an eigen-decomposition of W^T W."""
    out = np.zeros((len(p0), 12))
    for i, (a0, a1) in enumerate(zip(p0, p1)):
        c0, c1 = a0.sum(0) / 3, a1.sum(0) / 3
        W = (a1 - c1).T @ (a0 - c0) / 3
        w, V = np.linalg.eigh(W.T @ W)
        v1, v2 = V[:, 2], V[:, 1]
        u1, u2 = W @ v1, W @ v2
        u1 /= np.linalg.norm(u1)
        u2 -= (u1 @ u2) * u1
        u2 /= np.linalg.norm(u2)
        R = np.outer(u1, v1) + np.outer(u2, v2) + np.outer(np.cross(u1, u2), np.cross(v1, v2))
        out[i] = np.concatenate([c1 - R @ c0, R.ravel()])
    return out


def align3_svd_fp64(p0, p1):
    """Kabsch with LAPACK's SVD of W in fp64 (what the reference's Eigen::JacobiSVD stands for)."""
    out = np.zeros((len(p0), 12))
    for i, (a0, a1) in enumerate(zip(p0, p1)):
        c0, c1 = a0.sum(0) / 3, a1.sum(0) / 3
        W = (a1 - c1).T @ (a0 - c0) / 3
        Uu, s, Vt = np.linalg.svd(W)
        u1, u2, v1, v2 = Uu[:, 0], Uu[:, 1], Vt[0], Vt[1]
        R = np.outer(u1, v1) + np.outer(u2, v2) + np.outer(np.cross(u1, u2), np.cross(v1, v2))
        out[i] = np.concatenate([c1 - R @ c0, R.ravel()])
    return out


# ------------------------------------------------------------------------------------------- inlier rows and whole sequences
INLIER_SIZES = (3, 63, 64, 65, 255, 256, 257, 513)
INLIER_DELTAS = tuple(s * d for d in (1e-3, 1e-6, 1e-9, 1e-12, 1e-15) for s in (1, -1))


def _project(cam, q):
    fu, fv, cu, cv, b = (LD(cam[n]) for n in ("fu", "fv", "cu", "cv", "b"))
    return np.stack([fu * q[..., 0] / q[..., 2] + cu, fv * q[..., 1] / q[..., 2] + cv, fu * b / q[..., 2]], -1)


def inlier_pairs(cam, thresh, seed=11):
    """One pair per size of INLIER_SIZES.  The first three points are a well-conditioned congruent triangle that defines T;
    the others cycle through: the ten rows built so that e^2 = thresh (1 + delta), delta in INLIER_DELTAS (the second point is
    triangulated in long double from project(T p0) + sqrt(thresh (1 + delta)) w, |w| = 1, then rounded to fp64), a generic
    inlier (e^2 = thresh / 3), a generic outlier (10 thresh), and every 29th row a point behind the first camera (q2 <= 0)
    or a second point at depth 1e-3.  Returns a list of (p0, p1, delta) with delta = nan for rows not built around the
    threshold."""
    rng = np.random.default_rng(seed)
    out = []
    for n in INLIER_SIZES:
        R = _f(_rot(rng.normal(size=3), 0.08))
        t = _f(rng.uniform(-0.5, 0.5, size=3))
        p0 = np.zeros((n, 3))
        p0[:3] = np.array([[-2.0, 1.0, 14.0], [2.5, 0.5, 17.0], [0.3, -1.5, 12.0]]) + rng.uniform(-0.2, 0.2, size=(3, 3))
        z = rng.uniform(6, 40, size=n - 3)
        p0[3:] = np.stack([rng.uniform(-0.5, 0.5, n - 3) * z, rng.uniform(-0.2, 0.2, n - 3) * z, z], 1)
        q = _f(p0) @ R.T + t
        p1 = np.asarray(q, np.float64)
        delta = np.full(n, np.nan)
        for i in range(3, n):
            kind = (i - 3) % 12
            if (i - 3) % 29 == 28:
                if (i // 29) % 2:
                    p0[i] = [0.5, -0.25, -3.0]                    # behind the first camera: q2 < 0
                    p1[i] = [0.4, -0.2, 3.0]
                else:
                    p1[i, 2] = 1e-3
                continue
            e2 = LD(thresh) * (1 + LD(INLIER_DELTAS[kind])) if kind < 10 else LD(thresh) / 3 if kind == 10 else LD(thresh) * 10
            w = _f(rng.normal(size=3))
            w = w / np.sqrt((w * w).sum())
            uvd = _project(cam, q[i]) + np.sqrt(e2) * w
            p1[i] = np.asarray(triangulate(cam, uvd), np.float64)
            if kind < 10:
                delta[i] = INLIER_DELTAS[kind]
        out.append((p0, p1, delta))
    return out


def _sequence_poses(S, rng, step=0.3):
    """World-to-camera poses of a gently turning forward motion, (S, 12) fp64."""
    poses = np.zeros((S, 12))
    for k in range(S):
        Rk = _rot(np.array([0.05, 1.0, 0.02]), 0.004 * k)
        ck = np.array([0.02 * k, 0.0, step * k])                 # camera centre in the world
        poses[k] = np.concatenate([-Rk @ ck, Rk.ravel()])
    return poses


def observe(cam, poses, world, states_of, noise_px, rng, shuffle=False):
    """Observations of world points: states_of[k] = ids seen from state k (that order, or ordered by a random rank of the landmarks).  Returns state_start,
    point_id (uint32), uvd fp64 with Gaussian noise of noise_px on u, v, d."""
    start, ids, uvd = [0], [], []
    key = rng.permutation(len(world))
    for k, js in enumerate(states_of):
        js = np.asarray(js)
        if shuffle:                       # one random rank per landmark: every state lists its ids in that order, so the
            js = js[np.argsort(key[js], kind="stable")]      # positional pairing of the matches stays consistent
        R, t = poses[k][3:].reshape(3, 3), poses[k][:3]
        q = world[js] @ R.T + t
        assert q[:, 2].min() > 1.0
        z = np.asarray(_project(cam, _f(q)), np.float64) + noise_px * rng.normal(size=(len(js), 3))
        ids.append(js); uvd.append(z); start.append(start[-1] + len(js))
    return np.array(start, np.uint32), np.concatenate(ids).astype(np.uint32), np.ascontiguousarray(np.concatenate(uvd))


def make_sequence(cam, S, per_state=40, track=4, noise_px=0.2, seed=0, shuffle=False):
    """S states, each seeing per_state landmarks, every landmark seen from `track` consecutive states (per_state / track new
    ones per state).  Returns dict(state_start, point_id, uvd, num_points, first_pose, poses_gt)."""
    rng = np.random.default_rng(seed)
    poses = _sequence_poses(S, rng)
    new = per_state // track
    L = new * (S + track - 1)
    world = np.zeros((L, 3))
    for j in range(L):
        k = min(max(j // new - (track - 1) // 2, 0), S - 1)      # a state in the middle of the track
        z = rng.uniform(8, 40)
        pc = np.array([rng.uniform(-0.45, 0.45) * z, rng.uniform(-0.2, 0.2) * z, z])
        R, t = poses[k][3:].reshape(3, 3), poses[k][:3]
        world[j] = R.T @ (pc - t)
    states_of = [np.arange(new * k, new * k + per_state) for k in range(S)]
    st, ids, uvd = observe(cam, poses, world, states_of, noise_px, rng, shuffle)
    return dict(state_start=st, point_id=ids, uvd=uvd, num_points=L, first_pose=poses[0].copy(), poses_gt=poses)


CHAIN_SEED = 0             # tests/test_hp_frontend.py checks that the reference leaves no pair of these sequences ambiguous
MATCH_EDGE_PLAN = ((255, None), (256, 3), (257, 200), (257, "all"), (512, 200), (512, "all"), (256, 3), (256, "all"), (255, 200), (255, "all"))


def matching_edge_sequence(cam, seed=5, shuffle=False, noise_px=0.0, plan=MATCH_EDGE_PLAN):
    """States of 255, 256, 257 and 512 observations of which 3, 200 or all match the previous state (MATCH_EDGE_PLAN: size and
    the number of ids shared with the state before)."""
    rng = np.random.default_rng(seed)
    S = len(plan)
    poses = _sequence_poses(S, rng, step=0.1)
    states_of, nxt = [], 0
    for n, shared in plan:
        if shared is None:
            js = np.arange(nxt, nxt + n)
        elif shared == "all":
            js = states_of[-1].copy()
        else:
            prev = states_of[-1]
            keep = np.sort(rng.choice(prev, size=shared, replace=False))
            js = np.sort(np.concatenate([keep, np.arange(nxt, nxt + n - shared)]))
        nxt = max(nxt, int(js.max()) + 1)
        states_of.append(js)
    z = rng.uniform(8, 40, size=nxt)
    world = np.stack([rng.uniform(-0.45, 0.45, nxt) * z, rng.uniform(-0.2, 0.2, nxt) * z, z + 2.0], 1)
    st, ids, uvd = observe(cam, poses, world, states_of, noise_px, rng, shuffle)
    return dict(state_start=st, point_id=ids, uvd=uvd, num_points=nxt, first_pose=poses[0].copy(), poses_gt=poses,
                shared=[None if s is None else (len(states_of[i]) if s == "all" else s) for i, (_, s) in enumerate(plan)])


def selection_problem(cam, samples, seed=0, L=40, inliers=8):
    """Two states of L landmarks of which `inliers` move rigidly and the others are mismatched by 20-60 px, chosen -- from the
    draw sequence `samples` (iters, 3) for L matches -- so that no draw before iteration 256 lies inside the rigid set and,
    where the sequence is long enough, at least two later ones do: the first maximum then sits past the first 256-lane
    stride of the selection kernel and ties with later iterations.  Observations carry 1e-6 px of noise, so that all-inlier
    hypotheses differ from each other by ~1e-8, far above the bars, and all still score every rigid landmark."""
    rng = np.random.default_rng(seed)
    for _ in range(200000):
        I = np.sort(rng.choice(L, size=inliers, replace=False))
        inside = np.nonzero(np.isin(samples, I).all(1))[0]
        if len(inside) >= min(2, 1 + (len(samples) > 300)) and inside[0] >= 256:
            break
    else:
        raise AssertionError("no rigid set found")
    poses = _sequence_poses(2, rng)
    z = rng.uniform(8, 40, size=L)
    world = np.stack([rng.uniform(-0.45, 0.45, L) * z, rng.uniform(-0.2, 0.2, L) * z, z + 2.0], 1)
    st, ids, uvd = observe(cam, poses, world, [np.arange(L), np.arange(L)], 1e-6, rng)
    out = np.setdiff1d(np.arange(L), I)
    ang = rng.uniform(0, 2 * np.pi, len(out))
    uvd[L + out, 0] += rng.uniform(20, 60, len(out)) * np.cos(ang)
    uvd[L + out, 1] += rng.uniform(20, 60, len(out)) * np.sin(ang)
    return dict(state_start=st, point_id=ids, uvd=uvd, num_points=L, first_pose=poses[0].copy(), rigid=I, first_inside=int(inside[0]),
                inside=inside)
