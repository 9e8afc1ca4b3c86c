"""Edge batches of the pose-only residual blocks (prior 0, sun sensor 1, relative pose 2), shared by the CPU proof of the
row bars (test_hp_reference.py) and the device tests (test_gpu_hp_pose_factors.py).

The residual rotation (or the sun direction in the camera and the observed angles) is chosen first and the inputs are built
from it in long double, then rounded to the fp64 values both sides receive.  Residual angles of 1e-15 and below cannot
survive the rounding of a product of generic rotations, so those rows take exact rotations for the poses (the identity or a
signed permutation) and R_ref = R_res; from 1e-12 upwards the rotations are generic, and every pose is 20 to 100 units from
the origin so that t_ref - R_res t (t_1 - R_12 t_2) cancels.  The rows on the Huber switch are the exception: a relative
distance of 1e-13 between |r|^2 and a^2 can only be told from rounding on a row whose own bar is below it, so those poses
are within a unit of the origin.

`batches()` -> {name: (poses (P, 12), factors)}: at most 64 factors each, every pose touched by exactly one block (the
relative batches: 32 disjoint pairs at most).  `assert_edges(name, poses, factors, rows)` checks, on the long-double rows of
hp_reference.pose_factor_rows, that the batch holds each of its edges on both sides and that every guard quantity is
farther from its guard than its own bar C_ROW u mag."""
import functools

import numpy as np

import hp_reference as hp

LD = hp.LD
PI_LD = LD(4) * np.arctan(LD(1))
EPS = 2.0 ** -52
ANGLES = [("0", 0.0), ("1e-17", 1e-17), ("1e-16", 1e-16), ("2e-16", 2e-16), ("2.5e-16", 2.5e-16), ("1e-15", 1e-15), ("1e-12", 1e-12),
          ("1e-8", 1e-8), ("9e-6", 9e-6), ("1.1e-5", 1.1e-5), ("1e-3", 1e-3), ("1", 1.0),
          ("pi-1e-2", PI_LD - LD(1e-2)), ("pi-1e-4", PI_LD - LD(1e-4)), ("pi-1e-6", PI_LD - LD(1e-6)), ("pi-1e-8", PI_LD - LD(1e-8))]
EXACT_BELOW = 1e-11       # residual angles up to here also come with exact pose rotations
GENERIC_FROM = 1e-13      # and from here on with generic ones
HUBER_DISTANCES = (1e-3, 1e-9, 1e-13)
THRESHOLD_DISTANCE = 1e-9


def _skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], dtype=LD)


def exp_ld(theta, n):
    """Rodrigues in long double: rotation by `theta` about the unit axis `n`."""
    theta, n = LD(theta), np.asarray(n, LD)
    n = n / np.sqrt((n * n).sum())
    c, s = np.cos(theta), np.sin(theta)
    return c * np.eye(3, dtype=LD) + (1 - c) * np.outer(n, n) + s * _skew(n)


def _f64(v):
    return np.asarray(v, np.float64)


def _generic_rotation(rng):
    return _f64(exp_ld(rng.uniform(0.3, 2.5), rng.normal(size=3)))


_PERMS = [np.eye(3), np.array([[0, 0, 1.0], [1, 0, 0], [0, 1, 0]]), np.array([[0, -1.0, 0], [1, 0, 0], [0, 0, 1]]),
          np.array([[-1.0, 0, 0], [0, 0, 1], [0, 1, 0]])]


def _far(rng, lo=20.0, hi=100.0):
    d = rng.normal(size=3)
    return d / np.linalg.norm(d) * rng.uniform(lo, hi)


def _pose(t, R):
    return np.concatenate([_f64(t), _f64(R).ravel()])


def full_stiffness(rng, m=6):
    """A full, not diagonal stiffness (symmetric positive definite for the 6 x 6 blocks, non-symmetric for the 2 x 2)."""
    if m == 2:
        return np.array([[50.0, 7.0], [-3.0, 40.0]]) * rng.uniform(0.5, 2.0)
    A = rng.normal(size=(6, 6)) * 0.3
    return A @ A.T + np.diag([3.0] * 3 + [10.0] * 3)


def prior_factor(k, T, R_res, e_t, S, huber=0.0, exact=False):
    """A prior on pose k whose residual is (e_t, log R_res): R_ref = R_res R (R_res itself where the pose rotation is exact)."""
    t, R = np.asarray(T[:3], LD), np.asarray(T[3:], LD).reshape(3, 3)
    Rr = _f64(R_res) if exact and np.array_equal(_f64(R), np.eye(3)) else _f64(np.asarray(R_res, LD) @ R)
    Rres = np.asarray(Rr, LD) @ R.T
    return dict(pose=k, type=0, data=_pose(np.asarray(e_t, LD) + Rres @ t, Rr), stiffness=np.asarray(S).ravel(), huber=huber)


def relative_factor(k1, k2, T1, T2, R_res, e_t, S, huber=0.0):
    """A relative-pose block between k1 and k2 whose residual is (e_t, log R_res): R_ref = R_res (R_1 R_2^T)^T."""
    t1, R1 = np.asarray(T1[:3], LD), np.asarray(T1[3:], LD).reshape(3, 3)
    t2, R2 = np.asarray(T2[:3], LD), np.asarray(T2[3:], LD).reshape(3, 3)
    R12 = R1 @ R2.T
    Rr = np.asarray(_f64(np.asarray(R_res, LD) @ R12.T), LD)
    return dict(pose=k1, pose2=k2, type=2, data=_pose(np.asarray(e_t, LD) - Rr @ (t1 - R12 @ t2), Rr), stiffness=np.asarray(S).ravel(),
                huber=huber)


def direction(zen, az):
    """Unit vector with zenith acos(-y) = zen and azimuth atan2(x, z) = az (long double)."""
    zen, az = LD(zen), LD(az)
    return np.array([np.sin(zen) * np.sin(az), -np.cos(zen), np.sin(zen) * np.cos(az)], dtype=LD)


def sun_factor(k, T, s_c, o_c, S, taz=1000.0, tzen=1000.0, huber=0.0, scales=(2.7, 0.31)):
    """A sun block on pose k with R e_g = s_c and the observed direction o_c, both handed over unnormalised."""
    R = np.asarray(T[3:], LD).reshape(3, 3)
    return dict(pose=k, type=1, data=np.concatenate([_f64(scales[0] * np.asarray(o_c, LD)), _f64(scales[1] * (R.T @ np.asarray(s_c, LD))), [taz, tzen]]),
                stiffness=np.asarray(S).ravel(), huber=huber)


def _with_huber(poses, fct, rel, side):
    """`fct` with a Huber width a such that |r|^2 = a^2 (1 + side rel) in long double."""
    f0 = dict(fct, huber=0.0)
    sq = hp.pose_factor_rows(poses, [f0], mags=False)[0]["sq"]
    return dict(fct, huber=float(np.sqrt(sq / (1 + LD(side) * LD(rel)))), edge=("huber", rel, side))


# ------------------------------------------------------------------------------------------------------------------- batches
def _angle_rows(rng, relative):
    """(pose or pair of poses, R_res, e_t, tag) for every residual angle: exact rotations up to EXACT_BELOW, generic ones from
    GENERIC_FROM (two draws)."""
    out = []
    for tag, th in ANGLES:
        n = rng.normal(size=3)
        kinds = (["exact"] if float(th) <= EXACT_BELOW else []) + (["generic", "generic"] if float(th) >= GENERIC_FROM else [])
        for kind in kinds:
            if kind == "exact":
                P = _PERMS[rng.integers(1, 4)] if relative else np.eye(3)
                Ts = [_pose(_far(rng), P), _pose(np.zeros(3), P)]
            else:
                Ts = [_pose(_far(rng), _generic_rotation(rng)), _pose(np.zeros(3), _generic_rotation(rng))]
            Ts[1][:3] = Ts[0][:3] + rng.normal(size=3)          # the neighbour of an odometry block: a unit or two away
            out.append((Ts, exp_ld(th, n), rng.normal(size=3) * 0.05, (tag, kind)))
    return out


def _near_poses(rng):
    T1 = _pose(rng.normal(size=3) * 0.3, _generic_rotation(rng))
    return [T1, _pose(T1[:3] + rng.normal(size=3) * 0.3, _generic_rotation(rng))]


def _prior_batch(rng):
    poses, factors = [], []
    for Ts, Rres, e_t, tag in _angle_rows(rng, False):
        factors.append(dict(prior_factor(len(poses), Ts[0], Rres, e_t, full_stiffness(rng), exact=tag[1] == "exact"), edge=("angle",) + tag))
        poses.append(Ts[0])
    for rel in HUBER_DISTANCES:
        for side in (-1, 1):
            T = _near_poses(rng)[0]
            f = prior_factor(len(poses), T, exp_ld(0.05, rng.normal(size=3)), rng.normal(size=3) + 2.0, np.diag([3.0] * 3 + [1.0] * 3) + 0.05)
            poses.append(T)
            factors.append(_with_huber(np.asarray(poses), f, rel, side))
    for a in (0.01, 5.0):        # Huber far inside and far outside on generic rows
        T = _pose(_far(rng), _generic_rotation(rng))
        factors.append(dict(prior_factor(len(poses), T, exp_ld(0.3, rng.normal(size=3)), rng.normal(size=3) * 0.2, full_stiffness(rng), huber=a),
                            edge=("generic", a)))
        poses.append(T)
    return np.asarray(poses), factors


def _relative_batch(rng, rows):
    poses, factors = [], []
    for Ts, Rres, e_t, tag in rows:
        k = len(poses)
        factors.append(dict(relative_factor(k, k + 1, Ts[0], Ts[1], Rres, e_t, full_stiffness(rng)), edge=("angle",) + tag))
        poses += Ts
    return np.asarray(poses), factors


def _relative_huber_batch(rng):
    poses, factors = [], []
    for rel in HUBER_DISTANCES:
        for side in (-1, 1):
            Ts = _near_poses(rng)
            k = len(poses)
            poses += Ts
            f = relative_factor(k, k + 1, Ts[0], Ts[1], exp_ld(0.05, rng.normal(size=3)), rng.normal(size=3) + 2.0, np.diag([3.0] * 3 + [1.0] * 3) + 0.05)
            factors.append(_with_huber(np.asarray(poses), f, rel, side))
    for a in (0.01, 5.0, 0.0, 0.0):
        Ts = _angle_rows(rng, True)[-1][0]
        k = len(poses)
        poses += Ts
        factors.append(dict(relative_factor(k, k + 1, Ts[0], Ts[1], exp_ld(0.3, rng.normal(size=3)), rng.normal(size=3) * 0.2, full_stiffness(rng), huber=a),
                            edge=("generic", a)))
    return np.asarray(poses), factors


def _sun_batch(rng):
    poses, factors = [], []

    def add(s_c, o_c, edge, exact=False, near=False, **kw):
        T = _pose(rng.normal(size=3) * 0.3 if near else _far(rng), np.eye(3) if exact else _generic_rotation(rng))
        poses.append(T)
        factors.append(dict(sun_factor(len(poses) - 1, T, s_c, o_c, full_stiffness(rng, 2), **kw), edge=edge))
        return factors[-1]

    for eps in (1e-4, 1e-8, 1e-12, 5e-13):          # s_c[1] = +-(1 - eps): x^2 + z^2 = 2 eps down to 1e-12
        for sign in (1, -1):
            for exact in (False, True):
                az = rng.uniform(-3, 3)
                y = LD(sign) * (1 - LD(eps))
                h = np.sqrt((1 - y) * (1 + y))
                s_c = np.array([h * np.sin(LD(az)), y, h * np.cos(LD(az))], dtype=LD)
                zen = np.arccos(-y)
                add(s_c, direction(zen + (0.01 if sign > 0 else -0.01), az + 0.02), ("zenith", eps, sign), exact=exact)
    for d in (1e-6, 1e-10):                          # the azimuth residual on either side of +pi and of -pi
        for at in (1, -1):
            for side in (1, -1):
                eaz = LD(2.0 * at)
                oaz = eaz - at * (PI_LD + LD(side) * LD(d))
                add(direction(1.1, eaz), direction(1.13, oaz), ("wrap", d, at, side))
    for zero_az, zero_zen in ((1, 0), (0, 1), (1, 1), (0, 0)):       # |raz|, |rzen| within 1e-9 of their thresholds
        for _ in range(2):
            zen, az = rng.uniform(0.6, 2.4), rng.uniform(-2.5, 2.5)
            f = add(direction(zen, az), direction(zen + 0.03 * rng.choice([-1, 1]), az + 0.05 * rng.choice([-1, 1])), ("threshold", zero_az, zero_zen))
            g = hp.pose_factor_rows(np.asarray(poses), [f], mags=False)[0]["guards"]
            f["data"][6] = float(abs(g["raz_wrapped"]) * (1 + LD(THRESHOLD_DISTANCE) * (-1 if zero_az else 1)))
            f["data"][7] = float(abs(g["rzen"]) * (1 + LD(THRESHOLD_DISTANCE) * (-1 if zero_zen else 1)))
    for rel in HUBER_DISTANCES:
        for side in (-1, 1):
            f = add(direction(1.2, 0.4), direction(0.7, -0.6), None, near=True)
            factors[-1] = _with_huber(np.asarray(poses), f, rel, side)
    for a in (0.01, 500.0, 0.0, 0.0):
        zen, az = rng.uniform(0.6, 2.4), rng.uniform(-2.5, 2.5)
        add(direction(zen, az), direction(zen + rng.normal() * 0.02, az + rng.normal() * 0.02), ("generic", a), huber=a)
    return np.asarray(poses), factors


@functools.lru_cache(maxsize=None)
def batches():
    rng = np.random.default_rng(20)
    rows = _angle_rows(rng, True)
    small = [float(dict(ANGLES)[row[3][0]]) < 1e-4 for row in rows]      # relative_a: up to the series branch, relative_b: beyond it
    out = {"prior": _prior_batch(rng), "sun": _sun_batch(rng), "relative_a": _relative_batch(rng, [r for r, s in zip(rows, small) if s]),
           "relative_b": _relative_batch(rng, [r for r, s in zip(rows, small) if not s]), "relative_huber": _relative_huber_batch(rng)}
    for name, (poses, factors) in out.items():
        assert len(factors) <= 64 and poses.shape[0] <= 64, name
        touched = [k for f in factors for k in ([f["pose"]] + ([f["pose2"]] if f["type"] == 2 else []))]
        assert sorted(touched) == list(range(poses.shape[0])), name
    return out


@functools.lru_cache(maxsize=None)
def truth(name):
    """The long-double rows of a batch with their magnitudes (computed once, shared, never modified)."""
    poses, factors = batches()[name]
    return hp.pose_factor_rows(poses, factors)


# ------------------------------------------------------------------------------------------------------------- the edges held
def _clear(value, guard, mag):
    """|value - guard| beyond the bar of value."""
    return abs(float(LD(value) - LD(guard))) > hp.C_ROW * hp.U * float(mag)


def assert_edges(name, poses, factors, rows):
    assert len(rows) == len(factors) and all(r is not None for r in rows)      # no row left out
    edges = [f["edge"] for f in factors]
    for f, r, e in zip(factors, rows, edges):
        a = f.get("huber", 0.0)
        if a > 0:
            assert _clear(r["sq"], LD(a) * LD(a), r["mag_sq"]), (name, e, float(r["sq"]), a * a, r["mag_sq"])
        if f["type"] != 1:
            assert _clear(r["guards"]["angle"], EPS, r["mag_guards"]["angle"]), (name, e)
        else:
            g, m = r["guards"], r["mag_guards"]
            for gd in (np.pi, -np.pi):
                assert _clear(g["raz"], gd, m["raz"]), (name, e)
            assert _clear(abs(g["raz_wrapped"]), f["data"][6], m["raz_wrapped"]), (name, e)
            assert _clear(abs(g["rzen"]), f["data"][7], m["rzen"]), (name, e)
    if name in ("prior", "relative_a", "relative_b"):
        ang = {e[1:]: float(r["guards"]["angle"]) for e, r in zip(edges, rows) if e[0] == "angle"}
        for (tag, kind), v in ang.items():
            th = float(dict(ANGLES)[tag])
            if kind == "exact" or th >= 1e-8:
                assert abs(v - th) <= 1e-7 * th + 4e-16 * (th > 1), (name, tag, kind, v)
        if name != "relative_b":
            for tag in ("0", "1e-17", "1e-16", "2e-16"):
                assert ang[(tag, "exact")] <= EPS
            for tag in ("2.5e-16", "1e-15", "1e-12"):
                assert ang[(tag, "exact")] > EPS
        if name != "relative_a":
            for tag in ("pi-1e-2", "pi-1e-4", "pi-1e-6", "pi-1e-8"):
                assert 0 < float(PI_LD - LD(ang[(tag, "generic")])) < 1.1 * float(PI_LD - dict(ANGLES)[tag])
        if name != "relative_b":
            assert 0 < ang[("9e-6", "generic")] < 1e-5 < ang[("1.1e-5", "generic")]
    hub = {e[1:]: r["outlier"] for e, r in zip(edges, rows) if e and e[0] == "huber"}
    if name in ("prior", "sun", "relative_huber"):
        assert hub == {(rel, side): side > 0 for rel in HUBER_DISTANCES for side in (-1, 1)}, hub
    if name == "sun":
        wraps = {e[1:]: float(LD(r["guards"]["raz"]) - LD(at * np.pi)) * at for e, r in zip(edges, rows) if e and e[0] == "wrap" for at in [e[2]]}
        for (d, at, side), v in wraps.items():
            assert side * v > 0 and abs(abs(v) - d) < 1e-3 * d + 2e-15, (d, at, side, v)
        assert len(wraps) == 8
        zeroed = set()
        for f, r, e in zip(factors, rows, edges):
            if e and e[0] == "threshold":
                z = (abs(r["guards"]["raz_wrapped"]) > f["data"][6], abs(r["guards"]["rzen"]) > f["data"][7])
                assert z == (bool(e[1]), bool(e[2]))
                for v, t in ((r["guards"]["raz_wrapped"], f["data"][6]), (r["guards"]["rzen"], f["data"][7])):
                    assert abs(abs(float(v)) / t - 1) < 1.01 * THRESHOLD_DISTANCE
                zeroed.add(z)
        assert zeroed == {(True, False), (False, True), (True, True), (False, False)}
        seen = set()
        for f, e in zip(factors, edges):
            if e and e[0] == "zenith":
                eg = np.asarray(f["data"][3:6], LD)
                s_c = np.asarray(poses[f["pose"]][3:], LD).reshape(3, 3) @ (eg / np.sqrt((eg * eg).sum()))
                assert abs(float((1 - e[2] * s_c[1]) / LD(e[1])) - 1) < 1e-3 and abs(float((s_c[0] ** 2 + s_c[2] ** 2) / (2 * LD(e[1]))) - 1) < 1e-3, e
                seen.add(e[1:])
        assert seen == {(eps, s) for eps in (1e-4, 1e-8, 1e-12, 5e-13) for s in (1, -1)}
