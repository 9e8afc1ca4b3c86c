"""ssba_covariance_blocks: any (pose | point, pose | point) block of (J^T J)^-1 in one call, against a long-double truth.

Truth never comes from the device: the Jacobian rows are hp_reference.stereo_rows in long double, inverses are refined
solves (hp_reference.refined_solve: fp64 Cholesky + long-double residuals).  The tiny case inverts the full normal
matrix over poses AND points (no Schur formula); the others solve the reduced system for the pose columns and apply the
landmark formula  Sigma_ll = V^-1 + V^-1 W^T Sigma_TT W V^-1,  Sigma_il = -Sigma_iT W V^-1  in long double.
"""
import os
import subprocess
import time

import numpy as np
import pytest

import hp_reference as hp
from ceres_slam_amd import capi, synth
from ceres_slam_amd.solver import StereoBA

pytestmark = pytest.mark.gpu
LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Truth:
    """Long-double reference of one handle at its current parameters."""

    def __init__(self, ba, prob, stiffness, pose_const, huber=0.0, full=False, S=None):
        P, L = ba.poses.shape[0], ba.points.shape[0]
        self.rows = rows = hp.stereo_rows(prob.camera, ba.poses, ba.points, prob.obs_pose, prob.obs_point, prob.obs_uvd,
                                          stiffness, huber)
        self.fidx = fidx = hp.free_index(P, prob.obs_pose, pose_const)
        nf = int((fidx >= 0).sum())
        k, j = np.asarray(prob.obs_pose, np.int64), np.asarray(prob.obs_point, np.int64)
        f = fidx[k]
        Jp, Jl = rows["Jp"], rows["Jl"]
        W = np.einsum("nai,naj->nij", Jp, Jl)                   # (N, 6, 3)
        V = np.zeros((L, 3, 3), LD)
        np.add.at(V, j, np.einsum("nai,naj->nij", Jl, Jl))
        self.V = V
        self.kappa_V = np.array([np.linalg.cond(np.asarray(v, np.float64)) if np.abs(np.asarray(v, np.float64)).max() > 0 else np.inf
                                 for v in V])
        self.Vi = np.array([np.asarray(np.linalg.inv(np.asarray(v, np.float64)), LD) for v in V])
        # refine V^-1 once in long double (V is 3 x 3: one Newton step X <- X (2I - V X))
        self.Vi = np.array([x @ (2 * np.eye(3, dtype=LD) - v @ x) for v, x in zip(V, self.Vi)])
        self.obs_of = [[] for _ in range(L)]
        for n in range(k.shape[0]):
            if f[n] >= 0:
                self.obs_of[j[n]].append(n)
        self.W, self.f = W, f
        n6 = 6 * nf
        Hpp = np.zeros((n6, n6), LD)
        for n in np.nonzero(f >= 0)[0]:
            a = 6 * f[n]
            Hpp[a:a + 6, a:a + 6] += Jp[n].T @ Jp[n]
        if full:
            # the full normal matrix over free poses and points, inverted column by column
            N = n6 + 3 * L
            H = np.zeros((N, N), LD)
            H[:n6, :n6] = Hpp
            for n in np.nonzero(f >= 0)[0]:
                a, b = 6 * f[n], n6 + 3 * j[n]
                H[a:a + 6, b:b + 3] += W[n]
                H[b:b + 3, a:a + 6] += W[n].T
            for l in range(L):
                H[n6 + 3 * l:n6 + 3 * l + 3, n6 + 3 * l:n6 + 3 * l + 3] = V[l]
            self.Hinv = hp.refined_solve(H, np.eye(N))[0]
            self.n6 = n6
            return
        self.Hinv = None
        S = Hpp.copy()
        for l in range(L):
            obs = self.obs_of[l]
            if not obs:
                continue
            Wl = np.zeros((n6, 3), LD)
            for n in obs:
                Wl[6 * f[n]:6 * f[n] + 6] += W[n]
            S -= Wl @ self.Vi[l] @ Wl.T
        self.S = S
        self.Spp = hp.refined_solve(S, np.eye(n6))[0]

    def with_reduced_system(self, S):
        """The same reference with the pose block of the inverse taken from another reduced system (long-double solve)."""
        t = object.__new__(Truth)
        t.__dict__.update(self.__dict__)
        t.S = np.asarray(S, LD)
        t.Spp = hp.refined_solve(t.S, np.eye(S.shape[0]))[0]
        return t

    def pose_pose(self, a, b):
        fa, fb = self.fidx[a], self.fidx[b]
        if fa < 0 or fb < 0:
            return np.zeros((6, 6))
        M = self.Hinv if self.Hinv is not None else self.Spp
        return M[6 * fa:6 * fa + 6, 6 * fb:6 * fb + 6]

    def _wl(self, l):
        n6 = self.Spp.shape[0]
        Wl = np.zeros((n6, 3), LD)
        for n in self.obs_of[l]:
            Wl[6 * self.f[n]:6 * self.f[n] + 6] += self.W[n]
        return Wl

    def point(self, l):
        if self.Hinv is not None:
            b = self.n6 + 3 * l
            return self.Hinv[b:b + 3, b:b + 3]
        Wl, Vi = self._wl(l), self.Vi[l]
        return Vi + Vi @ Wl.T @ self.Spp @ Wl @ Vi

    def pose_point(self, a, l):
        fa = self.fidx[a]
        if fa < 0:
            return np.zeros((6, 3))
        if self.Hinv is not None:
            b = self.n6 + 3 * l
            return self.Hinv[6 * fa:6 * fa + 6, b:b + 3]
        return -self.Spp[6 * fa:6 * fa + 6] @ self._wl(l) @ self.Vi[l]


def _rel(a, t):
    t = np.asarray(t, np.float64)
    return float(np.abs(np.asarray(a, np.float64) - t).max() / max(np.abs(t).max(), 1e-300))


def _solved(P, L, track_len=6, seed=3, **kw):
    prob = synth.make_problem(P, L, track_len=track_len, seed=seed)
    ba = StereoBA.from_synth(prob, device=0, **kw)
    ba.solve(capi.default_options(max_num_iterations=50, use_nonmonotonic_steps=1))
    return prob, ba


def _pose_const(P):
    c = np.zeros(P, bool)
    c[0] = True
    return c


def test_tiny_every_block_against_the_full_inverse():
    P, L = 8, 120
    prob, ba = _solved(P, L)
    assert ba.stats().general_structure == 0
    tr = Truth(ba, prob, prob.stiffness(), _pose_const(P), full=True)
    pairs = [(("pose", a), ("pose", b)) for a in range(P) for b in range(P)]
    pairs += [(("point", l), ("point", l)) for l in range(L)]
    pairs += [(("pose", a), ("point", l)) for a in range(P) for l in range(L)]
    out = ba.covariance_blocks(pairs)
    worst = 0.0
    for (a, b), blk in zip(pairs, out):
        if a[0] == "pose" and b[0] == "pose":
            t = tr.pose_pose(a[1], b[1])
        elif a[0] == "point":
            t = tr.point(a[1])
        else:
            t = tr.pose_point(a[1], b[1])
        if a[0] == "pose" and tr.fidx[a[1]] < 0:
            assert not blk.any()
            continue
        if b[0] == "point" and tr.kappa_V[b[1]] > 1e8:
            continue
        worst = max(worst, _rel(blk, t))
    print("tiny: worst relative difference", worst)
    assert worst < 1e-8, worst


def _check_against_schur_truth(tag, ba, prob, stiffness, pose_const, far=True, sample=40):
    P, L = ba.poses.shape[0], ba.points.shape[0]
    tr = Truth(ba, prob, stiffness, pose_const)
    free = [k for k in range(P) if tr.fidx[k] >= 0]
    pairs = [(("pose", k), ("pose", k)) for k in range(P)]
    inpat = [(a, b) for a in free for b in free if a < b and abs(tr.fidx[a] // 12 - tr.fidx[b] // 12) <= 1]
    pairs += [(("pose", a), ("pose", b)) for a, b in inpat]
    if far:
        pairs += [(("pose", free[0]), ("pose", free[-1])), (("pose", free[-1]), ("pose", free[0]))]
    pairs += [(("point", l), ("point", l)) for l in range(L)]
    rng = np.random.default_rng(1)
    pl = [(int(a), int(l)) for a, l in zip(rng.choice(free, sample), rng.integers(0, L, sample))]
    pl += [(free[-1], 0), (free[0], L - 1)]
    pairs += [(("pose", a), ("point", l)) for a, l in pl] + [(("point", l), ("pose", a)) for a, l in pl]
    t0 = time.perf_counter()
    out = ba.covariance_blocks(pairs)
    print(f"{tag}: {len(pairs)} blocks in {1e3 * (time.perf_counter() - t0):.1f} ms")
    good = tr.kappa_V <= 1e8
    assert good.sum() > 0.5 * L, (tag, int(good.sum()), L)
    # the diagonal pose blocks against ssba_pose_covariance, and how far that validated route is from the truth
    e_route = 0.0
    for k in free[:: max(1, len(free) // 6)]:
        pc = ba.pose_covariance(k)
        assert _rel(out[k], pc) <= 1e-9, (tag, k, _rel(out[k], pc))
        e_route = max(e_route, _rel(pc, tr.pose_pose(k, k)))
    # (1) the device's own undamped reduced system, inverted in long double: isolates the selected inversion, the column
    #     sweeps and the landmark kernel from the rounding of the assembly (landmarks nearly unobserved in depth)
    # (2) the truth from the Jacobian rows: no farther than the fp64 route of ssba_pose_covariance is, and 1e-8 when that is
    S_dev = ba.lm_step(1e300)[0]
    for name, ref, bar in (("device S", tr.with_reduced_system(S_dev), 1e-8), ("truth", tr, max(1e-8, 20.0 * e_route))):
        worst = {"pose": 0.0, "point": 0.0, "pose_point": 0.0}
        for (a, b), blk in zip(pairs, out):
            if a[0] == "pose" and b[0] == "pose":
                t, key = ref.pose_pose(a[1], b[1]), "pose"
            elif a[0] == "point" and b[0] == "point":
                if not good[a[1]]:
                    continue
                t, key = ref.point(a[1]), "point"
            elif a[0] == "pose":
                if not good[b[1]]:
                    continue
                t, key = ref.pose_point(a[1], b[1]), "pose_point"
            else:
                if not good[a[1]]:
                    continue
                t, key = ref.pose_point(b[1], a[1]).T, "pose_point"
            if not np.asarray(t, np.float64).any():
                assert not blk.any(), (tag, a, b)
                continue
            worst[key] = max(worst[key], _rel(blk, t))
        print(tag, name, "bar", bar, "pose_covariance to truth", e_route, worst)
        assert max(worst.values()) < bar, (tag, name, bar, worst)
    return out


@pytest.mark.parametrize("P", [30, 100])
def test_windowed_layout_against_the_truth(P):
    prob, ba = _solved(P, 20 * P, track_len=8)
    assert ba.stats().general_structure == 0
    _check_against_schur_truth(f"windowed P={P}", ba, prob, prob.stiffness(), _pose_const(P), sample=60)


def test_general_layout_against_the_truth():
    from test_gpu_general_structure import _per_point_stiffness
    P = 24
    prob = synth.make_problem(P, 20 * P, track_len=6, seed=5)
    S = _per_point_stiffness(prob, seed=3)
    ba = StereoBA(prob.camera, prob.poses_init.copy(), prob.points_init.copy(), prob.obs_pose, prob.obs_point, prob.obs_uvd, S, device=0)
    assert ba.stats().general_structure == 1
    ba.solve(capi.default_options(max_num_iterations=50, use_nonmonotonic_steps=1))
    _check_against_schur_truth("general P=24", ba, prob, S, _pose_const(P))


def test_wide_handle_goes_to_the_general_layout():
    P = 40
    prob = synth.make_problem(P, 20 * P, track_len=16, seed=2)
    ba = StereoBA.from_synth(prob, device=0)
    assert ba.stats().wide_superblocks > 0
    _check_against_schur_truth("wide P=40", ba, prob, prob.stiffness(), _pose_const(P))
    assert ba.stats().general_structure == 1


# ------------------------------------------------------------------------------------------------------------ semantics
def test_semantics():
    P, L = 30, 600
    prob, ba = _solved(P, L)
    # constant pose (pose 0) -> zeros; (b, a) is the transpose of (a, b), bit for bit
    out = ba.covariance_blocks([(("pose", 0), ("pose", 3)), (("pose", 0), ("point", 5)), (("point", 5), ("pose", 0)),
                                (("pose", 2), ("pose", 29)), (("pose", 29), ("pose", 2)), (("pose", 4), ("pose", 7)),
                                (("pose", 7), ("pose", 4)), (("pose", 9), ("point", 180)), (("point", 180), ("pose", 9))])
    assert out[0].shape == (6, 6) and not out[0].any()
    assert out[1].shape == (6, 3) and not out[1].any() and out[2].shape == (3, 6) and not out[2].any()
    assert np.array_equal(out[3], out[4].T) and out[3].any()
    assert np.array_equal(out[5], out[6].T)
    assert np.array_equal(out[7], out[8].T) and out[7].any()
    # bad arguments
    for pairs, status in [([(("pose", P), ("pose", 0))], -1), ([(("point", L), ("point", L))], -1), ([(("point", 1), ("point", 2))], -6)]:
        with pytest.raises(capi.SsbaError) as e:
            ba.covariance_blocks(pairs)
        assert e.value.status == status
    req = (capi.CovBlock * 1)(capi.CovBlock(7, 0, 0, 0))
    o = np.zeros(36)
    assert ba.lib.ssba_covariance_blocks(ba.h, req, 1, capi.dptr(o)) == -1
    req = (capi.CovBlock * 1)(capi.CovBlock(1, 1, 1, 2))
    assert ba.lib.ssba_covariance_blocks(ba.h, req, 1, capi.dptr(o)) == -6


def test_lighting_terms_are_unsupported():
    # (constant point blocks exist only together with lighting terms, so their zero blocks are never reached here)
    prob, ph = synth.make_phong_problem(8, 60, track_len=5, seed=7)
    ba = StereoBA.from_synth(prob, lighting=ph.as_oracle_dict("truth"), device=0)
    with pytest.raises(capi.SsbaError) as e:
        ba.covariance_blocks([(("pose", 3), ("point", 1))])
    assert e.value.status == -6


def test_rank_deficient_problem_fails():
    P, L = 12, 240
    prob = synth.make_problem(P, L, track_len=6, seed=3)
    ba = StereoBA.from_synth(prob, device=0, pose_const=np.zeros(P, dtype=np.uint8))
    o = np.zeros(9)
    req = (capi.CovBlock * 1)(capi.CovBlock(1, 4, 1, 4))
    assert ba.lib.ssba_covariance_blocks(ba.h, req, 1, capi.dptr(o)) == -3


def test_a_later_solve_is_unchanged():
    P, L = 30, 600
    runs = []
    for ask in (False, True):
        prob = synth.make_problem(P, L, track_len=8, seed=6)
        ba = StereoBA.from_synth(prob, device=0)
        o = capi.default_options(max_num_iterations=3, use_nonmonotonic_steps=1)
        ba.solve(o)
        if ask:
            ba.pose_marginals()
            ba.point_marginals()
        s, log = ba.solve(capi.default_options(max_num_iterations=50, use_nonmonotonic_steps=1))
        runs.append((s.num_iterations, s.final_cost, {k: np.asarray(v).copy() for k, v in log.items()}, ba.poses.copy(), ba.points.copy()))
    a, b = runs
    assert a[0] == b[0] and a[1] == b[1]
    for k in a[2]:
        assert np.array_equal(a[2][k], b[2][k]), k
    assert np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])


def test_bit_reproducible():
    prob, ba = _solved(30, 600)
    a, b = ba.point_marginals(), ba.point_marginals()
    assert np.array_equal(a, b)
    assert np.array_equal(ba.pose_marginals(), ba.pose_marginals())


# ------------------------------------------------------------------------------------------------------------ C2 full size
def test_c2_every_marginal_in_one_call():
    prob = synth.make_problem(1000, 100_000, track_len=12, seed=42)
    ba = StereoBA.from_synth(prob, device=0)
    ba.solve(capi.default_options(max_num_iterations=10, use_nonmonotonic_steps=1))
    P, L = 1000, ba.points.shape[0]
    pairs = [(("pose", k), ("pose", k)) for k in range(P)] + [(("point", l), ("point", l)) for l in range(L)]
    ba.covariance_blocks(pairs[:10])          # warm-up
    t0 = time.perf_counter()
    out = ba.covariance_blocks(pairs)
    print(f"C2: {len(pairs)} marginals in {1e3 * (time.perf_counter() - t0):.1f} ms")
    poses = np.array(out[:P])
    pts = np.array(out[P:])
    assert np.isfinite(poses).all() and np.isfinite(pts).all()
    assert np.array_equal(poses, poses.transpose(0, 2, 1)) and np.array_equal(pts, pts.transpose(0, 2, 1))
    for k in range(1, P, 50):
        assert _rel(poses[k], ba.pose_covariance(k)) <= 1e-9, k


# ------------------------------------------------------------------------------------------------------------ shim
def test_python_shim_landmark_and_off_diagonal_blocks():
    from ceres_slam_amd import ceres_api as ceres
    P, L = 16, 300
    prob, ba = _solved(P, L)
    problem = ceres.Problem()
    cam = ceres.StereoCamera(**prob.camera)
    poses = [ba.poses[k].copy() for k in range(P)]
    points = [ba.points[j].copy() for j in range(L)]
    S = prob.stiffness()
    for n in range(prob.obs_pose.shape[0]):
        cost = ceres.StereoReprojectionErrorAutomatic.Create(cam, prob.obs_uvd[n], S)
        problem.AddResidualBlock(cost, None, poses[prob.obs_pose[n]], points[prob.obs_point[n]])
    for k in range(P):
        problem.SetParameterization(poses[k], ceres.SE3Perturbation.Create())
    problem.SetParameterBlockConstant(poses[0])
    cov = ceres.Covariance()
    blocks = [(poses[3], poses[3]), (points[7], points[7]), (poses[4], points[7]), (poses[2], poses[9])]
    assert cov.Compute(blocks, problem), cov.message
    ref = ba.covariance_blocks([(("pose", 3), ("pose", 3)), (("point", 7), ("point", 7)), (("pose", 4), ("point", 7)),
                                (("pose", 2), ("pose", 9))])
    o66, o33, o63, o36 = np.zeros(36), np.zeros(9), np.zeros(18), np.zeros(18)
    assert cov.GetCovarianceBlockInTangentSpace(poses[3], poses[3], o66)
    np.testing.assert_allclose(o66.reshape(6, 6), ref[0], rtol=1e-9, atol=1e-12 * np.abs(ref[0]).max())
    assert cov.GetCovarianceBlock(points[7], points[7], o33)
    np.testing.assert_allclose(o33.reshape(3, 3), ref[1], rtol=1e-9, atol=1e-12 * np.abs(ref[1]).max())
    assert cov.GetCovarianceBlockInTangentSpace(points[7], poses[4], o36)
    np.testing.assert_allclose(o36.reshape(3, 6), ref[2].T, rtol=1e-9, atol=1e-12 * np.abs(ref[2]).max())
    assert not cov.GetCovarianceBlock(poses[2], poses[9], np.zeros(144))
    # diagonal pose blocks only: still ssba_pose_covariance, bit for bit
    cov2 = ceres.Covariance()
    assert cov2.Compute([(poses[5], poses[5])], problem)
    assert cov2.GetCovarianceBlockInTangentSpace(poses[5], poses[5], o66)
    h = ba.pose_covariance(5)
    np.testing.assert_allclose(o66.reshape(6, 6), h, rtol=1e-9, atol=1e-12 * np.abs(h).max())


def test_cpp_example_blocks_match_the_c_abi():
    from ceres_slam_amd import build
    exe = build.build_examples("covariance_blocks_gpu")
    r = subprocess.run([exe, "16", "200"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    lines = [ln.split() for ln in r.stdout.decode().splitlines()]
    P, L, N = (int(x) for x in lines[0][1:])
    poses = np.zeros((P, 12)); points = np.zeros((L, 3)); ok, oj, uvd = [], [], []
    cp, cpt, cpp = {}, {}, {}
    for w in lines[1:]:
        if w[0] == "pose":
            poses[int(w[1])] = [float(x) for x in w[2:]]
        elif w[0] == "point":
            points[int(w[1])] = [float(x) for x in w[2:]]
        elif w[0] == "obs":
            ok.append(int(w[1])); oj.append(int(w[2])); uvd.append([float(x) for x in w[3:]])
        elif w[0] == "cov_pose":
            cp[int(w[1])] = np.array([float(x) for x in w[2:]]).reshape(6, 6)
        elif w[0] == "cov_point":
            cpt[int(w[1])] = np.array([float(x) for x in w[2:]]).reshape(3, 3)
        elif w[0] == "cov_pose_point":
            cpp[(int(w[1]), int(w[2]))] = np.array([float(x) for x in w[3:]]).reshape(6, 3)
    assert len(ok) == N and len(cp) == P and cpt and cpp
    cam = dict(fu=400.0, fv=400.0, cu=320.0, cv=240.0, b=0.24)
    const = np.zeros(P, dtype=np.uint8); const[0] = 1
    ba = StereoBA(cam, poses, points, np.array(ok), np.array(oj), np.array(uvd), np.eye(3), pose_const=const, device=0)
    pairs = [(("pose", k), ("pose", k)) for k in range(P)]
    (j,) = cpt.keys()
    ((k, j2),) = cpp.keys()
    pairs += [(("point", j), ("point", j)), (("pose", k), ("point", j2))]
    ref = ba.covariance_blocks(pairs)
    assert not cp[0].any()
    for kk in range(1, P):
        assert _rel(cp[kk], ref[kk]) <= 1e-9, kk
    assert _rel(cpt[j], ref[P]) <= 1e-9
    assert _rel(cpp[(k, j2)], ref[P + 1]) <= 1e-9
