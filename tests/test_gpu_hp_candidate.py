"""The second half of a trust-region iteration -- everything after the step exists -- against the long-double references of
tests/hp_reference.py (se3_plus, unit_plus, projected_plus, cost_at, gradient_max_norm, block_norms, trust_region_decision).

Every case drives one iteration of a real solve (solve_begin at initial_trust_region_radius = r with max_num_iterations = 1,
step(2), solve_end), reads the iteration log and the written-back blocks, and takes the step itself from the existing hooks at
the same (r, mu = 1e-8) on a second handle at the same point: ssba_lm_step / ssba_border_system, ssba_dogleg_step.  Checked,
each as a ratio <= 1 to a derived bar (printed in the CANDREF lines under -s):

1. log row 0: cost against cost_at(x), gradient_max_norm against the reference, ssba_evaluate's cost bit-equal to row 0;
2. an accepted step's written-back point: poses within the Plus bar of se3_plus(x, delta_dev), points within 1 u (plus 2 u
   |delta| for the dogleg's beta gn + gamma v; ssba_lm_step without lighting terms reports delta_l as candidate - p, which is
   exact for a small step: there the ratio is 0 and says only that the solve and the hook formed the same candidate -- the
   dogleg and lighting hooks report the step itself), normals and shared blocks within their bars; constant poses, unobserved
   landmarks and constant shared blocks bit-identical to the input; |R^T R - I| within its start value plus 6 Plus bars;
3. its cost (row 1) against cost_at at the device's own written-back fp64 point (no propagation term);
4. a rejected step's cost: the same start and radius with min_relative_decrease = -1e300 and ignore_convergence accepts the
   identical candidate, whose cost row 1 then comes from the linearisation pass instead of the evaluation pass: the two agree
   within the sum of their bars.  ssba_solve_end hands back the LOWEST-COST iterate, which after a cost increase is the start:
   the rejected candidate is never written back.  So both rows are also held against cost_at(Plus(x, delta_dev)) in long
   double with the Plus bar propagated through |r|^T |d r / d q| (|dR| |p| + |dt| + |R| |dp|);
5. step_norm (row 1) against |Plus(x, delta_dev) - x|_2 over all moved blocks, bar absolute in u |x| per entry;
6. cost_change, relative_decrease, step_is_successful and trust_region_radius of row 1 against trust_region_decision fed with
   the truth values and the hook's model cost change: rho within the bar propagated from the two cost bars; the flag and a
   dogleg radius equal, an LM radius within its propagated bar.  Before the solve under test runs, the same decision is made
   from the reference's OWN step (the refined long-double solve) and every comparison in it must be more than 4 propagated
   bars from its threshold -- no committed case may sit where fp64 could decide either way;
7. (second=True) after an accepted step, step(3) with max_num_iterations = 2: row 2's step_norm against the norm of a fresh
   hook step on a new handle at the written-back point with the radius the reference predicts (and mu = 1e-8) -- the radius,
   mu and decrease_factor that decide_body wrote are the ones the next iteration used.

The tolerance thresholds (function, parameter -- the only place x_norm is visible --, gradient, min_relative_decrease) are
reached from both sides with the option at v (1 +- 2^-20), v the truth value of the left-hand side, after asserting that
2^-20 v exceeds four times the propagated bar of v.

Further cases: bounds on the Phong and texture blocks with the full step passing the projected Armijo search at alpha = 1 and
one entry projected onto its bound; a pose-graph-only problem with a prior exactly on its pose (the first-order branch of
se3_plus); one C2-sized LM iteration, rejected and accepted.

A projected line search that contracts is in tests/test_gpu_hp_linesearch.py, which drives candidate_case with the step the
search accepted (line_search=).  Not compared here: LM landmark steps other than through the cost and rho
(see 2.)."""
import numpy as np
import pytest

import hp_reference as hp
from ceres_slam_amd import capi, synth
from ceres_slam_amd.solver import StereoBA
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

U, LD = hp.U, hp.LD
WORST = {}


def _report(tag, **kv):
    print("CANDREF", tag, " ".join(f"{k}={v:.3g}" if isinstance(v, float) else f"{k}={v}" for k, v in kv.items()))
    for k, v in kv.items():
        if isinstance(v, float) and k.startswith("r_"):
            WORST[k] = max(WORST.get(k, 0.0), v)


@pytest.fixture(scope="module", autouse=True)
def _worst_ratios():
    """Prints the worst ratio per quantity over the cases that ran (the figures quoted in DESIGN.md) when the module ends."""
    yield
    print("\nCANDREF worst", " ".join(f"{k}={v:.3g}" for k, v in sorted(WORST.items())))


f64 = lambda v: np.asarray(v, np.float64)


class Spec:
    """A problem without its point: observations, constants, loss, pose factors, lighting data."""

    def __init__(self, prob, obs=None, const=None, huber=0.0, factors=None, lighting=None, shared_free=0, use_bounds=False):
        self.cam, self.P, self.L = prob.camera, prob.num_poses, prob.num_points
        self.obs = obs if obs is not None else (prob.obs_pose, prob.obs_point, prob.obs_uvd)
        self.S = prob.stiffness()
        if const is None:
            const = np.zeros(self.P, bool)
            const[0] = True
        self.const, self.huber, self.factors, self.lighting, self.shared_free = np.asarray(const, bool), huber, factors, lighting, shared_free
        seen = np.bincount(np.asarray(self.obs[0], np.int64), minlength=self.P) > 0
        for fct in factors or []:
            seen[fct["pose"]] = True
            if "pose2" in fct:
                seen[fct["pose2"]] = True
        self.fidx = np.full(self.P, -1, np.int64)
        free = seen & ~self.const
        self.fidx[free] = np.arange(int(free.sum()))
        self.present = np.unique(np.asarray(self.obs[1], np.int64))
        # the driver's bounds on every material: ka, ks in [0, 1], alpha >= 1, kd in [0, 1]
        self.bounds = ([0.0, 0.0, 1.0, 0.0], [1.0, 1.0, np.inf, 1.0]) if use_bounds else None

    def start(self, prob):
        x = dict(poses=prob.poses_init.copy(), points=prob.points_init.copy())
        if self.lighting is not None:
            for k in ("normals", "light", "phong", "texture"):
                x[k] = np.array(self.lighting[k], np.float64)
        return x

    def lighting_at(self, x):
        if self.lighting is None:
            return None
        d = dict(self.lighting)
        for k in ("normals", "light", "phong", "texture"):
            d[k] = x[k]
        return d

    def handle(self, x):
        d = self.lighting_at(x)
        if d is not None:
            d = {k: (f64(v) if k in ("normals", "light", "phong", "texture") else v) for k, v in d.items()}
        return StereoBA(self.cam, f64(x["poses"]).copy(), f64(x["points"]).copy(), *self.obs, self.S, pose_const=self.const,
                        huber_a=self.huber, pose_factors=self.factors, lighting=d, shared_free=self.shared_free,
                        use_bounds=self.bounds is not None)

    def written_back(self, ba):
        x = dict(poses=ba.poses.copy(), points=ba.points.copy())
        if self.lighting is not None:
            x.update(normals=ba.normals.copy(), light=ba.light.copy(), phong=ba.phong.copy(), texture=ba.texture.copy())
        return x

    def remember(self, x):
        """cost(x) and reference(x, mu) of this very object are computed once from now on (the start of a case that several
        comparisons share; the point must not be modified)."""
        self._at, self._memo = x, {}

    def _remembered(self, x, key, make):
        if getattr(self, "_at", None) is not x:
            return make()
        if key not in self._memo:
            self._memo[key] = make()
        return self._memo[key]

    def cost(self, x, jacobians=True, rows=None):
        if rows is None:
            return self._remembered(x, ("cost", jacobians), lambda: self._cost(x, jacobians, None))
        return self._cost(x, jacobians, rows)

    def _cost(self, x, jacobians, rows):
        return hp.cost_at(self.cam, x["poses"], x["points"], *self.obs, self.S, huber_a=self.huber, factors=self.factors,
                          lighting=self.lighting_at(x), jacobians=jacobians, rows=rows)

    def shared(self, x):
        if not self.shared_free:
            return None
        return dict(light_type=self.lighting["light_type"], light=x["light"], phong=x["phong"], texture=x["texture"],
                    shared_free=self.shared_free, bounds=self.bounds)

    def rows(self, x, reuse=None):
        """The long-double rows at x (with the border columns of the free shared blocks).  reuse: rows of the same point
        (cost(x)["rows"]), whose lighting part is taken over."""
        if self.lighting is not None:
            return hp.phong_observation_rows(self.cam, x["poses"], x["points"], x["normals"], *self.obs, self.S, self.lighting_at(x),
                                             self.huber, self.shared_free, phong=None if reuse is None else reuse["phong"])
        return hp.stereo_rows(self.cam, x["poses"], x["points"], *self.obs, self.S, self.huber)

    def reference(self, x, mu, rows=None):
        return self._remembered(x, ("reference", mu), lambda: self._reference(x, mu, rows))

    def _reference(self, x, mu, rows=None):
        """DoglegReference at x (its gradient, and the step of the system damped at radius 1 / mu)."""
        if self.lighting is not None:
            rows = hp.phong_observation_rows(self.cam, x["poses"], x["points"], x["normals"], *self.obs, self.S, self.lighting_at(x),
                                             self.huber, self.shared_free, phong=None if rows is None else rows["phong"])
        elif rows is None:
            rows = hp.stereo_rows(self.cam, x["poses"], x["points"], *self.obs, self.S, self.huber)
        un = hp.unary_rows(f64(x["poses"]), self.factors) if self.factors else None
        return hp.DoglegReference(rows, self.obs[0], self.obs[1], self.fidx, self.L, mu, unary=un), rows

    def shared_vec(self, x):
        if not self.shared_free:
            return None
        parts = [np.asarray(x[k], LD).ravel() for b, k in ((1, "light"), (2, "phong"), (4, "texture")) if self.shared_free & b]
        return np.concatenate(parts)

    def norms(self, x, c=None):
        kw = {}
        if self.lighting is not None:
            kw.update(x_normals=x["normals"], c_normals=None if c is None else c["normals"])
            if self.shared_free:
                kw.update(x_shared=self.shared_vec(x), c_shared=None if c is None else self.shared_vec(c))
        return hp.block_norms(self.fidx, self.present, x["poses"], x["points"], None if c is None else c["poses"],
                              None if c is None else c["points"], **kw)

    def plus(self, x, ref, delta, combo=0.0):
        """Plus(x, delta) in long double over all blocks, and the entrywise bars of an fp64 evaluation.  combo: 2 for a step the
        device forms as beta gn + gamma v (two more roundings, u |delta| each, carried through Plus to first order)."""
        dp, dl, db = ref.split(np.asarray(delta, LD))
        return self.plus_blocks(x, dp, dl, db, combo)

    def plus_blocks(self, x, dp, dl, db, combo=0.0):
        """The same from the blocks: dp of the free poses (nf, 6), dl of the observed landmarks (in index order), db."""
        dp, dl = np.asarray(dp, LD), np.asarray(dl, LD)
        free = np.flatnonzero(self.fidx >= 0)
        c = dict(poses=np.asarray(x["poses"], LD).copy(), points=np.asarray(x["points"], LD).copy())
        bars = dict(poses=np.zeros((self.P, 12)), points=np.zeros((self.L, 3)))
        if free.size:
            c["poses"][free], bars["poses"][free] = hp.se3_plus(np.asarray(x["poses"], LD)[free], dp)
            if combo:
                T = np.abs(f64(x["poses"]))[free]
                e = combo * U * np.abs(f64(dp))
                vn = np.stack([np.sqrt((T[:, :3] ** 2).sum(1))] * 3 + [np.sqrt((T[:, 3:].reshape(-1, 3, 3) ** 2).sum(1))[:, k % 3]
                                                                     for k in range(9)], 1)
                bars["poses"][free] += np.sqrt((e[:, 3:] ** 2).sum(1))[:, None] * vn
                bars["poses"][free, :3] += e[:, :3]
        lm = self.present
        c["points"][lm] = c["points"][lm] + dl[:, :3]
        bars["points"][lm] = U * np.abs(f64(c["points"][lm])) + combo * U * np.abs(f64(dl[:, :3]))
        if self.lighting is not None:
            c["normals"], bars["normals"] = np.asarray(x["normals"], LD).copy(), np.zeros((self.L, 3))
            c["normals"][lm], bars["normals"][lm] = hp.unit_plus(np.asarray(x["normals"], LD)[lm], dl[:, 3:])
            bars["normals"][lm] += combo * U * np.sqrt((f64(dl[:, 3:]) ** 2).sum(1))[:, None]
            (c["light"], c["phong"], c["texture"]), (bars["light"], bars["phong"], bars["texture"]) = hp.projected_plus(
                self.lighting["light_type"], x["light"], x["phong"], x["texture"], db if self.shared_free else np.zeros(0),
                self.shared_free, self.bounds)
            if combo and self.shared_free:
                o = 0
                for b, k in ((1, "light"), (2, "phong"), (4, "texture")):
                    if self.shared_free & b:
                        n = bars[k].size
                        bars[k] = bars[k] + combo * U * (np.abs(f64(db[o: o + n])).reshape(bars[k].shape) if not (b == 1 and self.lighting["light_type"] == 1)
                                                         else float(np.sqrt((f64(db[:3]) ** 2).sum())))
                        o += n
        return c, bars

    def bars_norm(self, bars):
        keys = ["poses", "points"] + (["normals", "light", "phong", "texture"] if self.lighting is not None else [])
        return float(np.sqrt(sum((np.asarray(bars[k]) ** 2).sum() for k in keys)))


def _cost_propagation(spec, cand, cb, bars, asserted=False):
    """|r|^T |d r / d q| (|dR| |p| + |dt| + |R| |dp|) summed over the stereo rows: the effect of entrywise errors `bars` of the
    candidate on its cost (d r / d q = J_l R^T: R is orthonormal).  The lighting and pose-factor rows, the normals and the
    shared blocks are NOT carried: with them the term is understated, so a bar that an asserted ratio rests on
    (asserted=True: the cost of a rejected candidate) is taken only for stereo-only problems; elsewhere it enters margins that
    the committed cases clear by 1e2 and more."""
    assert not asserted or (spec.lighting is None and not spec.factors), "the propagated cost bar covers stereo rows only"
    if not np.asarray(spec.obs[0]).size:
        return 0.0
    rows = cb["rows"]
    k, j = np.asarray(spec.obs[0], np.int64), np.asarray(spec.obs[1], np.int64)
    R = np.abs(f64(cand["poses"]))[k, 3:].reshape(-1, 3, 3)
    A = np.abs(np.einsum("nai,nbi->nab", f64(rows["Jl"])[:, :3, :3], f64(cand["poses"])[k, 3:].reshape(-1, 3, 3)))
    dq = (np.einsum("nij,nj->ni", bars["poses"][k, 3:].reshape(-1, 3, 3), np.abs(f64(cand["points"]))[j]) + bars["poses"][k, :3]
          + np.einsum("nij,nj->ni", R, bars["points"][j]))
    return float((np.abs(f64(rows["r"]))[:, :3] * np.einsum("nab,nb->na", A, dq)).sum())


def _crossings(spec, x, db):
    """Which Phong / texture entries the unprojected x + delta_b leaves the box with (border order: light 3, Phong 3M, textures M)."""
    M = len(x["texture"])
    o = 3 if spec.shared_free & 1 else 0
    v = np.concatenate([np.asarray(x["phong"], LD).ravel(), np.asarray(x["texture"], LD).ravel()]) + np.asarray(db, LD)[o: o + 4 * M]
    lo = np.concatenate([np.tile(spec.bounds[0][:3], M), np.full(M, spec.bounds[0][3])])
    hi = np.concatenate([np.tile(spec.bounds[1][:3], M), np.full(M, spec.bounds[1][3])])
    return np.asarray((v < lo) | (v > hi))


def _options(strategy, dogleg_type, radius, **kw):
    base = dict(trust_region_strategy_type=strategy, dogleg_type=dogleg_type, initial_trust_region_radius=radius, max_num_iterations=1)
    base.update(kw)
    return base


def _hp_options(o):
    keys = ("max_num_iterations", "use_nonmonotonic_steps", "min_relative_decrease", "function_tolerance", "gradient_tolerance",
            "parameter_tolerance", "trust_region_strategy_type")
    return hp.trust_region_options(**{k: o[k] for k in keys if k in o})


def _solve(spec, x, o, steps, ignore=False):
    ba = spec.handle(x)
    ba.solve_begin(capi.default_options(**o), ignore_convergence=ignore)
    ba.step(steps)
    s = ba.solve_end()
    return ba, s, ba.iteration_log()


def _hook_step(spec, x, ref, strategy, dogleg_type, radius):
    """(delta over ref's parameter vector, mcc, |delta|_D or None, combo) from the hooks on a fresh handle at x."""
    ba = spec.handle(x)
    if strategy == 0:
        _, _, dp, dl, mcc = ba.lm_step(radius, want_S=False)
        db = ba.border_system()[3] if spec.shared_free else None
        return ba, ref.pack(dp[spec.fidx >= 0], dl[ref.sy.lm], db), mcc, None, 0.0, (dp, dl)
    st = ba.dogleg_step(radius, 1e-8, capi.default_options(trust_region_strategy_type=1, dogleg_type=dogleg_type))
    dp, dl = st.beta * st.gn_p + st.gamma * st.v_p, st.beta * st.gn_l + st.gamma * st.v_l
    db = st.beta * st.gn_b + st.gamma * st.v_b if spec.shared_free else None
    return ba, ref.pack(dp[spec.fidx >= 0], dl[ref.sy.lm], db), st.mcc, st.step_norm, 2.0, (dp, dl)


def _reference_step(spec, x, ref, rows, strategy, dogleg_type, radius):
    """The reference's own step at (radius, mu = 1e-8): (delta, mcc, its magnitude, |delta|_D)."""
    if strategy == 0:
        ref_r, _ = spec.reference(x, 1.0 / radius, rows)
        delta, _ = ref_r.gauss_newton()
        dl_norm = None
    else:
        gn, _ = ref.gauss_newton()
        sums = list(ref.param_sums(ref.v, gn)[0]) + [ref.row_sums(a, b)[0] for a, b in ((ref.v, ref.v), (gn, gn), (ref.v, gn))]
        sc = hp.dogleg_scalars(sums, radius, dogleg_type)
        delta, dl_norm = sc["beta"] * gn + sc["gamma"] * ref.v, sc["step_norm"]
    mcc, mag = ref.model_cost_change(delta)
    return delta, mcc, mag, dl_norm


def candidate_case(tag, spec, x, strategy, dogleg_type, radius, layout=None, second=False, expect=None, line_search=None, **okw):
    """line_search (bounds; tests/test_gpu_hp_linesearch.py): dict(alpha_ref, alpha, count) of a projected line search that
    contracts -- the step the reference's own search accepts along the reference's step, the one the device's search accepts
    along its own, and the number of evaluations.  The candidate is then Plus(x, alpha delta) (one more rounding, alpha *
    delta, on top of the step's own), while rho keeps the model cost change of the unscaled delta [DoLineSearch only rescales
    delta]; a failed search comes here with alpha = 1."""
    ls = line_search
    a_ref, a_dev = (LD(ls["alpha_ref"]), LD(ls["alpha"])) if ls else (LD(1), LD(1))
    o = _options(strategy, dogleg_type, radius, **okw)
    ho = _hp_options(o)
    ref, rows = spec.reference(x, 1e-8)
    c0 = spec.cost(x)
    xn, xn_bar = spec.norms(x)
    shared = spec.shared(x)
    gmax, gmax_bar = hp.gradient_max_norm(ref, spec.fidx, x["poses"], x.get("normals"), shared)
    state0 = hp.trust_region_state(c0["cost"], radius, ho)
    mcc_c = (ref.c_sum() + 2 * hp.C_DL_ROW) * U

    # ---- the decision from the reference's own step: every comparison more than 4 bars from its threshold
    d_ref, mcc_ref, mag_ref, dl_ref = _reference_step(spec, x, ref, rows, strategy, dogleg_type, radius)
    cand_ref, pb_ref = spec.plus(x, ref, a_ref * d_ref)
    cc_ref = spec.cost(cand_ref)
    sn_ref, sn_ref_bar = spec.norms(x, cand_ref)
    pre = hp.trust_region_decision(c0["cost"], cc_ref["cost"], mcc_ref, sn_ref, xn, state0, ho, dl_norm=dl_ref,
                                   bars=dict(x_cost=c0["bar"], candidate_cost=cc_ref["bar"] + _cost_propagation(spec, cand_ref, cc_ref, pb_ref),
                                             mcc=mcc_c * mag_ref, step_norm=sn_ref_bar + spec.bars_norm(pb_ref), x_norm=xn_bar))
    margin = min(pre["margins"].values())
    assert margin > 4, (tag, pre["margins"])
    assert pre["termination"] is None and pre["valid"], (tag, pre["termination"])
    if expect is not None:
        assert pre["accepted"] == (expect == "accepted"), (tag, pre["rho"])
    if spec.bounds is not None and ls is None:
        # the projected Armijo search takes the full step: cost(Plus(x, delta)) <= cost + 1e-4 g . delta, by more than the bars
        g_delta = float((ref.g * d_ref).sum())
        assert g_delta < 0 and float(cc_ref["cost"] - c0["cost"]) + 4 * (cc_ref["bar"] + c0["bar"]) < 0.5e-4 * g_delta, (tag, g_delta)
        out_of_box = _crossings(spec, x, ref.split(d_ref)[2])
        assert out_of_box.any(), (tag, "no entry's full step crosses its bound")

    # ---- the device: the hooks' step, then the solve under test
    ba_h, delta, mcc, dl_norm, combo, (dp_u, dl_u) = _hook_step(spec, x, ref, strategy, dogleg_type, radius)
    if layout is not None:
        layout(ba_h.stats())
    cost_eval = ba_h.evaluate()[0]
    ba, s, log = _solve(spec, x, o, 2)
    out = dict(margin=margin)
    if ls is not None:
        assert s.num_line_search_steps == ls["count"], (tag, s.num_line_search_steps, ls["count"])
    elif spec.bounds is not None:
        assert s.num_line_search_steps == 1, (tag, s.num_line_search_steps)            # one evaluation, at alpha = 1, for the one iteration
        crossed = _crossings(spec, x, ref.split(delta)[2])
        assert crossed.any() and np.array_equal(crossed, out_of_box), (tag, crossed, out_of_box)
    assert log["cost"].shape[0] >= 2, (tag, log)
    assert cost_eval == log["cost"][0], (tag, cost_eval, log["cost"][0])
    out["r_cost0"] = abs(float(LD(log["cost"][0]) - c0["cost"])) / c0["bar"]
    out["r_gmax"] = abs(float(LD(log["gradient_max_norm"][0]) - gmax)) / gmax_bar
    accepted = bool(log["step_is_successful"][1])
    assert accepted == pre["accepted"], (tag, accepted, pre["rho"], log["relative_decrease"][1])
    cand, pb = spec.plus(x, ref, a_dev * delta, combo + (2.0 if ls else 0.0))
    xw = spec.written_back(ba)
    keys = ["poses", "points"] + (["normals", "light", "phong", "texture"] if spec.lighting is not None else [])
    if accepted:
        assert log["cost"][1] < log["cost"][0]                  # so the written-back lowest-cost iterate is the candidate
        for k in keys:
            err = np.abs(f64(np.asarray(xw[k], LD) - cand[k]))
            moved = pb[k] > 0
            out["r_" + k] = float((err[moved] / pb[k][moved]).max()) if moved.any() else 0.0
            assert np.array_equal(f64(xw[k])[~moved], f64(x[k])[~moved]), (tag, k)       # what does not move is bit-identical
        assert np.array_equal(xw["poses"][spec.fidx < 0], x["poses"][spec.fidx < 0])
        unobserved = np.setdiff1d(np.arange(spec.L), spec.present)
        assert np.array_equal(xw["points"][unobserved], x["points"][unobserved])
        free = spec.fidx >= 0
        ortho = lambda T: np.abs(np.einsum("nki,nkj->nij", T[:, 3:].reshape(-1, 3, 3), T[:, 3:].reshape(-1, 3, 3)) - np.eye(3)).max((1, 2))
        ob = ortho(f64(x["poses"])[free]) + 6 * pb["poses"][free, 3:].max(1) + 8 * U
        out["r_ortho"] = float((ortho(xw["poses"][free]) / ob).max())
        cc = spec.cost(xw)
        cc_bar = cc["bar"]
        out["r_cost1"] = abs(float(LD(log["cost"][1]) - cc["cost"])) / cc_bar
    elif ls is not None:
        # a rejected candidate is never written back; the line-search hook hands out the fp64 trial point the same kernels form
        # (ls["trial"]), so its cost needs no propagated Plus bar
        for k in keys:
            assert np.array_equal(f64(xw[k]), f64(x[k])), (tag, k)
        cc = spec.cost(ls["trial"])
        cc_bar = cc["bar"]
        out["r_cost1"] = abs(float(LD(log["cost"][1]) - cc["cost"])) / cc_bar
    else:
        # the identical candidate, accepted: its cost row comes from the linearisation pass
        o2 = dict(o, min_relative_decrease=-1e300)
        ba2, s2, log2 = _solve(spec, x, o2, 2, ignore=True)
        assert log2["step_is_successful"][1] == 1 and log2["step_norm"][1] == log["step_norm"][1], (tag, log2)
        cc = spec.cost(cand)
        cc_bar = cc["bar"] + _cost_propagation(spec, cand, cc, pb, asserted=True)
        out["r_cost1"] = abs(float(LD(log["cost"][1]) - cc["cost"])) / cc_bar
        out["r_cost1_lin"] = abs(float(LD(log2["cost"][1]) - cc["cost"])) / cc_bar
        out["r_cost1_pair"] = abs(log2["cost"][1] - log["cost"][1]) / (2 * cc["bar"])
        assert np.array_equal(spec.written_back(ba2)["poses"], x["poses"])        # the lowest-cost iterate is still the start
    sn, sn_bar = spec.norms(x, cand)
    sn_bar += spec.bars_norm(pb)
    out["r_step_norm"] = abs(float(LD(log["step_norm"][1]) - sn)) / sn_bar
    # ---- the decision from the truth values at the device's own step
    mag = ref.model_cost_change(delta)[1]
    bars = dict(x_cost=c0["bar"], candidate_cost=cc_bar, mcc=0.0, step_norm=sn_bar, x_norm=xn_bar)
    dec = hp.trust_region_decision(c0["cost"], cc["cost"], mcc, sn, xn, state0, ho, dl_norm=dl_norm, bars=bars)
    dec_m = hp.trust_region_decision(c0["cost"], cc["cost"], mcc, sn, xn, state0, ho, dl_norm=dl_norm, bars=dict(bars, mcc=mcc_c * mag))
    out["margin_dev"] = min(dec_m["margins"].values())
    assert out["margin_dev"] > 1, (tag, dec_m["margins"])                          # (no committed case may fall below: see `pre`)
    out["r_cost_change"] = abs(float(LD(log["cost_change"][1]) - dec["cost_change"])) / (c0["bar"] + cc_bar + U * abs(float(dec["cost_change"])))
    out["r_rho"] = abs(float(LD(log["relative_decrease"][1]) - dec["rho"])) / (dec["rho_bar"] + 8 * U * abs(float(dec["rho"])))
    assert dec["accepted"] == accepted, (tag, dec["rho"])
    if strategy == 1:
        assert log["trust_region_radius"][1] == float(dec["radius"]), (tag, log["trust_region_radius"][1], dec["radius"])
    else:
        out["r_radius"] = abs(float(LD(log["trust_region_radius"][1]) - dec["radius"])) / (dec["radius_bar"] + 8 * U * float(dec["radius"]))
    if second and accepted:
        ba3, s3, log3 = _solve(spec, x, dict(o, max_num_iterations=2), 3)
        assert log3["cost"].shape[0] >= 3 and log3["cost"][1] == log["cost"][1], (tag, log3)
        ref1, rows1 = spec.reference(xw, 1e-8)
        _, delta2, _, _, combo2, _ = _hook_step(spec, xw, ref1, strategy, dogleg_type, float(dec["radius"]))
        cand2, pb2 = spec.plus(xw, ref1, delta2, combo2)
        sn2, sn2_bar = spec.norms(xw, cand2)
        sn2_bar += spec.bars_norm(pb2) + (dec["radius_bar"] / float(dec["radius"])) * float(sn2)      # |delta| moves by at most its share of a radius change
        out["r_step_norm2"] = abs(float(LD(log3["step_norm"][2]) - sn2)) / sn2_bar
    _report(tag, accepted=int(accepted), rho=float(dec["rho"]), **out)
    for k, v in out.items():
        if k.startswith("r_"):
            assert v <= 1.0, (tag, k, v, out)
    out.update(written_back=xw, log=log, delta=delta)
    return out


def _windowed(st):
    assert st.general_structure == 0


# ------------------------------------------------------------------------------------------------------------ windowed layout
def _tiny(huber):
    return synth.make_problem(8, 60, track_len=5, seed=7, outlier_fraction=0.1 if huber else 0.0)


STRATEGIES = [(0, 0), (1, 0), (1, 1)]


@pytest.mark.parametrize("strategy,dogleg_type", STRATEGIES)
@pytest.mark.parametrize("huber", [0.0, 1.345])
def test_windowed_tiny_from_the_initial_point(huber, strategy, dogleg_type):
    prob = _tiny(huber)
    spec = Spec(prob, huber=huber)
    candidate_case(f"tiny h={huber} s={strategy}/{dogleg_type}", spec, spec.start(prob), strategy, dogleg_type, 1e4, _windowed,
                   second=True)


def _oracle_iterate(prob, huber, k, **kw):
    """The oracle's point after k iterations, its log, on the CPU (the written-back lowest-cost iterate is the current one
    while the accepted costs decrease: asserted)."""
    op = orc.OracleProblem.from_synth(prob, huber_a=huber)
    s, log = op.solve(orc.default_options(max_num_iterations=k, **kw))
    ok = log["cost"][log["step_is_successful"] == 1]
    assert np.all(np.diff(np.concatenate([[log["cost"][0]], ok])) < 0)
    return dict(poses=op.poses.copy(), points=op.points.copy()), log


def test_windowed_rejected_step():
    """The third LM iteration of the outlier problem from radius 1 is rejected (rho ~ -0.07): from the oracle's second
    iterate, at the radius the oracle had there."""
    prob = _tiny(1.345)
    x, log = _oracle_iterate(prob, 1.345, 2, initial_trust_region_radius=1.0)
    spec = Spec(prob, huber=1.345)
    candidate_case("tiny rejected", spec, x, 0, 0, float(log["trust_region_radius"][2]), _windowed, expect="rejected")


@pytest.mark.parametrize("strategy,dogleg_type", [(0, 0), (1, 0)])
def test_windowed_near_convergence(strategy, dogleg_type):
    """From the oracle iterate whose next step changes the cost by about 1e-9 of it: the step is 1e-6 of |x|, the cost bars are
    a sizeable part of cost_change, and function_tolerance must sit below it for the iteration to run."""
    prob = _tiny(0.0)
    kw = dict(function_tolerance=1e-14, parameter_tolerance=1e-14, trust_region_strategy_type=strategy, dogleg_type=dogleg_type)
    _, full = _oracle_iterate(prob, 0.0, 30, **kw)
    rel = full["cost_change"][1:] / full["cost"][1:]
    i = 1 + int(np.flatnonzero((rel < 1e-8) & (full["step_is_successful"][1:] == 1))[0])
    assert 1e-11 < rel[i - 1] < 1e-8, rel
    x, log = _oracle_iterate(prob, 0.0, i - 1, **kw)
    spec = Spec(prob)
    candidate_case(f"tiny converging s={strategy} k={i - 1}", spec, x, strategy, dogleg_type, float(log["trust_region_radius"][i - 1]),
                   _windowed, expect="accepted", function_tolerance=1e-13, parameter_tolerance=1e-13)


@pytest.mark.parametrize("L", [63, 64, 65])
def test_landmark_group_edges(L):
    """The partial-sum edges of part_eval: one group of 64 landmarks short of, exactly, and one over."""
    prob = synth.make_problem(8, L, track_len=5, seed=L)
    spec = Spec(prob)

    def layout(st):
        assert st.general_structure == 0 and st.num_superblocks == 1
    candidate_case(f"lmg L={L}", spec, spec.start(prob), 0, 0, 1e4, layout)


def test_two_pose_update_blocks():
    """257 free poses: the second k_pose_update block holds one pose, and part_pose two entries."""
    prob = synth.make_problem(258, 1032, track_len=8, seed=5)
    spec = Spec(prob)

    def layout(st):
        assert st.general_structure == 0 and st.num_free_poses == 257
    candidate_case("257 poses", spec, spec.start(prob), 0, 0, 1e4, layout)


def test_constant_poses_inside_the_chain():
    """Constant poses inside the chain, a landmark seen only from constant poses (it still moves) and one seen by nobody (it
    must not, and counts in no norm)."""
    prob = synth.make_problem(40, 1600, track_len=12, seed=8)
    const = np.zeros(40, bool)
    const[[0, 12, 13, 25]] = True
    op, oj, ouvd = prob.obs_pose, prob.obs_point, prob.obs_uvd
    j_const = int(oj[op == 12][0])                   # keep only its observations from the constant poses 12 and 13
    j_none = int(oj[op == 30][0])
    keep = ~((oj == j_const) & ~np.isin(op, [12, 13])) & (oj != j_none)
    assert np.any(oj[keep] == j_const)
    spec = Spec(prob, obs=(op[keep], oj[keep], ouvd[keep]), const=const, huber=1.345)
    assert j_none not in spec.present and j_const in spec.present

    def layout(st):
        assert st.general_structure == 0 and st.num_free_poses == 36
    x = spec.start(prob)
    candidate_case("const_gaps", spec, x, 0, 0, 1e4, layout)


# ------------------------------------------------------------------------------------------------------------ general layout
def test_wide_superblocks():
    prob = synth.make_problem(14, 300, track_len=13, seed=3)
    spec = Spec(prob)

    def layout(st):
        assert st.general_structure == 1 and st.wide_superblocks == 1
    candidate_case("wide", spec, spec.start(prob), 0, 0, 1e4, layout)


@pytest.mark.parametrize("strategy,dogleg_type", [(0, 0), (1, 0)])
def test_dense_general(monkeypatch, strategy, dogleg_type):
    """k_backsub_eval_w<true> and obs_cost_S with one stiffness per observation."""
    monkeypatch.setenv("SSBA_FORCE_DENSE", "1")
    prob = synth.make_problem(15, 400, track_len=8, seed=3)
    rng = np.random.default_rng(5)
    Sobs = np.tile(prob.stiffness(), (prob.num_obs, 1, 1)) * rng.uniform(0.5, 1.5, (prob.num_obs, 1, 1))
    spec = Spec(prob, huber=1.345)
    spec.S = Sobs

    def layout(st):
        assert st.general_structure == 1 and st.wide_superblocks == 0
    candidate_case(f"dense s={strategy}", spec, spec.start(prob), strategy, dogleg_type, 1e4, layout)


def test_long_tracks_general(monkeypatch):
    monkeypatch.setenv("SSBA_NO_WIDE", "1")
    prob = synth.make_problem(30, 900, track_len=24, seed=3)
    spec = Spec(prob)

    def layout(st):
        assert st.general_structure == 1 and st.wide_superblocks == 0
    candidate_case("long tracks", spec, spec.start(prob), 0, 0, 1e4, layout)


# --------------------------------------------------------------------------------------------------------------- pose factors
@pytest.mark.parametrize("strategy,dogleg_type", [(0, 0), (1, 0)])
def test_sun_and_prior_rows(strategy, dogleg_type):
    from test_oracle_pose_factors import _sun_problem
    prob, factors = _sun_problem(huber=0.5)
    spec = Spec(prob, factors=factors, const=np.zeros(prob.num_poses, bool))

    def layout(st):
        assert st.general_structure == 0 and st.num_free_poses == prob.num_poses and st.num_superblocks == 1
    candidate_case(f"sun_prior s={strategy}", spec, spec.start(prob), strategy, dogleg_type, 1e4, layout)


@pytest.mark.parametrize("const", [None, 3])
def test_relative_pose_rows(const):
    """Odometry with a loop closure, and a relative-pose block next to a constant pose (general layout)."""
    from test_oracle_pose_factors import _odometry_factors
    prob = synth.make_problem(7, 100, track_len=4, seed=6)
    factors = _odometry_factors(prob, huber=0.05 if const is None else 0.0)
    c = np.zeros(prob.num_poses, bool)
    if const is not None:
        factors = [f for f in factors if f["type"] == 2]
        c[const] = True
    spec = Spec(prob, factors=factors, const=c)

    def layout(st):
        assert st.general_structure == 1
    candidate_case(f"odometry const={const}", spec, spec.start(prob), 0, 0, 1e4, layout)


# ------------------------------------------------------------------------------------------------------------- lighting terms
@pytest.mark.parametrize("light_type,shared_free,radius", [(0, 0, 3.0), (1, 0, 1e4), (0, 7, 1e4), (1, 7, 1e4)])
def test_lighting_terms(light_type, shared_free, radius):
    """(The point light with constant shared blocks rejects its first step at radius 1e4, rho = -323: radius 3 is accepted.)"""
    from test_gpu_hp_phong import _phong_case
    prob, d, obs, _ = _phong_case("tiny", light_type, 4)
    spec = Spec(prob, obs=obs, lighting=d, shared_free=shared_free)

    def layout(st):
        assert st.general_structure == 0 and st.num_free_poses == 7 and st.num_superblocks == 1 and st.num_active_points == 60
    candidate_case(f"phong lt={light_type} sf={shared_free}", spec, spec.start(prob), 0, 0, radius, layout, expect="accepted")


# ------------------------------------------------------------------------------------------------------- tolerance thresholds
def _truth_of_first_iteration(spec, x, radius):
    """The truth values of the first LM iteration from x at `radius` with the device's own step (the hook's): x_cost, gmax,
    x_norm, candidate cost at Plus(x, delta_dev) (its bar carries the Plus bar), step_norm, the hook's model cost change."""
    ref, rows = spec.reference(x, 1e-8)
    c0 = spec.cost(x)
    xn, xn_bar = spec.norms(x)
    shared = spec.shared(x)
    gmax, gmax_bar = hp.gradient_max_norm(ref, spec.fidx, x["poses"], x.get("normals"), shared)
    _, delta, mcc, _, combo, _ = _hook_step(spec, x, ref, 0, 0, radius)
    cand, pb = spec.plus(x, ref, delta, combo)
    cc = spec.cost(cand)
    sn, sn_bar = spec.norms(x, cand)
    return dict(c0=c0["cost"], c0_bar=c0["bar"], cc=cc["cost"], cc_bar=cc["bar"] + _cost_propagation(spec, cand, cc, pb), xn=xn,
                xn_bar=xn_bar, sn=sn, sn_bar=sn_bar + spec.bars_norm(pb), gmax=gmax, gmax_bar=gmax_bar, mcc=LD(mcc))


def _threshold_pair(spec, x, radius, option, v, v_bar):
    """Two solves with `option` at v (1 + 2^-20) and v (1 - 2^-20); 2^-20 v must exceed the propagated bar of v."""
    assert v_bar < 2.0 ** -20 * abs(float(v)) / 4, (option, float(v), v_bar)
    runs = []
    for sign in (+1, -1):
        o = _options(0, 0, radius, max_num_iterations=2, **{option: float(v) * (1 + sign * 2.0 ** -20)})
        ba = spec.handle(x)
        s, log = ba.solve(capi.default_options(**o))
        runs.append((s, log))
    _report(f"threshold {option}", v=float(v), rel_bar=v_bar / abs(float(v)), rows=(runs[0][1]["cost"].shape[0], runs[1][1]["cost"].shape[0]))
    return runs


def _constants_spec():
    """8 poses with a constant pose inside the chain and a landmark nobody observes: blocks x_norm must not count."""
    prob = _tiny(0.0)
    const = np.zeros(8, bool)
    const[[0, 4]] = True
    op, oj, ouvd = prob.obs_pose, prob.obs_point, prob.obs_uvd
    keep = oj != int(oj[op == 5][0])
    spec = Spec(prob, obs=(op[keep], oj[keep], ouvd[keep]), const=const)
    assert spec.present.shape[0] == prob.num_points - 1
    return spec, spec.start(prob)


def test_function_tolerance_threshold():
    """|cost_change| <= function_tolerance x_cost from both sides: CONVERGENCE in iteration 1 (no row for it), or a logged
    iteration 1."""
    spec, x = _constants_spec()
    t = _truth_of_first_iteration(spec, x, 1e4)
    v = abs(t["c0"] - t["cc"]) / t["c0"]
    (s_hi, log_hi), (s_lo, log_lo) = _threshold_pair(spec, x, 1e4, "function_tolerance", v, (2 * t["c0_bar"] + t["cc_bar"]) / float(t["c0"]))
    assert s_hi.termination_type == 0 and log_hi["cost"].shape[0] == 1, (s_hi.termination_type, log_hi)
    assert log_lo["cost"].shape[0] >= 2 and log_lo["step_is_successful"][1] == 1, log_lo


@pytest.mark.parametrize("which", ["stereo", "lighting"])
def test_parameter_tolerance_threshold_shows_x_norm(which):
    """step_norm <= p (x_norm + p), solved for p: the only place x_norm is visible.  p ~ step_norm / x_norm, so a constant
    pose, an unobserved landmark or a constant shared block counted in x_norm (or a free normal or shared block left out)
    moves p by per cents, against 2^-20."""
    if which == "stereo":
        spec, x = _constants_spec()
    else:
        from test_gpu_hp_phong import _phong_case
        prob, d, obs, _ = _phong_case("tiny", 1, 4)
        spec = Spec(prob, obs=obs, lighting=d, shared_free=5)          # light and textures free, Phong parameters constant
        x = spec.start(prob)
    t = _truth_of_first_iteration(spec, x, 1e4)
    p = (-t["xn"] + np.sqrt(t["xn"] * t["xn"] + 4 * t["sn"])) / 2
    assert abs(float(p * (t["xn"] + p) - t["sn"])) <= 1e-15 * float(t["sn"])
    p_bar = float(p) * (t["sn_bar"] / float(t["sn"]) + t["xn_bar"] / float(t["xn"]))
    (s_hi, log_hi), (s_lo, log_lo) = _threshold_pair(spec, x, 1e4, "parameter_tolerance", p, p_bar)
    assert s_hi.termination_type == 0 and log_hi["cost"].shape[0] == 1, (s_hi.termination_type, log_hi)
    assert log_lo["cost"].shape[0] >= 2 and log_lo["step_is_successful"][1] == 1, log_lo


def test_gradient_tolerance_threshold():
    """gmax <= gradient_tolerance from both sides: CONVERGENCE before iteration 1, or iteration 1 runs."""
    spec, x = _constants_spec()
    t = _truth_of_first_iteration(spec, x, 1e4)
    (s_hi, log_hi), (s_lo, log_lo) = _threshold_pair(spec, x, 1e4, "gradient_tolerance", t["gmax"], t["gmax_bar"])
    assert s_hi.termination_type == 0 and log_hi["cost"].shape[0] == 1, (s_hi.termination_type, log_hi)
    assert log_lo["cost"].shape[0] >= 2


def test_min_relative_decrease_threshold():
    """rho > min_relative_decrease is strict: rejected with the option just above the truth's rho, accepted just below."""
    spec, x = _constants_spec()
    t = _truth_of_first_iteration(spec, x, 1e4)
    rho = (t["c0"] - t["cc"]) / t["mcc"]
    (s_hi, log_hi), (s_lo, log_lo) = _threshold_pair(spec, x, 1e4, "min_relative_decrease", rho, (t["c0_bar"] + t["cc_bar"]) / float(t["mcc"]))
    assert log_hi["step_is_successful"][1] == 0 and log_lo["step_is_successful"][1] == 1, (log_hi, log_lo)
    assert log_hi["trust_region_radius"][1] == 5e3 and log_lo["trust_region_radius"][1] > 1e4
    # exactly on the threshold: the device's own rho as the option (the solve is deterministic) must reject
    rho_dev = float(log_lo["relative_decrease"][1])
    s_eq, log_eq = spec.handle(x).solve(capi.default_options(**_options(0, 0, 1e4, max_num_iterations=2, min_relative_decrease=rho_dev)))
    assert log_eq["relative_decrease"][1] == rho_dev and log_eq["step_is_successful"][1] == 0, log_eq


# ------------------------------------------------------------------------------------------------- the non-monotonic quotient
def test_non_monotonic_reference_quotient():
    """use_nonmonotonic_steps: after two accepted decreases the evaluator's reference cost is still the initial one
    (num_consecutive_nonmonotonic_steps stays 0 and never meets max_consecutive_nonmonotonic_steps), so the third LM
    iteration of the outlier problem from radius 1 -- rejected by the monotonic rule with rho_0 ~ -0.07 -- has rho_1 =
    (reference - candidate) / (accumulated + mcc) as the larger quotient and is accepted.  solve_begin resets the evaluator,
    so the state is reached inside one device solve: iterations 1 and 2 give the point (written back: their costs decrease)
    and, replayed through trust_region_decision from the device's log, the evaluator's state; iteration 3 is then predicted
    from the truth cost at Plus(x_2, delta_dev), delta_dev and its model cost change from the hook at x_2 and the logged
    radius."""
    prob = _tiny(1.345)
    spec = Spec(prob, huber=1.345)
    x0 = spec.start(prob)
    o = _options(0, 0, 1.0, use_nonmonotonic_steps=1, max_num_iterations=2)
    ho = _hp_options(o)
    ba2, s2, log2 = _solve(spec, x0, o, 3)
    assert log2["cost"].shape[0] == 3 and np.all(log2["step_is_successful"][1:] == 1) and np.all(np.diff(log2["cost"]) < 0), log2
    x2 = spec.written_back(ba2)
    ba3, s3, log3 = _solve(spec, x0, dict(o, max_num_iterations=3), 4)
    assert log3["cost"].shape[0] == 4 and np.array_equal(log3["cost"][:3], log2["cost"]), log3
    # the evaluator's state after two iterations, from the device's own log (the model cost change inverted from the logged rho by the
    # evaluator's formulas, as tests/test_hp_reference.py replays the oracle's logs)
    st = hp.trust_region_state(log2["cost"][0], 1.0, ho)
    x_cost = LD(log2["cost"][0])
    for i in (1, 2):
        cand = x_cost - LD(log2["cost_change"][i])
        rho_i = LD(log2["relative_decrease"][i])
        mcc_i = (st["se_current"] - cand) / rho_i
        if (st["se_reference"] - cand) / (st["se_acc_ref"] + mcc_i) > rho_i * (1 + 1e-12):      # rho_1 was the larger quotient
            mcc_i = (st["se_reference"] - cand) / rho_i - st["se_acc_ref"]
        d = hp.trust_region_decision(x_cost, cand, mcc_i, log2["step_norm"][i], 1e3, st, ho)
        assert d["accepted"] and abs(float(d["rho"] - rho_i)) <= 1e-12 * float(rho_i)
        assert abs(float(d["radius"]) - log2["trust_region_radius"][i]) <= 1e-12 * float(d["radius"])
        st, x_cost = d["state"], LD(log2["cost"][i])
    assert st["se_reference"] == LD(log2["cost"][0]) and st["se_reference"] != st["se_current"]
    radius = float(log2["trust_region_radius"][2])
    st["radius"] = LD(radius)
    # iteration 3 from the truth
    ref, rows = spec.reference(x2, 1e-8)
    c2 = spec.cost(x2)
    _, delta, mcc, _, combo, _ = _hook_step(spec, x2, ref, 0, 0, radius)
    cand, pb = spec.plus(x2, ref, delta, combo)
    cc = spec.cost(cand)
    cc_bar = cc["bar"] + _cost_propagation(spec, cand, cc, pb)
    sn, sn_bar = spec.norms(x2, cand)
    xn, xn_bar = spec.norms(x2)
    st["se_current"] = c2["cost"]                          # the truth of the current cost (the device's is within its bar)
    d = hp.trust_region_decision(c2["cost"], cc["cost"], mcc, sn, xn, st, ho,
                                 bars=dict(x_cost=c2["bar"], candidate_cost=cc_bar, step_norm=sn_bar + spec.bars_norm(pb), x_norm=xn_bar))
    c0_bar = spec.cost(x0)["bar"]
    rho_bar = d["rho_bar"] + (c0_bar + 8 * U * float(st["se_acc_ref"]) * abs(float(d["rho1"]))) / float(st["se_acc_ref"] + LD(mcc))
    assert d["rho1"] > d["rho0"] and d["rho0"] < 1e-3 < d["rho1"], (d["rho0"], d["rho1"])
    margin = abs(float(d["rho1"]) - 1e-3) / rho_bar
    assert margin > 4, margin
    r_rho = abs(float(LD(log3["relative_decrease"][3]) - d["rho"])) / (rho_bar + 8 * U * abs(float(d["rho"])))
    r_cc = abs(float(LD(log3["cost_change"][3]) - d["cost_change"])) / (c2["bar"] + cc_bar)
    r_radius = abs(float(LD(log3["trust_region_radius"][3]) - d["radius"])) / (d["radius_bar"] + 8 * U * float(d["radius"])
                                                                             + rho_bar * 18 * float(d["radius"]))       # |d radius / d rho| <= 18 radius
    _report("nonmonotonic third iteration", rho0=float(d["rho0"]), rho1=float(d["rho1"]), margin=margin, r_rho=r_rho, r_cost_change=r_cc,
            r_radius=r_radius)
    assert log3["step_is_successful"][3] == 1 and d["accepted"]
    assert r_rho <= 1 and r_cc <= 1 and r_radius <= 1, (r_rho, r_cc, r_radius)
    assert log3["cost"][3] > log3["cost"][2]              # the accepted step did raise the cost



# ------------------------------------------------------------------------------------------------- bounds: the projection active
def _start_with_a_crossing(spec, x, radius):
    """A feasible start at which the full LM step takes one Phong / texture entry across its bound: the entry that needs the
    smallest move is put half its own step inside the bound it moves towards, from the reference's step (CPU only)."""
    x = {k: np.array(v, np.float64) for k, v in x.items()}
    M = len(x["texture"])
    o = 3 if spec.shared_free & 1 else 0
    lo = np.concatenate([np.tile(spec.bounds[0][:3], M), np.full(M, spec.bounds[0][3])])
    hi = np.concatenate([np.tile(spec.bounds[1][:3], M), np.full(M, spec.bounds[1][3])])
    for _ in range(4):
        ref, _ = spec.reference(x, 1.0 / radius)
        db = f64(ref.split(ref.gauss_newton()[0])[2])
        if _crossings(spec, x, db).any():
            return x
        vals = np.concatenate([x["phong"].ravel(), x["texture"].ravel()])
        step = db[o: o + 4 * M]
        target = np.where(step < 0, lo, hi)
        new = target - 0.5 * step
        ok = np.isfinite(target) & (step != 0) & (new >= lo) & (new <= hi)
        e = int(np.argmin(np.where(ok, np.abs(vals - new), np.inf)))
        vals[e] = new[e]
        x["phong"], x["texture"] = vals[: 3 * M].reshape(M, 3).copy(), vals[3 * M:].copy()
    raise AssertionError("no start with a crossing found")


@pytest.mark.parametrize("light_type", [0, 1])
def test_lighting_with_bounds_and_an_active_projection(light_type):
    """Bounds on the Phong and texture blocks (ka, ks, kd in [0, 1], alpha >= 1): Plus projects onto the box
    (ph_border_update_block), the projected gradient of check_body does too, and every step goes through the projected Armijo
    search -- here from a start where the full step satisfies it at alpha = 1 (asserted from the reference; one line-search
    evaluation for the one iteration) and takes one material entry across its bound, so the written-back entry is the bound."""
    from test_gpu_hp_phong import _phong_case
    prob, d, obs, _ = _phong_case("tiny", light_type, 4)
    spec = Spec(prob, obs=obs, lighting=d, shared_free=7, use_bounds=True)
    x = _start_with_a_crossing(spec, spec.start(prob), 1e4)
    lo, hi = np.asarray(spec.bounds[0]), np.asarray(spec.bounds[1])
    assert np.all((x["phong"] >= lo[:3]) & (x["phong"] <= hi[:3])) and np.all((x["texture"] >= lo[3]) & (x["texture"] <= hi[3]))

    def layout(st):
        assert st.general_structure == 0 and st.num_free_poses == 7 and st.num_superblocks == 1
    candidate_case(f"phong bounds lt={light_type}", spec, x, 0, 0, 1e4, layout, expect="accepted")


# ----------------------------------------------------------------------------------------------------------- pose graph only
def test_pose_graph_only_with_a_prior_exactly_on_its_pose():
    """No stereo block at all (tests/blowup_test.cpp): odometry between poses 1..7 with a prior holding pose 1, and pose 0 on its
    own with a prior exactly on it (R = I, so R_ref R^T = I and t_ref - t = 0 without rounding).  The gradient and the step of
    pose 0 are exactly zero: se3_plus takes its first-order branch |eps_r| <= DBL_EPSILON in check_body (projected gradient)
    and in k_pose_update (candidate).  Pose 0 is bit-unchanged, nothing is NaN; the other poses, the costs, step_norm, rho and
    the radius are held to the truth as everywhere else (the gradient from unary_rows: no Schur system exists here)."""
    import types
    from test_oracle_pose_factors import _odometry_factors
    base = synth.make_problem(8, 200, track_len=4, seed=2)
    poses = base.poses_init.copy()
    poses[0] = np.concatenate([[3.0, -1.5, 20.25], np.eye(3).ravel()])
    factors = [f for f in _odometry_factors(base, loop=False) if f["type"] == 2 and f["pose"] != 0 and f.get("pose2") != 0]
    factors += [dict(pose=1, type=0, data=base.poses_gt[1], stiffness=np.eye(6) * 1e2),
                dict(pose=0, type=0, data=poses[0].copy(), stiffness=np.eye(6) * 1e2)]
    prob = types.SimpleNamespace(camera=base.camera, num_poses=8, num_points=0, poses_init=poses, points_init=np.zeros((0, 3)),
                                 obs_pose=np.zeros(0, np.uint32), obs_point=np.zeros(0, np.uint32), obs_uvd=np.zeros((0, 3)),
                                 stiffness=lambda: np.eye(3))
    spec = Spec(prob, const=np.zeros(8, bool), factors=factors)
    x = spec.start(prob)
    radius = 1e4
    o = _options(0, 0, radius)
    ho = _hp_options(o)
    # truth at x: cost, gradient (J^T r per pose from the pose-factor rows), projected gradient, x_norm
    c0 = spec.cost(x)
    un, um = hp.unary_rows(x["poses"], factors), hp._unary_magnitudes(x["poses"], factors)
    g, eg = np.zeros((8, 6), LD), np.zeros((8, 6))
    for b, m in zip(un, um):
        for k, J in b["blocks"]:
            g[k] += J.T @ b["r"]
            eg[k] += 2 * hp.C_TERMS * U * (np.abs(f64(J)).T @ m) + hp.C_TERMS * U * np.abs(f64(J.T @ b["r"]))
    assert np.all(g[0] == 0)
    Tn, pbar = hp.se3_plus(x["poses"], -g)
    T64 = np.abs(x["poses"])
    vn = np.stack([np.sqrt((T64[:, :3] ** 2).sum(1))] * 3 + [np.sqrt((T64[:, 3:].reshape(-1, 3, 3) ** 2).sum(1))[:, c % 3] for c in range(9)], 1)
    gbar = np.sqrt((eg[:, 3:] ** 2).sum(1))[:, None] * vn + pbar
    gbar[:, :3] += eg[:, :3]
    gmax = np.abs(np.asarray(x["poses"], LD) - Tn).max()
    xn, xn_bar = spec.norms(x)
    # the device
    ba_h = spec.handle(x)
    assert ba_h.stats().num_points == 0 and ba_h.stats().num_free_poses == 8
    _, _, dp, _, mcc = ba_h.lm_step(radius, want_S=False)
    assert np.all(dp[0] == 0), dp[0]
    cost_eval = ba_h.evaluate()[0]
    ba, s, log = _solve(spec, x, o, 2)
    for k, v in log.items():
        assert np.all(np.isfinite(v)), (k, v)
    assert log["cost"].shape[0] == 2 and log["step_is_successful"][1] == 1 and cost_eval == log["cost"][0]
    xw = spec.written_back(ba)
    assert np.all(np.isfinite(xw["poses"])) and np.array_equal(xw["poses"][0], x["poses"][0])
    cand, pb = spec.plus_blocks(x, dp, np.zeros((0, 3)), None)
    out = dict(r_cost0=abs(float(LD(log["cost"][0]) - c0["cost"])) / c0["bar"],
               r_gmax=abs(float(LD(log["gradient_max_norm"][0]) - gmax)) / float(gbar.max()),
               r_poses=float((np.abs(f64(np.asarray(xw["poses"], LD) - cand["poses"]))[1:] / pb["poses"][1:]).max()))
    cc = spec.cost(xw)
    out["r_cost1"] = abs(float(LD(log["cost"][1]) - cc["cost"])) / cc["bar"]
    sn, sn_bar = spec.norms(x, cand)
    sn_bar += spec.bars_norm(pb)
    out["r_step_norm"] = abs(float(LD(log["step_norm"][1]) - sn)) / sn_bar
    dec = hp.trust_region_decision(c0["cost"], cc["cost"], mcc, sn, xn, hp.trust_region_state(c0["cost"], radius, ho), ho,
                                   bars=dict(x_cost=c0["bar"], candidate_cost=cc["bar"], mcc=1e-8 * abs(mcc), step_norm=sn_bar, x_norm=xn_bar))
    assert dec["accepted"] and min(dec["margins"].values()) > 4, dec["margins"]
    out["r_rho"] = abs(float(LD(log["relative_decrease"][1]) - dec["rho"])) / (dec["rho_bar"] + 8 * U * abs(float(dec["rho"])))
    out["r_radius"] = abs(float(LD(log["trust_region_radius"][1]) - dec["radius"])) / (dec["radius_bar"] + 8 * U * float(dec["radius"]))
    _report("pose graph only", rho=float(dec["rho"]), **out)
    for k, v in out.items():
        assert v <= 1.0, (k, v, out)


# -------------------------------------------------------------------------------------------------------------------- scale
_C2 = {}


@pytest.mark.parametrize("radius,expect", [(1e4, "rejected"), (156.25, "accepted")])
def test_c2_one_lm_iteration(radius, expect):
    """One LM iteration at C2 (1 000 poses, 100 000 landmarks, 1.19 million rows: 1 563 part_eval entries, four in flight per
    lane of the decision, and four k_pose_update blocks) against the row-by-row long-double pass, with the step and its model
    cost change from the hook (the reference's own refined solve of a 6 000-row system is not formed: the decision's margins
    are taken with the device's step, the model cost change within the 1e-8 the dogleg and LM tests establish).  From the
    initial point radius 1e4 is rejected (rho = -1828: row 1's cost comes from the partial sums of the evaluation pass, and
    is held against cost_at(Plus(x, delta_dev)) with the Plus bars propagated) and radius 156.25 -- where the oracle's solve
    first accepts -- is accepted (rho = 0.077: row 1's cost at the device's own written-back point).  Row 0 cost, step_norm,
    cost_change, rho, the flag and the radius in both."""
    if not _C2:
        prob = synth.make_config("C2")
        spec = Spec(prob)
        x = spec.start(prob)
        _C2.update(spec=spec, x=x, c0=spec.cost(x, jacobians=False), xn=spec.norms(x))
    spec, x, c0, (xn, xn_bar) = _C2["spec"], _C2["x"], _C2["c0"], _C2["xn"]
    o = _options(0, 0, radius)
    ho = _hp_options(o)
    ba_h = spec.handle(x)
    st = ba_h.stats()
    assert st.general_structure == 0 and st.num_superblocks == 84
    _, _, dp, dl, mcc = ba_h.lm_step(radius, want_S=False)
    cost_eval = ba_h.evaluate()[0]
    ba_h.close()
    ba, s, log = _solve(spec, x, o, 2)
    c2_compare(f"c2 r={radius}", spec, x, c0, xn, xn_bar, radius, ho, expect, dp, dl, mcc, cost_eval, log, spec.written_back(ba))


def c2_compare(tag, spec, x, c0, xn, xn_bar, radius, ho, expect, dp, dl, mcc, cost_eval, log, xw):
    accepted = expect == "accepted"
    assert log["cost"].shape[0] == 2 and bool(log["step_is_successful"][1]) == accepted and cost_eval == log["cost"][0], log
    free = spec.fidx >= 0
    cand, pb = spec.plus_blocks(x, dp[free], dl[spec.present], None)
    out = dict(r_cost0=abs(float(LD(log["cost"][0]) - c0["cost"])) / c0["bar"])
    if accepted:
        out["r_poses"] = float((np.abs(f64(np.asarray(xw["poses"], LD) - cand["poses"]))[free] / pb["poses"][free]).max())
        assert np.array_equal(xw["poses"][~free], x["poses"][~free])
        assert np.all(np.abs(f64(np.asarray(xw["points"], LD) - cand["points"])) <= pb["points"])
        cc = spec.cost(xw, jacobians=False)
        cc_bar = cc["bar"]
    else:
        assert np.array_equal(xw["poses"], x["poses"]) and np.array_equal(xw["points"], x["points"])
        cc = spec.cost(cand)
        cc_bar = cc["bar"] + _cost_propagation(spec, cand, cc, pb, asserted=True)
    out["r_cost1"] = abs(float(LD(log["cost"][1]) - cc["cost"])) / cc_bar
    sn, sn_bar = spec.norms(x, cand)
    sn_bar += spec.bars_norm(pb)
    out["r_step_norm"] = abs(float(LD(log["step_norm"][1]) - sn)) / sn_bar
    dec = hp.trust_region_decision(c0["cost"], cc["cost"], mcc, sn, xn, hp.trust_region_state(c0["cost"], radius, ho), ho,
                                   bars=dict(x_cost=c0["bar"], candidate_cost=cc_bar, mcc=1e-8 * abs(mcc), step_norm=sn_bar, x_norm=xn_bar))
    assert dec["accepted"] == accepted and min(dec["margins"].values()) > 4, (dec["rho"], dec["margins"])
    out["r_cost_change"] = abs(float(LD(log["cost_change"][1]) - dec["cost_change"])) / (c0["bar"] + cc_bar + U * abs(float(dec["cost_change"])))
    rho_bar = hp.trust_region_decision(c0["cost"], cc["cost"], mcc, sn, xn, hp.trust_region_state(c0["cost"], radius, ho), ho,
                                       bars=dict(x_cost=c0["bar"], candidate_cost=cc_bar))["rho_bar"]
    out["r_rho"] = abs(float(LD(log["relative_decrease"][1]) - dec["rho"])) / (rho_bar + 8 * U * abs(float(dec["rho"])))
    out["r_radius"] = abs(float(LD(log["trust_region_radius"][1]) - dec["radius"])) / (dec["radius_bar"] + 8 * U * float(dec["radius"]))
    _report(tag, accepted=int(accepted), rho=float(dec["rho"]), margin=min(dec["margins"].values()), **out)
    for k, v in out.items():
        if k.startswith("r_"):
            assert v <= 1.0, (tag, k, v, out)
