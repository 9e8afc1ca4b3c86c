"""One trust-region iteration of a real multi-rank solve -- the partitioned reduced solve (ssba_set_partition) and the all-reduce
mode -- against the long-double references of tests/hp_reference.py.

The step hooks do not exist on these handles (begin_hook refuses a partitioned one; on a sharded one they run their own
single-GPU launch sequence), so the step is recovered from the written-back point of an accepted iteration: the pose step as
se3_minus(poses_w, x) (the long-double inverse of se3_plus), the landmark step as points_w - x.  tests/dist_worker.py mode
"step" runs a list of cases per launch of the ranks (all on device 0, collectives over gloo).  Per case, each as a ratio <= 1
(printed in the SHARDREF lines under -s):

precondition  the reference's own decision (refined long-double solve, its own candidate) is "accepted" with every comparison
              more than 4 propagated bars from its threshold: the `pre` block of test_gpu_hp_candidate.candidate_case;
ranks         bit-identical poses and identical log rows on all ranks, the shards' point_ids partition the landmarks,
              ssba_stats shows the intended path;
r_fe          forward error of the recovered pose step against x* (hp.refined_solve of the hp.SchurSystem at the radius; for the
              dogleg beta gn + gamma v of the truth's gn and v) within hp.solve_bars(kappa_2)[1] = min(4096 u kappa_2, 1e-8);
r_fe_ref      that bar is loose (the cap against values around 1e-13), so the same forward error is measured for the CPU oracle on
              the whole problem and for an unsharded handle on device 0, and the sharded value must not exceed 8 x the larger:
              another elimination order re-rounds the same sums, the partitioned plan adds the separator level and at most
              ceil(log2 n_sep) PCR steps -- three bits, which still expose a dropped or mis-scaled term of 1e-11 relative;
r_dl          the landmark step of every shard against the long-double back-substitution of the recovered pose step, normwise
              over the landmarks with kappa(V_j) <= 1e8, within the bar of test_gpu_hp_reference._check_back_substitution (LM, and
              the dogleg where it takes the Gauss-Newton step; on the other dogleg branches the landmark step beta gn_l + gamma
              v_l is no back-substitution of the pose step and enters through the cost at the written-back point, step_norm and
              rho);
log rows      row 0: cost against cost_at(x), gradient_max_norm; row 1: cost against cost_at at the written-back point,
              step_norm against |x_w - x|, cost_change, relative_decrease, the flag and the radius against
              hp.trust_region_decision fed with the truth costs and the truth's model cost change at the recovered step (bar
              mcc_c mag, plus the recovery bars carried through |g| and |J delta| |J|).

The truth of one (problem, loss, strategy, radius) is computed once and shared by the worlds and partitions that use it.

With free shared lighting blocks (the only route to launch_border_scale) the light, Phong and texture blocks are compared
with x + delta_b* of the truth's border step (r_light through hp.projected_plus, r_phong, r_texture; the pose bar carried over
|delta_b*|); the normals enter through the back-substitution of their tangent step and the cost at the written-back point."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import hp_reference as hp
from ceres_slam_amd import capi, sharding, synth
from oracle import oracle as orc
from test_gpu_hp_candidate import Spec, _cost_propagation, _hp_options, _options, _reference_step
from test_gpu_hp_reference import RADII, _back_substitution_bound

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
U, LD = hp.U, hp.LD
f64 = lambda v: np.asarray(v, np.float64)
WORST = {}
REF_FACTOR = 8.0


def _report(tag, **kv):
    print("SHARDREF", tag, " ".join(f"{k}={v:.3g}" if isinstance(v, float) else f"{k}={v}" for k, v in kv.items()))
    for k, v in kv.items():
        if isinstance(v, float) and k.startswith("r_"):
            WORST[k] = max(WORST.get(k, 0.0), v)


@pytest.fixture(scope="module", autouse=True)
def _worst_ratios():
    yield
    print("\nSHARDREF worst", " ".join(f"{k}={v:.3g}" for k, v in sorted(WORST.items())))


# ------------------------------------------------------------------------------------------------------------------ the truth
_TRUTH = {}


def truth(size, huber, strategy, dogleg_type, radius, light_type=None):
    """Everything of one case that does not depend on the device: the problem, the reference at x, the truth step with the
    kappa_2 of the system it came from, and the precondition (asserted).  light_type 0 / 1: the lighting problem of the
    worker's mode "step_phongfree" (light, Phong parameters and textures free, from the perturbed start)."""
    key = (tuple(size), huber, strategy, dogleg_type, radius, light_type)
    if key in _TRUTH:
        return _TRUTH[key]
    tag = f"P{size[0]} L{size[1]} T{size[2]} h={huber} s={strategy}/{dogleg_type} r={radius:g}" + ("" if light_type is None else f" lt={light_type}")
    if light_type is None:
        prob = synth.make_problem(size[0], size[1], track_len=size[2], seed=21, outlier_fraction=0.3 if huber > 0 else 0.0)
        spec = Spec(prob, huber=huber)
    else:
        prob, ph = synth.make_phong_problem(size[0], size[1], track_len=size[2], seed=21, light_type=light_type)
        spec = Spec(prob, lighting=ph.as_oracle_dict("perturbed"), shared_free=7)
    x = spec.start(prob)
    o = _options(strategy, dogleg_type, radius)
    ho = _hp_options(o)
    ref, rows = spec.reference(x, 1e-8)
    c0 = spec.cost(x)
    xn, xn_bar = spec.norms(x)
    gmax, gmax_bar = hp.gradient_max_norm(ref, spec.fidx, x["poses"], x.get("normals"), spec.shared(x))
    state0 = hp.trust_region_state(c0["cost"], radius, ho)
    mcc_c = (ref.c_sum() + 2 * hp.C_DL_ROW) * U
    if strategy == 0:
        ref_r, _ = spec.reference(x, 1.0 / radius, rows)
        d_ref, kappa = ref_r.gauss_newton()
        mcc_ref, mag_ref = ref.model_cost_change(d_ref)
        dl_ref, sy, backsub = None, ref_r.sy, True
    else:
        gn = ref.gauss_newton()
        ref.gauss_newton = lambda band=None: gn          # (one refined solve: _reference_step asks for it again)
        d_ref, mcc_ref, mag_ref, dl_ref = _reference_step(spec, x, ref, rows, strategy, dogleg_type, radius)
        kappa, sy, backsub = gn[1], ref.sy, bool(np.array_equal(d_ref, gn[0]))
    # ---- the precondition: the decision from the reference's own step, every comparison more than 4 bars from its threshold
    cand_ref, pb_ref = spec.plus(x, ref, d_ref)
    cc_ref = spec.cost(cand_ref)
    sn_ref, sn_ref_bar = spec.norms(x, cand_ref)
    pre = hp.trust_region_decision(c0["cost"], cc_ref["cost"], mcc_ref, sn_ref, xn, state0, ho, dl_norm=dl_ref,
                                   bars=dict(x_cost=c0["bar"], candidate_cost=cc_ref["bar"] + _cost_propagation(spec, cand_ref, cc_ref, pb_ref),
                                             mcc=mcc_c * mag_ref, step_norm=sn_ref_bar + spec.bars_norm(pb_ref), x_norm=xn_bar))
    margin = min(pre["margins"].values())
    assert margin > 4, (tag, pre["margins"])
    assert pre["termination"] is None and pre["valid"] and pre["accepted"], (tag, pre["termination"], pre["rho"])
    T = dict(tag=tag, size=tuple(size), huber=huber, light_type=light_type, strategy=strategy, dogleg_type=dogleg_type, radius=radius, prob=prob, spec=spec, x=x,
             o=o, ho=ho, ref=ref, c0=c0, xn=xn, xn_bar=xn_bar, gmax=gmax, gmax_bar=gmax_bar, state0=state0, mcc_c=mcc_c, d_ref=d_ref,
             x_star=np.asarray(ref.split(d_ref)[0], LD).ravel(), kappa=kappa, dl_ref=dl_ref, sy=sy, backsub=backsub, margin=margin,
             rho_ref=float(pre["rho"]))
    _TRUTH[key] = T
    return T


def _dogleg_norm_bar(T):
    """Bar of the device's |delta|_D (it enters the new radius as 3 |delta|_D after rho > 0.75): the six sums' bars carried
    through hp.dogleg_scalars by central differences."""
    ref = T["ref"]
    gn = ref.gauss_newton()[0]
    ps, pbar = ref.param_sums(ref.v, gn)
    rs = [ref.row_sums(a, b) for a, b in ((ref.v, ref.v), (gn, gn), (ref.v, gn))]
    sums, bars = list(ps) + [r[0] for r in rs], list(pbar) + [r[1] for r in rs]
    return hp.propagate(lambda s: dict(n=hp.dogleg_scalars(s, T["radius"], T["dogleg_type"])["step_norm"]), sums, bars)["n"]


# ------------------------------------------------------------------------------------------------------------- the comparison
def recovered_pose_step(T, poses_w):
    """(delta_p of the free poses (nf, 6) in long double, its bar, forward error against x*)."""
    free = T["spec"].fidx >= 0
    dp, dp_bar = hp.se3_minus(np.asarray(poses_w, np.float64)[free], T["x"]["poses"][free])
    return dp, dp_bar, hp.forward_error(dp.ravel(), T["x_star"])


def compare(tag, T, ranks, refs=None, wide=None):
    """`ranks`: per rank a dict with log (the columns of iteration_log), poses, points, point_ids and stats (None: not a
    device handle) -- the worker's record of one case.  refs: (oracle, unsharded) forward errors, or None."""
    spec, x, ref, prob = T["spec"], T["x"], T["ref"], T["prob"]
    strategy, radius = T["strategy"], T["radius"]
    r0 = ranks[0]
    out = dict(kappa=float(T["kappa"]), margin=T["margin"])
    # ---- ranks
    for r in ranks:
        assert r.get("status", 0) == 0, (tag, r.get("message"))
        assert r["poses"] == r0["poses"], (tag, "poses differ between ranks", r0["stats"], r["stats"])
        assert r["log"] == r0["log"], (tag, r0["log"], r["log"])
        if r["stats"] is not None:
            st = r["stats"]
            assert st["num_free_poses"] == prob.num_poses - 1, (tag, st)
            if wide:
                assert st["wide_superblocks"] > 0, (tag, st)
            else:
                assert st["wide_superblocks"] == 0 and st["general_structure"] == 0, (tag, st)
    ids = np.concatenate([np.asarray(r["point_ids"], np.int64) for r in ranks])
    assert np.array_equal(np.sort(ids), np.arange(spec.L)), (tag, "the shards' point_ids do not partition the landmarks")
    xw = dict(poses=f64(r0["poses"]).reshape(-1, 12), points=np.empty((spec.L, 3)))
    xw["points"][ids] = np.concatenate([f64(r["points"]).reshape(-1, 3) for r in ranks])
    lit = spec.lighting is not None
    if lit:
        xw["normals"] = np.empty((spec.L, 3))
        xw["normals"][ids] = np.concatenate([f64(r["normals"]).reshape(-1, 3) for r in ranks])
        for k in ("light", "phong", "texture"):
            assert all(r[k] == r0[k] for r in ranks), (tag, k, "differs between ranks")
            xw[k] = f64(r0[k]).reshape(np.shape(x[k]))
    log = {k: np.asarray(v) for k, v in r0["log"].items()}
    assert log["cost"].shape[0] >= 2, (tag, log)
    # ---- row 0
    c0 = T["c0"]
    out["r_cost0"] = abs(float(LD(log["cost"][0]) - c0["cost"])) / c0["bar"]
    out["r_gmax"] = abs(float(LD(log["gradient_max_norm"][0]) - T["gmax"])) / T["gmax_bar"]
    assert int(log["step_is_successful"][1]) == 1, (tag, T["rho_ref"], log["relative_decrease"][1])
    assert log["cost"][1] < log["cost"][0]                  # so the written-back lowest-cost iterate is the candidate
    assert np.array_equal(xw["poses"][spec.fidx < 0], x["poses"][spec.fidx < 0]), (tag, "a constant pose moved")
    unobserved = np.setdiff1d(np.arange(spec.L), spec.present)
    assert np.array_equal(xw["points"][unobserved], x["points"][unobserved])
    # ---- the pose step
    dp, dp_bar, fe = recovered_pose_step(T, xw["poses"])
    fe_bar = hp.solve_bars(T["kappa"])[1]
    out.update(fe=fe, r_fe=fe / fe_bar)
    if refs is not None:
        out.update(fe_oracle=refs[0], fe_single=refs[1], r_fe_ref=fe / (REF_FACTOR * max(refs)), x_oracle=fe / refs[0], x_single=fe / refs[1])
    # ---- the landmark step
    lm = spec.present
    dl = np.asarray(xw["points"], LD)[lm] - np.asarray(x["points"], LD)[lm]
    dl_bar = U * np.abs(xw["points"][lm])
    db = db_bar = None
    if lit:
        # the tangent step of a unit vector from its Plus: y = x + d - (d.x / x.x) x is parallel to n_w with y.x = x.x, and the part
        # of d along x, which Plus discards, is taken as zero (the rows do not see it: J x = 0, g.x = 0)
        def unit_minus(nw, n):
            nw, n = np.asarray(nw, LD).reshape(-1, 3), np.asarray(n, LD).reshape(-1, 3)
            d = nw * ((n * n).sum(1) / (nw * n).sum(1))[:, None] - n
            return d, hp.unit_plus(n, d)[1]
        dn, dn_bar = unit_minus(xw["normals"][lm], x["normals"][lm])
        dl, dl_bar = np.concatenate([dl, dn], 1), np.concatenate([dl_bar, dn_bar], 1)
        if spec.lighting["light_type"] == 1:
            d_light, b_light = unit_minus(xw["light"], x["light"])
            d_light, b_light = d_light[0], b_light[0]
        else:
            d_light, b_light = np.asarray(xw["light"], LD) - np.asarray(x["light"], LD), U * np.abs(xw["light"])
        db = np.concatenate([d_light] + [(np.asarray(xw[k], LD) - np.asarray(x[k], LD)).ravel() for k in ("phong", "texture")])
        db_bar = np.concatenate([b_light] + [U * np.abs(xw[k]).ravel() for k in ("phong", "texture")])
        # the shared blocks against x + delta_b*: the Phong parameters and textures are plain sums, the light goes through
        # projected_plus; the bar is the pose bar carried over |delta_b*|, plus the rounding of the sum / of Plus
        db_star = np.asarray(ref.split(T["d_ref"])[2], LD)
        (nl, nph, ntx), (bl, bph, btx) = hp.projected_plus(spec.lighting["light_type"], x["light"], x["phong"], x["texture"], db_star, 7)
        carry = fe_bar * float(np.sqrt((db_star ** 2).sum()))
        out["r_light"] = float((np.abs(f64(np.asarray(xw["light"], LD) - nl)) / (bl + carry)).max())
        out["r_phong"] = float((np.abs(f64(np.asarray(xw["phong"], LD) - nph)) / (bph + carry)).max())
        out["r_texture"] = float((np.abs(f64(np.asarray(xw["texture"], LD) - ntx)) / (btx + carry)).max())
    if T["backsub"]:
        sy = T["sy"]
        assert np.array_equal(sy.lm, lm)
        dl_true = sy.back_substitute(dp.ravel(), db)
        if lit:     # the part of the reference's normal step along the normal is discarded by Plus
            n = np.asarray(x["normals"], LD)[lm]
            dl_true[:, 3:] -= ((dl_true[:, 3:] * n).sum(1) / (n * n).sum(1))[:, None] * n
        bound = _back_substitution_bound(sy, f64(dp).ravel(), dl_true, x["points"], None if db is None else f64(db))
        keep = sy.kappa_V <= 1e8
        err = np.abs(f64(dl - dl_true)).max(1)
        out["r_dl"] = float(np.sqrt((err[keep] ** 2).sum()) / np.sqrt((bound[keep] ** 2).sum()))
        out["dl_skipped"] = int((~keep).sum())
    # ---- row 1
    cc = spec.cost(xw)
    out["r_cost1"] = abs(float(LD(log["cost"][1]) - cc["cost"])) / cc["bar"]
    sn, sn_bar = spec.norms(x, xw)
    out["r_step_norm"] = abs(float(LD(log["step_norm"][1]) - sn)) / sn_bar
    # ---- the decision from the truth costs and the truth's model cost change at the recovered step
    delta = ref.pack(dp, dl, db)
    mcc, mag = ref.model_cost_change(delta)
    dbar = f64(ref.pack(dp_bar, dl_bar, db_bar))
    rec = float((np.abs(f64(ref.g)) * dbar).sum()) + sum(float((np.abs(f64(a)) * b).sum()) for a, b in zip(ref.jx(delta), ref.jx_mag(dbar)))
    bars = dict(x_cost=c0["bar"], candidate_cost=cc["bar"], mcc=T["mcc_c"] * mag + rec, step_norm=sn_bar, x_norm=T["xn_bar"])
    dec = hp.trust_region_decision(c0["cost"], cc["cost"], mcc, sn, T["xn"], T["state0"], T["ho"], dl_norm=T["dl_ref"], bars=bars)
    out["margin_dev"] = min(dec["margins"].values())
    assert out["margin_dev"] > 1, (tag, dec["margins"])
    assert dec["accepted"], (tag, dec["rho"])
    out["r_cost_change"] = abs(float(LD(log["cost_change"][1]) - dec["cost_change"])) / (c0["bar"] + cc["bar"] + U * abs(float(dec["cost_change"])))
    out["r_rho"] = abs(float(LD(log["relative_decrease"][1]) - dec["rho"])) / (dec["rho_bar"] + 8 * U * abs(float(dec["rho"])))
    if strategy == 1:
        grows = dec["rho"] > 0.75 and 3 * T["dl_ref"] > LD(radius)
        rb = 3 * _dogleg_norm_bar(T) + 8 * U * float(dec["radius"]) if grows else 0.0
        d = abs(float(LD(log["trust_region_radius"][1]) - dec["radius"]))
        out["r_radius"] = d / rb if rb else (0.0 if d == 0 else float("inf"))
    else:
        out["r_radius"] = abs(float(LD(log["trust_region_radius"][1]) - dec["radius"])) / (dec["radius_bar"] + 8 * U * float(dec["radius"]))
    _report(tag, rho=float(dec["rho"]), **out)
    for k, v in out.items():
        if k.startswith("r_"):
            assert v <= 1.0, (tag, k, v, out)
    return out


def oracle_as_rank(T):
    """One iteration of the CPU oracle on the whole problem, in the form of a rank's record."""
    prob, spec = T["prob"], T["spec"]
    op = orc.OracleProblem(prob.camera, prob.poses_init, prob.points_init, prob.obs_pose, prob.obs_point, prob.obs_uvd, prob.stiffness(),
                           huber_a=T["huber"], lighting=spec.lighting, shared_free=spec.shared_free)
    s, log = op.solve(orc.default_options(num_threads=2, **T["o"]))
    rec = dict(log={k: f64(v).tolist() for k, v in log.items()}, poses=op.poses.tolist(), points=op.points.tolist(),
               point_ids=list(range(prob.num_points)), stats=None)
    if spec.lighting is not None:
        rec.update(normals=op.normals.tolist(), light=op.light.tolist(), phong=op.phong.tolist(), texture=op.texture.tolist())
    return rec


_REFS = {}


def _reference_errors(T):
    """(oracle, unsharded device handle): the forward errors of the same recovery on the two single-process solves."""
    key = (T["size"], T["huber"], T["strategy"], T["dogleg_type"], T["radius"], T["light_type"])
    if key not in _REFS:
        from ceres_slam_amd.solver import StereoBA
        fe_o = recovered_pose_step(T, oracle_as_rank(T)["poses"])[2]
        prob, spec = T["prob"], T["spec"]
        ba = StereoBA(prob.camera, prob.poses_init.copy(), prob.points_init.copy(), prob.obs_pose, prob.obs_point, prob.obs_uvd,
                      prob.stiffness(), huber_a=T["huber"], device=0, lighting=spec.lighting, shared_free=spec.shared_free)
        s, log = ba.solve(capi.default_options(**T["o"]))
        assert log["cost"].shape[0] >= 2 and log["step_is_successful"][1] == 1, (T["tag"], log)
        _REFS[key] = fe_o, recovered_pose_step(T, ba.poses)[2]
        ba.close()
    return _REFS[key]


# ----------------------------------------------------------------------------------------------------------------- the ranks
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_ranks(out, world, size, cases, mode="step"):
    """One launch of `world` ranks over the list of cases; the time limit covers the start-up of the processes (importing torch,
    the first HIP call: tens of seconds on a busy box) and two seconds per case.  Returns the cases' records, per case the
    list over the ranks."""
    port = _free_port()
    limit = 240 + 2 * len(cases)
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2", SSBA_TEST_SIZE=",".join(str(v) for v in size),
                   SSBA_TEST_CASES=json.dumps(cases))
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "dist_worker.py"), mode, out], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    try:
        outs = [p.communicate(timeout=limit)[0].decode(errors="replace") for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    per_rank = [json.load(open(f"{out}.{r}.json"))["cases"] for r in range(world)]
    return [[per_rank[r][i] for r in range(world)] for i in range(len(cases))]


def _case(radius, huber=0.0, strategy=0, dogleg=0, partition=None, env=None, light_type=None):
    tag = f"r={radius:g} h={huber} s={strategy}/{dogleg}" + ("" if not env else " " + ",".join(f"{k}={v}" for k, v in env.items()))
    return dict(tag=tag, radius=radius, huber=huber, strategy=strategy, dogleg=dogleg, partition=partition, env=env, light_type=light_type)


def _run_and_compare(tmp_path, name, size, world, cases, wide=False, check_stats=None, mode="step"):
    truths = [truth(size, c["huber"], c["strategy"], c["dogleg"], c["radius"], c["light_type"]) for c in cases]       # (the precondition, before any launch)
    records = _run_ranks(str(tmp_path / "step"), world, size, cases, mode)
    for c, T, ranks in zip(cases, truths, records):
        if check_stats is not None:
            check_stats(c, ranks)
        compare(f"{name} {T['tag']}" + ("" if not c["env"] else " " + c["tag"].split(" ")[-1]), T, ranks, _reference_errors(T), wide=wide)


# (radius, huber) per problem: RADII of test_gpu_hp_reference.py where the reference accepts the step.  The precondition refuses,
# as rejected by the reference itself, (61, 2400, 8) with the Huber loss at 1e4 (rho = -25) and with either dogleg at 1e4 (-62.5),
# and (133, 5300, 8) at 1e4 with and without the loss (rho = -0.77, -3131): a rejected step is never written back and cannot be
# recovered.  Radius 30 stands in for 1e4 there (accepted, every margin above 1e9 bars).
LM_RADII = {(61, 2400, 8): [(1e4, 0.0), (3.0, 0.0), (30.0, 1.345)], (58, 2300, 8): RADII, (85, 3400, 8): RADII,
            (133, 5300, 8): [(30.0, 0.0), (3.0, 0.0), (30.0, 1.345)]}
DOGLEG_RADII = (30.0, 3.0)

# ------------------------------------------------------------------------------------------------ the partitioned reduced solve
PCR = "SSBA_PCR_MAX_BLOCKS"
PARTITIONED = [
    # chains of 3, one pinned end each; n_sep = 1: no separator step
    ("w2_chains3", (61, 2400, 8), 2, [0, 2, 4], [None]),
    # the middle rank's chain has 2 blocks, both pinned, no interior; n_sep = 2
    ("w3_middle2", (61, 2400, 8), 3, [0, 1, 2, 4], [None]),
    # every chain has 2 blocks, the last super-block padded (9 poses); n_sep = 3: two separator steps, not a power of two
    ("w4_chains2_padded", (58, 2300, 8), 4, [0, 1, 2, 3, 4], [None]),
    # n_sep = 4; chains of 3 and 2
    ("w5_nsep4", (85, 3400, 8), 5, [0, 2, 3, 4, 5, 6], [None]),
    # chains of 6: even at level 0, so the `pin` level on rank 0; plain levels below a pinned PCR top
    ("w2_chains6_plain", (133, 5300, 8), 2, [0, 5, 10], [3]),
    # chains of 7 and 5: odd, then even (7 -> 4 -> pinned 3)
    ("w2_chains7_5_plain", (133, 5300, 8), 2, [0, 6, 10], [3, 2]),
]


@pytest.mark.parametrize("name,size,world,seps,pcr_max", PARTITIONED, ids=[p[0] for p in PARTITIONED])
def test_partitioned_lm_step_against_the_truth(tmp_path, name, size, world, seps, pcr_max):
    assert seps[-1] == (size[0] - 1 + 11) // 12 - 1 and len(seps) == world + 1
    cases = [_case(radius, huber, partition=seps, env=None if m is None else {PCR: str(m)}) for m in pcr_max for radius, huber in LM_RADII[size]]

    def check_stats(c, ranks):
        for r, rec in enumerate(ranks):
            chain = seps[r + 1] - seps[r] + 1
            top = rec["stats"]["pcr_blocks"]
            if c["env"]:
                assert 0 < top <= int(c["env"][PCR]) and top < chain, (name, r, rec["stats"])     # plain levels ran below the top
            else:
                assert top == chain, (name, r, rec["stats"])
    _run_and_compare(tmp_path, name, size, world, cases, check_stats=check_stats)


# ------------------------------------------------------------------------------------------------------------- all-reduce mode
@pytest.mark.parametrize("world", [2, 3])
def test_all_reduce_step_against_the_truth(tmp_path, world):
    """The segmented launch sequence (fuse_ctrl off, spb_in_place_ok off); DOGLEG in three segments with the six model sums
    added over the ranks in between."""
    cases = [_case(radius, huber) for radius, huber in LM_RADII[(61, 2400, 8)]]
    cases += [_case(radius, 0.0, 1, dogleg) for dogleg in (0, 1) for radius in DOGLEG_RADII]
    _run_and_compare(tmp_path, f"allreduce w{world}", (61, 2400, 8), world, cases)


@pytest.mark.parametrize("size", [(50, 1500, 16), (30, 900, 24)])
def test_all_reduce_wide_step_against_the_truth(tmp_path, size):
    """Tracks of 13 to 24: every rank forms the 144-row super-blocks of its landmarks and the ranks exchange L.wide.xw.  (At
    radius 1e4 the first step of the 16-track problem is rejected -- rho = -6.9 on the oracle --: radii 30 and 3.)"""
    cases = [_case(radius, 0.0, s, d) for radius in (30.0, 3.0) for s, d in ((0, 0), (1, 0), (1, 1))]
    _run_and_compare(tmp_path, f"wide T{size[2]} w2", size, 2, cases, wide=True)


# ------------------------------------------------------------------------------------------- free shared lighting blocks, two ranks
# the directional light's first step at radius 1e4 is rejected by the reference (rho = -0.137): radius 3 there
PHONG_RADIUS = {0: 1e4, 1: 3.0}


@pytest.mark.parametrize("light_type", [0, 1])
def test_all_reduce_free_shared_border_step_against_the_truth(tmp_path, light_type):
    """Light, Phong parameters and textures free on two ranks: the border sums are added over the ranks next to the reduced system
    and launch_border_scale takes the Jacobi scale of the free shared blocks from the summed diagonal."""
    cases = [_case(PHONG_RADIUS[light_type], light_type=light_type)]
    _run_and_compare(tmp_path, f"phongfree lt={light_type} w2", (16, 400, 6), 2, cases, mode="step_phongfree")
