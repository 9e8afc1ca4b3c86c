"""ceres::HuberLoss on the dense image blocks, on the device (ssba_set_huber_loss on an image handle,
ssba_image_pyramid_set_huber_loss; the LOSS = true instantiations of ceres_slam_amd/csrc/ssba_image.hip).

Reference: tests/image_loss_reference.py in float64 (tests/test_image_loss_reference.py pins it).  Bars: those of
tests/test_gpu_image_alignment.py and its conventions -- rows, S and rhs 1e-10 of the largest entry of the array compared,
delta_pose and delta_disp 1e-8, model cost change 1e-9, cost 1e-10; solves: the same accept / reject sequence, cost log 1e-9
entry by entry, pose 1e-6 (largest absolute difference), free disparities 1e-6 relative.  The loss has a branch (r^2 > a^2), so
every case asserts on the reference alone that no row it evaluated lies within 1e-9 of it (min_loss_margin), as the NEAREST
cases do for their rounding boundaries.

Shapes are those of tests/test_gpu_image_alignment.py (less than one wave, 5 and 24 work-groups, 1023 / 1024 / 1025 blocks,
invalid disparities at both ends, blocks out of bounds over two edges), each with an occluder in the tracked image
(synth.occlude_tracked).  Widths: 10 corrects no row, 1e-7 every in-bounds row with r != 0, 0.02 a part of them."""
import ctypes as C
import functools
import importlib.util
import json
import os
import subprocess

import numpy as np
import pytest

import image_loss_reference as ilr
import image_reference as ir
import pyramid_reference as pyr
import test_gpu_image_alignment as base
import test_image_loss_reference as cpu
from ceres_slam_amd import build, capi, synth
from ceres_slam_amd.solver import ImageAlignment, ImagePyramid, solve_image_batch

pytestmark = pytest.mark.gpu

K = 8
A_NONE, A_ALL, A_PART = 10.0, 1e-7, 0.02
LOG_COLUMNS = ("cost", "cost_change", "gradient_max_norm", "step_norm", "relative_decrease", "trust_region_radius", "step_is_successful")
_rel = base._rel


@functools.lru_cache(maxsize=None)
def _shape(name):
    """(occluded pair, start pose) on a shape of tests/test_gpu_image_alignment.py, "<shape>:plain" without the occluder; shared
    and never written."""
    if name.endswith(":plain"):
        return base._shape(name[:-6])
    pair, start = base._shape(name)
    occ = synth.occlude_tracked(pair, 0.10, 7)
    for a in (occ.track, occ.gradx, occ.grady):
        a.setflags(write=False)
    return occ, start


def _handle(name, interp, const, a=0.0, **kw):
    pair, start = _shape(name)
    return ImageAlignment(pair.camera, start.copy(), pair.disparity.copy(), pair.ref, pair.track, pair.gradx, pair.grady,
                          interpolation=interp, disparity_const=const, huber_a=a, **kw)


def _reference(name, interp, const, a):
    pair, _ = _shape(name)
    return ilr.ImageLossProblem(pair.camera, pair.ref, pair.track, pair.gradx, pair.grady, pair.disparity, interp, disp_const=const, huber_a=a)


@functools.lru_cache(maxsize=None)
def _reference_step(name, interp, const, radius, a):
    pair, start = _shape(name)
    pr = _reference(name, interp, const, a)
    return pr, pr.lm_step(start, pair.disparity, radius)


@functools.lru_cache(maxsize=None)
def _reference_solve(name, interp, const, a, max_iter=K):
    pair, start = _shape(name)
    pr = _reference(name, interp, const, a)
    T, d, log = pr.solve(start, pair.disparity, max_iter=max_iter)
    return pr, T, d, log


def _options(**kw):
    return capi.default_options(**{**dict(max_num_iterations=K, use_nonmonotonic_steps=1), **kw})


def _step_errors(st, pr, ref, shape, const):
    rows, cols = shape

    def full(x, width=None):
        out = np.zeros((rows * cols,) + (() if width is None else (width,)))
        out[pr.blk] = x
        return out.reshape((rows, cols) + (() if width is None else (width,)))
    return dict(r=_rel(st.residuals, full(ref["r"])), Jp=_rel(st.J_pose, full(ref["Jp"], 6)), Jd=_rel(st.J_disp, full(ref["Jd"])),
                S=_rel(st.S, ref["S"]), rhs=_rel(st.rhs, ref["rhs"]), dp=_rel(st.delta_pose, ref["dp"]),
                dd=_rel(st.delta_disp, full(ref["dd"])) if not const else float(np.abs(st.delta_disp).max()),
                mcc=abs(st.mcc - ref["mcc"]) / abs(ref["mcc"]), cost=abs(st.cost - ref["cost"]) / ref["cost"])


def _assert_step(e, const):
    assert e["r"] <= 1e-10 and e["Jp"] <= 1e-10 and e["Jd"] <= 1e-10
    assert e["S"] <= 1e-10 and e["rhs"] <= 1e-10
    assert e["dp"] <= 1e-8
    assert e["dd"] <= 1e-8 if not const else e["dd"] == 0.0
    assert e["mcc"] <= 1e-9 and e["cost"] <= 1e-10


# ---- 1. one step ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("const", [False, True], ids=["free", "const"])
@pytest.mark.parametrize("interp", [ir.NEAREST, ir.BILINEAR], ids=["nearest", "bilinear"])
@pytest.mark.parametrize("radius", [1e4, 3.0])
@pytest.mark.parametrize("name", base.STEP_SHAPES)
def test_one_step_against_the_float64_reference(name, radius, interp, const):
    """One finalized handle, the three widths set on it in turn (ssba_set_huber_loss after ssba_finalize), then the NULL loss."""
    pair, start = _shape(name)
    rows, cols = pair.disparity.shape
    ba = _handle(name, interp, const)
    steps = {}
    for a in (A_NONE, A_ALL, A_PART, 0.0):
        pr, ref = _reference_step(name, interp, const, radius, a)
        if interp == ir.NEAREST:
            assert pr.min_margin >= 1e-9, pr.min_margin
        raw_r, _, _, inb = pr.raw_rows(start, pair.disparity)
        corrected = (raw_r * raw_r > a * a) & inb
        if a > 0:
            assert pr.min_loss_margin >= 1e-9, (a, pr.min_loss_margin)
        if a == A_NONE:
            assert not corrected.any()
        if a == A_ALL:
            assert (corrected == (inb & (raw_r != 0))).all() and corrected.sum() > 0.5 * inb.sum()
        if a == A_PART:
            assert 0 < corrected.sum() < inb.sum()
        ba.set_huber_loss(a)
        st = steps[a] = ba.image_step(radius)
        e = _step_errors(st, pr, ref, (rows, cols), const)
        print(f"{name} radius {radius:g} interp {interp} const {const} a {a:g}: {pr.blk.shape[0]} blocks, {int(corrected.sum())} corrected, margin {pr.min_loss_margin:.1e}, "
              + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
        hole = np.ones(rows * cols, bool)
        hole[pr.blk] = False
        hole[pr.blk[~ref["inb"]]] = True
        for x in (st.residuals, st.J_disp, st.J_pose.reshape(rows * cols, 6)):
            assert not x.reshape(rows * cols, -1)[hole].any()                 # out-of-bounds rows stay exact zeros
        _assert_step(e, const)
        if a == A_PART:      # and the loss did something: the corrected rows are smaller than the raw ones
            assert np.abs(st.residuals.reshape(-1)[pr.blk][corrected]).max() < np.abs(raw_r[corrected]).max()
    # a width that corrects no row gives the NULL-loss step within the same bars
    none, null = steps[A_NONE], steps[0.0]
    e = dict(r=_rel(none.residuals, null.residuals), Jp=_rel(none.J_pose, null.J_pose), Jd=_rel(none.J_disp, null.J_disp), S=_rel(none.S, null.S),
             rhs=_rel(none.rhs, null.rhs), dp=_rel(none.delta_pose, null.delta_pose),
             dd=_rel(none.delta_disp, null.delta_disp) if not const else float(np.abs(none.delta_disp).max()),
             mcc=abs(none.mcc - null.mcc) / abs(null.mcc), cost=abs(none.cost - null.cost) / null.cost)
    _assert_step(e, const)
    assert ba.pose.tobytes() == start.tobytes() and ba.disparity.tobytes() == pair.disparity.tobytes()       # the hook writes nothing back


# ---- 2. whole solves -----------------------------------------------------------------------------------------------------
def _result(ba, s, log):
    return (log["cost"].tobytes(), log["step_is_successful"].tobytes(), ba.pose.tobytes(), ba.disparity.tobytes(), int(s.num_iterations))


@pytest.mark.parametrize("const", [False, True], ids=["free", "const"])
@pytest.mark.parametrize("interp", [ir.NEAREST, ir.BILINEAR], ids=["nearest", "bilinear"])
@pytest.mark.parametrize("name", ["40x30", "96x64"])
def test_solve_cut_at_8_iterations(name, interp, const):
    """Constant disparities: the occluded pair.  Free disparities: the pair without the occluder, because on the occluded pair the
    REFERENCE's own loop is chaotic with free BILINEAR disparities, with or without a loss: moving one entry of its start pose by
    1e-13 moves its cost log by 2.6e-10 after one iteration and by 4e-2 (a = 0.02) or 1.5e-1 (NULL loss) after eight at 40 x 30
    (the disparities under the repainted rectangle are free to chase an unrelated texture), so no bar on the log can be met
    there by anything that rounds differently.  Without the occluder the same probe stays below 1e-10 / 6e-8 (40 x 30 / 96 x 64)
    and 0.02 still corrects rows, which is asserted."""
    name = name if const else name + ":plain"
    pair, start = _shape(name)
    pr, T, d, log = _reference_solve(name, interp, const, A_PART)
    if interp == ir.NEAREST:
        assert pr.min_margin >= 1e-9, pr.min_margin
    assert pr.min_loss_margin >= 1e-9, pr.min_loss_margin
    raw_r, _, _, inb = pr.raw_rows(start, pair.disparity)
    assert ((raw_r * raw_r > A_PART * A_PART) & inb).sum() >= 20
    runs = []
    for _ in range(2):
        ba = _handle(name, interp, const, A_PART)
        s, dev = ba.solve(_options())
        runs.append(_result(ba, s, dev))
    assert runs[0] == runs[1]                                                   # two runs are bit-equal
    ok_ref = [int(b) for _, b in log]
    cost_ref = np.array([float(c) for c, _ in log])
    print(f"{name} interp {interp} const {const}: iterations {s.num_iterations - 1} / {len(log) - 1}, decisions {dev['step_is_successful'].tolist()} / {ok_ref}"
          f", cost log {_rel(dev['cost'][:len(log)], cost_ref[:len(dev['cost'])]):.2e}, pose {np.abs(ba.pose - T).max():.2e}, loss margin {pr.min_loss_margin:.1e}"
          + ("" if const else f", disparities {_rel(ba.disparity.reshape(-1)[pr.blk], d.reshape(-1)[pr.blk]):.2e}"))
    assert s.num_iterations == len(log)
    assert dev["step_is_successful"].tolist() == ok_ref
    assert (np.abs(dev["cost"] - cost_ref) <= 1e-9 * cost_ref).all()
    assert np.abs(ba.pose - T).max() <= 1e-6
    hole = np.ones(d.size, bool)
    hole[pr.blk] = False
    assert ba.disparity.reshape(-1)[hole].tobytes() == pair.disparity.reshape(-1)[hole].tobytes()
    if const:
        assert ba.disparity.tobytes() == pair.disparity.tobytes()
    else:
        got, want = ba.disparity.reshape(-1)[pr.blk], d.reshape(-1)[pr.blk].astype(np.float64)
        assert (np.abs(got - want) <= 1e-6 * np.abs(want)).all()
    # not the NULL-loss solve
    _, T0, _, log0 = _reference_solve(name, interp, const, 0.0)
    assert abs(log0[0][0] - log[0][0]) > 1e-4 * log0[0][0]


# ---- 3. the width on a finalized handle --------------------------------------------------------------------------------------
@pytest.mark.parametrize("const", [False, True], ids=["free", "const"])
def test_width_changes_on_a_finalized_handle(const):
    """14 iterations: the lazily captured graph of the first solve is dropped by ssba_set_huber_loss and captured again."""
    pair, start = _shape("40x30")
    o = _options(max_num_iterations=14)

    def solve(ba):
        ba.pose[:] = start
        ba.disparity[:] = pair.disparity
        s, log = ba.solve(o)
        return _result(ba, s, log)

    never = solve(_handle("40x30", ir.BILINEAR, const))
    ba = _handle("40x30", ir.BILINEAR, const)
    assert solve(ba) == never
    ba.set_huber_loss(A_PART)                       # finalized, after a solve
    with_loss = solve(ba)
    assert with_loss[0] != never[0] and with_loss[2] != never[2]
    assert with_loss == solve(_handle("40x30", ir.BILINEAR, const, A_PART))      # as a handle that had the width before ssba_finalize
    ba.set_huber_loss(0.0)
    assert solve(ba) == never                       # the NULL-loss solve again, bit for bit
    ba.set_huber_loss(-1.0)                         # a <= 0 is the NULL loss
    assert solve(ba) == never


def test_the_loss_before_the_image_blocks_and_on_an_unfinalized_handle():
    pair, start = _shape("40x30")
    want = _handle("40x30", ir.BILINEAR, True, A_PART).image_step(1e4)
    lib = capi.load()
    ba = _handle("40x30", ir.BILINEAR, True, finalize=False)
    assert lib.ssba_set_huber_loss(ba.h, A_PART) == 0
    ba.finalize()
    got = ba.image_step(1e4)
    assert got.cost == want.cost and got.S.tobytes() == want.S.tobytes() and got.residuals.tobytes() == want.residuals.tobytes()


# ---- 4. |r| = a exactly ----------------------------------------------------------------------------------------------------
def test_the_dyadic_case_on_the_device():
    """ref = 0, track = 0.25, a = 0.25: r^2 > a^2 is false, the rows are uncorrected and every block costs 1/2 * 0.0625, exactly;
    with a one ulp smaller the Huber formula applies."""
    pr, T, disp = cpu._dyadic(0.25)
    raw_r, raw_Jp, _, inb = pr.raw_rows(T, disp)
    n = int(inb.sum())
    one = np.ones_like(disp)
    ba = ImageAlignment(pr.cam, T.copy(), disp.copy(), 0.0 * one, 0.25 * one, one, one, interpolation=ir.BILINEAR, disparity_const=True, huber_a=0.25)
    st = ba.image_step(1e4)
    assert (st.residuals.reshape(-1)[pr.blk][inb] == 0.25).all() and not st.residuals.reshape(-1)[pr.blk][~inb].any()
    assert st.cost == n * 0.5 * 0.0625
    null = ImageAlignment(pr.cam, T.copy(), disp.copy(), 0.0 * one, 0.25 * one, one, one, interpolation=ir.BILINEAR, disparity_const=True).image_step(1e4)
    assert st.J_pose.tobytes() == null.J_pose.tobytes() and st.residuals.tobytes() == null.residuals.tobytes() and st.cost == null.cost
    a = float(np.nextafter(0.25, 0.0))
    ba.set_huber_loss(a)
    st = ba.image_step(1e4)
    pr2, _, _ = cpu._dyadic(a)
    ref = pr2.lm_step(T, disp, 1e4)
    r = st.residuals.reshape(-1)[pr.blk]
    assert (r[inb] < 0.25).all() and (r[inb] > 0.2499).all() and not r[~inb].any()
    assert np.abs(r - ref["r"]).max() <= 1e-15 and abs(st.cost - ref["cost"]) <= 1e-15 * ref["cost"]
    # (the cost itself cannot tell: 1/2 (2 a |r| - a^2) = 1/32 - ulp^2 / 2 rounds to 1/32; the corrected residual does)
    assert _rel(st.J_pose.reshape(-1, 6)[pr.blk], ref["Jp"]) <= 1e-10


# ---- 5. covariance ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp", [ir.NEAREST, ir.BILINEAR], ids=["nearest", "bilinear"])
def test_pose_covariance_of_the_corrected_rows(interp):
    pr, ref = _reference_step("96x64", interp, True, 1e4, A_PART)
    assert pr.min_loss_margin >= 1e-9
    ba = _handle("96x64", interp, True, A_PART)
    cov = ba.pose_covariance(0)
    want = np.linalg.inv(ref["H"])
    _, null = _reference_step("96x64", interp, True, 1e4, 0.0)
    print(f"covariance interp {interp}: {_rel(cov, want):.2e}; against the NULL-loss inverse {_rel(cov, np.linalg.inv(null['H'])):.2e}")
    assert _rel(cov, want) <= 1e-9
    assert _rel(cov, np.linalg.inv(null["H"])) > 1e-2
    free = _handle("40x30", interp, False, A_PART)       # the refusal with free disparities is unchanged
    with pytest.raises(capi.SsbaError) as e:
        free.pose_covariance(0)
    assert e.value.status == -3 and "free disparity" in str(e.value)


# ---- 6. batch --------------------------------------------------------------------------------------------------------------
BATCH = [("8x6", ir.BILINEAR, True, 0.05), ("40x30", ir.BILINEAR, False, 0.02), ("96x64", ir.NEAREST, True, 0.0), ("blocks1025", ir.NEAREST, False, 0.05),
         ("40x30", ir.BILINEAR, True, 0.02), ("ends", ir.BILINEAR, False, 0.0), ("oob", ir.BILINEAR, True, 0.05)]


def _full_result(ba, s, status):
    log = ba.iteration_log()
    return dict(pose=ba.pose.tobytes(), disparity=ba.disparity.tobytes(), log={k: log[k].tobytes() for k in LOG_COLUMNS},
                num_iterations=int(s.num_iterations), termination_type=int(s.termination_type),
                initial_cost=np.float64(s.initial_cost).tobytes(), final_cost=np.float64(s.final_cost).tobytes(), status=int(status))


@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_batch_members_with_their_own_widths_are_bit_equal_to_their_solo_solves(order):
    members = BATCH if order == "forward" else BATCH[::-1]
    o = _options(max_num_iterations=20)
    want = []
    for m in members:
        ba = _handle(*m)
        s = capi.Summary()
        rc = ba.lib.ssba_solve(ba.h, C.byref(o), C.byref(s))
        want.append(_full_result(ba, s, rc))
    hs = [_handle(*m) for m in members]
    got = [_full_result(h, s, st) for h, (s, st) in zip(hs, solve_image_batch(hs, o))]
    for m, g, w in zip(members, got, want):
        assert g == w, m
    # the widths matter: the same member with another width ends elsewhere
    assert want[members.index(BATCH[1])]["pose"] != want[members.index(BATCH[4])]["pose"]
    ba = _handle(*BATCH[4][:3], 0.0)
    ba.solve(o)
    assert ba.pose.tobytes() != want[members.index(BATCH[4])]["pose"]


def test_a_batch_without_a_loss_gives_the_recorded_solo_bits():
    """tests/golden/image_batch_solo.json (recorded before the loss existed) through its own loader: twelve handles whose width
    was set and taken back, in one batch."""
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location("record_image_batch_solo", os.path.join(here, "golden", "record_image_batch_solo.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    with open(os.path.join(here, "golden", "image_batch_solo.json")) as f:
        want = json.load(f)
    assert len(want) == 12
    keys = list(want)
    hs = []
    for key in keys:
        name, interp, const = key.split("/")
        ba = rec.shapes._handle(name, 1 if interp == "bilinear" else 0, const == "const")
        ba.set_huber_loss(0.02)
        ba.set_huber_loss(0.0)
        hs.append(ba)
    res = solve_image_batch(hs, capi.default_options(max_num_iterations=50, use_nonmonotonic_steps=1))
    for key, ba, (s, st) in zip(keys, hs, res):
        log = ba.iteration_log()
        got = dict(pose=ba.pose.tobytes().hex(), disparity=ba.disparity.tobytes().hex(), num_iterations=int(s.num_iterations),
                   termination_type=int(s.termination_type), log={k: log[k].tobytes().hex() for k in rec.LOG_COLUMNS})
        assert st == 0 and got == want[key], key


# ---- 7. coarse to fine -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _occluded_96x128(seed=3):
    """pyramid_reference.case_96x128 (seed 3) or the same recipe with another seed, the 8-bit tracked image occluded."""
    if seed == 3:
        pair, ref_u8, track_u8, _ = pyr.case_96x128()
    else:
        pair = synth.make_image_pair(96, 128, seed=seed, motion=10.0, min_wavelength_px=8.0)
        ref_u8, track_u8 = pyr.quantise(pair.ref), pyr.quantise(pair.track)
    occ = synth.occlude_tracked_u8(track_u8, 0.10, seed)
    levels = pyr.build(ref_u8, occ, pair.disparity, 3, 0, pyr.OF_TRACKED, 0.125)
    for a in [ref_u8, occ, pair.disparity, pair.pose_init]:
        a.setflags(write=False)
    return pair, ref_u8, occ, levels


def _pyramid(seed, a):
    pair, ref_u8, occ, _ = _occluded_96x128(seed)
    p = ImagePyramid(ref_u8, occ, pair.disparity, 3, disparity_level=0, gradient_source=capi.GRADIENT_OF_TRACKED, gradient_scale=0.125, camera=pair.camera)
    if a is not None:
        p.set_huber_loss(a)
    return p


SUMMARY_FIELDS = ("termination_type", "num_iterations", "num_successful_steps", "num_unsuccessful_steps", "initial_cost", "final_cost")


def _summary(s):
    return tuple(np.float64(getattr(s, f)).tobytes() for f in SUMMARY_FIELDS)


def test_pyramid_align_with_a_loss_against_the_reference_loop():
    pair, _, _, levels = _occluded_96x128()
    T, _, logs, margin = ilr.coarse_to_fine(levels, pair.camera, pair.pose_init, 2, 0, max_iter=50, huber_a=A_PART)
    assert margin >= 1e-9, margin
    pose, disp = pair.pose_init.copy(), pair.disparity.copy()
    rc, sums = _pyramid(3, A_PART).align(pose, disp, coarsest_level=2, disparity_const=True, options=_options(max_num_iterations=50))
    assert rc == 0 and len(sums) == 3
    for s, log in zip(sums, logs):
        costs = np.array([float(c) for c, _ in log])
        print(f"level: iterations {s.num_iterations} / {len(log)}, initial cost {abs(s.initial_cost - costs[0]) / costs[0]:.2e}, "
              f"final cost {abs(s.final_cost - costs.min()) / costs.min():.2e}")
        assert s.num_iterations == len(log)
        assert s.num_successful_steps == sum(int(b) for _, b in log)
        assert abs(s.initial_cost - costs[0]) <= 1e-9 * costs[0] and abs(s.final_cost - costs.min()) <= 1e-9 * costs.min()
    print(f"pose {np.abs(pose - T).max():.2e}, loss margin {margin:.1e}")
    assert np.abs(pose - T).max() <= 1e-6
    # the width reaches the levels: without it the same call ends elsewhere
    pose0, disp0 = pair.pose_init.copy(), pair.disparity.copy()
    rc, sums0 = _pyramid(3, None).align(pose0, disp0, coarsest_level=2, disparity_const=True, options=_options(max_num_iterations=50))
    assert rc == 0 and sums0[0].initial_cost > 1.5 * sums[0].initial_cost and np.abs(pose0 - pose).max() > 1e-6
    print(f"|pose - true|: with the loss {np.abs(pose - pair.pose_true).max():.2e}, without {np.abs(pose0 - pair.pose_true).max():.2e}")


def test_align_batch_of_two_pyramids_with_different_widths_against_the_solo_calls():
    o = _options(max_num_iterations=20)
    cases = ((3, A_PART), (10, 0.05))
    want = []
    for sd, a in cases:
        pair = _occluded_96x128(sd)[0]
        pose, disp = pair.pose_init.copy(), pair.disparity.copy()
        rc, sums = _pyramid(sd, a).align(pose, disp, coarsest_level=2, disparity_const=True, options=o)
        assert rc == 0
        want.append((pose.tobytes(), disp.tobytes(), [_summary(s) for s in sums]))
    pyrs = [_pyramid(sd, a) for sd, a in cases]
    poses = np.stack([_occluded_96x128(sd)[0].pose_init for sd, _ in cases]).copy()
    maps = [_occluded_96x128(sd)[0].disparity.copy() for sd, _ in cases]
    rc, sums, sts = ImagePyramid.align_batch(pyrs, poses, maps, coarsest_level=2, camera=_occluded_96x128(3)[0].camera, disparity_const=True, options=o)
    assert rc == 0 and sts == [0, 0]
    for k in range(2):
        assert (poses[k].tobytes(), maps[k].tobytes(), [_summary(s) for s in sums[k]]) == want[k], k
    # and each width is its own: pyramid 1 with pyramid 0's width ends elsewhere
    pair = _occluded_96x128(10)[0]
    pose, disp = pair.pose_init.copy(), pair.disparity.copy()
    _pyramid(10, A_PART).align(pose, disp, coarsest_level=2, disparity_const=True, options=o)
    assert pose.tobytes() != want[1][0]


def test_pyramid_set_huber_loss_refuses_a_null_pyramid():
    lib = capi.load()
    assert lib.ssba_image_pyramid_set_huber_loss(None, 0.02) == -1 and "ssba_image_pyramid_set_huber_loss" in lib.ssba_last_error().decode()


# ---- 8. what the loss is for -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", cpu.OCCLUDER_SEEDS)
def test_the_loss_halves_the_pose_error_under_an_occluder(seed):
    pair, ref = cpu.occluder_case(seed)
    err = {}
    for a in (0.0, cpu.OCCLUDER_A):
        T, iters, margin = ref[a]
        if a > 0:
            assert margin >= 1e-9, margin
        ba = ImageAlignment.from_synth(pair, interpolation=ir.BILINEAR, disparity_const=True, huber_a=a)
        s, _ = ba.solve(_options(max_num_iterations=40))
        err[a] = float(np.abs(ba.pose - pair.pose_true).max())
        print(f"occluder seed {seed} a {a:g}: iterations {s.num_iterations - 1} / {iters}, |pose - reference| {np.abs(ba.pose - T).max():.2e}, |pose - true| {err[a]:.3e}")
        assert s.num_iterations - 1 == iters
        assert np.abs(ba.pose - T).max() <= 1e-6
    assert err[cpu.OCCLUDER_A] <= 0.5 * err[0.0]


# ---- 9. the examples -------------------------------------------------------------------------------------------------------
def test_dense_stereo_example_with_huber_prints_the_python_pose(tmp_path):
    import re
    exe = build.build_examples("dense_stereo_gpu")
    pair, start = _shape("40x30")
    raw = tmp_path / "pair.raw"
    with open(raw, "wb") as f:
        f.write(np.array([30, 40, ir.BILINEAR, 1], np.int32).tobytes())
        f.write(np.array([pair.camera[k] for k in ("fu", "fv", "cu", "cv", "b")]).tobytes())
        f.write(start.tobytes())
        for a in (pair.disparity, pair.ref, pair.track, pair.gradx, pair.grady):
            f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    outs = {}
    for extra in ((), ("--huber", "0.02")):
        r = subprocess.run([exe, str(raw), *extra], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        outs[extra] = dict(ln.split(" ", 1) for ln in r.stdout.strip().splitlines())
    out = outs[("--huber", "0.02")]
    ba = _handle("40x30", ir.BILINEAR, True, 0.02)
    s, _ = ba.solve()
    assert int(re.search(r"Iterations: (\d+)", out["report"]).group(1)) == s.num_successful_steps + s.num_unsuccessful_steps
    pose = np.array([float(x) for x in out["pose"].split()])
    assert pose.tobytes() == ba.pose.tobytes()                  # 17 significant digits round-trip a double
    cov = np.array([float(x) for x in out["cov"].split()]).reshape(6, 6)
    assert cov.tobytes() == ba.pose_covariance(0).tobytes()
    assert outs[()]["pose"] != out["pose"]


def test_sequence_example_with_huber(tmp_path):
    exe = build.build_examples("dense_stereo_sequence_gpu")
    seq = synth.make_stereo_sequence(96, 128, 3, seed=10, motion=5.0, min_wavelength_px=8.0)
    left = seq.left.copy()
    left[1] = synth.occlude_tracked_u8(left[1], 0.10, 1)
    seq = synth.StereoSequence(camera=seq.camera, left=left, right=seq.right, poses_true=seq.poses_true, pose_init=seq.pose_init)
    raw = tmp_path / "sequence.raw"
    synth.write_stereo_sequence(str(raw), seq, 3, 0, bytes(capi.sgbm_params(num_disparities=16, block_size=15)))
    outs = []
    for extra in (["--huber", "0.02"], ["--huber", "0.02", "--sequential"], []):
        r = subprocess.run([exe, str(raw)] + extra, capture_output=True, timeout=120)
        assert r.returncode == 0, r.stdout.decode() + r.stderr.decode()
        outs.append(r.stdout)
    assert outs[0] == outs[1] and outs[0] != outs[2]
