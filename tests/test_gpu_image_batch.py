"""Batched dense alignment (ssba_image_solve_batch, ssba_image_pyramid_align_batch; k_imb_* in ceres_slam_amd/csrc/ssba_image.hip):
n image handles in shared launches, five per iteration of the whole batch.

The yardstick is always the same handle solved alone (ssba_solve, or the stepwise calls), compared TO THE BIT: the batched
linearisation and evaluation kernels call the very functions the solo kernels are wrappers over, the solve kernel compiles the
solo kernel's statements (shared as text), and every sum keeps its order.  The compiler is still free to contract a sum of two
products differently in two kernels, so the equality is what this file TESTS, not something the language guarantees.  No
tolerance appears in this file.  Compared for every
member: the pose, the whole disparity map (pixels without a block and constant ones included), every column of
ssba_iteration_log, num_iterations, termination_type, initial_cost, final_cost.

tests/test_image_batch_inputs.py pins, on the numpy loop alone, that the five members end after 6, 8, 9, 18 and 51 log entries;
here the batch is asserted to show exactly those counts, so a batch that stopped everyone at the first termination (or ran
everyone to the last) cannot pass.  blocks1025 (NEAREST, 5 work-groups, one lane in the last) sits beside 8 x 6's single partial
work-group."""
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import image_batch_members as bm
import image_reference as ir
import pyramid_reference as pr
from ceres_slam_amd import build, capi, synth
from ceres_slam_amd.solver import ImageAlignment, ImagePyramid, solve_image_batch

pytestmark = pytest.mark.gpu

LOG_COLUMNS = ("cost", "cost_change", "gradient_max_norm", "step_norm", "relative_decrease", "trust_region_radius", "step_is_successful")
SIX = bm.FIVE + ["blocks1025"]


def _options(**kw):
    return capi.default_options(**{**dict(max_num_iterations=bm.MAX_ITER, use_nonmonotonic_steps=1), **kw})


def _handle(name, start=None):
    pair, start0, interp, const = bm.member(name)
    return ImageAlignment(pair.camera, (start0 if start is None else start).copy(), pair.disparity.copy(), pair.ref, pair.track, pair.gradx,
                          pair.grady, interpolation=interp, disparity_const=const)


def _result(ba, s, status):
    """Everything that is compared, as bytes and integers."""
    log = ba.iteration_log()
    return dict(pose=ba.pose.tobytes(), disparity=ba.disparity.tobytes(), log={k: log[k].tobytes() for k in LOG_COLUMNS},
                num_iterations=int(s.num_iterations), termination_type=int(s.termination_type),
                initial_cost=np.float64(s.initial_cost).tobytes(), final_cost=np.float64(s.final_cost).tobytes(), status=int(status))


@functools.lru_cache(maxsize=None)
def _solo(name, start_key=None):
    """The member solved alone with ssba_solve; computed once and never written."""
    ba = _handle(name, None if start_key is None else np.frombuffer(start_key, dtype=np.float64))
    s = capi.Summary()
    rc = ba.lib.ssba_solve(ba.h, C.byref(_options()), C.byref(s))
    out = _result(ba, s, rc)
    ba.close()
    return out


def _batch(names, **kw):
    hs = [_handle(n) for n in names]
    res = solve_image_batch(hs, _options(), **kw)
    return hs, [_result(h, s, st) for h, (s, st) in zip(hs, res)]


def _assert_same(got, want, what):
    for k in ("status", "num_iterations", "termination_type", "initial_cost", "final_cost", "pose", "disparity"):
        assert got[k] == want[k], (what, k)
    for k in LOG_COLUMNS:
        assert got["log"][k] == want["log"][k], (what, "log", k)


def test_a_batch_of_one():
    _, (got,) = _batch(["s0"])
    _assert_same(got, _solo("s0"), "s0")
    assert got["num_iterations"] == bm.MEMBERS["s0"][4]


@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_six_members_end_at_different_iterations_each_as_alone(order):
    names = SIX if order == "forward" else SIX[::-1]
    _, got = _batch(names)
    for n, g in zip(names, got):
        _assert_same(g, _solo(n), n)
    counts = {n: g["num_iterations"] for n, g in zip(names, got)}
    print(order, counts)
    assert [counts[n] for n in bm.FIVE] == [bm.MEMBERS[n][4] for n in bm.FIVE] == [6, 8, 9, 18, 51]
    # free disparities moved, constant ones and pixels without a block did not
    for n, g in zip(names, got):
        pair, _, _, const = bm.member(n)
        assert (g["disparity"] == pair.disparity.tobytes()) == const, n


def _far_start():
    """The `oob` idea of tests/test_gpu_image_alignment.py pushed to the end: every block leaves the image."""
    pair = bm.member("s4")[0]
    return synth.pose_pack(np.array([500.0 * 6.0 / pair.camera["fu"], 0.0, 0.0]), np.eye(3))


def test_a_member_that_ends_at_once_leaves_the_others_undisturbed():
    far = _far_start()
    pair, _, interp, const = bm.member("s4")
    prr = ir.ImageProblem(pair.camera, pair.ref, pair.track, pair.gradx, pair.grady, pair.disparity, interp, disp_const=const)
    q, iz, u, v = prr.project(far, pair.disparity.reshape(-1)[prr.blk])
    assert not prr.in_bounds(u, v).any()
    hs = [_handle("s1"), _handle("s4", far), _handle("8x6")]
    res = solve_image_batch(hs, _options())
    got = [_result(h, s, st) for h, (s, st) in zip(hs, res)]
    want_far = _solo("s4", far.tobytes())
    print("member out of bounds: status", want_far["status"], "termination", want_far["termination_type"], "entries", want_far["num_iterations"])
    _assert_same(got[0], _solo("s1"), "s1")
    _assert_same(got[1], want_far, "far")
    _assert_same(got[2], _solo("8x6"), "8x6")
    assert want_far["num_iterations"] < _solo("s1")["num_iterations"]


def test_65_handles_of_8x6():
    """More problems than lanes in a wave."""
    names = ["tiny%d" % s for s in range(65)]
    _, got = _batch(names)
    for n, g in zip(names, got):
        _assert_same(g, _solo(n), n)
    assert len({g["num_iterations"] for g in got}) > 1


def test_two_runs_of_the_same_batch_give_the_same_bits():
    _, a = _batch(SIX)
    _, b = _batch(SIX)
    assert a == b


@pytest.mark.parametrize("names,entries", [(("8x6", "blocks1025", "tiny2"), 9), (("s1", "s0free", "s4"), 8)], ids=["last-step-rejected", "last-step-accepted"])
def test_ignore_convergence_runs_every_member_the_same_count(names, entries):
    """ignore_convergence with max_num_iterations = 8 is eight rounds for every member: solve_begin(ignore_convergence) /
    solve_step(8) / solve_end alone.  The log then holds iteration 0 and one entry per judged step that has been written: a
    rejected step is logged by its own decision, an accepted one by the NEXT round's check.  So a member whose eighth step is
    rejected logs 9 entries (the first group) and one whose eighth step is accepted logs 8 (the second group; the ninth entry
    would come with a ninth round).  Either way the batch equals the stepwise solo solve to the bit."""
    o = _options(max_num_iterations=8)
    hs = [_handle(n) for n in names]
    res = solve_image_batch(hs, o, ignore_convergence=True)
    for n, h, (s, st) in zip(names, hs, res):
        ba = _handle(n)
        ba.solve_begin(o, ignore_convergence=True)
        ba.step(8)
        want = _result(ba, ba.solve_end(), 0)
        got = _result(h, s, st)
        print(n, "entries", got["num_iterations"])
        _assert_same(got, want, n)
        assert got["num_iterations"] == entries, n


def test_members_are_ordinary_handles_afterwards():
    names = ["s1", "s0free", "s4"]
    hs, got = _batch(names)
    # a stepwise solve with a restart in the middle, from the blocks' first values: the first solo result again
    for n, h in zip(names[:2], hs[:2]):
        pair, start, _, _ = bm.member(n)
        h.pose[:] = start
        h.disparity[:] = pair.disparity
        h.solve_begin(_options())
        h.step(3)
        h.restart()
        h.step(bm.MAX_ITER + 3)
        s = h.solve_end()
        _assert_same(_result(h, s, 0), _solo(n), n)
    # and ssba_solve on it
    pair, start, _, _ = bm.member("s4")
    hs[2].pose[:] = start
    s, _ = hs[2].solve(_options())
    _assert_same(_result(hs[2], s, 0), _solo("s4"), "s4")
    # covariance of a constant-disparity member at its solved pose: the same handle solved alone
    alone = _handle("s1")
    alone.solve(_options())
    hs[0].pose[:] = alone.pose
    assert hs[0].pose_covariance(0).tobytes() == alone.pose_covariance(0).tobytes()


def test_refusals_leave_the_handles_usable():
    lib = capi.load()
    a, b = _handle("s1"), _handle("8x6")
    o = _options()

    def call(handles, n=None, opts=o):
        arr = (C.c_void_p * max(len(handles), 1))(*[h if h is None or isinstance(h, (int, C.c_void_p)) else h.h for h in handles])
        rc = lib.ssba_image_solve_batch(arr, len(handles) if n is None else n, C.byref(opts), 0, None, None)
        return rc, lib.ssba_last_error().decode()

    before = [(h.pose.tobytes(), h.disparity.tobytes()) for h in (a, b)]
    rc, msg = call([a, b], n=0)
    assert rc == -1 and "ssba_image_solve_batch" in msg and "n = 0" in msg
    rc, msg = call([a, None, b])
    assert rc == -1 and "ssba_image_solve_batch" in msg and "handle 1" in msg and "NULL" in msg
    rc, msg = call([a, b, a])
    assert rc == -1 and "handle 2" in msg and "twice" in msg
    rc, msg = call([a] * 2, n=capi.IMAGE_BATCH_MAX + 1)
    assert rc == -1 and "cap" in msg and str(capi.IMAGE_BATCH_MAX) in msg
    # handles on different devices: checked where the machine shows a second one
    pair, start, interp, const = bm.member("s1")
    try:
        other = ImageAlignment(pair.camera, start.copy(), pair.disparity.copy(), pair.ref, pair.track, pair.gradx, pair.grady, device=1)
    except capi.SsbaError:
        other = None
    if other is not None:
        rc, msg = call([a, other])
        assert rc == -1 and "handle 1" in msg and "device" in msg
    # a stereo handle
    from ceres_slam_amd.solver import StereoBA
    stereo = StereoBA.from_synth(synth.make_problem(24, 600, track_len=8, seed=1))
    rc, msg = call([a, stereo])
    assert rc == -6 and "handle 1" in msg and "image blocks" in msg
    rc, msg = call([a, b], opts=_options(trust_region_strategy_type=capi.DOGLEG))
    assert rc == -6 and "DOGLEG" in msg and "ssba_image_solve_batch" in msg
    b.set_kernel_timing(True)
    rc, msg = call([a, b])
    assert rc == -6 and "handle 1" in msg and "timing" in msg
    b.set_kernel_timing(False)
    pair, start, interp, const = bm.member("s4")
    raw = ImageAlignment(pair.camera, start.copy(), pair.disparity.copy(), pair.ref, pair.track, pair.gradx, pair.grady, finalize=False)
    rc, msg = call([a, b, raw])
    assert rc == -7 and "handle 2" in msg and "finalized" in msg
    b.solve_begin(o)
    b.step(2)
    rc, msg = call([b, a])
    assert rc == -7 and "handle 0" in msg and "stepwise" in msg
    b.step(1)                      # the refusal did not end the stepwise solve
    b.solve_end()
    assert [(h.pose.tobytes(), h.disparity.tobytes()) for h in (a,)] == before[:1]
    b.pose[:] = bm.member("8x6")[1]
    got = [_result(h, s, st) for h, (s, st) in zip((a, b), solve_image_batch([a, b], o))]
    _assert_same(got[0], _solo("s1"), "s1")
    _assert_same(got[1], _solo("8x6"), "8x6")


# ---- coarse to fine over several pyramids ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(seed):
    if seed == 3:
        pair, ref_u8, track_u8, _ = pr.case_96x128()
        return pair, ref_u8, track_u8
    pair = synth.make_image_pair(96, 128, seed=seed, motion=10.0, min_wavelength_px=8.0)
    out = (pair, pr.quantise(pair.ref), pr.quantise(pair.track))
    for a in (out[1], out[2], pair.disparity, pair.pose_init):
        a.setflags(write=False)
    return out


def _pyramid(seed, disparity=None):
    pair, ref_u8, track_u8 = _case(seed)
    return ImagePyramid(ref_u8, track_u8, pair.disparity if disparity is None else disparity, 3, disparity_level=0,
                        gradient_source=capi.GRADIENT_OF_TRACKED, gradient_scale=0.125, camera=pair.camera)


SUMMARY_FIELDS = ("termination_type", "num_iterations", "num_successful_steps", "num_unsuccessful_steps", "initial_cost", "final_cost")


def _summary(s):
    return tuple(np.float64(getattr(s, f)).tobytes() for f in SUMMARY_FIELDS)


def test_align_batch_of_two_pyramids_against_two_solo_calls():
    o = _options()
    seeds = (3, 10)
    want = []
    for sd in seeds:
        pair = _case(sd)[0]
        pose, disp = pair.pose_init.copy(), pair.disparity.copy()
        rc, sums = _pyramid(sd).align(pose, disp, coarsest_level=2, disparity_const=True, options=o)
        assert rc == 0
        want.append((pose.tobytes(), disp.tobytes(), [_summary(s) for s in sums]))
    pyrs = [_pyramid(sd) for sd in seeds]
    poses = np.stack([_case(sd)[0].pose_init for sd in seeds]).copy()
    maps = [_case(sd)[0].disparity.copy() for sd in seeds]
    rc, sums, sts = ImagePyramid.align_batch(pyrs, poses, maps, coarsest_level=2, camera=_case(3)[0].camera, disparity_const=True, options=o)
    assert rc == 0 and sts == [0, 0]
    for k in range(2):
        assert (poses[k].tobytes(), maps[k].tobytes(), [_summary(s) for s in sums[k]]) == want[k], k
    assert want[0][0] != want[1][0]


def test_align_batch_with_free_base_disparities():
    pair = _case(3)[0]
    d0 = pair.disparity.copy()
    rng = np.random.Generator(np.random.PCG64(5))
    idx = rng.choice(d0.size, size=d0.size // 20, replace=False)
    d0.reshape(-1)[idx] = np.array([np.nan, 0.0, -1.5])[np.arange(idx.shape[0]) % 3]
    o = _options(max_num_iterations=20)
    pose, disp = pair.pose_init.copy(), d0.copy()
    rc, sums = _pyramid(3, d0).align(pose, disp, coarsest_level=2, disparity_const=False, options=o)
    assert rc == 0
    poses, maps = pair.pose_init.copy().reshape(1, 12), [d0.copy()]
    rc, bsums, sts = ImagePyramid.align_batch([_pyramid(3, d0)], poses, maps, coarsest_level=2, disparity_const=False, options=o)
    assert rc == 0 and sts == [0]
    assert poses[0].tobytes() == pose.tobytes() and maps[0].tobytes() == disp.tobytes()
    assert [_summary(s) for s in bsums[0]] == [_summary(s) for s in sums]
    assert maps[0].tobytes() != d0.tobytes()


def test_align_batch_refusals():
    lib = capi.load()
    pair = _case(3)[0]
    p3 = _pyramid(3)
    small = synth.make_image_pair(24, 32, seed=1)
    p2 = ImagePyramid(pr.quantise(small.ref), pr.quantise(small.track), small.disparity, 2, camera=small.camera)          # two levels only
    p_dl = ImagePyramid(_case(3)[1], _case(3)[2], np.ascontiguousarray(pair.disparity[::2, ::2]) / 2, 3, disparity_level=1, camera=pair.camera)
    cam = capi.Camera(**pair.camera)
    o = _options()
    poses = np.stack([pair.pose_init, pair.pose_init]).copy()

    def call(pyrs, maps, n=None, top=2, interp=1, opts=o):
        hs = (C.c_void_p * 2)(*[p if p is None else p.h for p in pyrs])
        mp = (capi._dp * 2)(*[m if m is None else capi.dptr(m) for m in maps])
        rc = lib.ssba_image_pyramid_align_batch(hs, len(pyrs) if n is None else n, C.byref(cam), capi.dptr(poses), mp, top, interp, 1, C.byref(opts), None, None)
        return rc, lib.ssba_last_error().decode()

    m3, m2, mdl = pair.disparity.copy(), small.disparity.copy(), np.ascontiguousarray(pair.disparity[::2, ::2]) / 2
    name = "ssba_image_pyramid_align_batch"
    for rc, msg, word in [call([p3, p3], [m3, m3], n=0) + ("n = 0",), call([p3, None], [m3, m3]) + ("pyramid 1",),
                          call([p3, p3], [m3, None]) + ("pyramid 1",), call([p3, p2], [m3, m2]) + ("no such level",),
                          call([p3, p_dl], [m3, mdl]) + ("disparity_level",), call([p3, p3], [m3, m3], interp=2) + ("interpolation",)]:
        assert rc == -1 and name in msg and word in msg, (rc, msg, word)
    rc, msg = call([p3, p3], [m3, m3], opts=_options(trust_region_strategy_type=capi.DOGLEG))
    assert rc == -6 and name in msg and "DOGLEG" in msg
    assert poses.tobytes() == np.stack([pair.pose_init, pair.pose_init]).tobytes() and m3.tobytes() == pair.disparity.tobytes()


# ---- the sequence example -------------------------------------------------------------------------------------------------------
def test_sequence_example_batched_and_sequential_print_the_same_bytes(tmp_path):
    """examples/dense_stereo_sequence_gpu.cpp on a 4-frame 96 x 128 sequence: three pyramids built from the raw frames (the matcher
    on the device), aligned coarse to fine in one batched call, and one by one with --sequential."""
    exe = build.build_examples("dense_stereo_sequence_gpu")
    seq = synth.make_stereo_sequence(96, 128, 4, seed=10, motion=5.0, min_wavelength_px=8.0)
    assert seq.left.shape == (4, 96, 128) and seq.left.dtype == np.uint8 and (seq.left[0] != seq.left[1]).any() and (seq.left[0] != seq.right[0]).any()
    raw = tmp_path / "sequence.raw"
    synth.write_stereo_sequence(str(raw), seq, 3, 0, bytes(capi.sgbm_params(num_disparities=16, block_size=15)))
    outs = []
    for extra in ([], ["--sequential"]):
        r = subprocess.run([exe, str(raw)] + extra, capture_output=True, timeout=120)
        assert r.returncode == 0, r.stdout.decode() + r.stderr.decode()
        outs.append(r.stdout)
    assert outs[0] == outs[1]
    lines = outs[0].decode().strip().splitlines()
    assert [ln.split()[:2] for ln in lines] == [["frame", str(k)] for k in range(4)]
    T = np.array([[float(x) for x in ln.split()[2:]] for ln in lines])
    assert T[0].tolist() == [0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1] and (T[1] != T[0]).any() and (T[3] != T[2]).any()
    print("trajectory against the rendered one, largest translation error:", float(np.abs(T[:, :3] - seq.poses_true[:, :3]).max()))


# ---- the solo path against the parent commit ---------------------------------------------------------------------------------
def test_the_solo_path_gives_the_recorded_bits():
    """tests/golden/image_batch_solo.json was recorded by tests/golden/record_image_batch_solo.py on the commit before the solo
    kernels became wrappers over the shared bodies."""
    import importlib.util
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location("record_image_batch_solo", os.path.join(here, "golden", "record_image_batch_solo.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    with open(os.path.join(here, "golden", "image_batch_solo.json")) as f:
        want = json.load(f)
    assert len(want) == 12
    for key, w in want.items():
        name, interp, const = key.split("/")
        got = rec.record(name, 1 if interp == "bilinear" else 0, const == "const")
        assert got == w, key
