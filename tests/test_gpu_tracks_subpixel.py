"""Sub-pixel feature tracks on the device (libssba_tracks.so: ssba_track_refine, ssba_track_sequence_subpixel; k_tr_anchor,
k_tr_refine and k_tr_refine_items of ceres_slam_amd/csrc/ssba_tracks.hip) against the numpy statement
tests/tracks_refine_reference.py.

The sums are integers and the step is a handful of IEEE double operations that numpy performs alike, so every bar here is
equality to the bit.  SSBA_TRACK_REFINE_DISPARITY arises in the sequence only and needs a mismatch that the refinement then
contradicts; the CPU tests produce it on the statement, here it occurs only if a sequence below happens to hold one."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

import tracks_refine_cases as tc
import tracks_refine_reference as rr
from ceres_slam_amd import build, capi, synth, tracks
from ceres_slam_amd.solver import StereoBA
from test_gpu_tracks import PARAMS, SGBM, _disp16, _pair_translation_errors, _sequence, _solve_from_tracks

pytestmark = pytest.mark.gpu


# ---- track_refine ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stack(rows, cols):
    """A texture, four displaced views of it (one noisy), a constant image and a texture of rows."""
    s = np.stack([tc.sinusoids(rows, cols), tc.sinusoids(rows, cols, (0.5, 0.25)), tc.sinusoids(rows, cols, (1.4, -0.7), noise=2),
                  tc.sinusoids(rows, cols, (-3.3, 0.8)), tc.sinusoids(rows, cols, (2.6, 1.5)), np.full((rows, cols), 90, np.uint8),
                  tc.sinusoids(rows, cols, y_only=True)])
    s.setflags(write=False)
    return s


STACK_SHIFTS = [(0.0, 0.0), (0.5, 0.25), (1.4, -0.7), (-3.3, 0.8), (2.6, 1.5)]


@functools.lru_cache(maxsize=None)
def _items(rows, cols, n):
    """n seeded items, both modes mixed: anchors anywhere in the texture (some too close to the edge), targets any image of the
    stack, starts at the rounded shift plus up to two pixels and a fraction."""
    rng = np.random.Generator(np.random.PCG64(100 * rows + n))
    out = []
    for _ in range(n):
        ax, ay = int(rng.integers(6, cols - 6)), int(rng.integers(6, rows - 6))
        b = int(rng.integers(0, 7))
        sx, sy = STACK_SHIFTS[b] if b < 5 else (0.0, 0.0)
        x0 = 256 * (ax + int(np.rint(sx)) + int(rng.integers(-2, 3))) + int(rng.integers(-128, 129))
        y0 = 256 * (ay + int(np.rint(sy)) + int(rng.integers(-2, 3))) + int(rng.integers(-128, 129))
        out.append([0 if rng.random() < 0.9 else int(rng.integers(5, 7)), ax, ay, b, x0, y0, int(rng.integers(0, 2))])
    a = np.array(out, np.int32).reshape(-1, 7)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _want(rows, cols, n, **kw):
    return rr.refine(_stack(rows, cols), _items(rows, cols, n), **kw)


def _same_refinement(got, want):
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[2].dtype == np.uint32
    assert got[1].tobytes() == want[1].tobytes(), (got[1], want[1])
    assert got[0].tobytes() == want[0].tobytes() and got[2].tobytes() == want[2].tobytes(), (got, want)


@pytest.mark.parametrize("n", [1, 4, 5, 130])
@pytest.mark.parametrize("rows,cols", [(40, 56), (37, 131)])
def test_refine_items_equal_the_numpy_statement(rows, cols, n):
    want = _want(rows, cols, n)
    got = tracks.track_refine(_stack(rows, cols), _items(rows, cols, n))
    print(f"{rows}x{cols}, {n} items: statuses {np.bincount(want[1], minlength=7).tolist()}")
    _same_refinement(got, want)
    if n == 130:
        counts = np.bincount(want[1], minlength=7)
        assert counts[rr.OK] > 30 and counts[rr.EDGE] > 0 and counts[rr.FLAT] > 0 and (_items(rows, cols, n)[:, 6] == 1).sum() > 30


def test_refine_parameters_reach_the_kernel():
    for kw in (dict(iterations=2), dict(max_shift=1), dict(max_shift=8, iterations=64), dict(max_sad=150)):
        want = _want(40, 56, 130, **kw)
        _same_refinement(tracks.track_refine(_stack(40, 56), _items(40, 56, 130), **kw), want)
        assert want[1].tobytes() != _want(40, 56, 130)[1].tobytes(), kw      # the parameter changes the outcome of some item


def test_every_status_at_its_boundary():
    stack, seen = tc.status_stack(), set()
    for name, item, kw, expected in tc.status_cases():
        want = rr.refine(stack, [item], **kw)
        got = tracks.track_refine(stack, [item], **kw)
        print(f"{name}: status {got[1][0]}, position {got[0][0].tolist()}, sad {got[2][0]}")
        _same_refinement(got, want)
        assert got[1][0] == expected, name
        seen.add(int(got[1][0]))
    assert seen == {rr.OK, rr.EDGE, rr.FLAT, rr.FAR, rr.ITERATIONS, rr.SAD}


def test_a_stack_equals_solo_calls_and_two_runs_are_bit_equal():
    stack, items = _stack(40, 56), _items(40, 56, 130)
    a, b = tracks.track_refine(stack, items), tracks.track_refine(stack, items)
    _same_refinement(a, b)
    for k in (0, 1, 2, 3, 64, 129):
        pair = np.stack([stack[items[k, 0]], stack[items[k, 3]]])
        item = items[k].copy()
        item[0], item[3] = 0, 1
        solo = tracks.track_refine(pair, [item])
        assert all(s[0].tobytes() == g[k].tobytes() for s, g in zip(solo, a)), k
    empty = tracks.track_refine(stack, np.zeros((0, 7), np.int32))
    assert empty[0].shape == (0, 2) and empty[1].shape == (0,)


# ---- the sequence ------------------------------------------------------------------------------------------------------------
def _frames(rows, cols, source, frames):
    s = _sequence(rows, cols)
    return s.left[:frames], (dict(right=s.right[:frames]) if source == "right" else dict(disp16=_disp16(rows, cols)[:frames]))


@functools.lru_cache(maxsize=None)
def _reference(rows, cols, source, frames=4, min_track_length=2, temporal_radius=0, max_sad=0):
    left, kw = _frames(rows, cols, source, frames)
    out = rr.sequence_subpixel(left, refine=dict(max_sad=max_sad), min_track_length=min_track_length, temporal_radius=temporal_radius, **kw, **PARAMS)
    for a in out[:3]:
        a.setflags(write=False)
    return out


def _device(rows, cols, source, frames=4, max_sad=0, **extra):
    left, kw = _frames(rows, cols, source, frames)
    return tracks.track_sequence_subpixel(left, refine=dict(max_sad=max_sad), **kw, **PARAMS, **extra)


def _same_tracks(got, want):
    assert got[0].dtype == np.uint32 and got[1].dtype == np.uint32 and got[2].dtype == np.float64
    assert got[0].tobytes() == want[0].tobytes(), (got[0], want[0])
    assert got[4] == want[4], (got[4], want[4])
    assert got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes() and got[3] == want[3]


def _tied_to_the_old_call(got, old, max_shift=4):
    """Nothing dropped: the same observations of the same tracks as track_sequence, each within max_shift of its keypoint."""
    assert got[4] == 0
    assert got[0].tobytes() == old[0].tobytes() and got[1].tobytes() == old[1].tobytes() and got[3] == old[3]
    assert (np.abs(got[2][:, :2] - old[2][:, :2]) <= max_shift).all()
    assert (got[2][:, :2] * 256 % 1 == 0).all() and (got[2][:, :2] % 1 != 0).any()


@pytest.mark.parametrize("source", ["right", "disp16"])
@pytest.mark.parametrize("rows,cols", [(64, 96), (96, 128)])
def test_sequence_equals_the_numpy_statement(rows, cols, source):
    want = _reference(rows, cols, source)
    got = _device(rows, cols, source)
    print(f"{rows}x{cols} {source}: state_start {got[0].tolist()}, {got[3]} tracks, {got[4]} dropped; statuses "
          f"{np.bincount(np.concatenate(want[5]), minlength=7).tolist()}")
    _same_tracks(got, want)
    assert got[3] > 30
    if got[4] == 0:
        left, kw = _frames(rows, cols, source, 4)
        old = tracks.track_sequence(left, **kw, **PARAMS)
        _tied_to_the_old_call(got, old)
        if source == "disp16":
            assert got[2][:, 2].tobytes() == old[2][:, 2].tobytes()           # the map's disparity stays


@pytest.mark.parametrize("frames", [1, 2])
def test_one_and_two_frames(frames):
    for min_track_length in (1, 2):
        want = _reference(64, 96, "right", frames, min_track_length)
        _same_tracks(_device(64, 96, "right", frames, min_track_length=min_track_length), want)
    assert _reference(64, 96, "right", 1, 2)[3] == 0 and _reference(64, 96, "right", 1, 1)[3] > 30


@pytest.mark.parametrize("min_track_length", [1, 2, 3])
def test_min_track_length(min_track_length):
    want = _reference(96, 128, "right", 4, min_track_length)
    _same_tracks(_device(96, 128, "right", min_track_length=min_track_length), want)
    lengths = np.bincount(want[1], minlength=want[3])
    assert lengths.min() >= min_track_length and (lengths == min_track_length).any()


@pytest.mark.parametrize("temporal_radius", [0, 8])
@pytest.mark.parametrize("max_sad", [0, 2000])
def test_the_sad_gate_and_the_temporal_gate(max_sad, temporal_radius):
    """max_sad 2000 without a temporal gate drops observations (mismatches whose patches differ): ids are masked, lengths fall and
    the pruning acts on what remains.  min_track_length 3 makes the shortened tracks visible."""
    for min_track_length in (2, 3):
        want = _reference(96, 128, "right", 4, min_track_length, temporal_radius, max_sad)
        got = _device(96, 128, "right", max_sad=max_sad, temporal_radius=temporal_radius, min_track_length=min_track_length)
        print(f"max_sad {max_sad}, temporal_radius {temporal_radius}, min_track_length {min_track_length}: {len(got[1])} observations, {got[4]} dropped")
        _same_tracks(got, want)
    if max_sad and not temporal_radius:
        assert got[4] > 0
    if not max_sad:
        assert got[4] == 0


def test_a_constant_frame_in_the_middle_ends_and_restarts_the_tracks():
    s = _sequence(64, 96)
    left, right = s.left.copy(), s.right.copy()
    left[2] = right[2] = 90
    left = np.concatenate([left, s.left[3:]])                    # frames 0 1 | constant | 3 3: tracks on both sides of the gap
    right = np.concatenate([right, s.right[3:]])
    want = rr.sequence_subpixel(left, right, **PARAMS)
    got = tracks.track_sequence_subpixel(left, right, **PARAMS)
    _same_tracks(got, want)
    assert got[0][2] == got[0][3] and got[0][1] > 0 and got[0][5] > got[0][4] > got[0][3]
    # frames 3 and 4 are the same image: the refinement of frame 4 against the anchors of frame 3 returns the keypoints exactly
    n3 = got[0][4] - got[0][3]
    both = np.intersect1d(got[1][got[0][3]:got[0][4]], got[1][got[0][4]:], return_indices=True)
    assert n3 > 0 and len(both[0]) > 10
    assert (got[2][got[0][3]:got[0][4]][both[1]] == got[2][got[0][4]:][both[2]]).all()


def test_capacity_one_short_is_refused_and_nothing_is_written():
    s = _sequence(64, 96)
    want = _reference(64, 96, "right")
    need = len(want[1])
    lib, p, rp = tracks.load(), tracks.track_params(**PARAMS), tracks.refine_params()
    start, ids, uvd = np.full(5, 7, np.uint32), np.full(need, 7, np.uint32), np.full((need, 3), 7.0)
    nobs, npts, ndrop = C.c_uint64(7), C.c_uint32(7), C.c_uint64(7)
    args = lambda cap: (s.left.ctypes.data_as(tracks._u8p), s.right.ctypes.data_as(tracks._u8p), None, 4, 64, 96, C.byref(p), -1, cap,
                        start.ctypes.data_as(tracks._u32p), ids.ctypes.data_as(tracks._u32p), uvd.ctypes.data_as(tracks._dp), C.byref(nobs), C.byref(npts),
                        C.byref(rp), C.byref(ndrop))
    assert lib.ssba_track_sequence_subpixel(*args(need - 1)) == -1
    msg = lib.ssba_track_last_error().decode()
    assert msg.startswith("ssba_track_sequence_subpixel: ") and str(need) in msg
    assert (start == 7).all() and (ids == 7).all() and (uvd == 7.0).all() and nobs.value == 7 and npts.value == 7 and ndrop.value == 7
    with pytest.raises(capi.SsbaError):
        tracks.track_sequence_subpixel(s.left, s.right, capacity=need - 1, **PARAMS)
    assert lib.ssba_track_sequence_subpixel(*args(need)) == 0    # exactly enough; the library is usable after the refusal
    assert nobs.value == need and ndrop.value == want[4] and ids.tobytes() == want[1].tobytes() and uvd.tobytes() == want[2].tobytes()


def test_two_runs_are_bit_equal_and_the_old_call_is_untouched():
    a, b = _device(96, 128, "right", max_sad=2000), _device(96, 128, "right", max_sad=2000)
    _same_tracks(a, b)
    left, kw = _frames(96, 128, "right", 4)
    before = tracks.track_sequence(left, **kw, **PARAMS)
    _device(96, 128, "right")
    after = tracks.track_sequence(left, **kw, **PARAMS)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(before[:3], after[:3]))


# ---- end to end --------------------------------------------------------------------------------------------------------------
END_TO_END = dict(temporal_radius=8)


def test_subpixel_tracks_to_front_end_to_bundle_adjustment():
    """Tracks -> ssba_frontend_vo -> solve with temporal_radius 8: the device's tracks give the poses of the statement's tracks to
    the bit, and the summed per-pair translation error from sub-pixel tracks is below that from whole-pixel tracks under the same
    settings (both printed)."""
    s = _sequence(96, 128)
    want = _reference(96, 128, "right", 4, 2, 8, 0)
    got = _device(96, 128, "right", **END_TO_END)
    _same_tracks(got, want)
    poses, summary, stats = _solve_from_tracks(s.camera, *got[:4])
    poses_ref, _, _ = _solve_from_tracks(s.camera, *want[:4])
    assert poses.tobytes() == poses_ref.tobytes()
    whole = tracks.track_sequence(s.left, s.right, **PARAMS, **END_TO_END)
    poses_whole, summary_whole, _ = _solve_from_tracks(s.camera, *whole)
    e_sub, e_whole = _pair_translation_errors(poses, s.poses_true), _pair_translation_errors(poses_whole, s.poses_true)
    step = float(np.linalg.norm(s.poses_true[1][:3]))
    print(f"true step {step:.5f}; sub-pixel: {StereoBA.brief_report(summary)}; front end {stats}; per-pair translation error {['%.5f' % e for e in e_sub]}, sum {sum(e_sub):.5f}")
    print(f"whole pixel: {StereoBA.brief_report(summary_whole)}; per-pair translation error {['%.5f' % e for e in e_whole]}, sum {sum(e_whole):.5f}")
    assert sum(e_sub) < sum(e_whole)


def test_example_with_subpixel_prints_the_trajectory_of_the_python_route(tmp_path):
    exe = build.build_examples("sparse_stereo_sequence_gpu", "ssba_tracks")
    s = _sequence(96, 128)
    raw = tmp_path / "sequence.raw"
    synth.write_stereo_sequence(str(raw), s, 3, 0, bytes(capi.sgbm_params(**SGBM)))
    r = subprocess.run([exe, str(raw), "--fast-threshold", "10", "--subpixel", "--temporal-radius", "8", "--max-sad", "2000"], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stdout.decode() + r.stderr.decode()
    lines = r.stdout.decode().strip().splitlines()
    assert [ln.split()[:2] for ln in lines] == [["frame", str(k)] for k in range(4)]
    T = np.array([[float(x) for x in ln.split()[2:]] for ln in lines])
    poses, _, _ = _solve_from_tracks(s.camera, *_device(96, 128, "right", max_sad=2000, **END_TO_END)[:4])
    assert T.tobytes() == poses.tobytes()
    assert T[0].tolist() == [0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1] and (T[3] != T[2]).any()
