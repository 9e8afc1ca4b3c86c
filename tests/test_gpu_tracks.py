"""Sparse stereo feature tracks on the device (libssba_tracks.so: ssba_track_features, ssba_track_match, ssba_track_sequence;
ceres_slam_amd/csrc/ssba_tracks.hip) against the numpy statement tests/tracks_reference.py.

Everything is integer arithmetic, so every bar here is equality to the bit; there is no tolerance anywhere.

The sequences are synth.make_stereo_sequence(64, 96, 4, seed=1) and (96, 128, 4, seed=1) with fast_threshold 10.  The numpy
statement, run on the CPU with the committed pattern, gives 45, 50, 51, 49 stereo survivors per frame and 40, 43, 40 temporal
matches per pair at 64 x 96, and 135, 134, 141, 138 survivors and 113, 118, 120 matches at 96 x 128: every pair has far more
than the 3 matches ssba_frontend_vo needs."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

import tracks_reference as tr
from ceres_slam_amd import build, capi, frontend, synth, tracks
from ceres_slam_amd.solver import StereoBA, stereo_sgbm_batch

pytestmark = pytest.mark.gpu


# ---- features ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _noise_and_blocks(rows, cols, seed):
    """Mild noise with bright and dark rectangles: corners of every sign, flat regions, equal scores in plenty.  Never written."""
    rng = np.random.Generator(np.random.PCG64(seed))
    img = 110 + rng.integers(-6, 7, (rows, cols))
    for _ in range(rows * cols // 60):
        y, x = int(rng.integers(0, rows - 3)), int(rng.integers(0, cols - 3))
        h, w = int(rng.integers(2, 9)), int(rng.integers(2, 9))
        img[y:y + h, x:x + w] = int(rng.choice([30, 60, 170, 220]))
    img = np.clip(img, 0, 255).astype(np.uint8)
    img.setflags(write=False)
    return img


def _arc_images():
    out = np.full((32, 33, 33), 100, np.uint8)
    for a in range(16):
        for k in range(9):
            dx, dy = tr.RING[(a + k) % 16]
            out[a, 16 + dy, 16 + dx] = 160
            out[16 + a, 16 + dy, 16 + dx] = 30
    return out


def _check_features(images, **params):
    images = np.asarray(images)
    if images.ndim == 2:
        images = images[None]
    count, xy, score, desc = tracks.track_features(images, **params)
    m = tr.params(**params)["max_features"]
    assert xy.shape == (len(images), m, 2) and score.shape == (len(images), m) and desc.shape == (len(images), m, 8)
    for k, img in enumerate(images):
        wxy, wsc, wdesc = tr.features(img, **params)
        n = int(count[k])
        print(f"image {k} of {images.shape}: {n} keypoints on the device, {len(wxy)} in the numpy statement")
        assert n == len(wxy)
        assert xy[k, :n].tobytes() == wxy.tobytes() and score[k, :n].tobytes() == wsc.tobytes() and desc[k, :n].tobytes() == wdesc.tobytes()
        assert not xy[k, n:].any() and not score[k, n:].any() and not desc[k, n:].any()
    return count, xy, score, desc


def test_smallest_legal_image_has_one_keypoint_position():
    img = np.full((31, 31), 100, np.uint8)
    for k in range(9):
        dx, dy = tr.RING[(14 + k) % 16]                          # an arc that wraps 15 -> 0
        img[15 + dy, 15 + dx] = 190
    count, xy, score, _ = _check_features(img, fast_threshold=20, max_features=4)
    assert count.tolist() == [1] and xy[0, 0].tolist() == [15, 15] and score[0, 0] == 90


@pytest.mark.parametrize("rows,cols", [(40, 56), (37, 131)])
def test_features_on_noise_and_blocks(rows, cols):
    count, _, _, _ = _check_features(_noise_and_blocks(rows, cols, rows), fast_threshold=12, max_features=500)
    assert count[0] >= 8


def test_every_arc_start_bright_and_dark():
    count, xy, score, _ = _check_features(_arc_images(), fast_threshold=20, max_features=16)
    assert (count >= 1).all()
    for k in range(32):
        i = xy[k, :count[k]].tolist().index([16, 16])
        assert score[k, i] == (60 if k < 16 else 70)


def test_max_features_cuts_through_equal_scores():
    img = _noise_and_blocks(64, 200, 8)
    kept = tr.suppress(tr.scores(img, 12))
    values = np.sort(kept[kept > 0])[::-1]
    assert len(values) > 8 and values[7] == values[8], "the cut must fall between equal scores for this test to mean anything"
    count, _, _, _ = _check_features(img, fast_threshold=12, max_features=8)
    assert count.tolist() == [8]


def test_constant_image_has_no_keypoint_and_a_stack_equals_solo_calls():
    flat = np.full((40, 56), 77, np.uint8)
    count, _, _, _ = _check_features(flat, fast_threshold=0, max_features=32)
    assert count.tolist() == [0]
    stack = np.stack([_noise_and_blocks(40, 56, 40), flat, _noise_and_blocks(40, 56, 41)])
    got = _check_features(stack, fast_threshold=12, max_features=64)
    for k in range(3):
        solo = tracks.track_features(stack[k], fast_threshold=12, max_features=64)
        assert all(g[k].tobytes() == s[0].tobytes() for g, s in zip(got, solo)), k
    assert got[0][0] > 0 and got[0][1] == 0 and got[0][2] > 0


# ---- the matcher -------------------------------------------------------------------------------------------------------------
def _descriptors(n, seed, near=None):
    """n random descriptors; with `near`, copies of those with a few bits flipped, so that real matches exist."""
    rng = np.random.Generator(np.random.PCG64(seed))
    d = rng.integers(0, 1 << 32, (n, 8), dtype=np.uint64).astype(np.uint32)
    if near is not None and len(near) and n:
        src = rng.permutation(len(near))[:n]
        d[:len(src)] = near[src]
        for k in range(len(src)):
            for bit in rng.integers(0, 256, int(rng.integers(0, 12))):
                d[k, bit // 32] ^= np.uint32(1 << (bit % 32))
    xy = np.stack([rng.integers(15, 400, n), rng.integers(15, 60, n)], axis=1).astype(np.uint16)
    return d, xy


def _check_match(da, pa, db, pb, gate=tracks.GATE_NONE, **params):
    got = tracks.track_match(da, pa, db, pb, gate, **params)
    want = tr.match(da, pa, db, pb, gate, **params)
    assert got[0].dtype == np.int32 and got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), (got, want)
    return got


@pytest.mark.parametrize("na", [0, 1, 63, 65, 130])
def test_match_sizes_against_the_numpy_statement(na):
    matched = 0
    for nb in (0, 1, 63, 65, 130):
        db, pb = _descriptors(nb, 100 + nb)
        da, pa = _descriptors(na, 7 + na, near=db)
        for gate, kw in ((tracks.GATE_NONE, {}), (tracks.GATE_STEREO, dict(max_disparity=200, stereo_max_dy=12)), (tracks.GATE_TEMPORAL, dict(temporal_radius=90))):
            m, _ = _check_match(da, pa, db, pb, gate, max_hamming=80, **kw)
            matched += int((m >= 0).sum())
    assert matched > 0 or na == 0


def test_match_across_more_than_one_train_tile():
    db, pb = _descriptors(1100, 1)                                # three tiles of 512 on the train side, five query work-groups
    da, pa = _descriptors(1200, 2, near=db)
    m, _ = _check_match(da, pa, db, pb, max_hamming=64)
    assert (m >= 0).sum() > 500 and (m >= 512).any() and (m >= 1024).any()


def test_duplicates_the_cross_check_and_the_distance_bound():
    zero = np.zeros(8, np.uint32)
    one, three = zero.copy(), zero.copy()
    one[7], three[0] = 1 << 31, 0b111
    xy = np.array([[40 + k, 20] for k in range(4)], np.uint16)
    # duplicates on both sides: the tie goes to the smaller index on both sides, so only (0, 0) matches
    m, d = _check_match(np.stack([zero, zero]), xy[:2], np.stack([zero, zero, three]), xy[:3])
    assert m.tolist() == [0, -1] and d.tolist() == [0, -1]
    # a1's best is b0, but b0 prefers a0: a1 fails only the cross-check
    m, d = _check_match(np.stack([zero, one]), xy[:2], np.stack([zero]), xy[:1])
    assert m.tolist() == [0, -1]
    # a distance exactly at max_hamming and one above
    m, d = _check_match(np.stack([three]), xy[:1], np.stack([zero]), xy[:1], max_hamming=3)
    assert m.tolist() == [0] and d.tolist() == [3]
    m, d = _check_match(np.stack([three]), xy[:1], np.stack([zero]), xy[:1], max_hamming=2)
    assert m.tolist() == [-1] and d.tolist() == [-1]
    m, d = _check_match(np.stack([~zero]), xy[:1], np.stack([zero]), xy[:1], max_hamming=256)
    assert d.tolist() == [256]


def test_each_gate_at_its_boundary():
    d = np.zeros((1, 8), np.uint32)
    a = np.array([[100, 50]], np.uint16)
    stereo = dict(stereo_max_dy=5, max_disparity=40)
    for b, ok in (([90, 54], True), ([90, 55], False), ([90, 46], True), ([90, 45], False), ([100, 50], False), ([99, 50], True), ([60, 50], True),
                  ([59, 50], False), ([101, 50], False)):
        m, _ = _check_match(d, a, d, np.array([b], np.uint16), tracks.GATE_STEREO, **stereo)
        assert (m[0] == 0) == ok, b
    for b, ok in (([107, 43], True), ([108, 50], False), ([100, 58], False), ([93, 57], True), ([92, 50], False)):
        m, _ = _check_match(d, a, d, np.array([b], np.uint16), tracks.GATE_TEMPORAL, temporal_radius=7)
        assert (m[0] == 0) == ok, b
    m, _ = _check_match(d, a, d, np.array([[400, 15]], np.uint16), tracks.GATE_TEMPORAL, temporal_radius=0)      # 0: no gate
    assert m[0] == 0
    # the gate acts inside the search: the global best (distance 0) lies off the epipolar line, the gated best is taken instead
    db = np.zeros((2, 8), np.uint32)
    db[1, 0] = 0b11
    m, dist = _check_match(d, a, db, np.array([[90, 70], [90, 50]], np.uint16), tracks.GATE_STEREO, **stereo)
    assert m.tolist() == [1] and dist.tolist() == [2]


# ---- the sequence ------------------------------------------------------------------------------------------------------------
PARAMS = dict(fast_threshold=10)
SGBM = dict(num_disparities=16, block_size=15)


@functools.lru_cache(maxsize=None)
def _sequence(rows, cols):
    seq = synth.make_stereo_sequence(rows, cols, 4, seed=1)
    for a in (seq.left, seq.right, seq.poses_true):
        a.setflags(write=False)
    return seq


@functools.lru_cache(maxsize=None)
def _disp16(rows, cols):
    s = _sequence(rows, cols)
    d16, _ = stereo_sgbm_batch(s.left, s.right, **SGBM)
    d16.setflags(write=False)
    return d16


@functools.lru_cache(maxsize=None)
def _reference(rows, cols, source, frames=4, min_track_length=2):
    s = _sequence(rows, cols)
    kw = dict(right=s.right[:frames]) if source == "right" else dict(disp16=_disp16(rows, cols)[:frames])
    out = tr.sequence(s.left[:frames], min_track_length=min_track_length, **kw, **PARAMS)
    for a in out[:3]:
        a.setflags(write=False)
    return out


def _device(rows, cols, source, frames=4, **extra):
    s = _sequence(rows, cols)
    kw = dict(right=s.right[:frames]) if source == "right" else dict(disp16=_disp16(rows, cols)[:frames])
    return tracks.track_sequence(s.left[:frames], **kw, **PARAMS, **extra)


def _same_tracks(got, want):
    assert got[0].dtype == np.uint32 and got[1].dtype == np.uint32 and got[2].dtype == np.float64
    assert got[0].tobytes() == want[0].tobytes(), (got[0], want[0])
    assert got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes() and got[3] == want[3]


@pytest.mark.parametrize("source", ["right", "disp16"])
@pytest.mark.parametrize("rows,cols", [(64, 96), (96, 128)])
def test_sequence_equals_the_numpy_statement(rows, cols, source):
    want = _reference(rows, cols, source)
    got = _device(rows, cols, source)
    print(f"{rows}x{cols} {source}: state_start {got[0].tolist()}, {got[3]} tracks; before pruning {want[4]}")
    _same_tracks(got, want)
    assert min(want[4]["temporal"]) > 3 and got[3] > 30
    if source == "disp16":
        assert (got[2][:, 2] * 16 % 16 != 0).any()                 # sub-pixel disparities arrive


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


def test_a_constant_frame_in_the_middle_ends_and_restarts_the_tracks():
    s = _sequence(64, 96)
    left, right = s.left.copy(), s.right.copy()
    left[2] = right[2] = 90
    left = np.concatenate([left, s.left[3:]])                    # frames 0 1 | constant | 3 3: tracks on both sides of the gap
    right = np.concatenate([right, s.right[3:]])
    want = tr.sequence(left, right, **PARAMS)
    got = tracks.track_sequence(left, right, **PARAMS)
    _same_tracks(got, want)
    assert got[0][2] == got[0][3] and got[0][1] > 0 and got[0][5] > got[0][4] > got[0][3]
    first_after = got[1][got[0][3]:].min()
    assert first_after > got[1][:got[0][2]].max()                # no id crosses the empty frame


def test_capacity_one_short_is_refused_and_nothing_is_written():
    s = _sequence(64, 96)
    want = _reference(64, 96, "right")
    need = len(want[1])
    lib, p = tracks.load(), tracks.track_params(**PARAMS)
    start, ids, uvd = np.full(5, 7, np.uint32), np.full(need, 7, np.uint32), np.full((need, 3), 7.0)
    nobs, npts = C.c_uint64(7), C.c_uint32(7)
    args = lambda cap: (s.left.ctypes.data_as(tracks._u8p), s.right.ctypes.data_as(tracks._u8p), None, 4, 64, 96, C.byref(p), -1, cap,
                        start.ctypes.data_as(tracks._u32p), ids.ctypes.data_as(tracks._u32p), uvd.ctypes.data_as(tracks._dp), C.byref(nobs), C.byref(npts))
    assert lib.ssba_track_sequence(*args(need - 1)) == -1
    msg = lib.ssba_track_last_error().decode()
    assert msg.startswith("ssba_track_sequence: ") and str(need) in msg
    assert (start == 7).all() and (ids == 7).all() and (uvd == 7.0).all() and nobs.value == 7 and npts.value == 7
    with pytest.raises(capi.SsbaError):
        tracks.track_sequence(s.left, s.right, capacity=need - 1, **PARAMS)
    assert lib.ssba_track_sequence(*args(need)) == 0             # exactly enough; the library is usable after the refusal
    assert nobs.value == need and ids.tobytes() == want[1].tobytes() and uvd.tobytes() == want[2].tobytes()
    assert lib.ssba_track_sequence(*args(need)[:7], -1 + (1 << 20), *args(need)[8:]) == -1      # no such device


def test_two_runs_are_bit_equal():
    a, b = _device(96, 128, "right"), _device(96, 128, "right")
    _same_tracks(a, b)


# ---- end to end --------------------------------------------------------------------------------------------------------------
def _variant():
    return 1 if int(subprocess.run(["g++", "-dumpversion"], capture_output=True, text=True).stdout.split(".")[0]) >= 11 else 0


def _solve_from_tracks(camera, state_start, point_id, uvd, num_points):
    """Tracks -> ssba_frontend_vo -> StereoBA.solve, with the blocks numbered as the C++ shim numbers them (initialised points in
    order of first appearance, which is id order here)."""
    F = len(state_start) - 1
    obs_state = np.repeat(np.arange(F, dtype=np.uint32), np.diff(state_start.astype(np.int64)))
    first = np.array([0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1.0])
    poses, points, init, stats = frontend.compute_initial_guess_device(camera, F, num_points, obs_state, point_id, uvd, first, variant=_variant())
    sel = init[point_id]
    keep = np.nonzero(init)[0]
    remap = np.full(num_points, -1, np.int64)
    remap[keep] = np.arange(len(keep))
    ba = StereoBA(camera, poses.copy(), points[keep].copy(), obs_state[sel], remap[point_id[sel]].astype(np.uint32), uvd[sel], np.eye(3))
    options, summary = capi.default_options(max_num_iterations=1000, use_nonmonotonic_steps=1), capi.Summary()
    rc = ba.lib.ssba_solve(ba.h, C.byref(options), C.byref(summary))
    assert rc == capi.SSBA_OK, (rc, ba.lib.ssba_last_error().decode())
    out = ba.poses.copy()
    ba.close()
    return out, summary, stats


def _pair_translation_errors(poses, truth):
    errs = []
    for k in range(1, len(poses)):
        rel = frontend.se3_compose(poses[k], np.concatenate([-(poses[k - 1][3:].reshape(3, 3).T @ poses[k - 1][:3]), poses[k - 1][3:].reshape(3, 3).T.ravel()]))
        rel_true = frontend.se3_compose(truth[k], np.concatenate([-(truth[k - 1][3:].reshape(3, 3).T @ truth[k - 1][:3]), truth[k - 1][3:].reshape(3, 3).T.ravel()]))
        errs.append(float(np.linalg.norm(rel[:3] - rel_true[:3])))
    return errs


def test_tracks_to_front_end_to_bundle_adjustment():
    """No bar on the translation error: nobody has measured what whole-pixel disparities of about 7 px allow.  The figures are
    printed for both disparity sources (DESIGN.md section 4.2i records them)."""
    s = _sequence(96, 128)
    for source in ("right", "disp16"):
        got, want = _device(96, 128, source), _reference(96, 128, source)
        poses, summary, stats = _solve_from_tracks(s.camera, *got)
        poses_ref, summary_ref, _ = _solve_from_tracks(s.camera, *want[:4])
        assert poses.tobytes() == poses_ref.tobytes()
        assert (poses[1:] != poses[0]).any()
        step = float(np.linalg.norm(s.poses_true[1][:3]))
        print(f"{source}: {StereoBA.brief_report(summary)}; front end {stats}; true step {step:.5f}; per-pair translation error "
              f"{['%.5f' % e for e in _pair_translation_errors(poses, s.poses_true)]}")


@pytest.mark.parametrize("extra", [[], ["--sgbm"]], ids=["right", "sgbm"])
def test_example_prints_the_trajectory_of_the_python_route(tmp_path, extra):
    exe = build.build_examples("sparse_stereo_sequence_gpu", "ssba_tracks")
    s = _sequence(96, 128)
    raw = tmp_path / "sequence.raw"
    synth.write_stereo_sequence(str(raw), s, 3, 0, bytes(capi.sgbm_params(**SGBM)))
    r = subprocess.run([exe, str(raw), "--fast-threshold", "10"] + extra, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stdout.decode() + r.stderr.decode()
    lines = r.stdout.decode().strip().splitlines()
    assert [ln.split()[:2] for ln in lines] == [["frame", str(k)] for k in range(4)]
    T = np.array([[float(x) for x in ln.split()[2:]] for ln in lines])
    poses, _, _ = _solve_from_tracks(s.camera, *_device(96, 128, "disp16" if extra else "right"))
    assert T.tobytes() == poses.tobytes()
    assert T[0].tolist() == [0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1] and (T[3] != T[2]).any()
