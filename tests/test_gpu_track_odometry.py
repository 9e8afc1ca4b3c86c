"""The streaming odometry on the device (libssba_tracks.so: ssba_track_stream_enable_odometry / _pose, ssba_track_relative_pose;
k_od_match, k_od_pairs, k_od_align, k_od_score and k_od_solve of ceres_slam_amd/csrc/ssba_tracks_odometry.h) against the
statement tests/tracks_odometry_reference.py: exact draws, long-double hypotheses and decisions (hp_frontend), and the C oracle's
Levenberg-Marquardt on the two-view problem.

The refinement is held to the project's bars (as tests/test_gpu_pose_only.py): the same number of iteration records
and the same accept / reject sequence as the oracle, every logged cost to rtol 1e-9, the final cost to 1e-6 relative, the pose to
1e-6 absolute.  Measured on an MI355X over the cases below, at worst: cost log 1.8e-11 relative (m = 3), final cost 1.5e-13, pose
2.4e-14; every test prints its own figures."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

import hp_frontend as hp
import tracks_odometry_cases as oc
import tracks_odometry_reference as orf
from ceres_slam_amd import build, capi, synth, tracks
from ceres_slam_amd.solver import stereo_sgbm_batch
from test_gpu_tracks import SGBM

pytestmark = pytest.mark.gpu

ODO = dict(camera=oc.CAM, ransac_threshold=oc.THRESHOLD)


def _finite(r):
    return all(np.isfinite(r[k]).all() for k in ("T_ransac", "T")) and np.isfinite([r["info"]["initial_cost"], r["info"]["final_cost"]]).all()


# ---- relative_pose alone: the hypotheses, the counts, the winner -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _device(n, hypotheses):
    prev, cur, _ = oc.synthetic(n)
    return tracks.relative_pose(prev, cur, frame_index=oc.FRAME, ransac_iterations=hypotheses, **ODO)


def test_at_most_one_case_in_eight_is_ambiguous():
    amb = [c for c in oc.RANSAC_CASES if not oc.synthetic_reference(*c)["unambiguous"]]
    assert 8 * len(amb) <= len(oc.RANSAC_CASES), amb


@pytest.mark.parametrize("n,hypotheses", oc.RANSAC_CASES)
def test_flags_count_pose_and_winner_against_long_double(n, hypotheses):
    ref, got = oc.synthetic_reference(n, hypotheses), _device(n, hypotheses)
    info = got["info"]
    assert info["status"] == tracks.POSE_OK and info["num_matches"] == n and _finite(got)
    assert info["num_inliers"] == int(got["inlier"].sum())                     # the count is that of the set flags
    if not ref["unambiguous"]:
        pytest.skip("the reference's winner is ambiguous (capped by test_at_most_one_case_in_eight_is_ambiguous)")
    w = ref["winner"]
    bar_R, bar_t = hp.align_bars(ref["ref"])
    want = np.asarray(ref["ref"]["T"][w], np.float64)
    dR, dt = np.abs(got["T_ransac"][3:] - want[3:]).max(), np.abs(got["T_ransac"][:3] - want[:3])
    print(f"n {n} H {hypotheses}: winner {w} with {int(ref['count'][w])} inliers; |dR| {dR:.2e} (bar {bar_R[w]:.2e}), |dt| {dt.max():.2e} (bar {bar_t[w].max():.2e})")
    assert dR <= bar_R[w] and (dt <= bar_t[w]).all()                           # the winner's pose within align_bars: the same winner
    decided = ref["decided"][w]
    assert (got["inlier"].astype(bool)[decided] == ref["flag"][w][decided]).all()
    assert int(ref["lo"][w]) <= info["num_inliers"] <= int(ref["hi"][w])


@pytest.mark.parametrize("kind", ["collinear", "coincident", "outliers", "two"])
def test_degenerate_lists_give_a_status_and_no_nan(kind):
    prev, cur, hypotheses = oc.degenerate(kind)
    got = tracks.relative_pose(prev, cur, frame_index=3, ransac_iterations=hypotheses, **ODO)
    info = got["info"]
    print(kind, info, got["T"])
    assert _finite(got) and info["num_matches"] == len(prev) and info["num_inliers"] == int(got["inlier"].sum())
    R = got["T"][3:].reshape(3, 3)
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1) < 1e-12
    if kind == "two":
        assert info["status"] == tracks.POSE_FEW_MATCHES and got["T"].tolist() == hp.IDENTITY.tolist() and not got["inlier"].any()
    elif kind == "outliers":
        assert info["status"] == tracks.POSE_FEW_INLIERS and info["num_inliers"] == 0 and info["num_iterations"] == 0
        assert got["T"].tolist() == hp.IDENTITY.tolist() and got["T_ransac"].tolist() == hp.IDENTITY.tolist()
    else:
        assert info["status"] in (tracks.POSE_OK, tracks.POSE_FEW_INLIERS, tracks.POSE_NUMERICAL)
        if info["status"] != tracks.POSE_OK:
            assert got["T"].tobytes() == got["T_ransac"].tobytes()


def test_no_refinement_returns_the_ransac_pose():
    prev, cur, _ = oc.synthetic(64)
    got = tracks.relative_pose(prev, cur, frame_index=oc.FRAME, ransac_iterations=64, refine_iterations=0, **ODO)
    assert got["info"]["status"] == tracks.POSE_OK and got["T"].tobytes() == got["T_ransac"].tobytes() == _device(64, 64)["T_ransac"].tobytes()
    assert got["info"]["num_iterations"] == 1 and got["info"]["initial_cost"] == got["info"]["final_cost"] == got["cost_log"][0]


# ---- the refinement against the oracle, on the device's own inlier set -------------------------------------------------------
def _against_the_oracle(prev, cur, got, variance, iterations):
    summary, log, T = orf.refine(oc.CAM, prev, cur, got["inlier"], got["T_ransac"], variance, iterations)
    n, info = summary.num_iterations, got["info"]
    ok = log["step_is_successful"].tolist()
    print(f"m {info['num_inliers']}: records {info['num_iterations']} (oracle {n}), accepted {got['step_ok'][:n].tolist()} (oracle {ok})")
    print(f"  cost log rel {np.abs(got['cost_log'][:n] / log['cost'] - 1).max():.2e}, final cost rel {abs(info['final_cost'] / summary.final_cost - 1):.2e}, "
          f"pose abs {np.abs(got['T'] - T).max():.2e}")
    assert info["status"] == tracks.POSE_OK and info["num_iterations"] == n
    assert got["step_ok"][:n].tolist() == ok and not got["step_ok"][n:].any() and np.isnan(got["cost_log"][n:]).all()
    np.testing.assert_allclose(got["cost_log"][:n], log["cost"], rtol=1e-9, atol=0)
    assert info["initial_cost"] == got["cost_log"][0]
    np.testing.assert_allclose(info["final_cost"], summary.final_cost, rtol=1e-6, atol=0)
    np.testing.assert_allclose(got["T"], T, rtol=0, atol=1e-6)
    return log


@pytest.mark.parametrize("m", oc.REFINE_SIZES)
def test_the_refinement_equals_the_oracle(m):
    prev, cur, truth = oc.refine_case(m)
    got = tracks.relative_pose(prev, cur, frame_index=oc.FRAME, ransac_iterations=64, **ODO)
    assert got["info"]["num_inliers"] == m == int(got["inlier"].sum())
    _against_the_oracle(prev, cur, got, 4.0, 20)
    before, after = orf.pose_error(got["T_ransac"], truth), orf.pose_error(got["T"], truth)
    print(f"  |dt| to the truth {before[0]:.2e} -> {after[0]:.2e}")
    assert after[0] < before[0]


def test_a_rejected_step_and_another_variance():
    prev, cur, threshold = oc.rejected_step_case()
    got = tracks.relative_pose(prev, cur, frame_index=oc.FRAME, ransac_iterations=64, ransac_threshold=threshold, observation_variance=2.25, refine_iterations=30,
                               camera=oc.CAM)
    assert got["info"]["num_inliers"] == 40
    log = _against_the_oracle(prev, cur, got, 2.25, 30)
    assert 0 in log["step_is_successful"][1:].tolist() and 1 in log["step_is_successful"].tolist()


def test_the_iteration_limit_cuts_the_log():
    prev, cur, threshold = oc.rejected_step_case()
    got = tracks.relative_pose(prev, cur, frame_index=oc.FRAME, ransac_iterations=64, ransac_threshold=threshold, refine_iterations=6, camera=oc.CAM)
    _against_the_oracle(prev, cur, got, 4.0, 6)
    assert got["info"]["num_iterations"] == 7


def test_two_runs_give_the_same_bytes():
    prev, cur, _ = oc.synthetic(1025)
    a = tracks.relative_pose(prev, cur, frame_index=9, ransac_iterations=64, **ODO)
    b = tracks.relative_pose(prev, cur, frame_index=9, ransac_iterations=64, **ODO)
    for k in ("T_ransac", "T", "inlier", "cost_log", "step_ok"):
        assert a[k].tobytes() == b[k].tobytes(), k
    c = tracks.relative_pose(prev, cur, frame_index=10, ransac_iterations=64, **ODO)
    assert c["T_ransac"].tobytes() != a["T_ransac"].tobytes()                  # the frame index moves the draws


# ---- the stream --------------------------------------------------------------------------------------------------------------
FIRST = np.array([0.3, -0.2, 0.1, 0, 0, 1, 1, 0, 0, 0, 1, 0.0])              # a rotation that permutes the axes


@functools.lru_cache(maxsize=None)
def _disp16(rows, cols):
    s = oc.sequence(rows, cols)
    d16, _ = stereo_sgbm_batch(s.left, s.right, **SGBM)
    d16.setflags(write=False)
    return d16


def _pair(rows, cols, source, f):
    s = oc.sequence(rows, cols)
    return s.left[f], (dict(right=s.right[f]) if source == "right" else dict(disp16=_disp16(rows, cols)[f]))


def _stream_run(rows, cols, source, refine, odometry, window=2):
    out = []
    with tracks.TrackStream(rows, cols, window, refine=refine, odometry=odometry, **oc.PARAMS) as st:
        for f in range(oc.SHAPES[rows, cols]):
            left, kw = _pair(rows, cols, source, f)
            push = st.push(left, **kw)
            out.append((push, st.pose() if odometry else None, st.window(min(window, f + 1))))
    return out


@pytest.mark.parametrize("refine", [None, {}], ids=["whole", "subpixel"])
@pytest.mark.parametrize("source", ["right", "disp16"])
@pytest.mark.parametrize("rows,cols", sorted(oc.SHAPES))
def test_every_push_gives_the_pose_of_its_rebuilt_matches(rows, cols, source, refine):
    cam = oc.sequence(rows, cols).camera
    odo = dict(camera=cam, ransac_iterations=oc.HYPOTHESES, first_pose=FIRST)
    run = _stream_run(rows, cols, source, refine, odo)
    chain = FIRST.copy()
    for f, (push, (rel, absolute, info), _) in enumerate(run):
        if f == 0:
            assert info["status"] == tracks.POSE_FIRST_FRAME and rel.tolist() == hp.IDENTITY.tolist() and absolute.tobytes() == FIRST.tobytes()
            assert info["num_matches"] == info["num_inliers"] == info["num_iterations"] == 0
            continue
        prev, cur = orf.matches(run[f - 1][0], push)
        want = tracks.relative_pose(prev, cur, frame_index=f, **odo)
        assert info == want["info"], (f, info, want["info"])
        assert rel.tobytes() == want["T"].tobytes(), f
        R, t = rel[3:].reshape(3, 3), rel[:3]
        composed = np.concatenate([R @ chain[:3] + t, (R @ chain[3:].reshape(3, 3)).ravel()])
        np.testing.assert_allclose(absolute, composed, rtol=0, atol=4e-16 * (1 + np.abs(chain[:3]).sum()))
        chain = absolute
        print(f"{rows}x{cols} {source} frame {f}: {info}")
        assert info["num_matches"] == len(prev) > 20 and info["status"] == tracks.POSE_OK


def test_two_streams_fed_the_same_frames_give_the_same_bytes():
    odo = dict(camera=oc.sequence(64, 96).camera, ransac_iterations=oc.HYPOTHESES)
    a, b = _stream_run(64, 96, "right", {}, odo), _stream_run(64, 96, "right", {}, odo)
    for (pa, oa, _), (pb, ob, _) in zip(a, b):
        assert pa[0].tobytes() == pb[0].tobytes() and pa[1].tobytes() == pb[1].tobytes()
        assert oa[0].tobytes() == ob[0].tobytes() and oa[1].tobytes() == ob[1].tobytes() and oa[2] == ob[2]


@pytest.mark.parametrize("refine", [None, {}], ids=["whole", "subpixel"])
def test_odometry_leaves_the_pushes_and_windows_alone_and_a_plain_stream_has_no_pose(refine):
    odo = dict(camera=oc.sequence(96, 128).camera, ransac_iterations=oc.HYPOTHESES)
    plain, with_odometry = _stream_run(96, 128, "right", refine, None), _stream_run(96, 128, "right", refine, odo)
    want = oc.statement_pushes(96, 128, refine is not None)
    for f, ((pa, _, wa), (pb, _, wb)) in enumerate(zip(plain, with_odometry)):
        assert pa[2] == pb[2] == want[f][2]
        for x, y, z in zip(pa[:2] + wa[:3], pb[:2] + wb[:3], want[f][:2] + wa[:3]):
            assert x.tobytes() == y.tobytes() == z.tobytes()
        assert wa[3] == wb[3]
    with tracks.TrackStream(96, 128, 2, **oc.PARAMS) as st:
        st.push(*[oc.sequence(96, 128).left[0], oc.sequence(96, 128).right[0]])
        with pytest.raises(capi.SsbaError) as e:
            st.pose()
        assert e.value.status == -7 and "odometry" in str(e.value)
        with pytest.raises(capi.SsbaError) as e:
            st.enable_odometry(**odo)
        assert e.value.status == -7 and "first push" in str(e.value)
    with tracks.TrackStream(96, 128, 2, odometry=odo, **oc.PARAMS) as st:
        with pytest.raises(capi.SsbaError) as e:
            st.pose()                                                           # nothing pushed yet
        assert e.value.status == -7
        with pytest.raises(capi.SsbaError) as e:
            st.enable_odometry(**odo)                                           # twice
        assert e.value.status == -7


def test_refusals_on_a_live_stream():
    cam = oc.sequence(64, 96).camera
    with tracks.TrackStream(64, 96, 2, **oc.PARAMS) as st:
        for bad in (dict(ransac_iterations=0), dict(ransac_iterations=4097), dict(ransac_threshold=0.0), dict(observation_variance=-1.0),
                    dict(camera=dict(cam, fu=0.0)), dict(camera=dict(cam, b=-0.1)), dict(refine_iterations=1025)):
            with pytest.raises(capi.SsbaError) as e:
                st.enable_odometry(**dict(dict(camera=cam), **bad))
            assert e.value.status == -1, bad
        st.enable_odometry(camera=cam)                                          # the refusals left the stream usable
        st.push(oc.sequence(64, 96).left[0], oc.sequence(64, 96).right[0])
        assert st.pose()[2]["status"] == tracks.POSE_FIRST_FRAME
    with pytest.raises(capi.SsbaError) as e:
        tracks.relative_pose(np.ones((4097, 3)), np.ones((4097, 3)), camera=cam)
    assert e.value.status == -1 and "4096" in str(e.value)


# ---- the example -------------------------------------------------------------------------------------------------------------
def test_example_with_odometry_prints_the_streams_poses(tmp_path):
    rows, cols = 96, 128
    seq = oc.sequence(rows, cols)
    exe = build.build_examples("sparse_stereo_sequence_gpu", "ssba_tracks")
    raw = tmp_path / "sequence.raw"
    synth.write_stereo_sequence(str(raw), seq, 3, 0, bytes(capi.sgbm_params(**SGBM)))
    r = subprocess.run([exe, str(raw), "--fast-threshold", "10", "--stream", "4", "--subpixel", "--odometry"], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stdout.decode() + r.stderr.decode()
    lines = r.stdout.decode().strip().splitlines()
    assert [ln.split()[:2] for ln in lines] == [["frame", str(k)] for k in range(oc.SHAPES[rows, cols])]
    T = np.array([[float(x) for x in ln.split()[2:]] for ln in lines])
    with tracks.TrackStream(rows, cols, 4, refine={}, odometry=dict(camera=seq.camera), **oc.PARAMS) as st:
        for f in range(oc.SHAPES[rows, cols]):
            st.push(seq.left[f], seq.right[f])
            assert T[f].tobytes() == st.pose()[1].tobytes(), f                  # 17 digits: the doubles themselves
    assert T[0].tolist() == hp.IDENTITY.tolist() and (T[3] != T[2]).any()
    bad = subprocess.run([exe, str(raw), "--odometry"], capture_output=True, timeout=120)
    assert bad.returncode != 0 and b"--stream" in bad.stderr
