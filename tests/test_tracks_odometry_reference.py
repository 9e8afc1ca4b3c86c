"""The statement of the streaming odometry (tests/tracks_odometry_reference.py) on its own, the surface of the new calls of
libssba_tracks.so, their refusals that need no device, and the properties of the cases tests/test_gpu_track_odometry.py uses."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import hp_frontend as hp
import tracks_odometry_cases as oc
import tracks_odometry_reference as orf
from ceres_slam_amd import build, tracks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"ssba_track_default_odometry_params", "ssba_track_stream_enable_odometry", "ssba_track_stream_pose", "ssba_track_relative_pose"}


@pytest.mark.parametrize("n", [3, 4, 5, 64, 4096])
def test_the_draws_are_distinct_and_in_range(n):
    for frame in (0, 1, 7, 1000, 2 ** 20 + 3, 2 ** 32 - 1):
        s = orf.draws(frame, 4096, n)
        assert s.shape == (4096, 3) and s.min() >= 0 and s.max() < n
        assert (s[:, 0] != s[:, 1]).all() and (s[:, 0] != s[:, 2]).all() and (s[:, 1] != s[:, 2]).all()
    if n >= 64:                                                            # and they move: with the hypothesis, with the frame
        a, b = orf.draws(3, 4096, n), orf.draws(4, 4096, n)
        assert len({tuple(r) for r in a.tolist()}) > 4096 // 4 and (a != b).any(axis=1).mean() > 0.9
    if n == 3:
        assert sorted(orf.draws(11, 1, 3)[0].tolist()) == [0, 1, 2]


def test_the_mixer_and_the_counter_are_the_stated_integers():
    assert int(orf.mix([0])[0]) == 0
    x = 1
    x ^= x >> 16; x = x * 0x7FEB352D & 0xFFFFFFFF; x ^= x >> 15; x = x * 0x846CA68B & 0xFFFFFFFF; x ^= x >> 16
    assert int(orf.mix([1])[0]) == x
    # c = 3 (f H + h) mod 2^32: frame 2^32 / H restarts the sequence of frame 0
    assert orf.draws(2 ** 32 // 64, 64, 100).tolist() == orf.draws(0, 64, 100).tolist()


def test_header_symbols_and_sizes_agree():
    hdr = open(os.path.join(ROOT, "include", "ssba_tracks.h")).read()
    declared = set(re.findall(r"\b(ssba_track_[a-z_]+)\s*\(", hdr))
    assert NEW <= declared and declared == set(tracks.SYMBOLS), declared ^ set(tracks.SYMBOLS)
    build.build_library()
    out = subprocess.run(["nm", "-D", "--defined-only", tracks.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert {ln.split()[-1] for ln in out.splitlines() if ln.strip()} == declared
    assert C.sizeof(tracks.OdometryParams) == 5 * 8 + 4 * 8 + 12 * 8 and C.sizeof(tracks.PoseInfo) == 4 * 4 + 2 * 8
    for name, value in (("SSBA_TRACK_ODOMETRY_MAX", tracks.ODOMETRY_MAX), ("SSBA_TRACK_ODOMETRY_MAX_REFINE", tracks.ODOMETRY_MAX_REFINE),
                        ("SSBA_TRACK_POSE_OK", tracks.POSE_OK), ("SSBA_TRACK_POSE_FIRST_FRAME", tracks.POSE_FIRST_FRAME),
                        ("SSBA_TRACK_POSE_FEW_MATCHES", tracks.POSE_FEW_MATCHES), ("SSBA_TRACK_POSE_FEW_INLIERS", tracks.POSE_FEW_INLIERS),
                        ("SSBA_TRACK_POSE_NUMERICAL", tracks.POSE_NUMERICAL)):
        assert int(re.search(rf"#define {name} (\d+)", hdr).group(1)) == value
    p = tracks.odometry_params()
    assert (p.ransac_iterations, p.ransac_threshold, p.refine_iterations, p.observation_variance) == (400, 4.0, 20, 4.0)
    assert list(p.first_pose) == hp.IDENTITY.tolist()
    shim = open(os.path.join(ROOT, "include", "ceres_slam_amd", "feature_tracks.hpp")).read()
    assert all(call in shim for call in NEW - {"ssba_track_relative_pose"})
    assert not NEW & set(re.findall(r"\bssba_\w+", open(os.path.join(ROOT, "include", "ssba.h")).read()))
    # one statement of the alignment: the front end and the tracker include the same header, neither keeps a copy
    csrc = os.path.join(ROOT, "ceres_slam_amd", "csrc")
    for source in ("ssba_frontend.hip", "ssba_tracks_odometry.h"):
        text = open(os.path.join(csrc, source)).read()
        assert '#include "ssba_align3.h"' in text and "void align3(" not in text and "bool is_inlier(" not in text


def test_refusals_come_with_messages_before_a_device_is_looked_for():
    lib = tracks.load()
    cam = oc.CAM
    uvd = np.full((4, 3), 7.0)
    T, Tr, flags, info = np.full(12, 7.0), np.full(12, 7.0), np.full(4, 7, np.uint8), tracks.PoseInfo()
    r = "ssba_track_relative_pose"

    def call(params, n=4, prev=uvd, cur=uvd, T=T, info=info):
        return lib.ssba_track_relative_pose(None if params is None else C.byref(params), 0, n, None if prev is None else prev.ctypes.data_as(tracks._dp),
                                            None if cur is None else cur.ctypes.data_as(tracks._dp), -1, Tr.ctypes.data_as(tracks._dp),
                                            flags.ctypes.data_as(tracks._u8p), None if T is None else T.ctypes.data_as(tracks._dp),
                                            None if info is None else C.byref(info), None, None)

    def refused(name, rc, word=""):
        msg = lib.ssba_track_last_error().decode()
        assert rc == -1, (name, rc, msg)
        assert msg.startswith(name + ": ") and len(msg) > len(name) + 2 and word in msg, (msg, word)

    good = tracks.odometry_params(camera=cam)
    refused(r, call(None), "NULL")
    for kw, word in ((dict(ransac_iterations=0), "ransac_iterations"), (dict(ransac_iterations=4097), "ransac_iterations"),
                     (dict(ransac_threshold=0.0), "positive"), (dict(ransac_threshold=-4.0), "positive"), (dict(ransac_threshold=float("nan")), "positive"),
                     (dict(observation_variance=0.0), "positive"), (dict(refine_iterations=1025), "refine_iterations"),
                     (dict(camera=dict(cam, fu=0.0)), "fu"), (dict(camera=dict(cam, fv=-1.0)), "fv"), (dict(camera=dict(cam, b=0.0)), "b ")):
        refused(r, call(tracks.odometry_params(**dict(dict(camera=cam), **kw))), word)
    refused(r, call(tracks.odometry_params()), "positive")               # the default camera is all zero: the caller sets it
    refused(r, call(good, prev=None), "NULL")
    refused(r, call(good, cur=None), "NULL")
    refused(r, call(good, T=None), "NULL")
    refused(r, call(good, info=None), "NULL")
    refused(r, call(good, n=4097), "4096")
    handle = C.c_void_p(7)
    refused("ssba_track_stream_enable_odometry", lib.ssba_track_stream_enable_odometry(None, C.byref(good)), "NULL stream")
    refused("ssba_track_stream_enable_odometry", lib.ssba_track_stream_enable_odometry(handle, None), "NULL")
    refused("ssba_track_stream_enable_odometry", lib.ssba_track_stream_enable_odometry(handle, C.byref(tracks.odometry_params(camera=cam, ransac_iterations=0))),
            "ransac_iterations")
    refused("ssba_track_stream_pose", lib.ssba_track_stream_pose(None, T.ctypes.data_as(tracks._dp), T.ctypes.data_as(tracks._dp), None), "NULL stream")
    refused("ssba_track_stream_pose", lib.ssba_track_stream_pose(handle, None, T.ctypes.data_as(tracks._dp), None), "NULL output")
    assert (T == 7.0).all() and (Tr == 7.0).all() and (flags == 7).all()  # a refusal writes nothing
    lib.ssba_track_default_odometry_params(None)                          # allowed
    with pytest.raises(AttributeError):
        tracks.odometry_params(ransac_iteration=3)
    with pytest.raises(ValueError):
        tracks.relative_pose(np.ones((3, 3)), np.ones((4, 3)), camera=cam)


def test_matches_are_the_ids_in_both_pushes_in_the_current_order():
    prev = (np.array([5, 9, 2, 7], np.uint32), np.arange(12.0).reshape(4, 3), 0)
    cur = (np.array([7, 1, 5, 8, 2], np.uint32), 100 + np.arange(15.0).reshape(5, 3), 0)
    a, b = orf.matches(prev, cur)
    assert a.tolist() == prev[1][[3, 0, 2]].tolist() and b.tolist() == cur[1][[0, 2, 4]].tolist()
    a, b = orf.matches(prev, (np.zeros(0, np.uint32), np.zeros((0, 3)), 0))
    assert a.shape == b.shape == (0, 3)


# ---- the synthetic cases of the device tests ---------------------------------------------------------------------------------
def test_the_seeds_keep_the_ambiguous_cases_within_one_in_eight_and_the_refinement_cases_exact():
    amb = [c for c in oc.RANSAC_CASES if not oc.synthetic_reference(*c)["unambiguous"]]
    assert 8 * len(amb) <= len(oc.RANSAC_CASES), amb
    for n, hypotheses in oc.RANSAC_CASES:
        r = oc.synthetic_reference(n, hypotheses)
        assert r["winner"] >= 0 and r["count"][r["winner"]] >= 3
    for m in oc.REFINE_SIZES:                                              # every match an inlier of the winner, decided
        prev, cur, _ = oc.refine_case(m)
        r = orf.ransac(oc.CAM, prev, cur, oc.FRAME, 64, oc.THRESHOLD)
        assert r["unambiguous"] and int(r["lo"][r["winner"]]) == m
    for kind, status in (("outliers", "none"), ("two", None), ("collinear", 3), ("coincident", 3)):
        prev, cur, hypotheses = oc.degenerate(kind)
        r = orf.ransac(oc.CAM, prev, cur, 3, hypotheses, oc.THRESHOLD)
        if kind == "two":
            assert r is None
        elif kind == "outliers":
            assert r["winner"] == -1 and int(r["hi"].max()) == 0           # no hypothesis has an inlier, whatever the rounding
        else:
            assert int(r["ref"]["rank"][0]) < 2 and int(r["count"][0]) == status


def test_the_oracle_rejects_steps_on_the_far_start_and_accepts_later():
    prev, cur, threshold = oc.rejected_step_case()
    r = orf.ransac(oc.CAM, prev, cur, oc.FRAME, 64, threshold)
    w = r["winner"]
    assert int(r["lo"][w]) == 40
    summary, log, _ = orf.refine(oc.CAM, prev, cur, r["flag"][w], np.asarray(r["ref"]["T"][w], np.float64), 2.25, 30)
    ok = log["step_is_successful"].tolist()
    assert ok[0] == 0 and 0 in ok[1:] and 1 in ok and summary.final_cost < 0.01 * summary.initial_cost


# ---- the image sequences -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", sorted(oc.SHAPES))
def test_subpixel_pairs_are_unambiguous_and_the_solve_approaches_the_truth(rows, cols):
    seq, pushes = oc.sequence(rows, cols), oc.statement_pushes(rows, cols, True)
    truth = seq.poses_true[1]                                              # the true pose of every pair is T_step
    for f in range(1, len(pushes)):
        prev, cur = orf.matches(pushes[f - 1], pushes[f])
        assert 40 <= len(prev) <= 120
        r = orf.ransac(seq.camera, prev, cur, f, oc.HYPOTHESES, 4.0)
        assert r["unambiguous"], (rows, cols, f)
        w = r["winner"]
        T0 = np.asarray(r["ref"]["T"][w], np.float64)
        summary, log, T = orf.refine(seq.camera, prev, cur, r["flag"][w], T0)
        before, after = orf.pose_error(T0, truth), orf.pose_error(T, truth)
        print(f"{rows}x{cols} pair {f}: {len(prev)} matches, {int(r['count'][w])} inliers, {summary.num_iterations} iteration records, "
              f"max |dt| {before[0]:.4f} -> {after[0]:.4f}")
        assert 3 <= summary.num_iterations <= 4                            # the initial record and 2 or 3 steps
        assert after[0] < before[0]


def test_whole_pixel_sequences_have_matches_enough_for_parity():
    for rows, cols in sorted(oc.SHAPES):
        pushes = oc.statement_pushes(rows, cols, False)
        for f in range(1, len(pushes)):
            assert len(orf.matches(pushes[f - 1], pushes[f])[0]) >= 30
