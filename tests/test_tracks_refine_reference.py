"""The numpy statement of the sub-pixel refinement (tests/tracks_refine_reference.py) against analytic images with known shifts,
every status at its boundary, the quality of the refined sequence under the true poses, and the parts of libssba_tracks.so that
need no device: the symbol table, the struct sizes and the refusals of the new calls."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import tracks_reference as tr
import tracks_refine_cases as tc
import tracks_refine_reference as rr
from ceres_slam_amd import build, synth, tracks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, COLS, AX, AY = 40, 56, 28, 20


# ---- analytic images ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", [0, 2])
@pytest.mark.parametrize("mode", [rr.MODE_2D, rr.MODE_X])
def test_known_shifts_are_recovered_within_a_sixteenth_of_a_pixel(mode, noise):
    """The bar is the bilinear model's own bias on wavelengths of 8 pixels and more (0.047 px at worst in 70 prototype runs) with a
    margin of a third; the refinement starts from the rounded shift."""
    anchor, worst = tc.sinusoids(ROWS, COLS), 0.0
    for sx, sy in tc.SHIFTS:
        if mode == rr.MODE_X:
            sy = 0.0
        target = tc.sinusoids(ROWS, COLS, (sx, sy), noise=noise)
        x0, y0 = 256 * (AX + int(np.rint(sx))), 256 * (AY + int(np.rint(sy)))
        x, y, status, sad = rr.refine_one(anchor, AX, AY, target, x0, y0, mode)
        err = max(abs(x / 256 - AX - sx), abs(y / 256 - AY - sy))
        print(f"mode {mode}, noise {noise}, shift ({sx}, {sy}): status {status}, error {err:.4f} px, sad {sad}")
        assert status == rr.OK and err <= 1 / 16
        assert mode == rr.MODE_2D or y == y0
        worst = max(worst, err)
    print(f"worst {worst:.4f} px")


@pytest.mark.parametrize("mode", [rr.MODE_2D, rr.MODE_X])
def test_zero_shift_returns_the_start_exactly_with_sad_zero(mode):
    img = tc.sinusoids(ROWS, COLS)
    assert rr.refine_one(img, AX, AY, img, 256 * AX, 256 * AY, mode) == (256 * AX, 256 * AY, rr.OK, 0)
    assert rr.refine_one(img, 8, 8, img, 256 * 8, 256 * 8, mode) == (256 * 8, 256 * 8, rr.OK, 0)


def test_the_evaluation_against_a_scalar_loop():
    """The vectorised statement against the header's formulas written out pixel by pixel, at a position with both fractions."""
    A, B = tc.sinusoids(ROWS, COLS), tc.sinusoids(ROWS, COLS, (0.5, 0.25), noise=2)
    T, gx, gy = rr.template(A, AX, AY, rr.MODE_2D)
    px, py = 256 * AX + 77, 256 * AY - 130
    bx = by = total = 0
    for j in range(-7, 8):
        for i in range(-7, 8):
            X, Y = px + 256 * i, py + 256 * j
            x0, fx, y0, fy = X >> 8, X & 255, Y >> 8, Y & 255
            S = ((256 - fx) * (256 - fy) * int(B[y0, x0]) + fx * (256 - fy) * int(B[y0, x0 + 1]) + (256 - fx) * fy * int(B[y0 + 1, x0])
                 + fx * fy * int(B[y0 + 1, x0 + 1]))
            e = S - 65536 * int(A[AY + j, AX + i])
            bx += (int(A[AY + j, AX + i + 1]) - int(A[AY + j, AX + i - 1])) * e
            by += (int(A[AY + j + 1, AX + i]) - int(A[AY + j - 1, AX + i])) * e
            total += abs(e)
    assert rr.evaluate(B, T, gx, gy, px, py) == (bx, by, total >> 16)
    assert int(gx[7, 8]) == int(A[AY, AX + 2]) - int(A[AY, AX]) and int(gy[8, 7]) == int(A[AY + 2, AX]) - int(A[AY, AX])
    assert not rr.template(A, AX, AY, rr.MODE_X)[2].any()


def test_the_step_rounds_every_product_before_the_subtraction():
    """Operands chosen so that a fused multiply-subtract gives another integer than two rounded products do."""
    H11, H12, H22 = (1 << 25) + 1, (1 << 24) + 3, (1 << 25) + 5
    bx, by = (1 << 40) + 12345, (1 << 40) - 54321
    f = np.float64
    nx = f(H22) * f(bx) - f(H12) * f(by)
    det = f(H11 * H22 - H12 * H12) * f(128.0)
    assert rr.step(H11, H12, H22, bx, by, rr.MODE_2D)[0] == int(np.rint(nx / det))
    assert int(f(H22) * f(bx)) != H22 * bx                    # the product is not exact: the rounding is part of the statement
    assert rr.step(H11, H12, H22, 3 * H11 * 128 + H11 * 64, 0, rr.MODE_X) == (4, 0)      # 3.5 rounds to even
    assert rr.step(H11, H12, H22, 2 * H11 * 128 + H11 * 64, 0, rr.MODE_X) == (2, 0)      # 2.5 rounds to even


# ---- statuses ----------------------------------------------------------------------------------------------------------------
def test_every_status_at_its_boundary():
    stack, seen = tc.status_stack(), set()
    for name, item, kw, expected in tc.status_cases():
        x, y, status, sad = rr.refine_one(stack[item[0]], item[1], item[2], stack[item[3]], item[4], item[5], item[6], **kw)
        print(f"{name}: status {status}, position ({x}, {y}), sad {sad}")
        assert status == expected, name
        if status != rr.OK:
            assert (x, y) == (item[4], item[5]), name          # the start comes back
        seen.add(status)
    assert seen == {rr.OK, rr.EDGE, rr.FLAT, rr.FAR, rr.ITERATIONS, rr.SAD}
    by_name = {c[0]: c for c in tc.status_cases()}
    item, kw = by_name["moved by max_shift exactly"][1:3]
    assert rr.refine_one(stack[item[0]], item[1], item[2], stack[item[3]], item[4], item[5], item[6], **kw)[:2] == (item[4] + 512, item[5])
    with pytest.raises(AttributeError):
        rr.refine_params(max_shfit=2)


def test_disparity_status_and_the_anchor_of_an_observation():
    """The right view lies half a pixel to the RIGHT of the left one: whatever whole-pixel disparity the matcher believed, the
    refined one is negative."""
    left, right = tc.sinusoids(ROWS, COLS), tc.sinusoids(ROWS, COLS, (0.5, 0.0))
    u, v, d, status = rr.observation(left, AX, AY, left, right, AX, AY, 16, True)
    assert status == rr.DISPARITY and (u, v) == (256 * AX, 256 * AY) and -140 < d < -116
    true_right = tc.sinusoids(ROWS, COLS, (-1.5, 0.0))
    u, v, d, status = rr.observation(left, AX, AY, left, true_right, AX, AY, 16, True)
    assert status == rr.OK and (u, v) == (256 * AX, 256 * AY) and abs(d - 384) <= 16      # the anchor keeps its pixel; d = 1.5
    # not the anchor: the left position moves too, and the right one is searched on the refined row
    moved, moved_right = tc.sinusoids(ROWS, COLS, (0.5, 0.25)), tc.sinusoids(ROWS, COLS, (-1.0, 0.25))
    u, v, d, status = rr.observation(left, AX, AY, moved, moved_right, AX + 1, AY, 32, False)
    assert status == rr.OK and abs(u - 256 * (AX + 0.5)) <= 16 and abs(v - 256 * (AY + 0.25)) <= 16 and abs(d - 384) <= 16
    # with a disparity map only the left position is refined
    u2, v2, d2, status = rr.observation(left, AX, AY, moved, None, AX + 1, AY, 23, False)
    assert status == rr.OK and (u2, v2, d2) == (u, v, 16 * 23)
    assert rr.observation(left, AX, AY, np.full((ROWS, COLS), 9, np.uint8), None, AX, AY, 23, False)[3] == rr.FAR


# ---- sequence quality on the statement alone ---------------------------------------------------------------------------------
PARAMS = dict(fast_threshold=10)


@functools.lru_cache(maxsize=None)
def _sequence(rows, cols):
    return synth.make_stereo_sequence(rows, cols, 4, seed=1)


@functools.lru_cache(maxsize=None)
def _whole(rows, cols, temporal_radius=0):
    s = _sequence(rows, cols)
    return tr.sequence(s.left, s.right, temporal_radius=temporal_radius, **PARAMS)


@functools.lru_cache(maxsize=None)
def _refined(rows, cols, temporal_radius=0, max_sad=0):
    s = _sequence(rows, cols)
    return rr.sequence_subpixel(s.left, s.right, refine=dict(max_sad=max_sad), temporal_radius=temporal_radius, **PARAMS)


def _pair_errors(seq, start, ids, uvd):
    """Per pair (k, k + 1): |reprojection of frame k's triangulated points in frame k + 1 under the true poses - the observation
    there|, one (u, v, d) row per track seen in both frames."""
    out = []
    start = start.astype(np.int64)
    for k in range(len(start) - 2):
        a, b = slice(start[k], start[k + 1]), slice(start[k + 1], start[k + 2])
        _, ia, ib = np.intersect1d(ids[a], ids[b], return_indices=True)
        t0, R0 = synth.pose_unpack(seq.poses_true[k])
        t1, R1 = synth.pose_unpack(seq.poses_true[k + 1])
        R = R1 @ R0.T
        q = synth.triangulate(seq.camera, uvd[a][ia]) @ R.T + (t1 - R @ t0)
        out.append(np.abs(synth.project(seq.camera, q) - uvd[b][ib]))
    return out


@pytest.mark.parametrize("rows,cols", [(64, 96), (96, 128)])
def test_refined_tracks_reproject_four_times_better_than_whole_pixel_tracks(rows, cols):
    seq, whole, fine = _sequence(rows, cols), _whole(rows, cols), _refined(rows, cols)
    e_whole, e_fine = _pair_errors(seq, *whole[:3]), _pair_errors(seq, *fine[:3])
    assert len(e_whole) == len(e_fine) == 3
    for k in range(3):
        mw, mf = np.median(e_whole[k], axis=0), np.median(e_fine[k], axis=0)
        print(f"{rows}x{cols} pair {k}: median |du|, |dv|, |dd| whole pixel {np.round(mw, 3).tolist()}, refined {np.round(mf, 4).tolist()}, ratio "
              f"{np.round(mw / mf, 1).tolist()}; 90th percentile of the per-observation maximum {np.percentile(e_whole[k].max(axis=1), 90):.2f} -> "
              f"{np.percentile(e_fine[k].max(axis=1), 90):.3f}")
        assert (mf <= mw / 4).all()
    statuses = np.concatenate(fine[5])
    assert (statuses == rr.OK).all() and fine[4] == 0                      # no refinement fails to converge
    assert fine[0].tobytes() == whole[0].tobytes() and fine[1].tobytes() == whole[1].tobytes()      # nothing dropped: the same tracks
    assert (np.abs(fine[2][:, :2] - whole[2][:, :2]) <= 4).all()


def test_temporal_radius_eight_drops_nothing_and_removes_the_gross_mismatches():
    seq, fine = _sequence(96, 128), _refined(96, 128, temporal_radius=8)
    assert fine[4] == 0 and len(fine[1]) == 494 and len(fine[1]) == len(_whole(96, 128, 8)[1])
    assert sum(int((e.max(axis=1) > 3).sum()) for e in _pair_errors(seq, *fine[:3])) == 0
    assert sum(int((e.max(axis=1) > 3).sum()) for e in _pair_errors(seq, *_refined(96, 128)[:3])) == 7


def test_max_sad_2000_drops_at_most_five_percent():
    ungated, gated = _refined(96, 128), _refined(96, 128, max_sad=2000)
    survivors = len(np.concatenate(gated[5]))
    print(f"{gated[4]} of {survivors} survivors dropped, {len(ungated[1])} -> {len(gated[1])} observations after pruning")
    assert 0 < gated[4] <= 0.05 * len(ungated[1])
    assert (np.concatenate(gated[5]) == rr.SAD).sum() == gated[4]
    assert len(gated[1]) < len(ungated[1]) and gated[3] <= ungated[3]
    lengths = np.bincount(gated[1], minlength=gated[3])
    assert lengths.min() >= 2                                              # the pruning acts on the lengths that remain


# ---- library surface ---------------------------------------------------------------------------------------------------------
NEW = {"ssba_track_default_refine_params", "ssba_track_refine", "ssba_track_sequence_subpixel"}


def test_header_symbols_and_sizes_agree():
    hdr = open(os.path.join(ROOT, "include", "ssba_tracks.h")).read()
    declared = set(re.findall(r"\b(ssba_track_[a-z_]+)\s*\(", hdr))
    assert NEW <= declared and declared == set(tracks.SYMBOLS), declared ^ set(tracks.SYMBOLS)
    build.build_library()
    out = subprocess.run(["nm", "-D", "--defined-only", tracks.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert {ln.split()[-1] for ln in out.splitlines() if ln.strip()} == declared
    assert C.sizeof(tracks.RefineParams) == 3 * 4 and C.sizeof(tracks.TrackParams) == 7 * 4
    p = tracks.refine_params()
    assert {n: getattr(p, n) for n, _ in tracks.RefineParams._fields_} == rr.REFINE_DEFAULTS == dict(iterations=10, max_shift=4, max_sad=0)
    names = ["OK", "EDGE", "FLAT", "FAR", "ITERATIONS", "SAD", "DISPARITY"]
    for value, name in enumerate(names):
        assert re.search(rf"#define SSBA_TRACK_REFINE_{name} {value}\b", hdr)
        assert getattr(tracks, "REFINE_" + name) == value == getattr(rr, name)
    for call in sorted(NEW):                                               # the shim and the example reach the new entry
        assert call == "ssba_track_refine" or call in open(os.path.join(ROOT, "include", "ceres_slam_amd", "feature_tracks.hpp")).read()


def test_new_refusals_come_with_messages_before_a_device_is_looked_for():
    lib = tracks.load()
    u8, u32, i32 = tracks._u8p, tracks._u32p, tracks._i32p
    img = np.zeros((2, 31, 31), np.uint8)
    pi = img.ctypes.data_as(u8)
    items = np.array([[0, 15, 15, 1, 256 * 15, 256 * 15, 0], [1, 15, 15, 0, 256 * 15, 256 * 15, 1]], np.int32)
    xy, status, sad = np.full((2, 2), 7, np.int32), np.full(2, 7, np.int32), np.full(2, 7, np.uint32)
    ro = (xy.ctypes.data_as(i32), status.ctypes.data_as(i32), sad.ctypes.data_as(u32))
    start, ids, uvd = np.full(3, 7, np.uint32), np.full(8, 7, np.uint32), np.full((8, 3), 7.0)
    nobs, npts, ndrop = C.c_uint64(7), C.c_uint32(7), C.c_uint64(7)
    so = (8, start.ctypes.data_as(u32), ids.ctypes.data_as(u32), uvd.ctypes.data_as(tracks._dp), C.byref(nobs), C.byref(npts))
    tp = C.byref(tracks.track_params(max_features=4))
    ok = lambda **kw: C.byref(tracks.refine_params(**kw))
    it = lambda a: a.ctypes.data_as(i32)
    r, s = "ssba_track_refine", "ssba_track_sequence_subpixel"

    def refused(name, rc, word=""):
        msg = lib.ssba_track_last_error().decode()
        assert rc == -1, (name, rc, msg)
        assert msg.startswith(name + ": ") and len(msg) > len(name) + 2 and word in msg, (msg, word)

    for kw, word in ((dict(iterations=0), "iterations"), (dict(iterations=65), "iterations"), (dict(max_shift=0), "max_shift"), (dict(max_shift=9), "max_shift"),
                     (dict(max_sad=-1), "max_sad")):
        refused(r, lib.ssba_track_refine(pi, 2, 31, 31, it(items), 2, ok(**kw), -1, *ro), word)
        refused(s, lib.ssba_track_sequence_subpixel(pi, pi, None, 2, 31, 31, tp, -1, *so, ok(**kw), C.byref(ndrop)), word)
    refused(r, lib.ssba_track_refine(None, 2, 31, 31, it(items), 2, ok(), -1, *ro), "NULL")
    refused(r, lib.ssba_track_refine(pi, 2, 31, 31, None, 2, ok(), -1, *ro), "NULL")
    refused(r, lib.ssba_track_refine(pi, 2, 31, 31, it(items), 2, None, -1, *ro), "NULL")
    for k in range(3):
        refused(r, lib.ssba_track_refine(pi, 2, 31, 31, it(items), 2, ok(), -1, *[None if j == k else o for j, o in enumerate(ro)]), "NULL")
    refused(r, lib.ssba_track_refine(pi, 0, 31, 31, it(items), 2, ok(), -1, *ro), "n must")
    for rows, cols in ((30, 31), (31, 30), (8193, 31), (31, 8193)):
        refused(r, lib.ssba_track_refine(pi, 2, rows, cols, it(items), 2, ok(), -1, *ro), "31")
        refused(s, lib.ssba_track_sequence_subpixel(pi, pi, None, 2, rows, cols, tp, -1, *so, ok(), C.byref(ndrop)), "31")
    for column, value, word in ((0, 2, "image"), (0, -1, "image"), (3, 2, "image"), (3, -1, "image"), (6, 2, "mode"), (6, -1, "mode")):
        bad = items.copy()
        bad[1, column] = value
        refused(r, lib.ssba_track_refine(pi, 2, 31, 31, it(bad), 2, ok(), -1, *ro), word)
        assert "item 1" in lib.ssba_track_last_error().decode()
    assert lib.ssba_track_refine(pi, 2, 31, 31, None, 0, ok(), -1, None, None, None) == 0          # no items: done, without a device
    refused(r, lib.ssba_track_refine(pi, 2, 31, 31, None, 0, ok(max_shift=9), -1, None, None, None), "max_shift")
    refused(s, lib.ssba_track_sequence_subpixel(None, pi, None, 2, 31, 31, tp, -1, *so, ok(), C.byref(ndrop)), "NULL")
    refused(s, lib.ssba_track_sequence_subpixel(pi, pi, None, 2, 31, 31, tp, -1, *so, None, C.byref(ndrop)), "NULL")
    refused(s, lib.ssba_track_sequence_subpixel(pi, pi, None, 2, 31, 31, tp, -1, *so, ok(), None), "NULL")
    refused(s, lib.ssba_track_sequence_subpixel(pi, pi, None, 2, 31, 31, None, -1, *so, ok(), C.byref(ndrop)), "NULL")
    refused(s, lib.ssba_track_sequence_subpixel(pi, None, None, 2, 31, 31, tp, -1, *so, ok(), C.byref(ndrop)), "exactly one")
    refused(s, lib.ssba_track_sequence_subpixel(pi, pi, None, 0, 31, 31, tp, -1, *so, ok(), C.byref(ndrop)), "frames")
    refused(s, lib.ssba_track_sequence_subpixel(pi, pi, None, 2, 31, 31, C.byref(tracks.track_params(max_features=0)), -1, *so, ok(), C.byref(ndrop)), "max_features")
    for a in (xy, status, sad, start, ids):
        assert (a == 7).all()                                              # a refusal writes nothing
    assert (uvd == 7.0).all() and nobs.value == 7 and npts.value == 7 and ndrop.value == 7
    with pytest.raises(tracks.SsbaError) as e:
        tracks.track_refine(img, items, max_shift=9)
    assert e.value.status == -1 and "max_shift" in str(e.value)
    with pytest.raises(tracks.SsbaError):
        tracks.track_sequence_subpixel(img, img, refine=dict(iterations=0))
    with pytest.raises(AttributeError):
        tracks.track_refine(img, items, max_shfit=2)
    with pytest.raises(ValueError):
        tracks.track_sequence_subpixel(img, right=img[:1])
