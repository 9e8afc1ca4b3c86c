"""The numpy statement of the feature tracker (tests/tracks_reference.py) against hand-made cases, the committed BRIEF pattern,
the refusals of libssba_tracks.so that need no device, and its dynamic symbol table."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import tracks_reference as tr
from ceres_slam_amd import build, tracks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def arc_images(length, value, centre=100):
    """16 images of 33 x 33, one per arc start: `length` contiguous ring pixels around (16, 16) hold `value`, everything else
    `centre`."""
    out = np.full((16, 33, 33), centre, np.uint8)
    for a in range(16):
        for k in range(length):
            dx, dy = tr.RING[(a + k) % 16]
            out[a, 16 + dy, 16 + dx] = value
    return out


def test_nine_contiguous_ring_pixels_are_detected_with_the_expected_score():
    for value, want in ((160, 60), (30, 70)):                 # 16 bright and 16 dark images, the arcs that wrap included
        for img in arc_images(9, value):
            s = tr.scores(img, 20)
            assert s[16, 16] == want
            xy, sc, desc = tr.features(img, fast_threshold=20)
            assert [16, 16] in xy.tolist() and sc[xy.tolist().index([16, 16])] == want and desc.shape == (len(xy), 8)
            assert tr.scores(img, want)[16, 16] == 0 and tr.scores(img, want - 1)[16, 16] == want      # s > threshold, strictly


def test_eight_contiguous_ring_pixels_are_not():
    for value in (160, 30):
        for img in arc_images(8, value):
            assert tr.scores(img, 0).max() == 0 and len(tr.features(img, fast_threshold=0)[0]) == 0


def test_border_keeps_fifteen_pixels():
    rng = np.random.Generator(np.random.PCG64(5))
    s = tr.scores(rng.integers(0, 256, (40, 47), dtype=np.uint8), 5)
    inner = np.zeros_like(s, bool)
    inner[15:25, 15:32] = True
    assert (s[~inner] == 0).all() and (s[inner] > 0).any()
    assert tr.scores(np.zeros((30, 40), np.uint8), 0).max() == 0


def test_suppression_tie_goes_to_the_smaller_row_major_index():
    s = np.zeros((9, 9), np.int32)
    s[4, 3] = s[4, 4] = 50                                     # neighbours in a row
    s[6, 6], s[7, 5] = 40, 40                                  # diagonal neighbours: (6, 6) comes first
    s[1, 1], s[1, 2] = 30, 31
    k = tr.suppress(s)
    assert k[4, 3] == 50 and k[4, 4] == 0
    assert k[6, 6] == 40 and k[7, 5] == 0
    assert k[1, 1] == 0 and k[1, 2] == 31
    assert np.count_nonzero(k) == 3


def test_selection_keeps_the_smallest_indices_among_ties_at_the_cut_in_row_major_order():
    k = np.zeros((10, 10), np.int32)
    k[1, 7], k[2, 2], k[5, 5], k[7, 1], k[8, 8], k[9, 0] = 30, 90, 30, 30, 60, 30
    xy, sc = tr.select(k, 4)
    assert xy.tolist() == [[7, 1], [2, 2], [5, 5], [8, 8]] and sc.tolist() == [30, 90, 30, 60]
    xy, sc = tr.select(k, 2)
    assert xy.tolist() == [[2, 2], [8, 8]]
    xy, sc = tr.select(k, 100)
    assert len(xy) == 6 and xy[0].tolist() == [7, 1] and xy[-1].tolist() == [0, 9]


def test_descriptor_bits_follow_the_box_sums():
    rng = np.random.Generator(np.random.PCG64(11))
    img = rng.integers(0, 256, (40, 50), dtype=np.uint8)
    xy = np.array([[20, 17], [34, 24]], np.uint16)
    desc = tr.describe(img, xy)
    pat = tr.pattern()
    for k, (x, y) in enumerate(xy.astype(int)):
        for i in (0, 31, 32, 100, 255):
            ax, ay, bx, by = pat[i]
            a = int(img[y + ay - 2:y + ay + 3, x + ax - 2:x + ax + 3].astype(int).sum())
            b = int(img[y + by - 2:y + by + 3, x + bx - 2:x + bx + 3].astype(int).sum())
            assert (int(desc[k, i // 32]) >> (i % 32)) & 1 == int(a < b)


def test_matcher_statement_ties_cross_check_and_gates():
    d = np.zeros((3, 8), np.uint32)
    d[1, 0], d[2, 0] = 0b111, 0b1
    xy = np.array([[50, 20], [60, 20], [70, 20]], np.uint16)
    m, dist = tr.match(d[[0, 0]], xy[:2], d[[0, 0, 1]], xy, max_hamming=64)            # duplicates: ties go to the smaller index
    assert m.tolist() == [0, -1] and dist.tolist() == [0, -1]
    m, dist = tr.match(d[[2]], xy[:1], d[[0, 1]], xy[:2], max_hamming=0)               # distance 1 > max_hamming 0
    assert m.tolist() == [-1]
    m, dist = tr.match(d[[2]], xy[:1], d[[0, 1]], xy[:2], max_hamming=1)
    assert m.tolist() == [0] and dist.tolist() == [1]
    left, right = np.array([[50, 20]], np.uint16), np.array([[45, 24], [44, 25], [50, 20], [10, 20]], np.uint16)
    ok = tr.gate_matrix(left, right, tr.GATE_STEREO, tr.params(stereo_max_dy=5, max_disparity=40))
    assert ok.tolist() == [[True, False, False, True]]
    assert tr.gate_matrix(left, right, tr.GATE_TEMPORAL, tr.params(temporal_radius=5)).tolist() == [[True, False, True, False]]
    assert tr.gate_matrix(left, right, tr.GATE_TEMPORAL, tr.params(temporal_radius=0)).all()


def test_the_pattern_header_is_current():
    import brief_pattern as bp
    assert open(bp.HEADER).read() == bp.generate(), "run: python tools/brief_pattern.py --write"
    rows = np.array(bp.pattern())
    assert rows.shape == (256, 4) and np.abs(rows).max() <= 13 and (rows[:, :2] != rows[:, 2:]).any(axis=1).all()
    assert rows.tolist() == tr.pattern().tolist()              # the reference restates the recipe on its own
    assert len({tuple(r) for r in rows.tolist()}) > 250


def test_the_dynamic_symbol_table_is_exactly_the_header():
    hdr = open(os.path.join(ROOT, "include", "ssba_tracks.h")).read()
    declared = set(re.findall(r"\b(ssba_track_[a-z_]+)\s*\(", hdr))
    assert declared == set(tracks.SYMBOLS), declared ^ set(tracks.SYMBOLS)
    build.build_library()
    out = subprocess.run(["nm", "-D", "--defined-only", tracks.LIB_PATH], capture_output=True, text=True, check=True).stdout
    defined = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert defined == declared, defined ^ declared
    assert C.sizeof(tracks.TrackParams) == 7 * 4
    p = tracks.track_params()
    assert [getattr(p, n) for n, _ in tracks.TrackParams._fields_] == [tr.DEFAULTS[n] for n, _ in tracks.TrackParams._fields_]


def test_refusals_come_with_messages_before_a_device_is_looked_for():
    """Every argument refusal returns SSBA_ERR_INVALID_ARGUMENT where no device exists as well: the checks come first."""
    lib = tracks.load()
    u8, u16, u32, i16, i32 = tracks._u8p, tracks._u16p, tracks._u32p, tracks._i16p, tracks._i32p
    img = np.zeros((2, 31, 31), np.uint8)
    d16 = np.zeros((2, 31, 31), np.int16)
    pi, pd = img.ctypes.data_as(u8), d16.ctypes.data_as(i16)
    count, xy, score, desc = np.full(2, 7, np.uint32), np.full((2, 4, 2), 7, np.uint16), np.full((2, 4), 7, np.uint8), np.full((2, 4, 8), 7, np.uint32)
    fo = (count.ctypes.data_as(u32), xy.ctypes.data_as(u16), score.ctypes.data_as(u8), desc.ctypes.data_as(u32))
    start, ids, uvd = np.full(3, 7, np.uint32), np.full(8, 7, np.uint32), np.full((8, 3), 7.0)
    nobs, npts = C.c_uint64(7), C.c_uint32(7)
    so = (8, start.ctypes.data_as(u32), ids.ctypes.data_as(u32), uvd.ctypes.data_as(tracks._dp), C.byref(nobs), C.byref(npts))
    m, dist = np.full(2, 7, np.int32), np.full(2, 7, np.int32)
    mo = (m.ctypes.data_as(i32), dist.ctypes.data_as(i32))
    ok = lambda **kw: C.byref(tracks.track_params(max_features=4, **kw))
    da, pa = desc[0].ctypes.data_as(u32), xy[0].ctypes.data_as(u16)

    def refused(name, rc, word=""):
        msg = lib.ssba_track_last_error().decode()
        assert rc == -1, (name, rc, msg)
        assert msg.startswith(name + ": ") and len(msg) > len(name) + 2 and word in msg, (msg, word)

    bad_params = [dict(max_features=0), dict(max_features=4097), dict(fast_threshold=-1), dict(fast_threshold=255), dict(max_hamming=-1),
                  dict(max_hamming=257), dict(stereo_max_dy=-1), dict(max_disparity=-1), dict(temporal_radius=-1), dict(min_track_length=0)]
    f, s, mt = "ssba_track_features", "ssba_track_sequence", "ssba_track_match"
    for kw in bad_params:
        q = C.byref(tracks.track_params(**dict(dict(max_features=4), **kw)))
        refused(f, lib.ssba_track_features(pi, 2, 31, 31, q, -1, *fo))
        refused(s, lib.ssba_track_sequence(pi, pi, None, 2, 31, 31, q, -1, *so))
        refused(mt, lib.ssba_track_match(da, pa, 2, da, pa, 2, 0, q, -1, *mo))
    refused(f, lib.ssba_track_features(None, 2, 31, 31, ok(), -1, *fo), "NULL")
    refused(f, lib.ssba_track_features(pi, 2, 31, 31, None, -1, *fo), "NULL")
    refused(f, lib.ssba_track_features(pi, 2, 31, 31, ok(), -1, None, *fo[1:]), "NULL")
    refused(f, lib.ssba_track_features(pi, 0, 31, 31, ok(), -1, *fo))
    for rows, cols in ((30, 31), (31, 30), (8193, 31), (31, 8193)):
        refused(f, lib.ssba_track_features(pi, 2, rows, cols, ok(), -1, *fo), "31")
        refused(s, lib.ssba_track_sequence(pi, pi, None, 2, rows, cols, ok(), -1, *so), "31")
    refused(s, lib.ssba_track_sequence(None, pi, None, 2, 31, 31, ok(), -1, *so), "NULL")
    refused(s, lib.ssba_track_sequence(pi, pi, pd, 2, 31, 31, ok(), -1, *so), "exactly one")
    refused(s, lib.ssba_track_sequence(pi, None, None, 2, 31, 31, ok(), -1, *so), "exactly one")
    refused(s, lib.ssba_track_sequence(pi, pi, None, 0, 31, 31, ok(), -1, *so), "frames")
    refused(s, lib.ssba_track_sequence(pi, pi, None, 2, 31, 31, None, -1, *so), "NULL")
    refused(s, lib.ssba_track_sequence(pi, pi, None, 2, 31, 31, ok(), -1, 8, None, *so[2:]), "NULL")
    refused(mt, lib.ssba_track_match(None, pa, 2, da, pa, 2, 0, ok(), -1, *mo), "NULL")
    refused(mt, lib.ssba_track_match(da, pa, 2, da, None, 2, 0, ok(), -1, *mo), "NULL")
    refused(mt, lib.ssba_track_match(da, pa, 2, da, pa, 2, 0, ok(), -1, None, mo[1]), "NULL")
    refused(mt, lib.ssba_track_match(da, pa, 2, da, pa, 2, 3, ok(), -1, *mo), "gate")
    refused(mt, lib.ssba_track_match(da, pa, 65536, da, pa, 2, 0, ok(), -1, *mo), "65535")
    for a in (count, xy, score, desc, start, ids, m, dist):
        assert (a == 7).all()                                  # a refusal writes nothing
    assert (uvd == 7.0).all() and nobs.value == 7 and npts.value == 7
    with pytest.raises(tracks.SsbaError) as e:
        tracks.track_features(img, max_features=0)
    assert e.value.status == -1 and "max_features" in str(e.value)
    with pytest.raises(ValueError):
        tracks.track_sequence(img, right=img[:1])
