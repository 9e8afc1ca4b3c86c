"""The numpy statement of the streaming tracker (tests/tracks_stream_reference.py) against the batch statements it is built from,
the surface of the new calls of libssba_tracks.so and their refusals that need no device."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import tracks_reference as tr
import tracks_refine_reference as rr
import tracks_stream_reference as sr
from ceres_slam_amd import build, synth, tracks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = dict(fast_threshold=10)
SHAPES = {(64, 96): 6, (96, 128): 4}


@functools.lru_cache(maxsize=None)
def _sequence(rows, cols, seed=1):
    seq = synth.make_stereo_sequence(rows, cols, SHAPES[rows, cols], seed=seed)
    for a in (seq.left, seq.right):
        a.setflags(write=False)
    return seq


@functools.lru_cache(maxsize=None)
def _disp16(rows, cols):
    """No matcher runs without a device: a seeded map of disparities of 2.5 ... 12 pixels with invalid (0 and negative) patches."""
    rng = np.random.Generator(np.random.PCG64(rows))
    F = SHAPES[rows, cols]
    d = rng.integers(40, 193, (F, rows, cols)).astype(np.int16)
    for f in range(F):
        for _ in range(12):
            y, x = int(rng.integers(0, rows - 8)), int(rng.integers(0, cols - 8))
            d[f, y:y + 8, x:x + 8] = int(rng.choice([0, -16]))
    d.setflags(write=False)
    return d


def _sources(rows, cols, source):
    s = _sequence(rows, cols)
    return dict(right=s.right) if source == "right" else dict(disp16=_disp16(rows, cols))


def _pushed(rows, cols, source, window, refine=None, **params):
    s, kw = _sequence(rows, cols), _sources(rows, cols, source)
    st = sr.Stream(window, refine=refine, **PARAMS, **params)
    outs = [st.push(s.left[f], **{k: v[f] for k, v in kw.items()}) for f in range(SHAPES[rows, cols])]
    return st, outs


def _same(got, want):
    assert got[0].dtype == np.uint32 and got[1].dtype == np.uint32 and got[2].dtype == np.float64
    assert got[0].tobytes() == want[0].tobytes(), (got[0], want[0])
    assert got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes() and got[3] == want[3]


@pytest.mark.parametrize("min_track_length", [1, 2, 3])
@pytest.mark.parametrize("source", ["right", "disp16"])
@pytest.mark.parametrize("rows,cols", sorted(SHAPES))
def test_whole_pixel_windows_equal_the_batch_statement_on_their_frames(rows, cols, source, min_track_length):
    F, s, kw = SHAPES[rows, cols], _sequence(rows, cols), _sources(rows, cols, source)
    st, _ = _pushed(rows, cols, source, F, min_track_length=min_track_length)
    for w in (1, 2, 3, F):
        want = tr.sequence(s.left[F - w:], **{k: v[F - w:] for k, v in kw.items()}, min_track_length=min_track_length, **PARAMS)
        _same(st.window(w), want)
    assert st.window(F)[3] > 10 or min_track_length == 3
    _same(st.window(), st.window(F))


def test_whole_pixel_windows_while_the_stream_runs_and_through_a_short_ring():
    s = _sequence(64, 96)
    st = sr.Stream(3, **PARAMS)
    for f in range(6):
        st.push(s.left[f], s.right[f])
        for w in range(1, min(3, f + 1) + 1):
            _same(st.window(w), tr.sequence(s.left[f + 1 - w:f + 1], s.right[f + 1 - w:f + 1], **PARAMS))
    with pytest.raises(AssertionError):
        st.window(4)


@pytest.mark.parametrize("source", ["right", "disp16"])
@pytest.mark.parametrize("rows,cols", sorted(SHAPES))
def test_the_full_history_subpixel_window_equals_the_batch_statement(rows, cols, source):
    F, s = SHAPES[rows, cols], _sequence(rows, cols)
    st, outs = _pushed(rows, cols, source, F, refine={})
    want = rr.sequence_subpixel(s.left, **_sources(rows, cols, source), **PARAMS)
    _same(st.window(F), want)
    assert [o[2] for o in outs] == [int((st_ != rr.OK).sum()) for st_ in want[5]] and sum(o[2] for o in outs) == want[4]


def _restricted(left, right, first, refine, **params):
    """The all-frames statement restricted to the frames from `first` on, pruned and renumbered by the window rule; then the
    number of kept tracks whose anchor lies in a frame before `first`."""
    p = tr.params(**params)
    _, ids, _ = rr.link(left, right, **params)
    full = rr.sequence_subpixel(left, right, refine=refine, **dict(params, min_track_length=1))
    start, uvd, status = full[0].astype(np.int64), full[2], full[5]
    anchor_frame, order, length = {}, [], {}
    for f, mine in enumerate(ids):
        for t in mine.tolist():
            anchor_frame.setdefault(t, f)
            if f >= first and t not in length:
                order.append(t)                                            # first survivor in the window: frame, then keypoint slot
                length[t] = 0
        if f >= first:
            for t in mine[status[f] == rr.OK].tolist():
                length[t] += 1
    kept = [t for t in order if length[t] >= p["min_track_length"]]
    renamed = {t: k for k, t in enumerate(kept)}
    out_start, out_ids, out_uvd = [0], [], []
    for f in range(first, len(left)):
        rows_of_frame = uvd[start[f]:start[f + 1]]                          # min_track_length 1: every OK survivor, in keypoint order
        ok_ids = ids[f][status[f] == rr.OK].tolist()
        assert len(ok_ids) == len(rows_of_frame)
        keep = [k for k, t in enumerate(ok_ids) if t in renamed]
        out_ids += [renamed[ok_ids[k]] for k in keep]
        out_uvd.append(rows_of_frame[keep])
        out_start.append(len(out_ids))
    outside = sum(1 for t in kept if anchor_frame[t] < first)
    return (np.array(out_start, np.uint32), np.array(out_ids, np.uint32), np.concatenate(out_uvd).reshape(-1, 3), len(kept)), outside


def test_a_short_subpixel_window_keeps_the_anchors_from_before_the_window():
    s = _sequence(64, 96)
    params = dict(temporal_radius=8, **PARAMS)
    st = sr.Stream(3, refine={}, **params)
    for f in range(6):
        st.push(s.left[f], s.right[f])
    want, outside = _restricted(s.left, s.right, 3, {}, **params)
    got = st.window(3)
    _same(got, want)
    assert outside > 10 and got[3] > 30
    # and it is NOT the batch statement on those three frames: there the templates are the window's own first patches
    batch = rr.sequence_subpixel(s.left[3:], s.right[3:], **params)
    assert got[0].tobytes() == batch[0].tobytes() and got[1].tobytes() == batch[1].tobytes() and got[2].tobytes() != batch[2].tobytes()


@pytest.mark.parametrize("refine", [None, dict(max_sad=2000)], ids=["whole", "subpixel"])
def test_push_outputs_are_the_issued_ids_and_the_dropped_counts(refine):
    s = _sequence(96, 128)
    st, outs = _pushed(96, 128, "right", 4, refine=refine)
    _, ids, next_id = rr.link(s.left, s.right, **PARAMS)
    assert st.next_id == next_id
    if refine is None:
        for f in range(4):
            assert outs[f][0].tolist() == ids[f].tolist() and outs[f][2] == 0
            assert outs[f][1].shape == (len(ids[f]), 3) and (outs[f][1][:, :2] % 1 == 0).all()
        return
    status = rr.sequence_subpixel(s.left, s.right, refine=refine, **PARAMS)[5]
    for f in range(4):
        assert outs[f][0].tolist() == ids[f][status[f] == rr.OK].tolist() and outs[f][2] == int((status[f] != rr.OK).sum())
    assert sum(o[2] for o in outs) > 0


@pytest.mark.parametrize("refine", [None, {}], ids=["whole", "subpixel"])
def test_a_constant_frame_gives_an_empty_ring_entry_ends_every_track_and_the_ids_go_on_after_it(refine):
    s = _sequence(64, 96)
    left, right = s.left[:5].copy(), s.right[:5].copy()
    left[2] = right[2] = 90
    st = sr.Stream(5, refine=refine, **PARAMS)
    outs = [st.push(left[f], right[f]) for f in range(5)]
    assert len(outs[2][0]) == 0 and outs[2][1].shape == (0, 3) and len(st.ring[2]["ids"]) == 0
    assert outs[3][0].min() > max(outs[0][0].max(), outs[1][0].max())      # no id crosses the empty frame
    assert (st.ring[3]["source"] < 0).all() and (st.ring[4]["source"] >= 0).sum() > 10
    got = st.window(5)
    want = tr.sequence(left, right, **PARAMS) if refine is None else rr.sequence_subpixel(left, right, **PARAMS)
    _same(got, want)
    assert got[0][2] == got[0][3] and got[0][1] > 0 and got[0][5] > got[0][4] > got[0][3]


# ---- library surface ---------------------------------------------------------------------------------------------------------
NEW = {"ssba_track_stream_create", "ssba_track_stream_push", "ssba_track_stream_window", "ssba_track_stream_destroy"}


def test_header_symbols_and_sizes_agree():
    hdr = open(os.path.join(ROOT, "include", "ssba_tracks.h")).read()
    declared = set(re.findall(r"\b(ssba_track_[a-z_]+)\s*\(", hdr))
    assert NEW <= declared and declared == set(tracks.SYMBOLS), declared ^ set(tracks.SYMBOLS)
    build.build_library()
    out = subprocess.run(["nm", "-D", "--defined-only", tracks.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert {ln.split()[-1] for ln in out.splitlines() if ln.strip()} == declared
    assert C.sizeof(tracks.RefineParams) == 3 * 4 and C.sizeof(tracks.TrackParams) == 7 * 4
    cap = int(re.search(r"#define SSBA_TRACK_STREAM_MAX_WINDOW (\d+)", hdr).group(1))
    assert cap >= 64 and cap == tracks.STREAM_MAX_WINDOW
    shim = open(os.path.join(ROOT, "include", "ceres_slam_amd", "feature_tracks.hpp")).read()
    assert all(call in shim for call in NEW)                               # the shim reaches every new entry
    assert not NEW & set(re.findall(r"\bssba_\w+", open(os.path.join(ROOT, "include", "ssba.h")).read()))


def test_new_refusals_come_with_messages_before_a_device_is_looked_for():
    lib = tracks.load()
    u8, u32, i16 = tracks._u8p, tracks._u32p, tracks._i16p
    img, d16 = np.zeros((31, 31), np.uint8), np.zeros((31, 31), np.int16)
    pi, pd = img.ctypes.data_as(u8), d16.ctypes.data_as(i16)
    handle = C.c_void_p(7)
    ids, uvd, start = np.full(4, 7, np.uint32), np.full((4, 3), 7.0), np.full(3, 7, np.uint32)
    nobs, ndrop, nobs64, npts = C.c_uint32(7), C.c_uint32(7), C.c_uint64(7), C.c_uint32(7)
    po = (ids.ctypes.data_as(u32), uvd.ctypes.data_as(tracks._dp), C.byref(nobs), C.byref(ndrop))
    wo = (4, start.ctypes.data_as(u32), ids.ctypes.data_as(u32), uvd.ctypes.data_as(tracks._dp), C.byref(nobs64), C.byref(npts))
    tp = lambda **kw: C.byref(tracks.track_params(**dict(dict(max_features=4), **kw)))
    rp = lambda **kw: C.byref(tracks.refine_params(**kw))
    c, p, w = "ssba_track_stream_create", "ssba_track_stream_push", "ssba_track_stream_window"

    def refused(name, rc, word=""):
        msg = lib.ssba_track_last_error().decode()
        assert rc == -1, (name, rc, msg)
        assert msg.startswith(name + ": ") and len(msg) > len(name) + 2 and word in msg, (msg, word)

    for kw in (dict(max_features=0), dict(max_features=4097), dict(fast_threshold=-1), dict(fast_threshold=255), dict(max_hamming=-1), dict(max_hamming=257),
               dict(stereo_max_dy=-1), dict(max_disparity=-1), dict(temporal_radius=-1), dict(min_track_length=0)):
        refused(c, lib.ssba_track_stream_create(31, 31, tp(**kw), None, 2, -1, C.byref(handle)))
    for kw, word in ((dict(iterations=0), "iterations"), (dict(iterations=65), "iterations"), (dict(max_shift=0), "max_shift"), (dict(max_shift=9), "max_shift"),
                     (dict(max_sad=-1), "max_sad")):
        refused(c, lib.ssba_track_stream_create(31, 31, tp(), rp(**kw), 2, -1, C.byref(handle)), word)
    refused(c, lib.ssba_track_stream_create(31, 31, None, None, 2, -1, C.byref(handle)), "NULL")
    refused(c, lib.ssba_track_stream_create(31, 31, tp(), None, 2, -1, None), "NULL")
    for rows, cols in ((30, 31), (31, 30), (8193, 31), (31, 8193)):
        refused(c, lib.ssba_track_stream_create(rows, cols, tp(), None, 2, -1, C.byref(handle)), "31")
    for window in (0, tracks.STREAM_MAX_WINDOW + 1):
        refused(c, lib.ssba_track_stream_create(31, 31, tp(), rp(), window, -1, C.byref(handle)), "window")
    assert handle.value == 7
    refused(p, lib.ssba_track_stream_push(None, pi, pi, None, *po), "NULL stream")
    refused(p, lib.ssba_track_stream_push(handle, None, pi, None, *po), "NULL")
    refused(p, lib.ssba_track_stream_push(handle, pi, pi, pd, *po), "exactly one")
    refused(p, lib.ssba_track_stream_push(handle, pi, None, None, *po), "exactly one")
    for k in range(4):
        refused(p, lib.ssba_track_stream_push(handle, pi, pi, None, *[None if j == k else o for j, o in enumerate(po)]), "NULL output")
    refused(w, lib.ssba_track_stream_window(None, 1, *wo), "NULL stream")
    refused(w, lib.ssba_track_stream_window(handle, 0, *wo), "frames")
    refused(w, lib.ssba_track_stream_window(handle, 1, 4, None, *wo[2:]), "NULL output")
    refused(w, lib.ssba_track_stream_window(handle, 1, 4, wo[1], None, *wo[3:]), "NULL output")
    refused(w, lib.ssba_track_stream_window(handle, 1, *wo[:4], None, wo[5]), "NULL output")
    lib.ssba_track_stream_destroy(None)                                    # allowed
    for a in (ids, start):
        assert (a == 7).all()                                              # a refusal writes nothing
    assert (uvd == 7.0).all() and nobs.value == 7 and ndrop.value == 7 and nobs64.value == 7 and npts.value == 7
    with pytest.raises(tracks.SsbaError) as e:
        tracks.TrackStream(31, 31, 0)
    assert e.value.status == -1 and "window" in str(e.value)
    with pytest.raises(tracks.SsbaError):
        tracks.TrackStream(31, 31, 2, refine=dict(max_shift=9))
    with pytest.raises(AttributeError):
        tracks.TrackStream(31, 31, 2, max_featurse=4)
