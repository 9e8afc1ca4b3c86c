"""ctypes binding of include/ssba_tracks.h (ceres_slam_amd/libssba_tracks.so): sparse stereo feature tracks from raw frames.

A loader of its own: the library shares nothing with libssba.so, and capi.SYMBOLS stays the list of include/ssba.h.  HIP only:
without the library or a device every call raises, there is no CPU path (the numpy statement lives under tests/)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .capi import Camera, SsbaError

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libssba_tracks.so")

#: every symbol include/ssba_tracks.h declares
SYMBOLS = ["ssba_track_default_params", "ssba_track_features", "ssba_track_match", "ssba_track_sequence", "ssba_track_last_error",
           "ssba_track_default_refine_params", "ssba_track_refine", "ssba_track_sequence_subpixel", "ssba_track_stream_create",
           "ssba_track_stream_push", "ssba_track_stream_window", "ssba_track_stream_destroy", "ssba_track_default_odometry_params",
           "ssba_track_stream_enable_odometry", "ssba_track_stream_pose", "ssba_track_relative_pose"]
BORDER, MAX_FEATURES, DESC_WORDS = 15, 4096, 8
GATE_NONE, GATE_STEREO, GATE_TEMPORAL = 0, 1, 2
REFINE_OK, REFINE_EDGE, REFINE_FLAT, REFINE_FAR, REFINE_ITERATIONS, REFINE_SAD, REFINE_DISPARITY = range(7)
REFINE_2D, REFINE_X_ONLY = 0, 1
STREAM_MAX_WINDOW = 256
ODOMETRY_MAX, ODOMETRY_MAX_REFINE = 4096, 1024
POSE_OK, POSE_FIRST_FRAME, POSE_FEW_MATCHES, POSE_FEW_INLIERS, POSE_NUMERICAL = range(5)

_u8p, _u16p, _u32p, _i16p, _i32p = (C.POINTER(t) for t in (C.c_uint8, C.c_uint16, C.c_uint32, C.c_int16, C.c_int32))
_dp = C.POINTER(C.c_double)


class TrackParams(C.Structure):
    """ssba_track_params; track_params(**kw) fills in the library's defaults."""
    _fields_ = [(n, C.c_int32) for n in ("fast_threshold", "max_features", "stereo_max_dy", "max_disparity", "max_hamming", "temporal_radius",
                                         "min_track_length")]


class RefineParams(C.Structure):
    """ssba_track_refine_params; refine_params(**kw) fills in the library's defaults."""
    _fields_ = [(n, C.c_int32) for n in ("iterations", "max_shift", "max_sad")]


class OdometryParams(C.Structure):
    """ssba_track_odometry_params; odometry_params(**kw) fills in the library's defaults."""
    _fields_ = [("camera", Camera), ("ransac_iterations", C.c_uint32), ("ransac_threshold", C.c_double), ("refine_iterations", C.c_uint32),
                ("observation_variance", C.c_double), ("first_pose", C.c_double * 12)]


class PoseInfo(C.Structure):
    """ssba_track_pose_info"""
    _fields_ = [("status", C.c_int32), ("num_matches", C.c_uint32), ("num_inliers", C.c_uint32), ("num_iterations", C.c_uint32),
                ("initial_cost", C.c_double), ("final_cost", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


_lib = None


def load():
    """Load libssba_tracks.so; raises if it was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `python -m ceres_slam_amd.build` (the tracker is HIP-only, there is no CPU fallback)")
    L = C.CDLL(LIB_PATH)
    P = C.POINTER(TrackParams)
    L.ssba_track_default_params.argtypes = [P]
    L.ssba_track_default_params.restype = None
    L.ssba_track_features.argtypes = [_u8p, C.c_uint32, C.c_uint32, C.c_uint32, P, C.c_int, _u32p, _u16p, _u8p, _u32p]
    L.ssba_track_match.argtypes = [_u32p, _u16p, C.c_uint32, _u32p, _u16p, C.c_uint32, C.c_int, P, C.c_int, _i32p, _i32p]
    L.ssba_track_sequence.argtypes = [_u8p, _u8p, _i16p, C.c_uint32, C.c_uint32, C.c_uint32, P, C.c_int, C.c_uint64, _u32p, _u32p, _dp,
                                      C.POINTER(C.c_uint64), _u32p]
    R = C.POINTER(RefineParams)
    L.ssba_track_default_refine_params.argtypes = [R]
    L.ssba_track_default_refine_params.restype = None
    L.ssba_track_refine.argtypes = [_u8p, C.c_uint32, C.c_uint32, C.c_uint32, _i32p, C.c_uint32, R, C.c_int, _i32p, _i32p, _u32p]
    L.ssba_track_sequence_subpixel.argtypes = L.ssba_track_sequence.argtypes + [R, C.POINTER(C.c_uint64)]
    L.ssba_track_stream_create.argtypes = [C.c_uint32, C.c_uint32, P, R, C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]
    L.ssba_track_stream_push.argtypes = [C.c_void_p, _u8p, _u8p, _i16p, _u32p, _dp, _u32p, _u32p]
    L.ssba_track_stream_window.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, _u32p, _u32p, _dp, C.POINTER(C.c_uint64), _u32p]
    L.ssba_track_stream_destroy.argtypes = [C.c_void_p]
    L.ssba_track_stream_destroy.restype = None
    L.ssba_track_last_error.restype = C.c_char_p
    O = C.POINTER(OdometryParams)
    L.ssba_track_default_odometry_params.argtypes = [O]
    L.ssba_track_default_odometry_params.restype = None
    L.ssba_track_stream_enable_odometry.argtypes = [C.c_void_p, O]
    L.ssba_track_stream_pose.argtypes = [C.c_void_p, _dp, _dp, C.POINTER(PoseInfo)]
    L.ssba_track_relative_pose.argtypes = [O, C.c_uint32, C.c_uint32, _dp, _dp, C.c_int, _dp, _u8p, _dp, C.POINTER(PoseInfo), _dp, _i32p]
    _lib = L
    return L


def check(status: int, where: str):
    if status != 0:
        raise SsbaError(status, where, load().ssba_track_last_error().decode(errors="replace"))


def track_params(**kw) -> TrackParams:
    p = TrackParams()
    load().ssba_track_default_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, int(v))
    return p


def refine_params(**kw) -> RefineParams:
    p = RefineParams()
    load().ssba_track_default_refine_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, int(v))
    return p


def odometry_params(**kw) -> OdometryParams:
    """camera: a dict or a capi.Camera; first_pose: 12 numbers [t | R row-major]; the other fields by name."""
    p = OdometryParams()
    load().ssba_track_default_odometry_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        if k == "camera":
            p.camera = v if isinstance(v, Camera) else Camera(**{n: float(v[n]) for n in ("fu", "fv", "cu", "cv", "b")})
        elif k == "first_pose":
            p.first_pose = (C.c_double * 12)(*np.asarray(v, dtype=np.float64).reshape(12))
        elif k in ("ransac_iterations", "refine_iterations"):
            setattr(p, k, int(v))
        else:
            setattr(p, k, float(v))
    return p


def relative_pose(uvd_prev, uvd_cur, frame_index: int = 0, device: int = -1, **odometry):
    """The odometry's kernels on a list of matches paired by position (ssba_track_relative_pose).  Returns a dict: T_ransac (12,),
    inlier (n,) uint8, T (12,), info (PoseInfo.as_dict), cost_log and step_ok (refine_iterations + 1 entries each)."""
    a = np.ascontiguousarray(uvd_prev, dtype=np.float64).reshape(-1, 3)
    b = np.ascontiguousarray(uvd_cur, dtype=np.float64).reshape(-1, 3)
    if len(a) != len(b):
        raise ValueError("the matches are paired by position")
    p = odometry_params(**odometry)
    Tr, T, flags, info = np.zeros(12), np.zeros(12), np.zeros(max(len(a), 1), np.uint8), PoseInfo()
    log, ok = np.zeros(int(p.refine_iterations) + 1), np.zeros(int(p.refine_iterations) + 1, np.int32)
    check(load().ssba_track_relative_pose(C.byref(p), int(frame_index), len(a), a.ctypes.data_as(_dp), b.ctypes.data_as(_dp), device, Tr.ctypes.data_as(_dp),
                                          flags.ctypes.data_as(_u8p), T.ctypes.data_as(_dp), C.byref(info), log.ctypes.data_as(_dp), ok.ctypes.data_as(_i32p)),
          "ssba_track_relative_pose")
    return dict(T_ransac=Tr, inlier=flags[:len(a)].copy(), T=T, info=info.as_dict(), cost_log=log, step_ok=ok)


def _stack(images, dtype, what):
    a = np.ascontiguousarray(images, dtype=dtype)
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3:
        raise ValueError(f"{what}: a (rows, cols) image or an (n, rows, cols) stack")
    return a


def track_features(images, device: int = -1, **params):
    """Detector and descriptor over a stack (ssba_track_features).  Returns count (n,), xy (n, max_features, 2) uint16,
    score (n, max_features) uint8, desc (n, max_features, 8) uint32; zeros behind each count."""
    img = _stack(images, np.uint8, "images")
    p = track_params(**params)
    n, rows, cols = img.shape
    m = max(int(p.max_features), 1)
    count, xy = np.zeros(n, np.uint32), np.zeros((n, m, 2), np.uint16)
    score, desc = np.zeros((n, m), np.uint8), np.zeros((n, m, DESC_WORDS), np.uint32)
    check(load().ssba_track_features(img.ctypes.data_as(_u8p), n, rows, cols, C.byref(p), device, count.ctypes.data_as(_u32p), xy.ctypes.data_as(_u16p),
                                     score.ctypes.data_as(_u8p), desc.ctypes.data_as(_u32p)), "ssba_track_features")
    return count, xy, score, desc


def track_match(desc_a, xy_a, desc_b, xy_b, gate: int = GATE_NONE, device: int = -1, **params):
    """The cross-checked matcher alone (ssba_track_match).  Returns match_a, dist_a (int32, -1: no match)."""
    da = np.ascontiguousarray(desc_a, dtype=np.uint32).reshape(-1, DESC_WORDS)
    db = np.ascontiguousarray(desc_b, dtype=np.uint32).reshape(-1, DESC_WORDS)
    pa = np.ascontiguousarray(xy_a, dtype=np.uint16).reshape(-1, 2)
    pb = np.ascontiguousarray(xy_b, dtype=np.uint16).reshape(-1, 2)
    if len(pa) != len(da) or len(pb) != len(db):
        raise ValueError("one position per descriptor")
    p = track_params(**params)
    match, dist = np.full(len(da), -1, np.int32), np.full(len(da), -1, np.int32)
    check(load().ssba_track_match(da.ctypes.data_as(_u32p), pa.ctypes.data_as(_u16p), len(da), db.ctypes.data_as(_u32p), pb.ctypes.data_as(_u16p), len(db),
                                  int(gate), C.byref(p), device, match.ctypes.data_as(_i32p), dist.ctypes.data_as(_i32p)), "ssba_track_match")
    return match, dist


def track_sequence(left, right=None, disp16=None, device: int = -1, capacity: int | None = None, **params):
    """Frames to tracks (ssba_track_sequence): state_start (F + 1,), point_id (N,), uvd (N, 3), num_points -- the inputs of
    frontend.compute_initial_guess_device / ssba_frontend_vo.  Exactly one of right (F images) and disp16 (F int16 maps, the
    format solver.stereo_sgbm_batch returns) is given.  capacity: room for observations, by default one per keypoint slot."""
    L = _stack(left, np.uint8, "left")
    F, rows, cols = L.shape
    R = None if right is None else _stack(right, np.uint8, "right")
    D = None if disp16 is None else _stack(disp16, np.int16, "disp16")
    for other, what in ((R, "right"), (D, "disp16")):
        if other is not None and other.shape != L.shape:
            raise ValueError(f"{what} must have the shape of left")
    p = track_params(**params)
    cap = F * max(int(p.max_features), 0) if capacity is None else int(capacity)
    start, ids, uvd = np.zeros(F + 1, np.uint32), np.zeros(max(cap, 1), np.uint32), np.zeros((max(cap, 1), 3))
    nobs, npts = C.c_uint64(0), C.c_uint32(0)
    check(load().ssba_track_sequence(L.ctypes.data_as(_u8p), None if R is None else R.ctypes.data_as(_u8p), None if D is None else D.ctypes.data_as(_i16p),
                                     F, rows, cols, C.byref(p), device, cap, start.ctypes.data_as(_u32p), ids.ctypes.data_as(_u32p), uvd.ctypes.data_as(_dp),
                                     C.byref(nobs), C.byref(npts)), "ssba_track_sequence")
    n = int(nobs.value)
    return start, ids[:n].copy(), uvd[:n].copy(), int(npts.value)


def track_refine(images, items, device: int = -1, **refine):
    """The sub-pixel refinement alone (ssba_track_refine).  items (N, 7) int32: anchor image, ax, ay, target image, x0_q8, y0_q8,
    mode (REFINE_2D or REFINE_X_ONLY).  Returns xy_q8 (N, 2) int32 (the start where the status is not REFINE_OK), status (N,)
    int32 and sad (N,) uint32."""
    img = _stack(images, np.uint8, "images")
    it = np.ascontiguousarray(items, dtype=np.int32).reshape(-1, 7)
    p = refine_params(**refine)
    n, rows, cols = img.shape
    xy, status, sad = np.zeros((len(it), 2), np.int32), np.zeros(len(it), np.int32), np.zeros(len(it), np.uint32)
    check(load().ssba_track_refine(img.ctypes.data_as(_u8p), n, rows, cols, it.ctypes.data_as(_i32p), len(it), C.byref(p), device, xy.ctypes.data_as(_i32p),
                                   status.ctypes.data_as(_i32p), sad.ctypes.data_as(_u32p)), "ssba_track_refine")
    return xy, status, sad


def track_sequence_subpixel(left, right=None, disp16=None, device: int = -1, capacity: int | None = None, refine=None, **params):
    """track_sequence with every observation refined to 1/256 pixel against its track's first patch
    (ssba_track_sequence_subpixel).  refine: a dict of RefineParams fields.  Returns track_sequence's tuple plus num_dropped, the
    number of observations whose refinement did not end REFINE_OK."""
    L = _stack(left, np.uint8, "left")
    F, rows, cols = L.shape
    R = None if right is None else _stack(right, np.uint8, "right")
    D = None if disp16 is None else _stack(disp16, np.int16, "disp16")
    for other, what in ((R, "right"), (D, "disp16")):
        if other is not None and other.shape != L.shape:
            raise ValueError(f"{what} must have the shape of left")
    p, rp = track_params(**params), refine_params(**(refine or {}))
    cap = F * max(int(p.max_features), 0) if capacity is None else int(capacity)
    start, ids, uvd = np.zeros(F + 1, np.uint32), np.zeros(max(cap, 1), np.uint32), np.zeros((max(cap, 1), 3))
    nobs, npts, ndrop = C.c_uint64(0), C.c_uint32(0), C.c_uint64(0)
    check(load().ssba_track_sequence_subpixel(L.ctypes.data_as(_u8p), None if R is None else R.ctypes.data_as(_u8p),
                                              None if D is None else D.ctypes.data_as(_i16p), F, rows, cols, C.byref(p), device, cap, start.ctypes.data_as(_u32p),
                                              ids.ctypes.data_as(_u32p), uvd.ctypes.data_as(_dp), C.byref(nobs), C.byref(npts), C.byref(rp), C.byref(ndrop)),
          "ssba_track_sequence_subpixel")
    n = int(nobs.value)
    return start, ids[:n].copy(), uvd[:n].copy(), int(npts.value), int(ndrop.value)


class TrackStream:
    """Frames pushed one by one into a tracker whose state stays on the device (ssba_track_stream_create).  window: how many of
    the most recent frames window() can cover.  refine: None for whole-pixel observations, or a dict of RefineParams fields (an
    empty one: the defaults) for sub-pixel ones against each track's first patch, however long ago that was.  odometry: None, or a
    dict of OdometryParams fields (camera at least): every push then also yields a pose, see pose()."""

    def __init__(self, rows: int, cols: int, window: int, device: int = -1, refine=None, odometry=None, **params):
        self.rows, self.cols, self.window_frames, self.pushed = int(rows), int(cols), int(window), 0
        self.params = track_params(**params)
        rp = None if refine is None else refine_params(**refine)
        self._h = C.c_void_p()
        check(load().ssba_track_stream_create(self.rows, self.cols, C.byref(self.params), None if rp is None else C.byref(rp), self.window_frames, device,
                                              C.byref(self._h)), "ssba_track_stream_create")
        if odometry is not None:
            try:
                self.enable_odometry(**odometry)
            except Exception:
                self.close()
                raise

    def enable_odometry(self, **odometry):
        """ssba_track_stream_enable_odometry: before the first push only."""
        if self._h is None:
            raise ValueError("the stream is closed")
        p = odometry_params(**odometry)
        check(load().ssba_track_stream_enable_odometry(self._h, C.byref(p)), "ssba_track_stream_enable_odometry")

    def pose(self):
        """The last push's (T_k_km1, T_k_0, info): [t | R row-major] with p_k = R p_km1 + t, T_k_0 = T_k_km1 o T_km1_0; info is a dict
        of status (POSE_OK ...), num_matches, num_inliers, num_iterations, initial_cost, final_cost.  No device work."""
        if self._h is None:
            raise ValueError("the stream is closed")
        rel, chain, info = np.zeros(12), np.zeros(12), PoseInfo()
        check(load().ssba_track_stream_pose(self._h, rel.ctypes.data_as(_dp), chain.ctypes.data_as(_dp), C.byref(info)), "ssba_track_stream_pose")
        return rel, chain, info.as_dict()

    def _image(self, a, dtype, what):
        a = np.ascontiguousarray(a, dtype=dtype)
        if a.shape != (self.rows, self.cols):
            raise ValueError(f"{what}: a ({self.rows}, {self.cols}) image")
        return a

    def push(self, left, right=None, disp16=None):
        """One stereo pair: left and exactly one of right / disp16 (the same one in every push).  Returns ids (n,) uint32 as issued,
        global to the stream; uvd (n, 3) of the frame's kept survivors in keypoint order; num_dropped."""
        if self._h is None:
            raise ValueError("the stream is closed")
        L = self._image(left, np.uint8, "left")
        R = None if right is None else self._image(right, np.uint8, "right")
        D = None if disp16 is None else self._image(disp16, np.int16, "disp16")
        m = max(int(self.params.max_features), 1)
        ids, uvd = np.zeros(m, np.uint32), np.zeros((m, 3))
        nobs, ndrop = C.c_uint32(0), C.c_uint32(0)
        check(load().ssba_track_stream_push(self._h, L.ctypes.data_as(_u8p), None if R is None else R.ctypes.data_as(_u8p),
                                            None if D is None else D.ctypes.data_as(_i16p), ids.ctypes.data_as(_u32p), uvd.ctypes.data_as(_dp), C.byref(nobs),
                                            C.byref(ndrop)), "ssba_track_stream_push")
        self.pushed += 1
        n = int(nobs.value)
        return ids[:n].copy(), uvd[:n].copy(), int(ndrop.value)

    def window(self, frames: int | None = None, capacity: int | None = None):
        """The last `frames` pushed frames (default: as many as the stream keeps) as track_sequence returns them: state_start,
        point_id, uvd, num_points."""
        if self._h is None:
            raise ValueError("the stream is closed")
        F = min(self.window_frames, self.pushed) if frames is None else int(frames)
        cap = max(F, 0) * max(int(self.params.max_features), 0) if capacity is None else int(capacity)
        start, ids, uvd = np.zeros(max(F, 0) + 1, np.uint32), np.zeros(max(cap, 1), np.uint32), np.zeros((max(cap, 1), 3))
        nobs, npts = C.c_uint64(0), C.c_uint32(0)
        check(load().ssba_track_stream_window(self._h, max(F, 0), cap, start.ctypes.data_as(_u32p), ids.ctypes.data_as(_u32p), uvd.ctypes.data_as(_dp),
                                              C.byref(nobs), C.byref(npts)), "ssba_track_stream_window")
        n = int(nobs.value)
        return start, ids[:n].copy(), uvd[:n].copy(), int(npts.value)

    def close(self):
        if self._h is not None:
            load().ssba_track_stream_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
