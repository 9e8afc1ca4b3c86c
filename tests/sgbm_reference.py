"""Numpy statement of the semi-global matcher (Hirschmueller 2008) in the single-pass, five-direction mode in which the
reference's dense driver calls it (cv::StereoSGBM sgbm(0, 64, 15), tests/dense_stereo_test.cpp:61-65): the truth for
ceres_slam_amd/csrc/ssba_sgbm.hip.  Written from the rules include/ssba.h states, entirely in integers, independently of the
kernels.  OpenCV is not available where the tests run, so bit parity with cv::StereoSGBM is unpinned; tests/test_sgbm_reference.py
pins this file by known answers.

    computable  x in [maxD, cols), maxD = min_disparity + D; W columns; everything else is invalid
    pre-filter  P = clamp(sobel_x(I), -cap, cap) + cap, rows reflected, 0 gradient in the first and last column
    pixel cost  Birchfield-Tomasi on the pre-filtered rows plus a quarter of Birchfield-Tomasi on the raw rows
    block cost  the sum over block_size x block_size, rows clamped to the image, columns to the computable range
    paths       L(p, d) = C(p, d) + min(L(q, d), L(q, d -+ 1) + P1, min L(q) + P2) - min L(q) for the predecessors
                (x-1, y), (x+1, y), (x-1, y-1), (x, y-1), (x+1, y-1); S = their sum
    winner      argmin S (smallest d on ties), uniqueness, sub-pixel parabola with C's truncating division
    left-right  per row, the right view's map from the winners that passed uniqueness; disp12_max_diff < 0 switches it off
"""
import numpy as np

DEFAULTS = dict(min_disparity=0, num_disparities=64, block_size=15, p1=0, p2=0, disp12_max_diff=0, pre_filter_cap=0, uniqueness_ratio=0,
                speckle_window_size=0, speckle_range=0, full_dp=0)
PATHS = ((-1, 0), (1, 0), (-1, -1), (0, -1), (1, -1))        # predecessor offsets (dx, dy)
BIG = 1 << 40
MAX_COLS = 5461            # the device holds a row's twelve byte signals in 64 KiB of LDS


class Unsupported(ValueError):
    """SSBA_ERR_UNSUPPORTED; a plain ValueError is SSBA_ERR_INVALID_ARGUMENT."""


def derive(rows, cols, **params):
    """The parameter check and the derived constants.  Raises ValueError / Unsupported exactly where the C call refuses."""
    unknown = set(params) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"unknown parameters {sorted(unknown)}")
    p = dict(DEFAULTS, **{k: int(v) for k, v in params.items()})
    D, bs = p["num_disparities"], p["block_size"]
    if p["min_disparity"] < 0:
        raise ValueError("min_disparity must not be negative")
    if D < 16 or D > 256 or D % 16:
        raise ValueError("num_disparities must be a multiple of 16 in 16 ... 256")
    if bs < 1 or bs > 15 or bs % 2 == 0:
        raise ValueError("block_size must be odd in 1 ... 15")
    if not 0 <= p["uniqueness_ratio"] <= 100:
        raise ValueError("uniqueness_ratio must be in 0 ... 100")
    if p["pre_filter_cap"] > 127:
        raise ValueError("pre_filter_cap above 127: the filtered image no longer fits 8 bits")
    if p["full_dp"]:
        raise ValueError("the eight-direction mode is not built")
    if rows < 2:
        raise ValueError("the pre-filter reflects rows: at least 2")
    maxD = p["min_disparity"] + D
    if cols <= maxD:
        raise ValueError("no computable column: cols must exceed min_disparity + num_disparities")
    if maxD > 2047:
        raise ValueError("min_disparity + num_disparities above 2047: disp16 no longer fits 16 bits")
    cap = max(p["pre_filter_cap"], 15) | 1
    P1 = p["p1"] if p["p1"] > 0 else 2
    P2 = max(p["p2"] if p["p2"] > 0 else 5, P1 + 1)
    if (2 * cap + 63) * bs * bs + P2 > 65535:
        raise ValueError("block cost plus P2 exceeds 16 bits")
    if p["speckle_window_size"] or p["speckle_range"]:
        raise Unsupported("the speckle filter is not built")
    if cols > MAX_COLS or rows * (cols - maxD) * D >= 1 << 31:
        raise Unsupported("image too large")
    return dict(min_d=p["min_disparity"], D=D, maxD=maxD, W=cols - maxD, r=bs // 2, cap=cap, P1=P1, P2=P2, uniq=p["uniqueness_ratio"],
                lr=p["disp12_max_diff"])


def prefilter(img, cap):
    I = np.asarray(img).astype(np.int64)
    rows, cols = I.shape
    y = np.arange(rows)
    ym, yp = np.where(y == 0, 1, y - 1), np.where(y == rows - 1, rows - 2, y + 1)
    g = np.zeros_like(I)
    dx = I[:, 2:] - I[:, :-2]
    g[:, 1:-1] = dx[ym] + 2 * dx + dx[yp]
    return np.clip(g, -cap, cap) + cap


def half_sample_range(A):
    """(min, max) of A[x] and its two half-sample neighbours along a row; floor division, the neighbour clamped to the row."""
    A = np.asarray(A).astype(np.int64)
    lo = (A + np.concatenate([A[..., :1], A[..., :-1]], axis=-1)) // 2
    hi = (A + np.concatenate([A[..., 1:], A[..., -1:]], axis=-1)) // 2
    return np.minimum(A, np.minimum(lo, hi)), np.maximum(A, np.maximum(lo, hi))


def birchfield_tomasi(A, B, xa, xb):
    """The cost of A at columns xa against B at columns xb (arrays that broadcast); A, B: (rows, cols)."""
    A, B = np.asarray(A).astype(np.int64), np.asarray(B).astype(np.int64)
    (amin, amax), (bmin, bmax) = half_sample_range(A), half_sample_range(B)
    a, b = A[:, xa], B[:, xb]
    c0 = np.maximum(0, np.maximum(a - bmax[:, xb], bmin[:, xb] - a))
    c1 = np.maximum(0, np.maximum(b - amax[:, xa], amin[:, xa] - b))
    return np.minimum(c0, c1)


def pixel_cost(left, right, k):
    """c[y][x - maxD][d - min_d] on the computable columns."""
    cols = np.asarray(left).shape[1]
    xa = np.arange(k["maxD"], cols)[:, None]
    xb = xa - (k["min_d"] + np.arange(k["D"]))[None, :]
    return (birchfield_tomasi(prefilter(left, k["cap"]), prefilter(right, k["cap"]), xa, xb)
            + (birchfield_tomasi(left, right, xa, xb) >> 2))


def block_cost(c, r):
    rows, W, _ = c.shape
    ys = np.clip(np.arange(rows)[:, None] + np.arange(-r, r + 1)[None, :], 0, rows - 1)
    xs = np.clip(np.arange(W)[:, None] + np.arange(-r, r + 1)[None, :], 0, W - 1)
    horiz = sum(c[:, xs[:, i], :] for i in range(2 * r + 1))
    return sum(horiz[ys[:, j]] for j in range(2 * r + 1))


def _advance(C, Lq, P1, P2):
    m = Lq.min(axis=-1, keepdims=True)
    pad = np.full(Lq.shape[:-1] + (1,), BIG, dtype=np.int64)
    below = np.concatenate([pad, Lq[..., :-1]], axis=-1) + P1
    above = np.concatenate([Lq[..., 1:], pad], axis=-1) + P1
    return C + np.minimum(np.minimum(Lq, below), np.minimum(above, m + P2)) - m


def path_costs(C, P1, P2):
    """The five L volumes, in the order of PATHS."""
    C = np.asarray(C).astype(np.int64)
    rows, W, _ = C.shape
    out = []
    for dx, dy in PATHS:
        L = C.copy()
        if dy == 0:
            xs = range(1, W) if dx < 0 else range(W - 2, -1, -1)
            for x in xs:
                L[:, x] = _advance(C[:, x], L[:, x + dx], P1, P2)
        else:
            x = np.arange(W)
            inside = (x + dx >= 0) & (x + dx < W)
            for y in range(1, rows):
                L[y, x[inside]] = _advance(C[y, x[inside]], L[y - 1, x[inside] + dx], P1, P2)
        out.append(L)
    return out


def trunc_div(n, d):
    """C's integer division (towards zero) for d > 0."""
    n, d = np.asarray(n, dtype=np.int64), np.asarray(d, dtype=np.int64)
    return np.where(n >= 0, n // d, -((-n) // d))


def select(S, min_d, uniq):
    """(winner as a disparity, its S, valid after uniqueness, disp16 before the left-right check); S: (rows, W, D)."""
    S = np.asarray(S).astype(np.int64)
    D = S.shape[-1]
    k = S.argmin(axis=-1)                                    # the first minimum: the smallest d
    smin = np.take_along_axis(S, k[..., None], axis=-1)[..., 0]
    d = np.arange(D)
    rival = (np.abs(d - k[..., None]) > 1) & (S * (100 - uniq) < smin[..., None] * 100)
    valid = ~rival.any(axis=-1)
    inner = (k > 0) & (k < D - 1)
    km, kp = np.clip(k - 1, 0, D - 1), np.clip(k + 1, 0, D - 1)
    sm = np.take_along_axis(S, km[..., None], axis=-1)[..., 0]
    sp = np.take_along_axis(S, kp[..., None], axis=-1)[..., 0]
    den = np.maximum(sm + sp - 2 * smin, 1)
    frac = np.where(inner, trunc_div((sm - sp) * 16 + den, 2 * den), 0)
    return k + min_d, smin, valid, 16 * (k + min_d) + frac


def left_right(dstar, smin, valid, disp16, min_d, maxD, cols, max_diff):
    """valid after the left-right check.  All arrays (rows, W) on the computable columns."""
    rows, W = dstar.shape
    cost2 = np.full((rows, cols), BIG, dtype=np.int64)
    disp2 = np.full((rows, cols), min_d - 1, dtype=np.int64)
    ys = np.arange(rows)
    for xi in range(W - 1, -1, -1):
        x2 = maxD + xi - dstar[:, xi]
        take = valid[:, xi] & (smin[:, xi] < cost2[ys, x2])
        cost2[ys[take], x2[take]] = smin[take, xi]
        disp2[ys[take], x2[take]] = dstar[take, xi]
    x = maxD + np.arange(W)[None, :]
    lo, hi = disp16 >> 4, (disp16 + 15) >> 4
    bad = np.ones((rows, W), dtype=bool)
    for dd in (lo, hi):
        at = x - dd
        inside = (at >= 0) & (at < cols)
        d2 = disp2[ys[:, None], np.clip(at, 0, cols - 1)]
        bad &= inside & (d2 >= min_d) & (np.abs(d2 - dd) > max_diff)
    return valid & ~bad


def finish(disp16_w, valid, rows, cols, min_d, maxD):
    disp16 = np.full((rows, cols), (min_d - 1) * 16, dtype=np.int16)
    disp16[:, maxD:] = np.where(valid, disp16_w, (min_d - 1) * 16).astype(np.int16)
    ok = np.zeros((rows, cols), dtype=bool)
    ok[:, maxD:] = valid
    disparity = np.where(ok, disp16.astype(np.float64) / 16.0, np.nan)
    return disp16, disparity


def from_volume(S, cols, min_d, uniq, max_diff):
    """Everything after the aggregation, for hand-made volumes: S (rows, W, D) -> (disp16, disparity)."""
    S = np.asarray(S)
    rows, W, D = S.shape
    maxD = min_d + D
    assert cols == maxD + W
    dstar, smin, valid, d16 = select(S, min_d, uniq)
    if max_diff >= 0:
        valid = left_right(dstar, smin, valid, d16, min_d, maxD, cols, max_diff)
    return finish(d16, valid, rows, cols, min_d, maxD)


def aggregate(left, right, k):
    C = block_cost(pixel_cost(left, right, k), k["r"])
    return C, sum(path_costs(C, k["P1"], k["P2"]))


def sgbm(left, right, **params):
    """(disp16 int16, disparity float64 with NaN at invalid pixels) of the rectified 8-bit pair."""
    left, right = np.asarray(left), np.asarray(right)
    if left.dtype != np.uint8 or right.dtype != np.uint8 or left.ndim != 2 or left.shape != right.shape:
        raise ValueError("the pair must be two uint8 images of one shape")
    rows, cols = left.shape
    k = derive(rows, cols, **params)
    _, S = aggregate(left, right, k)
    return from_volume(S, cols, k["min_d"], k["uniq"], k["lr"])
