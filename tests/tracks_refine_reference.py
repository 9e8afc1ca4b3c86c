"""The numpy statement of the sub-pixel refinement of include/ssba_tracks.h (ssba_track_refine, ssba_track_sequence_subpixel):
the 15 x 15 template around a track's anchor, its position in a target image to 1/256 pixel by Gauss-Newton steps on the
bilinear model.  Sums are Python / int64 integers; the only floating point is the step, in IEEE doubles with every product
rounded on its own, so the device equals this file to the bit.  Features and matching come from tracks_reference; the linking
is restated here because the ids are needed before pruning."""
import numpy as np

import tracks_reference as tr

OK, EDGE, FLAT, FAR, ITERATIONS, SAD, DISPARITY = range(7)
REFINE_DEFAULTS = dict(iterations=10, max_shift=4, max_sad=0)
RADIUS = 7                                   # the template is 15 x 15, its gradients need 17 x 17
MODE_2D, MODE_X = 0, 1

_J, _I = np.meshgrid(np.arange(-RADIUS, RADIUS + 1), np.arange(-RADIUS, RADIUS + 1), indexing="ij")      # row offset j, column offset i


def refine_params(**kw):
    p = dict(REFINE_DEFAULTS)
    for k in kw:
        if k not in p:
            raise AttributeError(k)
    p.update(kw)
    return p


def template(A, ax, ay, mode):
    """T, gx, gy (15 x 15 int64; gx and gy are twice the central difference) or None when the 17 x 17 support leaves the image."""
    A = np.asarray(A)
    rows, cols = A.shape
    if ax - RADIUS - 1 < 0 or ay - RADIUS - 1 < 0 or ax + RADIUS + 1 >= cols or ay + RADIUS + 1 >= rows:
        return None
    I = A.astype(np.int64)
    y, x = ay + _J, ax + _I
    T = I[y, x]
    gx = I[y, x + 1] - I[y, x - 1]
    gy = I[y + 1, x] - I[y - 1, x] if mode == MODE_2D else np.zeros_like(gx)
    return T, gx, gy


def leaves(B, px, py):
    """True when a bilinear tap of the window at (px, py) falls outside B."""
    rows, cols = np.asarray(B).shape
    bx, by = px >> 8, py >> 8
    return bx - RADIUS < 0 or by - RADIUS < 0 or bx + RADIUS + 1 >= cols or by + RADIUS + 1 >= rows


def evaluate(B, T, gx, gy, px, py):
    """bx, by (Python ints) and sad of one evaluation at (px, py), which must not leave B."""
    I = np.asarray(B).astype(np.int64)
    X, Y = px + 256 * _I, py + 256 * _J
    x0, fx, y0, fy = X >> 8, X & 255, Y >> 8, Y & 255
    S = (256 - fx) * (256 - fy) * I[y0, x0] + fx * (256 - fy) * I[y0, x0 + 1] + (256 - fx) * fy * I[y0 + 1, x0] + fx * fy * I[y0 + 1, x0 + 1]
    e = S - 65536 * T
    return int((gx * e).sum()), int((gy * e).sum()), int(np.abs(e).sum()) >> 16


def step(H11, H12, H22, bx, by, mode):
    """(dx, dy) as Python ints: doubles, every operand converted first, every product rounded before the subtraction."""
    f = np.float64
    if mode == MODE_X:
        return int(np.rint(f(bx) / (f(H11) * f(128.0)))), 0
    det = f(H11 * H22 - H12 * H12) * f(128.0)                        # the integer is below 2^53: exact
    nx = f(H22) * f(bx) - f(H12) * f(by)
    ny = f(H11) * f(by) - f(H12) * f(bx)
    return int(np.rint(nx / det)), int(np.rint(ny / det))


def refine_one(A, ax, ay, B, x0, y0, mode, **kw):
    """(x_q8, y_q8, status, sad): the position of A's template around (ax, ay) in B, started at (x0, y0).  The position is the
    start when the status is not OK; sad is that of the last evaluation made, 0 when none was."""
    p = refine_params(**kw)
    ax, ay, x0, y0 = int(ax), int(ay), int(x0), int(y0)
    t = template(A, ax, ay, mode)
    if t is None:
        return x0, y0, EDGE, 0
    T, gx, gy = t
    H11, H12, H22 = int((gx * gx).sum()), int((gx * gy).sum()), int((gy * gy).sum())
    flat = H11 <= 0 if mode == MODE_X else H11 * H22 - H12 * H12 <= 0
    px, py, sad = x0, y0, 0
    for _ in range(p["iterations"]):
        if leaves(B, px, py):
            return x0, y0, EDGE, sad
        if flat:
            return x0, y0, FLAT, sad
        bx, by, sad = evaluate(B, T, gx, gy, px, py)
        dx, dy = step(H11, H12, H22, bx, by, mode)
        px, py = px - dx, py - dy
        if max(abs(px - x0), abs(py - y0)) > 256 * p["max_shift"]:
            return x0, y0, FAR, sad
        if max(abs(dx), abs(dy)) <= 1:
            break
    else:
        return x0, y0, ITERATIONS, sad
    if p["max_sad"] > 0 and sad > p["max_sad"]:
        return x0, y0, SAD, sad
    return px, py, OK, sad


def refine(images, items, **kw):
    """ssba_track_refine: items (N, 7) = anchor image, ax, ay, target image, x0_q8, y0_q8, mode."""
    images = np.asarray(images)
    if images.ndim == 2:
        images = images[None]
    items = np.asarray(items, dtype=np.int64).reshape(-1, 7)
    xy, status, sad = np.zeros((len(items), 2), np.int32), np.zeros(len(items), np.int32), np.zeros(len(items), np.uint32)
    for k, (ia, ax, ay, ib, x0, y0, mode) in enumerate(items.tolist()):
        xy[k, 0], xy[k, 1], status[k], sad[k] = refine_one(images[ia], ax, ay, images[ib], x0, y0, mode, **kw)
    return xy, status, sad


def observation(A, ax, ay, L, R, x, y, d16, is_anchor, **kw):
    """(u_q8, v_q8, d_q8, status) of one survivor at whole pixel (x, y) with disparity d16 / 16 in frame images L and R (R None:
    the disparity comes from a map and stays), against the template around (ax, ay) of its track's anchor image A."""
    u, v, status = 256 * int(x), 256 * int(y), OK
    if not is_anchor:
        u, v, status, _ = refine_one(A, ax, ay, L, u, v, MODE_2D, **kw)
    if status != OK:
        return u, v, 16 * int(d16), status
    if R is None:
        return u, v, 16 * int(d16), OK
    xr, _, status, _ = refine_one(A, ax, ay, R, u - 16 * int(d16), v, MODE_X, **kw)
    if status == OK and u - xr <= 0:
        status = DISPARITY
    return u, v, u - xr, status


def link(left, right=None, disp16=None, **kw):
    """Survivors per frame (xy, desc, d16) and their ids before pruning, as tracks_reference.sequence issues them."""
    p = tr.params(**kw)
    assert (right is None) != (disp16 is None)
    frames = []
    for f in range(len(left)):
        xy, _, desc = tr.features(left[f], **p)
        if right is not None:
            rxy, _, rdesc = tr.features(right[f], **p)
            m, _ = tr.match(desc, xy, rdesc, rxy, tr.GATE_STEREO, **p)
            d16 = np.zeros(len(xy), np.int64)
            d16[m >= 0] = 16 * (xy[m >= 0, 0].astype(np.int64) - rxy[m[m >= 0], 0].astype(np.int64))
        else:
            d16 = np.asarray(disp16[f]).astype(np.int64)[xy[:, 1], xy[:, 0]]
        live = d16 > 0
        frames.append((xy[live], desc[live], d16[live]))
    ids, next_id = [], 0
    for f in range(len(left)):
        xy, desc, _ = frames[f]
        mine = np.full(len(xy), -1, np.int64)
        if f:
            m, _ = tr.match(frames[f - 1][1], frames[f - 1][0], desc, xy, tr.GATE_TEMPORAL, **p)
            a = np.nonzero(m >= 0)[0]
            mine[m[a]] = ids[f - 1][a]
        fresh = np.nonzero(mine < 0)[0]
        mine[fresh] = next_id + np.arange(len(fresh))
        next_id += len(fresh)
        ids.append(mine)
    return frames, ids, next_id


def sequence_subpixel(left, right=None, disp16=None, refine=None, **kw):
    """ssba_track_sequence_subpixel: state_start, point_id, uvd, num_points, num_dropped, and the statuses of every survivor
    (one int array per frame) for the tests that count them."""
    p = tr.params(**kw)
    rp = refine_params(**(refine or {}))
    frames, ids, next_id = link(left, right, disp16, **p)
    anchor = {}
    for f, mine in enumerate(ids):
        for j, t in enumerate(mine.tolist()):
            anchor.setdefault(t, (f, j))                                   # the (frame, slot) that issued the id
    q8, status = [], []
    for f, (xy, _, d16) in enumerate(frames):
        out, st = np.zeros((len(xy), 3), np.int64), np.zeros(len(xy), np.int64)
        for j in range(len(xy)):
            fa, ja = anchor[int(ids[f][j])]
            ax, ay = (int(c) for c in frames[fa][0][ja])
            u, v, d, st[j] = observation(left[fa], ax, ay, left[f], None if right is None else right[f], xy[j, 0], xy[j, 1], d16[j], (fa, ja) == (f, j), **rp)
            out[j] = (u, v, d)
        q8.append(out)
        status.append(st)
    length = np.zeros(next_id, np.int64)
    for f in range(len(frames)):
        np.add.at(length, ids[f][status[f] == OK], 1)
    kept = length >= p["min_track_length"]
    renamed = np.cumsum(kept) - 1
    start, out_ids, out_uvd = [0], [], []
    for f in range(len(frames)):
        k = (status[f] == OK) & kept[ids[f]] if len(ids[f]) else np.zeros(0, bool)
        out_ids.append(renamed[ids[f][k]] if len(ids[f]) else np.zeros(0, np.int64))
        out_uvd.append(q8[f][k].astype(np.float64) / 256.0)
        start.append(start[-1] + int(k.sum()))
    dropped = int(sum((s != OK).sum() for s in status))
    return (np.array(start, np.uint32), np.concatenate(out_ids).astype(np.uint32), np.concatenate(out_uvd).reshape(-1, 3), int(kept.sum()), dropped, status)
