"""The numpy statement of include/ssba_tracks.h: FAST scores, 3 x 3 suppression, selection, BRIEF-256, the gated cross-checked
matcher and the track ids.  Integer arithmetic throughout, so the device equals it to the bit; nothing here is shared with the
library's source, the pattern recipe included (it is restated below and compared with the committed header by a test)."""
import numpy as np

BORDER = 15
RING = [(0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3), (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1), (-2, -2), (-1, -3)]
GATE_NONE, GATE_STEREO, GATE_TEMPORAL = 0, 1, 2
DEFAULTS = dict(fast_threshold=20, max_features=1000, stereo_max_dy=5, max_disparity=128, max_hamming=64, temporal_radius=0, min_track_length=2)


def params(**kw):
    p = dict(DEFAULTS)
    for k in kw:
        if k not in p:
            raise AttributeError(k)
    p.update(kw)
    return p


def pattern():
    """(256, 4) rows (ax, ay, bx, by): the header's recipe."""
    s, rows = 20161021, []

    def draw():
        nonlocal s
        s = (s * 1103515245 + 12345) % (1 << 31)
        return (s >> 16) % 27 - 13

    while len(rows) < 256:
        r = (draw(), draw(), draw(), draw())
        if r[:2] != r[2:]:
            rows.append(r)
    return np.array(rows, dtype=np.int64)


def scores(img, fast_threshold):
    """(rows, cols) int32: the ring score where the pixel is a candidate, 0 elsewhere."""
    I = np.asarray(img).astype(np.int32)
    rows, cols = I.shape
    out = np.zeros((rows, cols), np.int32)
    if rows < 2 * BORDER + 1 or cols < 2 * BORDER + 1:
        return out
    ys, xs = slice(BORDER, rows - BORDER), slice(BORDER, cols - BORDER)
    c = I[ys, xs]
    d = np.stack([I[BORDER + dy:rows - BORDER + dy, BORDER + dx:cols - BORDER + dx] - c for dx, dy in RING])
    bright = np.full(c.shape, -255, np.int32)
    dark = np.full(c.shape, -255, np.int32)
    for a in range(16):
        arc = d[[(a + k) % 16 for k in range(9)]]
        bright = np.maximum(bright, arc.min(axis=0))
        dark = np.maximum(dark, (-arc).min(axis=0))
    s = np.maximum(0, np.maximum(bright, dark))
    out[ys, xs] = np.where(s > fast_threshold, s, 0)
    return out


def suppress(s):
    """Scores of the survivors of the 3 x 3 rule, 0 elsewhere."""
    rows, cols = s.shape
    p = np.pad(s, 1)
    keep = s > 0
    for j in (-1, 0, 1):
        for i in (-1, 0, 1):
            if i == 0 and j == 0:
                continue
            q = p[1 + j:1 + j + rows, 1 + i:1 + i + cols]
            before = j < 0 or (j == 0 and i < 0)
            keep &= (s > q) | ((s == q) & (not before))
    return np.where(keep, s, 0)


def select(kept, max_features):
    """Row-major (x, y) uint16 pairs and scores of at most max_features survivors: highest scores, then smallest indices."""
    flat = kept.ravel()
    idx = np.nonzero(flat)[0]
    if len(idx) > max_features:
        order = np.lexsort((idx, -flat[idx]))          # by score descending, then by index
        idx = np.sort(idx[order[:max_features]])
    cols = kept.shape[1]
    xy = np.stack([idx % cols, idx // cols], axis=1).astype(np.uint16)
    return xy, flat[idx].astype(np.uint8)


def box_sums(img):
    """5 x 5 integer sums; entries within 2 pixels of an edge are not used by a legal keypoint and hold 0."""
    I = np.asarray(img).astype(np.int64)
    rows, cols = I.shape
    out = np.zeros((rows, cols), np.int64)
    acc = np.zeros((rows - 4, cols - 4), np.int64)
    for j in range(5):
        for i in range(5):
            acc += I[j:j + rows - 4, i:i + cols - 4]
    out[2:rows - 2, 2:cols - 2] = acc
    return out


def describe(img, xy):
    """(K, 8) uint32: bit i at word i / 32, position i % 32."""
    box, pat = box_sums(img), pattern()
    x, y = xy[:, 0].astype(np.int64)[:, None], xy[:, 1].astype(np.int64)[:, None]
    bits = box[y + pat[None, :, 1], x + pat[None, :, 0]] < box[y + pat[None, :, 3], x + pat[None, :, 2]]      # (K, 256)
    weights = (1 << np.arange(32, dtype=np.uint64))
    return (bits.reshape(-1, 8, 32).astype(np.uint64) * weights).sum(axis=2).astype(np.uint32)


def features(img, **kw):
    p = params(**kw)
    xy, sc = select(suppress(scores(img, p["fast_threshold"])), p["max_features"])
    return xy, sc, describe(img, xy)


def hamming(da, db):
    """(na, nb) distances of two sets of 8-word descriptors."""
    a = np.ascontiguousarray(da, dtype=np.uint32).reshape(-1, 8).view(np.uint8)
    b = np.ascontiguousarray(db, dtype=np.uint32).reshape(-1, 8).view(np.uint8)
    if len(a) == 0 or len(b) == 0:
        return np.zeros((len(a), len(b)), np.int64)
    return np.unpackbits(a[:, None, :] ^ b[None, :, :], axis=2).sum(axis=2).astype(np.int64)


def gate_matrix(xy_a, xy_b, gate, p):
    xa, ya = (np.asarray(xy_a).reshape(-1, 2)[:, k].astype(np.int64)[:, None] for k in (0, 1))
    xb, yb = (np.asarray(xy_b).reshape(-1, 2)[:, k].astype(np.int64)[None, :] for k in (0, 1))
    if gate == GATE_STEREO:
        return (np.abs(ya - yb) < p["stereo_max_dy"]) & (xa - xb > 0) & (xa - xb <= p["max_disparity"])
    if gate == GATE_TEMPORAL and p["temporal_radius"] > 0:
        return (np.abs(xa - xb) <= p["temporal_radius"]) & (np.abs(ya - yb) <= p["temporal_radius"])
    return np.ones((xa.shape[0], xb.shape[1]), bool)


def match(desc_a, xy_a, desc_b, xy_b, gate=GATE_NONE, **kw):
    """match_a, dist_a (int32; -1: none): each the other's best under the gate, the smallest index on ties, distance <= max_hamming."""
    p = params(**kw)
    na, nb = len(np.asarray(xy_a).reshape(-1, 2)), len(np.asarray(xy_b).reshape(-1, 2))
    m, dist = np.full(na, -1, np.int32), np.full(na, -1, np.int32)
    if na == 0 or nb == 0:
        return m, dist
    h = hamming(desc_a, desc_b)
    ok = gate_matrix(xy_a, xy_b, gate, p)
    big = np.int64(1) << 40
    best_b = np.where(ok, h * 65536 + np.arange(nb)[None, :], big).min(axis=1)
    best_a = np.where(ok, h * 65536 + np.arange(na)[:, None], big).min(axis=0)
    for a in range(na):
        if best_b[a] == big:
            continue
        b, d = int(best_b[a] % 65536), int(best_b[a] // 65536)
        if best_a[b] != big and int(best_a[b] % 65536) == a and d <= p["max_hamming"]:
            m[a], dist[a] = b, d
    return m, dist


def sequence(left, right=None, disp16=None, **kw):
    """state_start (F + 1) uint32, point_id uint32, uvd (N, 3) float64, num_points; stats: survivors per frame and temporal matches
    per pair, before pruning."""
    p = params(**kw)
    assert (right is None) != (disp16 is None)
    F = len(left)
    frames = []
    for f in range(F):
        xy, _, desc = features(left[f], **p)
        if right is not None:
            rxy, _, rdesc = features(right[f], **p)
            m, _ = match(desc, xy, rdesc, rxy, GATE_STEREO, **p)
            d16 = np.zeros(len(xy), np.int64)
            d16[m >= 0] = 16 * (xy[m >= 0, 0].astype(np.int64) - rxy[m[m >= 0], 0].astype(np.int64))
        else:
            d16 = np.asarray(disp16[f]).astype(np.int64)[xy[:, 1], xy[:, 0]]
        live = d16 > 0
        frames.append((xy[live], desc[live], d16[live]))
    ids, next_id, temporal = [], 0, []
    for f in range(F):
        xy, desc, _ = frames[f]
        mine = np.full(len(xy), -1, np.int64)
        if f:
            pxy, pdesc, _ = frames[f - 1]
            m, _ = match(pdesc, pxy, desc, xy, GATE_TEMPORAL, **p)
            a = np.nonzero(m >= 0)[0]
            mine[m[a]] = ids[f - 1][a]
            temporal.append(len(a))
        fresh = np.nonzero(mine < 0)[0]
        mine[fresh] = next_id + np.arange(len(fresh))
        next_id += len(fresh)
        ids.append(mine)
    length = np.bincount(np.concatenate(ids).astype(np.int64), minlength=next_id) if next_id else np.zeros(0, np.int64)
    kept = length >= p["min_track_length"]
    renamed = np.cumsum(kept) - 1
    start, out_ids, out_uvd = [0], [], []
    for f in range(F):
        xy, _, d16 = frames[f]
        k = kept[ids[f]] if len(ids[f]) else np.zeros(0, bool)
        out_ids.append(renamed[ids[f][k]] if len(ids[f]) else np.zeros(0, np.int64))
        out_uvd.append(np.stack([xy[k, 0].astype(np.float64), xy[k, 1].astype(np.float64), d16[k] / 16.0], axis=1))
        start.append(start[-1] + int(k.sum()))
    stats = dict(survivors=[len(fr[0]) for fr in frames], temporal=temporal)
    return (np.array(start, np.uint32), np.concatenate(out_ids).astype(np.uint32), np.concatenate(out_uvd).reshape(-1, 3), int(kept.sum()), stats)
